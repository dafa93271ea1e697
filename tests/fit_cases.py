"""The scenes and shared checks of the overlay-fit tests (tests/test_fit_cpu.py, tests/test_gpu_fit.py): three
synthetic images with the fixture layers drawn by np_map_model.overlay from a known slice of a long track with known
settings, the recovery criterion, and the parity contract against np_fit_model.py.  Everything expensive is computed
once per process and shared."""
import functools
import os
from fractions import Fraction

import numpy as np

import noaa_apt_amd as apt
import np_fit_model as fm
import np_map_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHP = os.path.join(ROOT, "tests", "golden", "shapefiles")
MARGIN = 16
# scene -> (h, (lat, lon, az) of the long track, truth (shift, yaw, hscale, vscale))
SCENES = {
    1: (240, (-40.0, -66.0, 8.0), (6, 0.02, 1.04, 0.97)),
    2: (160, (8.0, -58.0, 192.0), (-7, -0.013, 0.973, 1.033)),
    3: (120, (-52.0, -68.0, 8.0), (3, 0.026, 1.05, 0.955)),
}
# the last round's steps: the recovery criterion is one of them on every axis
FINAL_STEPS = (1, 0.005, 0.01, 0.01)
EXCUSED_CAP = 0.05


def fit_settings(**over):
    kw = dict(channel="A", margin_rows=MARGIN, shift_step=4, n_shift=3, yaw_step=0.02, n_yaw=2, hscale_step=0.04,
              n_hscale=2, vscale_step=0.04, n_vscale=2, rounds=3, radius=2, spacing_deg=0.05, min_points=64)
    kw.update(over)
    return apt.FitSettings(**kw)


def params_of(st):
    ch = {"A": 0, "B": 1}.get(st.channel, st.channel)
    return fm.Params(ch, st.margin_rows, st.shift_step, st.n_shift, st.yaw_step, st.n_yaw, st.hscale_step, st.n_hscale,
                     st.vscale_step, st.n_vscale, st.rounds, st.radius, st.spacing_deg, st.min_points)


@functools.lru_cache(maxsize=None)
def parts():
    return {"countries": apt.read_shapefile(os.path.join(SHP, "countries.shp"), 5),
            "lakes": apt.read_shapefile(os.path.join(SHP, "lakes.shp"), 5)}


@functools.lru_cache(maxsize=None)
def layers():
    p = parts()
    return apt.MapLayers(countries=p["countries"], lakes=p["lakes"])


@functools.lru_cache(maxsize=None)
def points():
    return fm.sample_points(parts(), 0.05)


def background(h):
    gray = (np.random.default_rng(1).random((h, 2080)) * 60 + 90).astype(np.uint8)
    return np.concatenate([np.repeat(gray[:, :, None], 3, axis=2), np.full((h, 2080, 1), 255, np.uint8)], axis=2)


@functools.lru_cache(maxsize=None)
def scene(k):
    """(image (h, 2080) u8, long track (h + 2 M, 2), truth)"""
    h, start, truth = SCENES[k]
    track = mm.great_circle_track(*start, h + 2 * MARGIN)
    s, yaw, hscale, vscale = truth
    white = {name: (255, 255, 255, 255) for name in ("countries", "lakes")}
    img, _, _ = mm.overlay(background(h), track[MARGIN + s:MARGIN + s + h], parts(),
                           {"yaw": yaw, "hscale": hscale, "vscale": vscale}, white)
    image = np.ascontiguousarray(img[:, :, 0])
    image.setflags(write=False)
    track.setflags(write=False)
    return image, track, truth


@functools.lru_cache(maxsize=None)
def problem(k):
    image, track, _ = scene(k)
    return fm.Problem(image, track, points(), params_of(fit_settings()))


_ROUND_CACHE = {}


def model_round(prob, key, rho, centre):
    """np_fit_model's (score, count, margin) of one round from a centre, after min_points; cached per problem key."""
    k = (key, rho, tuple(centre))
    if k not in _ROUND_CACHE:
        raw_s, raw_c, margin = prob.round_scores(rho, centre)
        s, c = prob.apply_min_points(raw_s, raw_c)
        _ROUND_CACHE[k] = (s, c, margin)
    return _ROUND_CACHE[k]


@functools.lru_cache(maxsize=None)
def model_fit(k):
    return problem(k).fit()


def record(info):
    """every field of a FitResult that does not depend on the clock"""
    head = tuple(getattr(info, f) for f in ("status", "reason", "height", "n_rounds", "n_points", "n_candidates",
                                            "shift_rows", "time_offset_ms", "yaw", "hscale", "vscale", "q", "count", "done"))
    rounds = tuple(tuple(getattr(r, f) for f, _ in apt.FitRound._fields_) for r in info.round)
    return head + rounds


def recovered(final, truth):
    return all(abs(float(f) - float(t)) <= step * (1 + 1e-9) for f, t, step in zip(final, truth, FINAL_STEPS))


def final_of(fit):
    return (fit.shift_rows, fit.map_settings.yaw, fit.map_settings.hscale, fit.map_settings.vscale)


def check_record_against_model(fit, prob, key, label):
    """The parity contract: per round, from the centre the record reports, {score, count} equal the model's bit for bit
    on every candidate whose margin is at least TAU; at most 5 % of a round may be excused; the reported winner is the
    arg-max of the returned scores under the tie rule, as exact rationals.  Returns the excused masks per round."""
    masks = []
    assert fit.scores is not None and len(fit.rounds) >= 1
    for rho, e in enumerate(fit.rounds):
        centre = (e.c_shift, e.c_yaw, e.c_hscale, e.c_vscale)
        want_s, want_c, margin = model_round(prob, key, rho, centre)
        got = fit.scores[rho]
        excused = margin < fm.TAU
        n_exc = int(np.count_nonzero(excused))
        print(f"{label} round {rho}: centre {centre}, {n_exc} of {excused.size} candidates excused")
        assert n_exc <= EXCUSED_CAP * excused.size, (label, rho, n_exc)
        assert np.array_equal(got["score"][~excused], want_s[~excused]), (label, rho)
        assert np.array_equal(got["count"][~excused], want_c[~excused]), (label, rho)
        assert not got["zero"].any()
        best = fm.pick(got["score"], got["count"])
        assert best is not None and best == e.index, (label, rho, best, e.index)
        assert (e.score, e.count) == (int(got["score"][best]), int(got["count"][best]))
        assert e.q == float(e.score) / float(e.count)
        assert Fraction(e.score, e.count) == max(Fraction(int(s), int(c)) for s, c in zip(got["score"], got["count"]) if c)
        assert (e.w_shift, e.w_yaw, e.w_hscale, e.w_vscale) == prob.candidate(rho, centre, best), (label, rho)
        masks.append(excused)
    return masks
