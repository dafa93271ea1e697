"""The overlay fit without a GPU: the numpy model (np_fit_model.py) meets the recovery criterion on
the three scenes of fit_cases.py, the plain C++ twin (aptgpu_fit_overlay_host) meets it too and equals the model under
the parity contract, the fit's geometry is the overlay's, the sampler, the record's reasons and every refusal."""
import ctypes as C
import math

import numpy as np
import pytest

import fit_cases as fc
import np_fit_model as fm
import np_map_model as mm

import noaa_apt_amd as apt
from test_sat_cpu import TLE_2020, decaying_case, orbit


def host(image, track, settings=None, initial=None, scores=True, layers=None):
    return apt.fit_overlay_host(image, track, layers or fc.layers(), initial, settings or fc.fit_settings(),
                                return_scores=scores)


@pytest.mark.parametrize("k", sorted(fc.SCENES))
def test_model_recovers_the_scene(k):
    rounds, final, reason = fc.model_fit(k)
    truth = fc.scene(k)[2]
    print(f"scene {k}: model {final}, truth {truth}; rounds {[r.get('winner') for r in rounds]}")
    assert reason == 0 and len(rounds) == 3
    assert fc.recovered(final, truth)
    for r in rounds:
        inside = r["raw_count"][r["raw_count"] > 0]
        assert r["score"].size == 875 and 1000 <= inside.min() and inside.max() <= 4000
        assert np.count_nonzero(r["margin"] < fm.TAU) <= fc.EXCUSED_CAP * 875


@pytest.mark.parametrize("k", sorted(fc.SCENES))
def test_twin_recovers_the_scene_and_equals_the_model(k):
    image, track, truth = fc.scene(k)
    fit = host(image, track)
    print(f"scene {k}: twin {fc.final_of(fit)}, q {fit.q}, count {fit.count}")
    assert fit.reason == 0 and fit.info.status == 0 and len(fit.rounds) == 3 and fit.info.n_points == len(fc.points())
    assert fc.recovered(fc.final_of(fit), truth)
    fc.check_record_against_model(fit, fc.problem(k), k, f"twin, scene {k}")
    last = fit.rounds[-1]
    assert fc.final_of(fit) == (last.w_shift, last.w_yaw, last.w_hscale, last.w_vscale)
    assert (fit.q, fit.count, fit.time_offset_ms) == (last.q, last.count, 500 * fit.shift_rows)
    assert np.array_equal(fit.track, track[fc.MARGIN + fit.shift_rows:fc.MARGIN + fit.shift_rows + image.shape[0]])


def test_scene_1_overshoots_and_comes_back():
    rounds = host(*fc.scene(1)[:2]).rounds
    assert (rounds[1].w_shift, rounds[2].w_shift) == (8, 6)  # rounds are not monotone


def test_exact_recovery_reproduces_the_scene():
    image, track, truth = fc.scene(1)
    fit = host(image, track, scores=False)
    assert fc.final_of(fit) == truth
    white = {name: (255, 255, 255, 255) for name in ("countries", "lakes")}
    ms = fit.map_settings
    again, _, _ = mm.overlay(fc.background(image.shape[0]), fit.track, fc.parts(),
                             {"yaw": ms.yaw, "hscale": ms.hscale, "vscale": ms.vscale}, white)
    assert np.array_equal(again[:, :, 0], image)


def test_geometry_is_the_overlays():
    """(x, y) of a candidate are latlon_to_rel_px's minus the row's x offset, within 1e-9 px."""
    h, s, yaw, hscale, vscale = 240, 5, 0.013, 1.03, 0.97
    track = fc.scene(1)[1]
    f = fm.Shift(track, fc.MARGIN, s, h)
    a, b, ps = f.angles(fm.unit_of_deg(fc.points()))
    x, y, fcol, frow = fm.place(a, b, yaw, hscale / 0.0005, h * vscale / f.d, h, f.bx)
    pick = np.flatnonzero((ps > 0.5) & (frow >= 5) & (frow < h) & (np.abs(fcol) < 450))[::7][:400]
    assert len(pick) >= 200
    rows = track[fc.MARGIN + s:fc.MARGIN + s + h]
    sc = mm.Scalars(rows, yaw, hscale, vscale)
    xoff = [mm.rel_px(sc, (float(p[0]), float(p[1])))[0] for p in rows]
    worst = 0.0
    for i in pick:
        lon, lat = fc.points()[i]
        mx, my = mm.rel_px(sc, (float(lat) / 180.0 * math.pi, float(lon) / 180.0 * math.pi))
        mx -= xoff[mm.est_row(my, h)]
        worst = max(worst, abs(mx - x[i]), abs(my - y[i]))
    print(f"{len(pick)} points: the worst difference is {worst:.3e} px")
    assert worst <= 1e-9


# ---- the sampler
def test_sampler_equals_the_model_bit_for_bit():
    got = apt.fit_sample_points(fc.layers(), None, 0.05)
    assert got.shape == (43615, 2) and got.tobytes() == fc.points().tobytes()
    lakes = apt.fit_sample_points(fc.layers(), [apt.MAP_LAKES], 0.05)
    assert lakes.tobytes() == fm.sample_points(fc.parts(), 0.05, ("lakes",)).tobytes()
    coarse = apt.fit_sample_points(fc.layers(), None, 0.37)
    assert coarse.tobytes() == fm.sample_points(fc.parts(), 0.37).tobytes()


def test_sampler_edge_cases():
    parts = {"states": [np.array([[1.0, 2.0], [1.5, 2.0]])],
             "countries": [np.array([[10.0, 20.0]]), np.array([[0.0, 0.0], [0.01, 0.02], [0.26, 0.02]])]}
    layers = apt.MapLayers(states=parts["states"], countries=parts["countries"])
    got = apt.fit_sample_points(layers, None, 0.05)
    # the one-vertex part; a segment shorter than the spacing gives its first end; 0.25 / 0.05 = 5 steps (or 6 where
    # the quotient rounds above 5: the model decides); states are not in the default mask
    assert got.tobytes() == fm.sample_points(parts, 0.05).tobytes()
    assert got[0].tolist() == [10.0, 20.0] and got[1].tolist() == [0.0, 0.0] and got[2].tolist() == [0.01, 0.02]
    assert len(got) in (7, 8)
    both = apt.fit_sample_points(layers, [apt.MAP_STATES, apt.MAP_COUNTRIES], 0.05)
    assert both.tobytes() == fm.sample_points(parts, 0.05, ("states", "countries")).tobytes() and len(both) - len(got) in (10, 11)
    assert len(apt.fit_sample_points(apt.MapLayers(), None, 0.05)) == 0


def test_sampler_point_cap():
    seg = np.array([[-128.0, 0.0], [128.0, 0.0]])  # 256 degrees: the quotients below are exact
    layers = apt.MapLayers(countries=[seg])
    assert len(apt.fit_sample_points(layers, None, 2.0 ** -14)) == 1 << 22
    with pytest.raises(apt.InvalidError, match="2\\^22"):
        apt.fit_sample_points(layers, None, 2.0 ** -15)
    with pytest.raises(apt.InvalidError, match="2\\^22"):
        apt.fit_sample_points(apt.MapLayers(countries=[seg, np.array([[0.0, 0.0]])]), None, 2.0 ** -14)
    with pytest.raises(OverflowError):
        fm.sample_points({"countries": [seg]}, 2.0 ** -15)


# ---- scores, counts and the record
def _small(h):
    """scene 3's geometry cut to h rows"""
    _, start, (s, yaw, hscale, vscale) = fc.SCENES[3]
    track = mm.great_circle_track(*start, h + 2 * fc.MARGIN)
    white = {name: (255, 255, 255, 255) for name in ("countries", "lakes")}
    img, _, _ = mm.overlay(fc.background(h), track[fc.MARGIN + s:fc.MARGIN + s + h], fc.parts(),
                           {"yaw": yaw, "hscale": hscale, "vscale": vscale}, white)
    return np.ascontiguousarray(img[:, :, 0]), track


def test_sixteen_rows():
    image, track = _small(16)
    st = fc.fit_settings(min_points=8, rounds=2)
    fit = host(image, track, st)
    assert fit.info.height == 16 and fit.reason == 0 and len(fit.rounds) == 2
    fc.check_record_against_model(fit, fm.Problem(image, track, fc.points(), fc.params_of(st)), "h16", "twin, h = 16")


def test_no_margin_shifts_out_of_range_never_win():
    image, long_track, _ = fc.scene(3)
    track = long_track[fc.MARGIN:fc.MARGIN + image.shape[0]]
    st = fc.fit_settings(margin_rows=0, rounds=2)
    fit = host(image, track, st)
    assert fit.shift_rows == 0 and all(r.w_shift == 0 for r in fit.rounds)
    per_shift = 125
    for rho in range(2):
        s = fit.scores[rho].reshape(7, per_shift)
        assert not s["count"][[0, 1, 2, 4, 5, 6]].any() and not s["score"][[0, 1, 2, 4, 5, 6]].any()
        assert s["count"][3].all()
    fc.check_record_against_model(fit, fm.Problem(image, track, fc.points(), fc.params_of(st)), "m0", "twin, M = 0")


def test_constant_image_is_flat_and_keeps_the_initial_settings():
    image, track, _ = fc.scene(3)
    flat = np.full_like(image, 77)
    initial = apt.MapSettings(0.01, 1.02, 0.99, countries_color=(1, 2, 3, 4))
    fit = host(flat, track, initial=initial)
    assert fit.reason == apt.FIT_REASON_FLAT and fit.info.status == 0 and fit.info.n_rounds == 1 and fit.info.done == 1
    assert fc.final_of(fit) == (0, 0.01, 1.02, 0.99) and fit.time_offset_ms == 0 and (fit.q, fit.count) == (-1.0, 0)
    assert fit.map_settings.countries_color == (1, 2, 3, 4)
    assert fit.rounds[0].score == 0 and fit.rounds[0].index == 0 and fit.rounds[0].count >= 64
    assert not fit.scores["score"].any() and not fit.scores[1:]["count"].any()
    assert np.array_equal(fit.track, track[fc.MARGIN:fc.MARGIN + image.shape[0]])


def test_min_points_above_every_count_gives_no_candidate():
    image, track, _ = fc.scene(3)
    with pytest.raises(apt.InternalError, match="APTGPU_FIT_REASON_NO_CANDIDATE") as e:
        host(image, track, fc.fit_settings(min_points=100000))
    info = e.value.info
    assert (info.status, info.reason, info.n_rounds, info.height) == (1, apt.FIT_REASON_NO_CANDIDATE, 1, 120)
    assert info.round[0].q == -1.0


def test_channel_b_reads_the_other_half():
    image, track, truth = fc.scene(3)
    moved = np.full_like(image, 120)
    moved[:, 1040:] = image[:, :1040]
    a = host(image, track)
    b = host(moved, track, fc.fit_settings(channel="B"))
    assert fc.final_of(a) == fc.final_of(b) and fc.recovered(fc.final_of(b), truth)
    assert a.scores.tobytes() == b.scores.tobytes()
    assert host(moved, track, fc.fit_settings(channel="A"), scores=False).reason == apt.FIT_REASON_FLAT


def test_initial_settings_are_round_zeros_centre():
    image, track, truth = fc.scene(3)
    fit = host(image, track, initial=apt.MapSettings(0.02, 1.04, 0.96))
    e = fit.rounds[0]
    assert (e.c_shift, e.c_yaw, e.c_hscale, e.c_vscale) == (0, 0.02, 1.04, 0.96)
    # (another start may end in another optimum: shift and vscale trade against each other; what is
    # checked here is that the search is the model's from that start)
    fc.check_record_against_model(fit, fc.problem(3), 3, "twin, scene 3 from (0.02, 1.04, 0.96)")


def test_a_wide_box_and_many_candidates_per_shift():
    """R_0 = 64 (the widest box), and 1331 candidates of one shift"""
    image, track, _ = fc.scene(3)
    st = fc.fit_settings(radius=16, rounds=3, n_shift=0, yaw_step=0.004, n_yaw=5, hscale_step=0.01, n_hscale=5,
                         vscale_step=0.01, n_vscale=5)
    fit = host(image, track, st)
    assert fit.info.n_candidates == 1331
    fc.check_record_against_model(fit, fm.Problem(image, track, fc.points(), fc.params_of(st)), "wide", "twin, R = 64")


def test_scales_that_reach_zero_are_invalid():
    image, track, _ = fc.scene(3)
    st = fc.fit_settings(rounds=1, hscale_step=0.5, vscale_step=0.5)
    fit = host(image, track, st)
    s = fit.scores[0].reshape(7, 5, 5, 5)
    assert not s["count"][:, :, 0, :].any() and not s["count"][:, :, :, 0].any()  # hscale = 0 and vscale = 0
    fc.check_record_against_model(fit, fm.Problem(image, track, fc.points(), fc.params_of(st)), "zero", "twin, scale 0")


# ---- the orbit form
def _orbit_scene():
    ms, h = 1580246771392, 120
    o = orbit(TLE_2020, "NOAA 19", "start", ms)
    long_track = apt.margin_track(o, h, fc.MARGIN)
    white = {name: (255, 255, 255, 255) for name in ("countries", "lakes")}
    img, _, _ = mm.overlay(fc.background(h), long_track[fc.MARGIN + 3:fc.MARGIN + 3 + h], fc.parts(),
                           {"yaw": 0.01, "hscale": 1.02, "vscale": 0.98}, white)
    return ms, h, o, long_track, np.ascontiguousarray(img[:, :, 0])


def test_margin_track():
    ms, h, o, long_track, _ = _orbit_scene()
    assert long_track.shape == (h + 2 * fc.MARGIN, 2)
    assert np.array_equal(long_track[fc.MARGIN:fc.MARGIN + h], apt.sat_track_host(o, h))
    end = orbit(TLE_2020, "NOAA 19", "end", ms + 500 * h)
    assert np.array_equal(apt.margin_track(end, h, fc.MARGIN), long_track)


def test_orbit_form_equals_the_track_form():
    ms, h, o, long_track, image = _orbit_scene()
    a = host(image, o)
    b = host(image, long_track)
    assert fc.record(a.info) == fc.record(b.info) and a.scores.tobytes() == b.scores.tobytes()
    assert a.shift_rows != 0 and a.reason == 0 and len(a.rounds) == 3
    assert a.track is None and b.orbit is None
    assert (a.orbit.ref_time.kind, a.orbit.ref_time.unix_ms) == (apt.RefTime.START, ms + a.time_offset_ms)
    assert (a.orbit.sat_name, a.orbit.custom_tle) == (o.sat_name, o.custom_tle)
    assert (a.orbit.draw_map.yaw, a.orbit.draw_map.hscale, a.orbit.draw_map.vscale) == fc.final_of(a)[1:]
    # the moved orbit's track is the fitted slice
    assert np.array_equal(apt.sat_track_host(a.orbit, h), b.track)
    e = host(image, orbit(TLE_2020, "NOAA 19", "end", ms + 500 * h))
    assert fc.record(e.info) == fc.record(a.info)
    assert (e.orbit.ref_time.kind, e.orbit.ref_time.unix_ms) == (apt.RefTime.END, ms + 500 * h + a.time_offset_ms)


def test_sgp4_failure_is_an_error():
    image, _, _ = fc.scene(3)
    tle, ms = decaying_case()
    with pytest.raises(apt.InternalError, match="SGP4"):
        host(image, orbit(tle, "NOAA 15", "start", ms + 400 * 500))


# ---- refusals: none touches a device
class _Sized(apt.FitSettings):
    def _c(self, struct_size=None):
        return super()._c(struct_size=8)


REFUSALS = {
    "struct_size": (_Sized(), "struct_size"),
    "flags": (fc.fit_settings(flags=1), "flag"),
    "channel 2": (fc.fit_settings(channel=2), "channel"),
    "channel -1": (fc.fit_settings(channel=-1), "channel"),
    "layer mask": (fc.fit_settings(layers=[3]), "layer"),
    "rounds 0": (fc.fit_settings(rounds=0), "rounds"),
    "rounds 9": (fc.fit_settings(rounds=9, radius=0), "rounds"),
    "negative yaw step": (fc.fit_settings(yaw_step=-0.01), "steps"),
    "negative hscale step": (fc.fit_settings(hscale_step=-0.01), "steps"),
    "negative vscale step": (fc.fit_settings(vscale_step=-0.01), "steps"),
    "nan step": (fc.fit_settings(yaw_step=float("nan")), "steps"),
    "shift step 0": (fc.fit_settings(shift_step=0), "shift_step"),
    "negative shift step": (fc.fit_settings(shift_step=-4), "shift_step"),
    "negative n_shift": (fc.fit_settings(n_shift=-1), "negative"),
    "negative n_yaw": (fc.fit_settings(n_yaw=-1), "negative"),
    "negative n_hscale": (fc.fit_settings(n_hscale=-1), "negative"),
    "negative n_vscale": (fc.fit_settings(n_vscale=-1), "negative"),
    "negative margin": (fc.fit_settings(margin_rows=-1), "negative"),
    "negative radius": (fc.fit_settings(radius=-1), "negative"),
    "min_points 0": (fc.fit_settings(min_points=0), "min_points"),
    "R_0 66": (fc.fit_settings(radius=33, rounds=2), "64"),
    "R_0 128": (fc.fit_settings(radius=1, rounds=8), "64"),
    "spacing 0": (fc.fit_settings(spacing_deg=0.0), "spacing_deg"),
    "spacing negative": (fc.fit_settings(spacing_deg=-0.05), "spacing_deg"),
    "spacing nan": (fc.fit_settings(spacing_deg=float("nan")), "spacing_deg"),
    "candidates": (fc.fit_settings(n_shift=16, n_yaw=16, n_hscale=16, n_vscale=16), "2\\^20"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_settings_refusals(name):
    st, text = REFUSALS[name]
    image, track, _ = fc.scene(3)
    with pytest.raises(apt.InvalidError, match=text):
        apt.fit_overlay_host(image, track, fc.layers(), None, st)
    with pytest.raises(apt.InvalidError, match=text):  # the GPU form refuses before it touches a device
        apt.fit_overlay(image, track, fc.layers(), None, st)


def test_call_refusals():
    image, track, _ = fc.scene(3)
    for fn in (apt.fit_overlay_host, apt.fit_overlay):
        with pytest.raises(apt.InvalidError, match="16 rows"):
            fn(image[:15], track[:15 + 2 * fc.MARGIN], fc.layers(), None, fc.fit_settings())
        with pytest.raises(apt.InvalidError, match="exactly one"):
            fn(image, None, fc.layers(), None, fc.fit_settings())
        with pytest.raises(apt.InvalidError, match="MapLayers"):
            fn(image, track, None, None, fc.fit_settings())
        with pytest.raises(apt.InvalidError, match="2080"):
            fn(image[:, :2000], track, fc.layers(), None, fc.fit_settings())
        with pytest.raises(apt.InternalError, match="positions") as e:  # the count: found before any launch
            fn(image, track[:-1], fc.layers(), None, fc.fit_settings())
        assert (e.value.info.status, e.value.info.reason, e.value.info.height) == (1, 7, 120)
    with pytest.raises(apt.InvalidError, match="16 rows"):
        apt.fit_overlay_device(0x1000, 15, track, fc.layers(), None, fc.fit_settings())
    with pytest.raises(apt.InvalidError, match="flag"):
        apt.fit_overlay_device(0x1000, 120, track, fc.layers(), None, fc.fit_settings(flags=2))
    with pytest.raises(apt.InvalidError, match="image"):
        apt.fit_overlay_device(0, 120, track, fc.layers(), None, fc.fit_settings())


def test_both_track_and_orbit_are_refused():
    image, track, _ = fc.scene(3)
    L = apt.lib()
    co, keep = orbit(TLE_2020, "NOAA 19", "start", 1580246771392)._c()
    cs = fc.fit_settings()._c()
    err = C.create_string_buffer(256)
    f64p, u8p = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    args = (image.ctypes.data_as(u8p), 120, track.ctypes.data_as(f64p), len(track), C.byref(co), fc.layers()._p, None,
            C.byref(cs), None, None, None, err, 256)
    assert L.aptgpu_fit_overlay_host(*args) == 4 and b"exactly one" in err.value
    assert L.aptgpu_fit_overlay(None, *args) == 4 and b"exactly one" in err.value
    assert L.aptgpu_fit_overlay_device(None, C.c_void_p(0x1000), 120, None, *args[2:]) == 4
    del keep


def test_default_settings_and_abi():
    c = apt.api._CFitSettings()
    apt.lib().aptgpu_fit_default_settings(C.byref(c))
    d = apt.FitSettings()._c()
    assert bytes(c) == bytes(d)
    assert (c.margin_rows, c.shift_step, c.n_shift, c.rounds, c.radius, c.min_points) == (120, 8, 15, 4, 2, 64)
    assert (c.yaw_step, c.n_yaw, c.hscale_step, c.n_hscale, c.vscale_step, c.n_vscale, c.spacing_deg) == \
        (0.02, 3, 0.04, 3, 0.04, 3, 0.05)
    assert apt.abi_version() == 2
    assert C.sizeof(apt.api._CFitSettings) == 88 and C.sizeof(apt.FitRound) == 80 and C.sizeof(apt.FitResult) == 736
