"""The overlay fit on the GPU (fit_overlay, fit_overlay_device) against np_fit_model.py under the parity
contract of fit_cases.py: per round, from the centre the record reports, every candidate's {score, count} equals the
model's bit for bit unless a decision of one of its points lies within np_map_model.TAU of its boundary; the excused
candidates are counted, printed and capped at 5 % of a round.  The GPU's sums equal the C++ twin's on the same set, the
three scenes meet the recovery criterion, and the result goes into process() as it is."""
import numpy as np
import pytest
import torch

import fit_cases as fc
import np_fit_model as fm
import np_map_model as mm

import noaa_apt_amd as apt
from test_sat_cpu import TLE_2020, decaying_case, orbit

pytestmark = pytest.mark.gpu


def gpu(image, track, settings=None, initial=None, scores=True):
    return apt.fit_overlay(image, track, fc.layers(), initial, settings or fc.fit_settings(), return_scores=scores)


def host(image, track, settings=None, initial=None):
    return apt.fit_overlay_host(image, track, fc.layers(), initial, settings or fc.fit_settings(), return_scores=True)


def check_against_twin(fit, twin, masks, label):
    """the GPU's sums equal the twin's wherever the model excuses neither; the records agree when nothing is excused"""
    assert len(fit.rounds) == len(twin.rounds), label
    for rho, excused in enumerate(masks):
        g, t = fit.rounds[rho], twin.rounds[rho]
        if (g.c_shift, g.c_yaw, g.c_hscale, g.c_vscale) != (t.c_shift, t.c_yaw, t.c_hscale, t.c_vscale):
            print(f"{label} round {rho}: the twin started from another centre (an excused candidate won a round)")
            return
        assert np.array_equal(fit.scores[rho][~excused], twin.scores[rho][~excused]), (label, rho)


@pytest.mark.parametrize("k", sorted(fc.SCENES))
def test_scene(k):
    image, track, truth = fc.scene(k)
    fit = gpu(image, track)
    print(f"scene {k}: GPU {fc.final_of(fit)}, q {fit.q}, count {fit.count}; truth {truth}")
    assert fit.reason == 0 and fit.info.status == 0 and len(fit.rounds) == 3 and fit.info.done == 1
    assert fc.recovered(fc.final_of(fit), truth)
    masks = fc.check_record_against_model(fit, fc.problem(k), k, f"GPU, scene {k}")
    check_against_twin(fit, host(image, track), masks, f"scene {k}")
    assert np.array_equal(fit.track, track[fc.MARGIN + fit.shift_rows:fc.MARGIN + fit.shift_rows + image.shape[0]])


def test_device_form_equals_the_host_image_form():
    image, track, _ = fc.scene(3)
    a = gpu(image, track)
    d_image = torch.from_numpy(np.array(image)).to("cuda:0")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    b = apt.fit_overlay_device(d_image.data_ptr(), image.shape[0], track, fc.layers(), None, fc.fit_settings(),
                               stream=stream.cuda_stream, return_scores=True)
    c = apt.fit_overlay_device(d_image.data_ptr(), image.shape[0], track, fc.layers(), None, fc.fit_settings())
    assert fc.record(a.info) == fc.record(b.info) == fc.record(c.info)
    assert a.scores.tobytes() == b.scores.tobytes() and c.scores is None


def test_hand_over_to_process():
    image, track, truth = fc.scene(1)
    fit = gpu(image, track, scores=False)
    assert fc.final_of(fit) == truth  # exact on this scene
    h = image.shape[0]
    white = (255, 255, 255, 255)
    ms = apt.MapSettings(fit.map_settings.yaw, fit.map_settings.hscale, fit.map_settings.vscale, white, white, white)
    # the background as a signal, mapped dark (two samples outside the video set the limits), so every fragment shows
    signal = fc.background(h)[:, :, 0].astype(np.float32)
    signal[0, 0], signal[0, 1] = 0.0, 1000.0
    plain = apt.process(None, signal.ravel(), apt.Contrast.MINMAX, rotate=apt.Rotate.NO)
    drawn = apt.process(None, signal.ravel(), apt.Contrast.MINMAX, rotate=apt.Rotate.NO,
                        orbit=apt.MapOverlay(fit.track, ms, fc.layers()))
    changed = np.any(drawn[:, :, :3] != plain[:, :, None], axis=2)[:, :1040]
    scene_lines = (image != fc.background(h)[:, :, 0])[:, :1040]
    strong = (image.astype(np.int32) - fc.background(h)[:, :, 0] >= 32)[:, :1040]
    assert strong.sum() > 1000 and changed[strong].all()
    # ... and nothing is drawn away from the scene's own lines (a fragment too faint to move the scene's gray may
    # still move the darker one, next to a line pixel)
    near = np.zeros_like(scene_lines)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            near |= np.roll(np.roll(scene_lines, dr, axis=0), dc, axis=1)
    assert not (changed & ~near).any()


def test_sixteen_rows():
    _, start, (s, yaw, hscale, vscale) = fc.SCENES[3]
    track = mm.great_circle_track(*start, 16 + 2 * fc.MARGIN)
    white = {name: (255, 255, 255, 255) for name in ("countries", "lakes")}
    img, _, _ = mm.overlay(fc.background(16), track[fc.MARGIN + s:fc.MARGIN + s + 16], fc.parts(),
                           {"yaw": yaw, "hscale": hscale, "vscale": vscale}, white)
    image = np.ascontiguousarray(img[:, :, 0])
    st = fc.fit_settings(min_points=8, rounds=2)
    fit = gpu(image, track, st)
    assert fit.info.height == 16 and len(fit.rounds) == 2
    masks = fc.check_record_against_model(fit, fm.Problem(image, track, fc.points(), fc.params_of(st)), "h16", "GPU, h = 16")
    check_against_twin(fit, host(image, track, st), masks, "h = 16")


def test_no_margin_shifts_out_of_range_never_win():
    image, long_track, _ = fc.scene(3)
    track = long_track[fc.MARGIN:fc.MARGIN + image.shape[0]]
    st = fc.fit_settings(margin_rows=0, rounds=2)
    fit = gpu(image, track, st)
    assert fit.shift_rows == 0 and all(r.w_shift == 0 for r in fit.rounds)
    for rho in range(2):
        s = fit.scores[rho].reshape(7, 125)
        assert not s["count"][[0, 1, 2, 4, 5, 6]].any() and not s["score"][[0, 1, 2, 4, 5, 6]].any()
    fc.check_record_against_model(fit, fm.Problem(image, track, fc.points(), fc.params_of(st)), "m0", "GPU, M = 0")


def test_constant_image_is_flat_and_keeps_the_initial_settings():
    image, track, _ = fc.scene(3)
    flat = np.full_like(image, 77)
    fit = gpu(flat, track, initial=apt.MapSettings(0.01, 1.02, 0.99))
    twin = host(flat, track, initial=apt.MapSettings(0.01, 1.02, 0.99))
    assert fit.reason == apt.FIT_REASON_FLAT and fit.info.status == 0 and fit.info.n_rounds == 1
    assert fc.final_of(fit) == (0, 0.01, 1.02, 0.99) and (fit.q, fit.count, fit.time_offset_ms) == (-1.0, 0, 0)
    assert not fit.scores["score"].any() and not fit.scores[1:]["count"].any()
    assert fit.rounds[0].index == twin.rounds[0].index == 0


def test_min_points_above_every_count_gives_no_candidate():
    image, track, _ = fc.scene(3)
    with pytest.raises(apt.InternalError, match="APTGPU_FIT_REASON_NO_CANDIDATE") as e:
        gpu(image, track, fc.fit_settings(min_points=100000))
    info = e.value.info
    assert (info.status, info.reason, info.n_rounds, info.height, info.done) == (1, apt.FIT_REASON_NO_CANDIDATE, 1, 120, 1)


def test_channel_b_reads_the_other_half():
    image, track, truth = fc.scene(3)
    moved = np.full_like(image, 120)
    moved[:, 1040:] = image[:, :1040]
    a = gpu(image, track)
    b = gpu(moved, track, fc.fit_settings(channel="B"))
    assert fc.record(a.info) == fc.record(b.info) and a.scores.tobytes() == b.scores.tobytes()
    assert fc.recovered(fc.final_of(b), truth)


def test_a_wide_box_and_many_candidates_per_shift():
    """R_0 = 64: the edge kernel's small tile; 1331 candidates of one shift: more than one LDS pass of 1024, the second
    one partly filled.  (Every tile of points ends mid-wave: the valid points of a shift are no multiple of 64.)"""
    image, track, _ = fc.scene(3)
    st = fc.fit_settings(radius=16, rounds=3, n_shift=0, yaw_step=0.004, n_yaw=5, hscale_step=0.01, n_hscale=5,
                         vscale_step=0.01, n_vscale=5)
    fit = gpu(image, track, st)
    assert fit.info.n_candidates == 1331
    masks = fc.check_record_against_model(fit, fm.Problem(image, track, fc.points(), fc.params_of(st)), "wide", "GPU, R = 64")
    check_against_twin(fit, host(image, track, st), masks, "R = 64")


def test_more_rows_than_the_lds_holds():
    """h = 4104 > 4096: bx is read from global memory; one round of 81 candidates on a noise image"""
    h = 4104
    track = mm.great_circle_track(-58.0, -70.0, 8.0, h + 2 * 2)
    rng = np.random.default_rng(5)
    image = (rng.random((h, 2080)) * 200).astype(np.uint8)
    st = fc.fit_settings(margin_rows=2, shift_step=2, n_shift=1, n_yaw=1, n_hscale=1, n_vscale=1, rounds=1, radius=1)
    fit = gpu(image, track, st)
    prob = fm.Problem(image, track, fc.points(), fc.params_of(st))
    masks = fc.check_record_against_model(fit, prob, "tall", "GPU, h = 4104")
    assert int(fit.scores["count"].max()) > 5000
    check_against_twin(fit, host(image, track, st), masks, "h = 4104")


def test_scales_that_reach_zero_are_invalid():
    image, track, _ = fc.scene(3)
    st = fc.fit_settings(rounds=1, hscale_step=0.5, vscale_step=0.5)
    fit = gpu(image, track, st)
    s = fit.scores[0].reshape(7, 5, 5, 5)
    assert not s["count"][:, :, 0, :].any() and not s["count"][:, :, :, 0].any()
    fc.check_record_against_model(fit, fm.Problem(image, track, fc.points(), fc.params_of(st)), "zero", "GPU, scale 0")


def test_orbit_form_equals_the_track_form():
    ms, h = 1580246771392, 120
    o = orbit(TLE_2020, "NOAA 19", "start", ms)
    long_track = apt.margin_track(o, h, fc.MARGIN)
    white = {name: (255, 255, 255, 255) for name in ("countries", "lakes")}
    img, _, _ = mm.overlay(fc.background(h), long_track[fc.MARGIN + 3:fc.MARGIN + 3 + h], fc.parts(),
                           {"yaw": 0.01, "hscale": 1.02, "vscale": 0.98}, white)
    image = np.ascontiguousarray(img[:, :, 0])
    a = gpu(image, o)
    b = gpu(image, long_track)
    prob = fm.Problem(image, long_track, fc.points(), fc.params_of(fc.fit_settings()))
    # (SGP4 on the device and on the host may differ by ulps: each form against the model from the host's track, under
    # the same contract; the answers agree)
    fc.check_record_against_model(b, prob, "orbit", "GPU, the track form")
    fc.check_record_against_model(a, prob, "orbit", "GPU, the orbit form")
    assert fc.final_of(a) == fc.final_of(b) and a.shift_rows != 0
    assert (a.orbit.ref_time.kind, a.orbit.ref_time.unix_ms) == (apt.RefTime.START, ms + 500 * a.shift_rows)
    assert (a.orbit.draw_map.yaw, a.orbit.draw_map.hscale, a.orbit.draw_map.vscale) == fc.final_of(a)[1:]
    e = gpu(image, orbit(TLE_2020, "NOAA 19", "end", ms + 500 * h), scores=False)
    assert fc.final_of(e) == fc.final_of(a) and e.orbit.ref_time.unix_ms == ms + 500 * h + a.time_offset_ms
    # the moved orbit goes into process() as it is
    signal = fc.background(h)[:, :, 0].astype(np.float32).ravel()
    out = apt.process(None, signal, apt.Contrast.MINMAX, rotate=apt.Rotate.NO, orbit=a.orbit, layers=fc.layers())
    assert out.shape == (h, 2080, 4)


def test_sgp4_failure_is_reported():
    image, _, _ = fc.scene(3)
    tle, ms = decaying_case()  # SGP4 fails from row 300 after ms on: every row of this track
    with pytest.raises(apt.InternalError, match="SGP4") as e:
        gpu(image, orbit(tle, "NOAA 15", "start", ms + 400 * 500))
    assert (e.value.info.status, e.value.info.reason, e.value.info.done) == (1, apt.SAT_REASON_SGP4, 1)
    assert e.value.info.n_rounds == 0


def test_timing_fills_the_record():
    image, track, _ = fc.scene(3)
    fit = gpu(image, track, fc.fit_settings(timing=True), scores=False)
    plain = gpu(image, track, scores=False)
    assert fc.record(fit.info) == fc.record(plain.info)
    assert fit.info.ms_edge > 0 and fit.info.ms_angles > 0 and fit.info.ms_score > 0 and fit.info.ms_pick > 0
    assert (plain.info.ms_edge, plain.info.ms_score) == (0.0, 0.0)
