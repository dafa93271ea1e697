"""The flywheel sync stage without a GPU (include/aptgpu.h §4c): the C++ twin (track_sync_host) against
the numpy model of np_track_model.py bit for bit, the tie rules on silence, the power-of-two gain, the path's
invariants, every refusal — on the GPU entry points too, which refuse before they touch a device — and what the stage
is for: the noisy recordings of the table in §21, on which the reference's picker loses the rows and the tracker does
not.  (The definition's refusal "4 w >= L" cannot be reached through the ABI: w <= 64 and pw >= 1 imply 4 w < L.)"""
import ctypes as C

import numpy as np
import pytest

import np_track_model as tm
import track_cases as tc

import noaa_apt_amd as apt
from noaa_apt_amd import api

f32 = np.float32


def rate_of(pw):
    return apt.Rate.hz(4160 * pw)


SMALL = [(pw, n) for pw in tc.PWS for n in tc.lengths(pw)]


# ---------------------------------------------------------------- the model alone
def test_model_template_is_generate_sync_frame():
    for pw in tc.PWS:
        frame = apt.generate_sync_frame(rate_of(pw))
        assert np.array_equal(frame > 0, tm.template_plus(pw))
        assert int((frame > 0).sum()) == 14 * pw and frame.size == 38 * pw


def test_model_score_of_a_clean_frame_is_one():
    pw = 3
    x = np.full(4 * 2080 * pw, 100.0, f32)
    g = np.where(tm.template_plus(pw), 900.0, 100.0).astype(f32)
    x[5000:5000 + g.size] = g
    s = tm.score(x, pw)
    assert int(np.argmax(s)) == 5000 and abs(float(s[5000]) - 1.0) < 1e-5
    assert s[0] == 0.0  # a constant window: no evidence


# ---------------------------------------------------------------- the twin, bit for bit
@pytest.mark.parametrize("kind", tc.KINDS)
@pytest.mark.parametrize("pw,n", SMALL)
def test_twin_score_bits(pw, n, kind):
    x = tc.signal(kind, pw, n)
    got = apt.track_sync_host(x, rate_of(pw), rows=False, return_score=True)[3]
    want = tc.model_score(kind, pw, n)
    assert got.size == n - 38 * pw
    assert np.array_equal(tc.bits(got), tc.bits(want))
    if kind in ("zeros", "constant"):
        assert not got.any()
    if kind == "nonfinite":  # every window that holds the NaN or the Inf scores 0
        for at in (n // 3, n // 2 + 7):
            lo, hi = max(0, at - 38 * pw + 1), min(got.size, at + 1)
            assert not got[lo:hi].any()


@pytest.mark.parametrize("w,lam", tc.SETTINGS)
@pytest.mark.parametrize("kind", tc.KINDS)
@pytest.mark.parametrize("pw,n", SMALL)
def test_twin_track(pw, n, kind, w, lam):
    x = tc.signal(kind, pw, n)
    got = apt.track_sync_host(x, rate_of(pw), apt.TrackSettings(w, lam), return_info=True)
    tc.check_track(got, tc.model_track(kind, pw, n, w, lam), (pw, n, kind, w, lam))
    tc.check_invariants(got[0], pw, n, w, (pw, n, kind, w, lam))
    info = got[3]
    L = 2080 * pw
    assert info.status == 0 and info.n_positions == got[0].size and info.n == n and info.end == got[0][-1]
    assert info.n_rows == int((got[0].astype(np.int64) + L <= n).sum()) == got[2].shape[0]


@pytest.mark.parametrize("pw", tc.PWS)
def test_silence_exercises_every_tie_rule(pw):
    L = 2080 * pw
    n = 3 * L + 38 * pw + 17
    for w, lam in tc.SETTINGS:
        pos, sc, rows = apt.track_sync_host(np.zeros(n, f32), rate_of(pw), apt.TrackSettings(w, lam))
        assert pos.tolist() == [17, 17 + L, 17 + 2 * L], (pw, w, lam, pos)
        assert not sc.any() and rows.shape == (3, 2080) and not rows.any()


@pytest.mark.parametrize("gain", (10, -10))
@pytest.mark.parametrize("pw", tc.PWS)
def test_power_of_two_gain(pw, gain):
    n = tc.lengths(pw)[2]
    x = tc.scaled("noise", pw, n, gain)
    pos, sc, rows, s = apt.track_sync_host(x, rate_of(pw), apt.TrackSettings(8, 0.1), return_score=True)
    assert np.array_equal(tc.bits(s), tc.bits(tc.model_score("noise", pw, n)))  # the unscaled signal's bits
    assert np.array_equal(tc.bits(s), tc.bits(tc.model_score("noise", pw, n, gain)))
    want = tc.model_track("noise", pw, n, 8, 0.1)
    assert np.array_equal(pos.astype(np.int64), want[0]) and np.array_equal(tc.bits(sc), tc.bits(want[1]))
    assert np.array_equal(tc.bits(rows), tc.bits(tc.model_track("noise", pw, n, 8, 0.1, gain)[2]))


def test_default_settings_are_8_and_a_tenth():
    pw, n = 3, tc.lengths(3)[2]
    x = tc.signal("noise", pw, n)
    tc.check_track(apt.track_sync_host(x, rate_of(pw)), tc.model_track("noise", pw, n, 8, 0.1), "defaults")


# ---------------------------------------------------------------- refusals
def _refused(call, text):
    with pytest.raises(apt.InvalidError) as e:
        call()
    assert text in str(e.value), str(e.value)


ENTRY_POINTS = {
    "host": lambda x, rate, st: apt.track_sync_host(x, rate, st),
    "gpu": lambda x, rate, st: apt.track_sync(x, rate, st),
    "gpu-list": lambda x, rate, st: apt.track_sync([x, x], rate, st),
}


@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_refusals(entry):
    """every one is APTGPU_ERR_INVALID before a device is touched: the GPU forms refuse on a machine without one"""
    call = ENTRY_POINTS[entry]
    x = tc.signal("noise", 3, tc.lengths(3)[0])
    r3 = rate_of(3)
    _refused(lambda: call(x[:-1], r3, None), "shorter than one row")
    _refused(lambda: call(x, apt.Rate.hz(12481), None), "multiple of 4160")
    _refused(lambda: call(x, apt.Rate.hz(0), None), "multiple of 4160")
    _refused(lambda: call(x, apt.Rate.hz(4160 * 9), None), "1..8")
    _refused(lambda: call(x, r3, apt.TrackSettings(65, 0.1)), "max_jitter")
    _refused(lambda: call(x, r3, apt.TrackSettings(8, -0.1)), "penalty")
    _refused(lambda: call(x, r3, apt.TrackSettings(8, float("nan"))), "penalty")
    _refused(lambda: call(x, r3, apt.TrackSettings(8, float("inf"))), "penalty")
    _refused(lambda: call(x, r3, apt.TrackSettings(8, 0.1)._c(struct_size=8)), "struct_size")
    _refused(lambda: call(x, r3, "8"), "TrackSettings")


def test_refusals_of_the_other_forms():
    x = tc.signal("noise", 3, tc.lengths(3)[0])
    _refused(lambda: apt.sync_score(x[:-1], rate_of(3)), "shorter than one row")
    _refused(lambda: apt.sync_score(x, apt.Rate.hz(4160 * 9)), "1..8")
    _refused(lambda: apt.track_sync_host(x, rate_of(3), result_struct_size=8), "aptgpu_track_result")
    st = apt.Settings.profile("standard")
    _refused(lambda: apt.decode_tracked(None, st, x, apt.Rate.hz(11025), apt.TrackSettings(65, 0.1)), "max_jitter")
    odd = apt.Settings.profile("standard")
    odd.work_rate = 12481
    _refused(lambda: apt.decode_tracked(None, odd, x, apt.Rate.hz(11025)), "multiple of 4160")


def test_abi_version_and_struct_sizes():
    assert apt.abi_version() == 2
    assert C.sizeof(api._CTrackSettings) == 16 and C.sizeof(apt.TrackResult) == 40


# ---------------------------------------------------------------- what the stage is for
@pytest.mark.parametrize("row", range(len(tc.TABLE)))
def test_tracker_holds_on_the_noisy_recordings(row, oracle):
    """Rows 1, 2 and 5 of the table (ppm = 0): every tracked position within pw = 3 work samples of truth (measured
    0.5; one pixel is the margin).  Rows 3, 4 and 6 (slanted): within 8 (measured at most 6.8)."""
    sigma, ppm, dropout, bound = tc.TABLE[row]
    f = tc.filtered(row)
    pos, sc, rows = apt.track_sync_host(f, apt.Rate.hz(tc.WORK_RATE), apt.TrackSettings(8, 0.1))
    tc.check_track((pos, sc, rows), tc.model_table(row), f"table row {row + 1}")
    tc.check_invariants(pos, tc.PW, f.size, 8, f"table row {row + 1}")
    err = tc.errors(pos, ppm)
    print(f"table row {row + 1}: sigma {sigma:g} ppm {ppm:g} dropout {dropout}: {pos.size} positions, "
          f"max error {err.max():.2f}, off by > 3: {(err > 3).sum()}, median score {np.median(sc):.3f}")
    assert err.max() <= bound, (row, err.max())


def test_reference_picker_loses_the_rows_the_tracker_keeps(oracle):
    """On row 5 (sigma 20 000, dropout) the reference's own positions have more than half their rows beyond 1000."""
    f = tc.filtered(4)
    ref = oracle.find_sync(f, tc.WORK_RATE)
    err = tc.errors(ref, 0.0)
    print(f"reference picker on row 5: {ref.size} positions, {(err > 1000).sum()} beyond 1000, max {err.max():.0f}")
    assert (err > 1000).sum() * 2 > ref.size
    assert tc.errors(tc.model_table(4)[0], 0.0).max() <= 3.0


def test_oracle_refuses_the_weak_recording_and_the_tracker_keeps_its_rows(oracle):
    """the recording of test_gpu_track.py's decode_tracked test: the reference finds less than five frames on it"""
    with pytest.raises(oracle.OracleError, match="less than 5 sync frames"):
        oracle.decode(tc.weak_recording(), tc.RATE, True)
    f, pos, sc, rows = tc.weak_model()
    assert oracle.find_sync(f, tc.WORK_RATE).size < 5
    got = apt.track_sync_host(f, apt.Rate.hz(tc.WORK_RATE))
    tc.check_track(got, (pos, sc, rows), "weak recording")
    assert rows.shape[0] >= 10 and (sc[:3] > 0.8).all() and (np.diff(pos[:3]) == 6240).all()
