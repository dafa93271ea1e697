"""Live flywheel sync without a GPU (include/aptgpu.h §4e): the C++ twin
(aptgpu_stream_create_tracked_host) against np_live_track_model.py on the oracle's filtered signal after every push,
chunking invariance, the relation to the one-shot tracker, relocks, the benefit over the picker, reset, bounded state
and every refusal — on the GPU form too, which refuses before it touches a device."""
import ctypes as C

import numpy as np
import pytest

import live_track_cases as lc
import np_track_model as tm
import stream_cases as sc
import track_cases as tc

import noaa_apt_amd as apt
from noaa_apt_amd import api

f32 = np.float32


def twin(rate, profile, track, dtype=f32, max_push=None):
    return apt.LiveDecoder(lc.settings_of(profile), apt.Rate.hz(rate), dtype=dtype, max_push=max_push, host=True, track=track)


def run_case(key, x, rate, profile, chunking, lag=8, w=8, lam=0.1, dtype=f32, max_push=None, sizes=None):
    g = lc.geometry(rate, profile)
    with twin(rate, profile, apt.LiveTrackSettings(lag, w, lam), dtype, max_push) as dec:
        if sizes is None:
            sizes = sc.chunk_sizes(chunking, x.size, rate, g, dec.info.max_push)
        before = dec.get_info()
        calls, err = lc.run_tracked(dec, x.astype(dtype), sizes)
        after = dec.get_info()
    want, want_error = lc.expected(key, rate, profile, sizes, w, lam, lag)
    what = (key, rate, profile, chunking, lag, w, lam)
    out = lc.check_calls(calls, err, want, want_error, sizes, what)
    assert bytes(before) == bytes(after), what  # bounded state: nothing depends on how much was pushed
    return out, calls, before


def small(kind, rate, profile, chunking, **kw):
    return run_case((kind, lc.ROWS), lc.recording(kind, rate, profile), rate, profile, chunking, **kw)


# ---------------------------------------------------------------- 1. bits and schedule
@pytest.mark.parametrize("lag", lc.LAGS)
@pytest.mark.parametrize("kind", lc.KINDS)
def test_every_signal_and_lag_matches_the_model_after_every_push(kind, lag, oracle):
    small(kind, 11025, "standard", "half_second", lag=lag)


@pytest.mark.parametrize("rate,profile", lc.RATES)
def test_every_pixel_width(rate, profile, oracle):
    small("apt_noisy", rate, profile, "random")
    small("nonfinite", rate, profile, "half_second", lag=1)


@pytest.mark.parametrize("w,lam", lc.SETTINGS)
def test_the_track_settings(w, lam, oracle):
    small("apt_noisy", 11025, "standard", "4096", w=w, lam=lam)
    small("zeros", 11025, "standard", "4096", w=w, lam=lam, lag=1)


def test_s16_samples_track_like_their_f32_values(oracle):
    (pos, s, rows), _, _ = small("apt_noisy", 11025, "standard", "4096", dtype=np.int16)
    (pos_f, s_f, rows_f), _, _ = small("apt_noisy", 11025, "standard", "4096")
    assert np.array_equal(pos, pos_f) and np.array_equal(sc.bits(s), sc.bits(s_f)) and np.array_equal(sc.bits(rows), sc.bits(rows_f))


# ---------------------------------------------------------------- 2. chunk invariance
@pytest.mark.parametrize("lag", (1, 8))
def test_every_chunking_gives_the_same_output(lag, oracle):
    """... each of them the model's; "one" is a catch-up push that crosses all twelve checkpoints in one launch sequence"""
    outs = []
    for chunking in sc.CHUNKINGS:
        max_push = 3000 if chunking == "over_max_push" else (1 << 18 if chunking == "one" else None)
        out, calls, info = small("apt_noisy", 11025, "standard", chunking, lag=lag, max_push=max_push)
        if chunking == "one":
            assert info.max_push > lc.recording("apt_noisy", 11025, "standard").size and calls[0][4][1] >= 6
        outs.append(out)
    for pos, s, rows in outs[1:]:
        assert np.array_equal(pos, outs[0][0]) and np.array_equal(sc.bits(s), sc.bits(outs[0][1]))
        assert np.array_equal(sc.bits(rows), sc.bits(outs[0][2]))


def test_one_sample_pushes_across_a_checkpoint(oracle):
    """stream_cases' single_samples surround the input sample at which row 5 of the work signal ends: checkpoint 5 falls
    38 pw work samples later, inside the 2 000 one-sample pushes"""
    rate, profile = 11025, "standard"
    _, calls, _ = small("apt_noisy", rate, profile, "single_samples", lag=1)
    cps = [c[4][1] for c in calls]
    first = next(k for k, e in enumerate(cps) if e == 6)
    assert 1 <= first <= 2000 and cps[first - 1] == 5


def test_a_small_max_push_wraps_every_ring(oracle):
    """a 40 s recording through max_push = 2 048: the input ring, the F and score rings (one capacity, the info's cap_f),
    the sums' ring and the back-pointers' (the tracker's record lists both) wrap at least three times"""
    x, _, rate, profile = lc.table_case(0)
    (pos, _, _), calls, info = run_case(("table", 0), x, rate, profile, "half_second", lag=8, max_push=2048)
    work_len = calls[-1][3][0]
    assert info.max_push == 2048 and x.size >= 3 * info.cap_in and work_len >= 3 * info.cap_f, (info.cap_in, info.cap_f, work_len)
    assert info.cap_corr == 0
    with twin(rate, profile, apt.LiveTrackSettings(8), max_push=2048) as dec:
        t = dec.track_results()
    L = 2080 * info.pw
    assert 2 * L <= t.cap_best and 12 * L <= t.cap_bp and work_len >= 3 * t.cap_best and work_len >= 3 * t.cap_bp, (t.cap_best, t.cap_bp)
    (pos_d, _, _), _, _ = run_case(("table", 0), x, rate, profile, "half_second", lag=8)
    assert np.array_equal(pos, pos_d)


# ---------------------------------------------------------------- 3. rule 6
def test_a_lag_of_all_checkpoints_is_the_one_shot_tracker(oracle):
    rate, profile = 11025, "standard"
    (pos, s, rows), calls, _ = small("apt_noisy", rate, profile, "half_second", lag=64)
    assert all(c[0].shape[0] == 0 for c in calls[:-1])  # nothing before finish()
    f = lc.filtered_of("apt_noisy", rate, profile)
    wpos, wsc, wrows, _ = tm.track(f, 3, 8, 0.1)
    tc.check_track((pos, s, rows), (wpos[:rows.shape[0]], wsc[:rows.shape[0]], wrows), "one-shot")
    assert calls[-1][4][2] == wpos.size and calls[-1][4][3] == 0


def test_the_weak_recording_at_a_lag_of_all_checkpoints(oracle):
    x, f, rate, profile = lc.weak_case()
    (pos, s, rows), calls, _ = run_case(("weak",), x, rate, profile, "4096", lag=64)
    assert all(c[0].shape[0] == 0 for c in calls[:-1])
    _, wpos, wsc, wrows = tc.weak_model()
    k = wrows.shape[0]
    tc.check_track((pos, s, rows), (wpos[:k], wsc[:k], wrows), "weak")
    assert calls[-1][4][2] == wpos.size == 12


# ---------------------------------------------------------------- 4. relocks
@pytest.mark.parametrize("lag", (1, 8))
def test_silence_relocks_at_finish(lag, oracle):
    _, calls, _ = small("zeros", 11025, "standard", "half_second", lag=lag)
    assert calls[-1][4][3] == 1 and calls[-2][4][3] == 0  # (the model's count, matched above: one relock, in finish())


def test_a_greedy_tracker_in_heavy_noise_relocks_often(oracle):
    x, _, rate, profile = lc.table_case(5)
    _, calls, _ = run_case(("table", 5), x, rate, profile, "half_second", lag=1)
    assert calls[-1][4][3] == 22


@pytest.mark.parametrize("lag", (8, 16))
@pytest.mark.parametrize("row", (2, 3, 5))
def test_the_noisy_table_recordings_match_the_model(row, lag, oracle):
    """DESIGN.md §24's table: compared to the model only, no threshold (the lag costs accuracy there by design); the
    figures the table records are printed"""
    x, _, rate, profile = lc.table_case(row)
    (pos, _, _), calls, _ = run_case(("table", row), x, rate, profile, "half_second", lag=lag)
    err = tc.errors(pos, tc.TABLE[row][1])
    same = np.intersect1d(pos, tc.model_table(row)[0]).size
    print(f"table {row} lag {lag}: {pos.size} released, {same} same as the one-shot, {calls[-1][4][3]} relocks, "
          f"{int((err > 3).sum())} off (max {err.max():.1f})")


# ---------------------------------------------------------------- 5. the benefit
def test_the_tracker_holds_where_the_picker_does_not(oracle):
    """sigma 20 000 and a 4 s dropout (§21's table, recording 4) at the default lag"""
    x, _, rate, profile = lc.table_case(4)
    (pos, _, rows), calls, _ = run_case(("table", 4), x, rate, profile, "half_second", lag=8)
    err = tc.errors(pos, tc.TABLE[4][1])
    assert pos.size >= 75 and err.max() <= 3.0 and calls[-1][4][3] == 0, (pos.size, err.max())
    with apt.LiveDecoder(sc.settings_of(profile), apt.Rate.hz(rate), host=True) as dec:
        plain, _ = sc.run_stream(dec, x, sc.chunk_sizes("half_second", x.size, rate, lc.geometry(rate, profile)))
    ppos = np.concatenate([c[1] for c in plain]).astype(np.int64)
    assert ppos.size >= 70 and (tc.errors(ppos, tc.TABLE[4][1]) > 3.0).sum() > ppos.size // 2


# ---------------------------------------------------------------- 7. reset, the bound, refusals
def test_reset_starts_over(oracle):
    rate, profile = 11025, "standard"
    x = lc.recording("apt_noisy", rate, profile)
    sizes = sc.chunk_sizes("half_second", x.size, rate, lc.geometry(rate, profile))
    want, _ = lc.expected(("apt_noisy", lc.ROWS), rate, profile, sizes, lag=1)
    with twin(rate, profile, apt.LiveTrackSettings(1)) as dec:
        dec.push(x[:30000])
        dec.reset()
        calls, err = lc.run_tracked(dec, x, sizes)
        lc.check_calls(calls, err, want, None, sizes, "after reset")
        with pytest.raises(apt.InvalidError, match="finished"):
            dec.push(x[:10])
        dec.reset()
        calls, err = lc.run_tracked(dec, x, sizes)
        lc.check_calls(calls, err, want, None, sizes, "after finish and reset")


def test_rows_cap_below_the_bound_is_refused_and_the_bound_holds(oracle):
    rate, profile = 11025, "standard"
    x = lc.recording("apt_noisy", rate, profile)
    with twin(rate, profile, apt.LiveTrackSettings(0)) as dec:
        b = dec.rows_bound(x.size)
        assert 12 <= b <= 3 * 12 + 8
        with pytest.raises(apt.InvalidError, match="rows_cap"):
            dec.push(x, rows_cap=b - 1)
        rows, _ = dec.push(x, rows_cap=b)
        assert rows.shape[0] == 11
        # (the twelfth position has no full row behind it: committed by finish(), not released)
        assert dec.finish(rows_cap=dec.rows_bound(0))[0].shape[0] == 0 and dec.track_result.n_positions == 12


def test_too_short_for_the_tracker(oracle):
    rate, profile = 11025, "standard"
    x = lc.recording("apt_noisy", rate, profile)[:5000]
    with twin(rate, profile, apt.LiveTrackSettings(8)) as dec:
        assert dec.push(x)[0].shape[0] == 0
        with pytest.raises(apt.InternalError, match="track: the signal is shorter than one row and one sync frame"):
            dec.finish()
        assert dec.result.n_rows == 0 and dec.result.status == 1


@pytest.mark.parametrize("host", (True, False))
def test_refusals_come_before_any_device(host):
    """(this machine may have no GPU: a refusal that touched one would be a HipError)"""
    st, rate = lc.settings_of("standard"), apt.Rate.hz(11025)

    def refused(track, settings=st, match=None):
        with pytest.raises(apt.InvalidError, match=match):
            apt.LiveDecoder(settings, rate, host=host, track=track)

    refused(apt.LiveTrackSettings(65), match="lag_rows")
    refused(apt.LiveTrackSettings(8)._c(struct_size=8), match="struct_size")
    refused(apt.LiveTrackSettings(8)._c(struct_size=0), match="struct_size")
    refused(apt.LiveTrackSettings(8, 65), match="max_jitter")
    refused(apt.LiveTrackSettings(8, 8, -0.5), match="penalty")
    refused(apt.LiveTrackSettings(8, 8, float("nan")), match="penalty")
    refused("lag 8", match="LiveTrackSettings")
    wide = lc.settings_of("standard")
    wide.work_rate = 9 * 4160  # a work rate the tracker does not serve (pw 9)
    refused(apt.LiveTrackSettings(8), settings=wide, match="work_rate")
    # what the plain stream refuses stays refused, with its own class
    with pytest.raises(apt.UnsupportedError):
        apt.LiveDecoder(st, rate, host=host, track=apt.LiveTrackSettings(8), context=apt.Context(mode=apt.MODE_FAST))


def test_the_track_entry_points_refuse_a_plain_stream():
    with apt.LiveDecoder(lc.settings_of("standard"), apt.Rate.hz(11025), host=True) as dec:
        with pytest.raises(apt.InvalidError, match="not a tracked stream"):
            dec.track_results()
        assert dec.scores is None and not dec.tracked
    with twin(11025, "standard", apt.LiveTrackSettings(8)) as dec:
        res = api.StreamTrackResult(struct_size=8)
        err = C.create_string_buffer(256)
        assert apt.lib().aptgpu_stream_track_results(dec._p, C.byref(res), err, 256) == 4 and b"struct_size" in err.value
        with pytest.raises(apt.InvalidError, match="host handle"):
            dec.scores_device(None)


def test_decode_live_with_a_tracker(oracle):
    rate, profile = 11025, "standard"
    x = lc.recording("apt_noisy", rate, profile)
    rows, pos, s, info = apt.decode_live(None, lc.settings_of(profile), np.array_split(x, 9), apt.Rate.hz(rate), True, host=True,
                                         track=apt.LiveTrackSettings(8), return_info=True)
    (wpos, wsc, wrows), _, _ = small("apt_noisy", rate, profile, "one")
    assert np.array_equal(pos.astype(np.int64), wpos) and np.array_equal(sc.bits(s), sc.bits(wsc))
    assert np.array_equal(sc.bits(rows), sc.bits(wrows.reshape(-1))) and info.n_positions == 12


# ---------------------------------------------------------------- 6. from IQ
@pytest.mark.parametrize("chunking", ("quarter_second", "one"))
def test_tracked_live_iq_decoder_equals_a_tracked_live_decoder_fed_the_one_shot_audio(chunking):
    import fm_stream_cases as fsc
    rec = fsc.live_recording()
    audio, _ = apt.fm_demodulate_host(rec.iq, rec.settings)
    track = apt.LiveTrackSettings(2)
    with apt.LiveIqDecoder(apt.Settings(), rec.settings, host=True, track=track) as live, \
            apt.LiveDecoder(apt.Settings(), apt.Rate.hz(48000), host=True, track=track) as dec:
        rows, trk = lc.iq_against_decoder(live, dec, audio, rec, fsc.live_sizes(chunking, rec.n))
    assert rows.shape[0] >= 13 and trk[2] >= rows.shape[0]
    sizes = fsc.live_sizes("quarter_second", rec.n)
    edges = np.concatenate([[0], np.cumsum(sizes)])
    chunks = (rec.iq[2 * a:2 * b] for a, b in zip(edges[:-1], edges[1:]))
    got = apt.decode_live_iq(None, apt.Settings(), rec.settings, chunks, True, host=True, track=track, return_info=True)
    assert got[0].tobytes() == rows.reshape(-1).tobytes() and got[1].size == rows.shape[0] == got[2].size
    assert lc.track_record_of(got[3]) == trk


@pytest.mark.parametrize("host", (True, False))
def test_tracked_live_iq_refusals_come_before_any_device(host):
    import fm_stream_cases as fsc
    rec = fsc.live_recording()
    for track, match in ((apt.LiveTrackSettings(65), "lag_rows"), (apt.LiveTrackSettings(8)._c(struct_size=4), "struct_size"),
                         (apt.LiveTrackSettings(8, 65), "max_jitter")):
        with pytest.raises(apt.InvalidError, match=match):
            apt.LiveIqDecoder(apt.Settings(), rec.settings, host=host, track=track)
    with apt.LiveIqDecoder(apt.Settings(), rec.settings, host=True) as live:
        with pytest.raises(apt.InvalidError, match="not a tracked stream"):
            live.track_results()
