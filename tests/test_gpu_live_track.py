"""Live flywheel sync on the GPU (include/aptgpu.h §4e): the kernels against np_live_track_model.py on the
oracle's filtered signal after every push, and against the C++ twin push for push — chunkings, ring wraps, the relation
to the one-shot tracker, relocks, the benefit over the picker, the device-resident entry points, reset."""
import numpy as np
import pytest

import live_track_cases as lc
import np_track_model as tm
import stream_cases as sc
import track_cases as tc

import noaa_apt_amd as apt

pytestmark = pytest.mark.gpu
f32 = np.float32


def decoder(rate, profile, track, dtype=f32, max_push=None, host=False, context=None):
    return apt.LiveDecoder(lc.settings_of(profile), apt.Rate.hz(rate), context=context, dtype=dtype, max_push=max_push, host=host,
                           track=track)


def check_same(calls, twin_calls, what):
    assert len(calls) == len(twin_calls), what
    for k, (a, b) in enumerate(zip(calls, twin_calls)):
        assert a[3] == b[3] and a[4] == b[4], (what, k, a[3:], b[3:])
        assert np.array_equal(a[1], b[1]) and np.array_equal(sc.bits(a[2]), sc.bits(b[2])), (what, k)
        assert a[0].shape == b[0].shape and np.array_equal(sc.bits(a[0]), sc.bits(b[0])), (what, k)


def run_both(key, x, rate, profile, chunking, lag=8, w=8, lam=0.1, dtype=f32, max_push=None):
    """the GPU and the twin through the same chunking: the model's output after every push, the same bits per push"""
    g = lc.geometry(rate, profile)
    track = apt.LiveTrackSettings(lag, w, lam)
    what = (key, rate, profile, chunking, lag, w, lam)
    with decoder(rate, profile, track, dtype, max_push) as dec, decoder(rate, profile, track, dtype, max_push, host=True) as tw:
        sizes = sc.chunk_sizes(chunking, x.size, rate, g, dec.info.max_push)
        before = dec.get_info()
        calls, err = lc.run_tracked(dec, x.astype(dtype), sizes)
        assert bytes(before) == bytes(dec.get_info()), what  # info and device_bytes unchanged by pushing
        twin_calls, twin_err = lc.run_tracked(tw, x.astype(dtype), sizes)
        for field in ("cap_in", "cap_f", "cap_corr", "max_push", "l", "m", "pw"):
            assert getattr(before, field) == getattr(tw.info, field), field
    check_same(calls, twin_calls, what)
    assert (err is None) == (twin_err is None) and str(err) == str(twin_err), (what, err, twin_err)
    want, want_error = lc.expected(key, rate, profile, sizes, w, lam, lag)
    out = lc.check_calls(calls, err, want, want_error, sizes, what)
    return out, calls, before


def small(kind, rate, profile, chunking, **kw):
    return run_both((kind, lc.ROWS), lc.recording(kind, rate, profile), rate, profile, chunking, **kw)


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
@pytest.mark.parametrize("chunking", sc.CHUNKINGS)
def test_every_chunking(chunking, oracle):
    """each the model's output, so all the same; "one" is a catch-up push across all twelve checkpoints in one launch
    sequence, "single_samples" crosses checkpoint 5 in one-sample pushes"""
    max_push = 3000 if chunking == "over_max_push" else (1 << 18 if chunking == "one" else None)
    _, calls, info = small("apt_noisy", 11025, "standard", chunking, lag=1, max_push=max_push)
    if chunking == "one":
        assert info.max_push > lc.recording("apt_noisy", 11025, "standard").size and calls[0][4][1] >= 6
    if chunking == "single_samples":
        cps = [c[4][1] for c in calls]
        first = next(k for k, e in enumerate(cps) if e == 6)
        assert 1 <= first <= 2000 and cps[first - 1] == 5


def test_a_small_max_push_wraps_every_ring(oracle):
    x, _, rate, profile = lc.table_case(0)
    _, calls, info = run_both(("table", 0), x, rate, profile, "half_second", lag=8, max_push=2048)
    work_len = calls[-1][3][0]
    assert info.max_push == 2048 and x.size >= 3 * info.cap_in and work_len >= 3 * info.cap_f, (info.cap_in, info.cap_f, work_len)
    with decoder(rate, profile, apt.LiveTrackSettings(8), max_push=2048) as dec:
        t = dec.track_results()
    L = 2080 * info.pw
    assert 2 * L <= t.cap_best and 12 * L <= t.cap_bp and work_len >= 3 * t.cap_best and work_len >= 3 * t.cap_bp, (t.cap_best, t.cap_bp)


# ---------------------------------------------------------------- 3. rule 6
def test_a_lag_of_all_checkpoints_is_the_one_shot_tracker(oracle):
    rate, profile = 11025, "standard"
    (pos, s, rows), calls, _ = small("apt_noisy", rate, profile, "half_second", lag=64)
    assert all(c[0].shape[0] == 0 for c in calls[:-1])
    wpos, wsc, wrows, _ = tm.track(lc.filtered_of("apt_noisy", rate, profile), 3, 8, 0.1)
    tc.check_track((pos, s, rows), (wpos[:rows.shape[0]], wsc[:rows.shape[0]], wrows), "one-shot")
    assert calls[-1][4][2] == wpos.size and calls[-1][4][3] == 0


def test_the_weak_recording_at_a_lag_of_all_checkpoints(oracle):
    x, _, rate, profile = lc.weak_case()
    (pos, s, rows), calls, _ = run_both(("weak",), x, rate, profile, "4096", lag=64)
    assert all(c[0].shape[0] == 0 for c in calls[:-1])
    _, wpos, wsc, wrows = tc.weak_model()
    k = wrows.shape[0]
    tc.check_track((pos, s, rows), (wpos[:k], wsc[:k], wrows), "weak")


# ---------------------------------------------------------------- 4. relocks
def test_relocks_match_the_model(oracle):
    _, calls, _ = small("zeros", 11025, "standard", "half_second", lag=8)
    assert calls[-1][4][3] == 1
    x, _, rate, profile = lc.table_case(5)
    _, calls, _ = run_both(("table", 5), x, rate, profile, "half_second", lag=1)
    assert calls[-1][4][3] == 22


@pytest.mark.parametrize("row,lag", ((2, 8), (3, 16), (5, 8)))
def test_the_noisy_table_recordings_match_the_model(row, lag, oracle):
    """compared to the model (and the twin) only, no threshold: the lag costs accuracy there by design"""
    x, _, rate, profile = lc.table_case(row)
    run_both(("table", row), x, rate, profile, "half_second", lag=lag)


# ---------------------------------------------------------------- 5. the benefit
def test_the_tracker_holds_where_the_picker_does_not(oracle):
    x, _, rate, profile = lc.table_case(4)
    (pos, _, _), calls, _ = run_both(("table", 4), x, rate, profile, "half_second", lag=8)
    err = tc.errors(pos, tc.TABLE[4][1])
    assert pos.size >= 75 and err.max() <= 3.0 and calls[-1][4][3] == 0, (pos.size, err.max())
    with apt.LiveDecoder(sc.settings_of(profile), apt.Rate.hz(rate)) as dec:
        plain, _ = sc.run_stream(dec, x, sc.chunk_sizes("half_second", x.size, rate, lc.geometry(rate, profile)))
    ppos = np.concatenate([c[1] for c in plain]).astype(np.int64)
    assert ppos.size >= 70 and (tc.errors(ppos, tc.TABLE[4][1]) > 3.0).sum() > ppos.size // 2


# ---------------------------------------------------------------- 7. the device-resident form, reset
@pytest.mark.parametrize("rate,profile,lag,max_push,dtype", ((11025, "standard", 1, None, f32), (44100, "fast", 8, 9000, np.int16)))
def test_device_resident_against_the_twin(rate, profile, lag, max_push, dtype, oracle):
    """push_device / finish_device with rows_cap exactly at rows_bound and a sentinel row behind it, one push longer than a
    small max_push (several launch sequences, nothing read back between them): the twin's bits push for push"""
    import torch
    x = lc.recording("apt_noisy", rate, profile).astype(dtype)
    sizes = sc.chunk_sizes("half_second", x.size, rate, lc.geometry(rate, profile))
    sizes = [sizes[0] + sizes[1] + sizes[2]] + sizes[3:]
    track = apt.LiveTrackSettings(lag)
    with decoder(rate, profile, track, dtype, max_push, host=True) as tw:
        want, want_err = lc.run_tracked(tw, x, sizes)
    assert want_err is None
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    calls = []
    with torch.cuda.stream(stream):
        d_x = torch.from_numpy(x.copy()).to(dev)
        with decoder(rate, profile, track, dtype, max_push, context=apt.Context(device=0, stream=stream.cuda_stream)) as dec:
            if max_push:
                assert sizes[0] > dec.info.max_push
            with pytest.raises(apt.InvalidError, match="rows_cap"):
                dec.push_device(d_x.data_ptr(), 16, d_x.data_ptr(), d_x.data_ptr(), dec.rows_bound(16) - 1)
            at = 0
            for c in sizes + [None]:
                cap = dec.rows_bound(c or 0)
                d_rows = torch.full(((cap + 1) * 2080,), -7.0, dtype=torch.float32, device=dev)
                d_pos = torch.full((cap + 1,), -1, dtype=torch.int64, device=dev)
                d_sc = torch.full((cap + 1,), -7.0, dtype=torch.float32, device=dev)
                stream.synchronize()
                dec.scores_device(d_sc.data_ptr())
                if c is None:
                    dec.finish_device(d_rows.data_ptr(), d_pos.data_ptr(), cap)
                else:
                    dec.push_device(d_x.data_ptr() + at * x.itemsize, c, d_rows.data_ptr(), d_pos.data_ptr(), cap)
                    at += c
                r, t = dec.results(), dec.track_results()
                k = int(r.n_rows)
                rows, pos, s = d_rows.cpu().numpy().reshape(-1, 2080), d_pos.cpu().numpy(), d_sc.cpu().numpy()
                assert (rows[k:] == -7.0).all() and (pos[k:] == -1).all() and (s[k:] == -7.0).all()
                calls.append((rows[:k].copy(), pos[:k].astype(np.uint64), s[:k].copy(),
                              (int(r.work_len), int(r.scan_pos), k, int(r.n_sync), int(r.n_in), int(r.rows_total)),
                              (int(t.m), int(t.next_checkpoint), int(t.n_positions), int(t.n_relocks),
                               int(t.last_position) if t.has_position else None)))
    check_same(calls, want, (rate, profile, lag, "device"))


def test_reset_reproduces_the_output(oracle):
    rate, profile = 11025, "standard"
    x = lc.recording("apt_noisy", rate, profile)
    sizes = sc.chunk_sizes("4096", x.size, rate, lc.geometry(rate, profile))
    want, _ = lc.expected(("apt_noisy", lc.ROWS), rate, profile, sizes, lag=1)
    with decoder(rate, profile, apt.LiveTrackSettings(1)) as dec:
        dec.push(x[:30000])
        dec.reset()
        first, err = lc.run_tracked(dec, x, sizes)
        with pytest.raises(apt.InvalidError, match="finished"):
            dec.push(x[:10])
        dec.reset()
        again, err2 = lc.run_tracked(dec, x, sizes)
    assert err is None and err2 is None
    check_same(first, again, "reset")
    lc.check_calls(again, err2, want, None, sizes, "after reset")


def test_too_short_for_the_tracker(oracle):
    rate, profile = 11025, "standard"
    x = lc.recording("apt_noisy", rate, profile)[:5000]
    with decoder(rate, profile, apt.LiveTrackSettings(8)) as dec:
        assert dec.push(x)[0].shape[0] == 0
        with pytest.raises(apt.InternalError, match="track: the signal is shorter than one row and one sync frame"):
            dec.finish()
        assert dec.result.n_rows == 0 and dec.result.status == 1


# ---------------------------------------------------------------- 6. from IQ
def test_tracked_live_iq_decoder_equals_a_tracked_live_decoder_fed_the_one_shot_audio():
    import fm_stream_cases as fsc
    rec = fsc.live_recording()
    audio, _ = apt.fm_demodulate(rec.iq, rec.settings)
    track = apt.LiveTrackSettings(2)
    with apt.LiveIqDecoder(apt.Settings(), rec.settings, track=track) as live, \
            apt.LiveDecoder(apt.Settings(), apt.Rate.hz(48000), track=track) as dec:
        rows, trk = lc.iq_against_decoder(live, dec, audio, rec, fsc.live_sizes("quarter_second", rec.n))
    assert rows.shape[0] >= 13 and trk[2] >= rows.shape[0]


def test_tracked_live_iq_decoder_device_resident():
    """push_device / finish_device of the coupling with rows_cap at the bound and a sentinel behind rows, positions and
    lock indicators: the host-fed form's bits"""
    import fm_stream_cases as fsc
    import torch
    rec = fsc.live_recording()
    track = apt.LiveTrackSettings(2)
    sizes = [rec.n // 3, rec.n - rec.n // 3]
    want = []
    with apt.LiveIqDecoder(apt.Settings(), rec.settings, track=track) as fed:
        p = 0
        for k in sizes + [None]:
            r, q = fed.finish() if k is None else fed.push(rec.iq[2 * p:2 * (p + k)])
            p += k or 0
            want.append((r, q, fed.scores, lc.track_record_of(fed.track_result)))
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        d_iq = torch.from_numpy(rec.iq.copy()).to(dev)
        with apt.LiveIqDecoder(apt.Settings(), rec.settings, track=track, context=apt.Context(device=0, stream=stream.cuda_stream)) as live:
            p = 0
            for k, (wr, wq, ws, wt) in zip(sizes + [None], want):
                cap = live.rows_bound(k or 0)
                d_rows = torch.full(((cap + 1) * 2080,), -7.0, dtype=torch.float32, device=dev)
                d_pos = torch.full((cap + 1,), -1, dtype=torch.int64, device=dev)
                d_sc = torch.full((cap + 1,), -7.0, dtype=torch.float32, device=dev)
                stream.synchronize()
                live.scores_device(d_sc.data_ptr())
                if k is None:
                    live.finish_device(d_rows.data_ptr(), d_pos.data_ptr(), cap)
                else:
                    live.push_device(d_iq.data_ptr() + 2 * p * rec.iq.itemsize, k, d_rows.data_ptr(), d_pos.data_ptr(), cap)
                    p += k
                n = int(live.results().n_rows)
                rows, pos, sc_ = d_rows.cpu().numpy().reshape(-1, 2080), d_pos.cpu().numpy(), d_sc.cpu().numpy()
                assert (rows[n:] == -7.0).all() and (pos[n:] == -1).all() and (sc_[n:] == -7.0).all()
                assert rows[:n].tobytes() == wr.tobytes() and pos[:n].tolist() == wq.tolist() and sc_[:n].tobytes() == ws.tobytes()
                assert lc.track_record_of(live.track_results()) == wt
