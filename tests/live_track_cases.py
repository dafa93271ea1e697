"""Cases the live flywheel sync tests share (test_live_track_cpu.py, test_gpu_live_track.py): small recordings, the
oracle's filtered signal of each (computed once, read-only), the model's expectation per push (np_live_track_model.py on
that signal plus the chunk boundaries — never the code under test) and the comparison after every push."""
import functools

import numpy as np

import np_live_track_model as lm
import np_stream_model as sm
import stream_cases as sc
import track_cases as tc

import noaa_apt_amd as apt
from noaa_apt_amd.testing.synth import synth_apt

f32 = np.float32
# (input rate, profile): pw 1 (the smallest pixel width the stream front end serves: the standard profile at a work
# rate of 4160 Hz), pw 3 (11 025 Hz, standard) and pw 4 through another resampler
RATES = ((11025, "pw1"), (11025, "standard"), (44100, "fast"))
KINDS = ("apt_noisy", "zeros", "constant", "nonfinite")
LAGS = (0, 1, 8, 64)
# track_cases.SETTINGS, all of which the ABI admits at these pixel widths (4 w < L)
SETTINGS = tc.SETTINGS
ROWS = 12


def work_rate(profile):
    return 4160 if profile == "pw1" else sc.PROFILE_RATES[profile]


def oracle_settings(profile):
    if profile == "pw1":
        return dict(sc.oracle_settings("standard"), work_rate=4160)
    return sc.oracle_settings(profile)


def settings_of(profile):
    if profile == "pw1":
        st = sc.settings_of("standard")
        st.work_rate = 4160
        return st
    return sc.settings_of(profile)


@functools.lru_cache(maxsize=None)
def geometry(rate, profile):
    """stream_cases.geometry, for the pw 1 settings as well (the tap counts are the oracle's own)"""
    if profile != "pw1":
        return sc.geometry(rate, profile)
    from oracle import binding as oracle
    _, steps = oracle.decode(synth_apt(rate, 5.5, 3), rate, False, settings=oracle_settings(profile), want_steps=True)
    return sm.Geometry(rate, 4160, steps["resample_filter"].size, steps["filter_filter"].size)


def work_target(rate, profile, rows=ROWS):
    g = geometry(rate, profile)
    return rows * g.spr + g.G + 17  # track_cases.lengths' shape: whole rows, a sync frame and a few samples


@functools.lru_cache(maxsize=None)
def recording(kind, rate, profile, rows=ROWS):
    """audio whose finished work signal is the shortest one of at least rows L + G + 17 samples"""
    g = geometry(rate, profile)
    n = g.samples_for(work_target(rate, profile, rows))
    if kind == "zeros":
        x = np.zeros(n, f32)
    elif kind == "constant":
        x = np.full(n, 1234.0, f32)
    else:
        # a pass with its sync frames under noise: the scores are not all alike, and some rows are weak
        x = synth_apt(rate, n / rate + 0.01, 23, noise_sigma=6000.0, start_px=450.0)[:n].copy()
        x = np.rint(x).astype(f32)  # (whole numbers, so that the s16 form is the same signal)
        np.clip(x, -32768, 32767, out=x)
        if kind == "nonfinite":
            x[n // 3] = np.nan
            x[n // 2 + 7] = np.inf
    assert x.size == n
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def filtered_of(kind, rate, profile, rows=ROWS):
    from oracle import binding as oracle
    _, steps = oracle.decode(recording(kind, rate, profile, rows), rate, False, settings=oracle_settings(profile), want_steps=True)
    f = steps["filtered"]
    assert f.size == geometry(rate, profile).work_len(recording(kind, rate, profile, rows).size, True)
    f.setflags(write=False)
    return f


def table_case(row):
    """(audio, filtered, rate, profile) of a recording of track_cases' table"""
    return tc.recording(row), tc.filtered(row), tc.RATE, "standard"


def weak_case():
    return tc.weak_recording(), tc.weak_model()[0], tc.RATE, "standard"


@functools.lru_cache(maxsize=None)
def _model(key, rate, profile, w, lam, lag):
    if key[0] == "weak":
        sig = weak_case()[1]
    elif key[0] == "table":
        sig = tc.filtered(key[1])
    else:
        sig = filtered_of(key[0], rate, profile, key[1])
    return lm.Model(sig, work_rate(profile) // 4160, w, lam, lag)


def expected(key, rate, profile, sizes, w=8, lam=0.1, lag=8):
    """the model's calls for the pushes `sizes` and the finish: [(positions, scores, rows, record)], error text or None"""
    g = geometry(rate, profile)
    mdl = _model(key, rate, profile, w, lam, lag)
    mdl.reset()
    calls, n = [], 0
    for c in sizes:
        n += c
        calls.append(mdl.push(g.work_len(n, False)) + (mdl.record(),))
    pos, s, rows, error = mdl.push(g.work_len(n, True), True)
    calls.append((pos, s, rows, mdl.record()))
    return calls, error


def run_tracked(dec, x, sizes):
    """pushes x in chunks of `sizes`, then finishes: per call (rows, positions, scores, stream record, tracker record)"""
    calls, at, err = [], 0, None

    def record():
        r, t = dec.result, dec.track_result
        return ((int(r.work_len), int(r.scan_pos), int(r.n_rows), int(r.n_sync), int(r.n_in), int(r.rows_total)),
                (int(t.m), int(t.next_checkpoint), int(t.n_positions), int(t.n_relocks),
                 int(t.last_position) if t.has_position else None))

    for c in sizes:
        rows, pos = dec.push(x[at:at + c])
        at += c
        calls.append((rows, pos, dec.scores) + record())
    assert at == x.size
    try:
        rows, pos = dec.finish()
        scores = dec.scores
    except apt.AptError as e:
        err = e
        rows, pos, scores = np.zeros((0, 2080), f32), np.zeros(0, np.uint64), np.zeros(0, f32)
    calls.append((rows, pos, scores) + record())
    return calls, err


def check_calls(calls, err, want, want_error, sizes, what):
    """after EVERY push: rows released, positions, scores and rows bit for bit, m, the checkpoint count, n_relocks"""
    assert len(calls) == len(want), what
    n_in = released = 0
    for k, ((rows, pos, scores, rec, trk), (wpos, wsc, wrows, wrec)) in enumerate(zip(calls, want)):
        at = (what, "finish" if k == len(sizes) else ("push", k))
        if k < len(sizes):
            n_in += sizes[k]
        if want_error is not None and k == len(sizes):
            assert isinstance(err, apt.InternalError) and str(err) == want_error, (at, err)
            continue
        assert np.array_equal(np.asarray(pos, np.int64), wpos), (at, pos, wpos)
        assert scores.shape == wsc.shape and np.array_equal(sc.bits(scores), sc.bits(wsc)), at
        assert rows.shape == wrows.shape and np.array_equal(sc.bits(rows), sc.bits(wrows)), at
        released += wpos.size
        assert trk == wrec, (at, trk, wrec)
        assert rec[1] == wrec[0] and rec[2] == wpos.size and rec[3] == wrec[2] and rec[4] == n_in and rec[5] == released, (at, rec, wrec)
    if want_error is None:
        assert err is None, (what, err)
    all_pos = np.concatenate([c[1] for c in calls]).astype(np.int64)
    all_sc = np.concatenate([c[2] for c in calls])
    all_rows = np.concatenate([c[0] for c in calls])
    return all_pos, all_sc, all_rows


def track_record_of(t):
    return (int(t.m), int(t.next_checkpoint), int(t.n_positions), int(t.n_relocks), int(t.last_position) if t.has_position else None)


def iq_against_decoder(live, dec, audio, rec, sizes):
    """pushes rec.iq into `live` (a tracked LiveIqDecoder) and the matching slices of the demodulated `audio` into `dec`
    (a tracked LiveDecoder): rows, positions, scores and both records equal after every push and after finish.
    -> (all rows, the last tracker record)"""
    import fm_stream_cases as fsc
    import np_fm_model as fm
    rows, p = [], 0
    for k in list(sizes) + [None]:
        if k is None:
            (r1, q1), (r2, q2) = live.finish(), dec.finish()
        else:
            a0, a1 = fm.out_len(p, rec.t, rec.d), fm.out_len(p + k, rec.t, rec.d)
            assert live.rows_bound(k) == dec.rows_bound(a1 - a0)
            r1, q1 = live.push(rec.iq[2 * p:2 * (p + k)])
            r2, q2 = dec.push(audio[a0:a1])
            p += k
        assert r1.tobytes() == r2.tobytes() and q1.tolist() == q2.tolist(), p
        assert live.scores.tobytes() == dec.scores.tobytes() and live.scores.size == r1.shape[0], p
        assert fsc.record_of(live.result) == fsc.record_of(dec.result), p
        assert track_record_of(live.track_result) == track_record_of(dec.track_result), p
        rows.append(r1)
    return np.concatenate(rows), track_record_of(live.track_result)
