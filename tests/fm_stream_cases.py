"""Cases for the streaming FM demodulator's tests (test_fm_stream_cpu.py, test_gpu_fm_stream.py): the recordings of
fm_cases.BOUND_CASES 0, 1, 2, 3 and 6 cut to at most 20 000 frames (D = 50: T + 40 D), the chunkings every test walks,
and one walk that checks the release schedule and the info after EVERY push against the host formulas of DESIGN.md §23:
    M(n) = (n - T) / D + 1 (0 below T), out_len(n) = max(M(n) - 1, 0), carry(n) = n - out_len(n) D."""
import functools
import types

import numpy as np

import fm_cases as fc
import np_fm_model as fm

import noaa_apt_amd as apt

CASES = [fc.BOUND_CASES[i] for i in (0, 1, 2, 3, 6)]
IDS = [fc.IDS[i] for i in (0, 1, 2, 3, 6)]
CHUNKINGS = ["one", "boundaries", "4096", "random", "ones_then_rest", "over_max_push"]
MAX_PUSH_SMALL = 1000


@functools.lru_cache(maxsize=None)
def cut(case):
    """the case's recording cut for the stream tests: settings, frames, T, D (the array is read-only)"""
    c = fc.case(*case)
    t, d = c.info.n_taps, c.settings.decimation
    n = t + 40 * d if d == 50 else min(20000, c.iq.size // 2)
    iq = c.iq[:2 * n]
    return types.SimpleNamespace(settings=c.settings, iq=iq, n=n, t=t, d=d, case=c)


def sizes_of(chunking, n, t, d, seed=5):
    if chunking in ("one", "over_max_push"):
        return [n]
    if chunking == "boundaries":  # the exact release boundaries: T - 1, T, T + D - 1, T + D frames
        return [t - 1, 1, d - 1, 1, n - t - d]
    if chunking == "4096":
        return [4096] * (n // 4096) + ([n % 4096] if n % 4096 else [])
    if chunking == "ones_then_rest":
        k = t + 3 * d + 11
        return [1] * k + [n - k]
    assert chunking == "random"
    rng = np.random.default_rng(seed)
    out, left = [0, 1, 1, 0, 7, d + 1], n - 10 - d  # zeros, ones and sizes that are no multiple of 8 or of D for sure
    while left:
        k = min(int(rng.integers(0, 3 * t + 1)), left)
        out.append(k)
        left -= k
    return out


def max_push_of(chunking):
    return MAX_PUSH_SMALL if chunking == "over_max_push" else None


def check_info(info, n, t, d):
    assert info.frames == n and info.outputs == fm.out_len(n, t, d), (info.frames, info.outputs, n)
    assert info.carry_frames == n - fm.out_len(n, t, d) * d < t + d
    assert info.n_taps == t and info.decimation == d


def walk(stream, iq, sizes, t, d, push=None):
    """pushes iq in `sizes`; after every push: the count and the info.  -> the concatenated outputs"""
    push = push or (lambda chunk: stream.push(chunk))
    got, p = [], 0
    for k in sizes:
        expect = fm.out_len(p + k, t, d) - fm.out_len(p, t, d)
        assert stream.out_len(k) == expect
        a = push(iq[2 * p:2 * (p + k)])
        p += k
        assert a.size == expect and a.dtype == np.float32, (p, k, a.size, expect)
        check_info(stream.get_info(), p, t, d)
        got.append(a)
    assert p == iq.size // 2
    return np.concatenate(got) if got else np.zeros(0, np.float32)


def non_finite_recording():
    """test_non_finite_frames' settings (D = 5, F32, 12 kHz): a NaN frame and an Inf frame at a chunk seam and T / 2
    before one -> (settings, clean iq, dirty iq, sizes, mask of the outputs that must be NaN)"""
    c = fc.case(5, 12000.0, fm.F32, 0.5)
    t, d, n = c.info.n_taps, 5, 20000
    clean = c.iq[:2 * n].copy()
    seam_a, seam_b = 6001, 13004
    sizes = [seam_a, seam_b - seam_a, n - seam_b]
    dirty = clean.copy()
    i_nan, i_inf = seam_a, seam_b - t // 2  # the first frame of a chunk; T / 2 before a seam
    dirty[2 * i_nan], dirty[2 * i_inf + 1] = np.nan, np.inf
    bad_v = np.zeros(fm.out_len(n, t, d) + 1, bool)
    for i in (i_nan, i_inf):  # v[m] reads frames [m d, m d + t)
        bad_v[max(-(-(i - t + 1) // d), 0):i // d + 1] = True
    return c.settings, clean, dirty, sizes, bad_v[:-1] | bad_v[1:], t, d


LIVE_D, LIVE_SHIFT, LIVE_SECONDS = 5, 25000.0, 8.0


@functools.lru_cache(maxsize=None)
def live_recording(seconds=LIVE_SECONDS):
    """the 8 s D = 5 s16 recording of test_gpu_fm.test_end_to_end_rows_and_stream_order (14 rows)"""
    st = fc.settings(LIVE_D, LIVE_SHIFT, fm.S16)
    iq = fc.recording(LIVE_D, LIVE_SHIFT, fm.S16, seconds, seed=23)
    iq.flags.writeable = False
    info = apt.fm_design(st)
    return types.SimpleNamespace(settings=st, iq=iq, n=iq.size // 2, t=info.n_taps, d=LIVE_D)


def live_sizes(chunking, n, seed=9):
    if chunking == "one":
        return [n]
    if chunking == "quarter_second":
        k = 240000 // 4
        return [k] * (n // k) + ([n % k] if n % k else [])
    assert chunking == "random"
    rng = np.random.default_rng(seed)
    out, left = [], n
    while left:
        k = min(int(rng.integers(0, 400001)), left)
        out.append(k)
        left -= k
    return out


def record_of(res):
    return (int(res.work_len), int(res.scan_pos), int(res.n_rows), int(res.n_sync))


def live_against_decoder(live, dec, audio, rec, sizes):
    """pushes rec.iq into `live` (a LiveIqDecoder) and the matching slices of `audio` into `dec` (a LiveDecoder): rows,
    positions and records equal after every push and after finish.  -> all rows"""
    rows, p = [], 0
    for k in sizes:
        a0, a1 = fm.out_len(p, rec.t, rec.d), fm.out_len(p + k, rec.t, rec.d)
        assert live.rows_bound(k) == dec.rows_bound(a1 - a0)
        r1, q1 = live.push(rec.iq[2 * p:2 * (p + k)])
        r2, q2 = dec.push(audio[a0:a1])
        p += k
        assert r1.tobytes() == r2.tobytes() and q1.tolist() == q2.tolist(), p
        assert record_of(live.result) == record_of(dec.result), p
        rows.append(r1)
    r1, q1 = live.finish()
    r2, q2 = dec.finish()
    assert r1.tobytes() == r2.tobytes() and q1.tolist() == q2.tolist()
    assert record_of(live.result) == record_of(dec.result)
    rows.append(r1)
    return np.concatenate(rows)
