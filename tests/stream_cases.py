"""Cases the live-decode tests share (test_stream_cpu.py, test_gpu_stream.py): recordings, chunkings, the oracle's
reference for each recording (computed once, read-only) and the checks of DESIGN.md §22 — parity with decode() bit for
bit, the release schedule of np_stream_model.py after every push, the records."""
import functools

import numpy as np

import np_stream_model as sm

import noaa_apt_amd as apt
from noaa_apt_amd.testing.synth import synth_apt, synth_noise

f32 = np.float32
PROFILE_RATES = {"standard": 12480, "fast": 16640, "slow": 20800}
# (input rate, profile): l / m = 832 / 735, 13 / 50, 1 / 2, 1 / 1, 832 / 2205 (pw 4), 1 / 1 (pw 5)
RATES = ((11025, "standard"), (48000, "standard"), (24960, "standard"), (12480, "standard"), (44100, "fast"), (20800, "slow"))
CHUNKINGS = ("one", "half_second", "4096", "random", "single_samples", "over_max_push")
SIGNALS = ("apt", "apt_ppm", "noise", "zeros", "constant", "nonfinite")
LOW_RATES = ((8000, "standard"), (6000, "standard"))  # 39 / 25 and 52 / 25: more than a row of work signal per 4 096 samples


def most_copies(ref):
    """the largest number of peaks the oracle pushed at one position"""
    return int(np.unique(ref.peaks, return_counts=True)[1].max())


def oracle_settings(profile):
    from oracle import binding as oracle
    return {"standard": oracle.STANDARD, "fast": oracle.FAST, "slow": oracle.SLOW}[profile]


@functools.lru_cache(maxsize=None)
def geometry(rate, profile):
    """the tap counts are the oracle's own (its steps on a recording long enough to decode)"""
    from oracle import binding as oracle
    x = synth_apt(rate, 5.5, 3)
    _, steps = oracle.decode(x, rate, False, settings=oracle_settings(profile), want_steps=True)
    return sm.Geometry(rate, PROFILE_RATES[profile], steps["resample_filter"].size, steps["filter_filter"].size)


@functools.lru_cache(maxsize=None)
def recording(kind, rate, profile, rows_x100, seed=11):
    """a recording whose finished work signal is the shortest one of at least rows_x100 / 100 rows"""
    g = geometry(rate, profile)
    n = g.samples_for(-(-rows_x100 * g.spr // 100))
    if rows_x100 == 999:  # ... or the longest one below ten rows
        n = g.samples_for(10 * g.spr) - 1
    seconds = n / rate + 0.01
    if kind in ("apt", "nonfinite"):
        x = synth_apt(rate, seconds, seed)[:n].copy()
    elif kind == "apt_ppm":
        x = synth_apt(rate, seconds, seed, ppm=120.0)[:n].copy()
    elif kind == "noise":
        x = synth_noise(rate, seconds, seed)[:n].copy()
    elif kind == "zeros":
        x = np.zeros(n, f32)
    elif kind == "constant":
        x = np.full(n, 1234.0, f32)
    elif kind == "fading":
        # a bare carrier that fades for 14 s and then stays level: the correlation climbs sample after sample, the picker
        # keeps replacing ONE peak for 28 rows, and the event after the climb pushes all the missing peaks at once
        t = np.arange(n) / rate
        x = np.rint(20000.0 * (1.0 - 0.9 * np.minimum(t / 14.0, 1.0)) * np.cos(2 * np.pi * 2400.0 * t)).astype(f32)
    else:
        raise ValueError(kind)
    if kind == "nonfinite":
        x[n // 2] = np.nan
        x[(2 * n) // 3 + 5] = np.inf
    assert x.size == n
    x.setflags(write=False)
    return x


class Reference:
    """what the oracle says about one recording"""
    pass


@functools.lru_cache(maxsize=None)
def reference(kind, rate, profile, rows_x100, sync, seed=11):
    from oracle import binding as oracle
    g = geometry(rate, profile)
    x = recording(kind, rate, profile, rows_x100, seed)
    st = oracle_settings(profile)
    ref = Reference()
    ref.g, ref.x, ref.sync = g, x, sync
    ref.error = None
    try:
        ref.rows = oracle.decode(x, rate, sync, settings=st).reshape(-1, 2080)
    except oracle.OracleError as e:
        ref.error, ref.rows = str(e), None
    # the filtered signal and the correlation: of this recording, or — one that is too short to have them — of its
    # continuation to 12.37 rows, which is the same wherever the stream may look before finish()
    if g.work_len(x.size, True) >= 10 * g.spr:
        full = x
    else:
        assert kind == "apt"
        full = recording(kind, rate, profile, 1237, seed)
        assert np.array_equal(full[:x.size], x)
    _, steps = oracle.decode(full, rate, False, settings=st, want_steps=True)
    F = steps["filtered"]
    ref.work_len = g.work_len(x.size, True)
    assert full is not x or F.size == ref.work_len
    corr = None
    if sync:
        pos, corr = oracle.find_sync(F, PROFILE_RATES[profile], return_correlation=True)
        ref.peaks = pos.astype(np.int64)
    ref.model = sm.Model(g, corr, sync)
    if sync and full is x:
        assert np.array_equal(ref.model.positions, ref.peaks)  # the replay is the oracle's scan
        ref.positions = np.array([p for p in ref.peaks[:-1] if p + g.spr < F.size], np.int64)
        ref.n_sync = ref.peaks.size
    elif full is x:
        ref.positions = np.arange(F.size // g.spr, dtype=np.int64) * g.spr
        ref.n_sync = 0
    if ref.rows is not None:
        assert ref.rows.shape[0] == ref.positions.size
        ref.rows.setflags(write=False)
    return ref


def chunk_sizes(name, n, rate, g, max_push=None):
    if name == "one":
        return [n]
    if name == "half_second":
        c = rate // 2
    elif name == "4096":
        c = 4096
    elif name == "over_max_push":
        assert max_push and n > 3 * max_push
        return [max_push // 2, 2 * max_push + max_push // 3, n - (max_push // 2 + 2 * max_push + max_push // 3)]
    elif name == "random":
        rng = np.random.default_rng(n)
        out, left = [], n
        while left:
            c = int(rng.integers(0, 3001))
            if len(out) % 7 == 3:
                c = 0
            if len(out) % 7 == 5:
                c = 1
            c = min(c, left)
            out.append(c)
            left -= c
        return out
    elif name == "single_samples":
        # 1-sample pushes across 2000 samples around the input sample at which row 5 of the work signal ends
        mid = 5 * g.spr * g.m // g.l
        a = max(0, mid - 1000)
        return [a] + [1] * 2000 + [n - a - 2000]
    else:
        raise ValueError(name)
    return [c] * (n // c) + ([n % c] if n % c else [])


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def settings_of(profile):
    return apt.Settings.profile(profile)


def run_stream(dec, x, sizes):
    """pushes x in chunks of `sizes`, then finishes: ([(rows, positions, record fields)] per call, error or None)"""
    calls, at, err = [], 0, None
    for c in sizes:
        rows, pos = dec.push(x[at:at + c])
        at += c
        r = dec.result
        calls.append((rows, pos, (int(r.work_len), int(r.scan_pos), int(r.n_rows), int(r.n_sync), int(r.n_in), int(r.rows_total))))
    assert at == x.size
    try:
        rows, pos = dec.finish()
    except apt.AptError as e:
        err = e
        rows, pos = np.zeros((0, 2080), f32), np.zeros(0, np.uint64)
    r = dec.result
    calls.append((rows, pos, (int(r.work_len), int(r.scan_pos), int(r.n_rows), int(r.n_sync), int(r.n_in), int(r.rows_total))))
    return calls, err


def check_against_reference(calls, err, ref, sizes, what):
    """assertions 1 and 2 of the issue: parity with the oracle and the model's release schedule after every push"""
    g = ref.g
    sched = ref.model.schedule(sizes)
    released, n_in = 0, 0
    for k, (want, (rows, pos, rec)) in enumerate(zip(sched, calls[:-1])):
        n_in += sizes[k]
        w, scan, n_rows, n_sync = want
        assert rec[:4] == (w, scan, n_rows, n_sync), (what, "push", k, rec, want)
        assert rows.shape == (n_rows, 2080) and pos.shape == (n_rows,), (what, k)
        released += n_rows
        assert rec[4] == n_in and rec[5] == released, (what, k, rec)
    w, scan, n_rows, n_sync, text = ref.model.finish(n_in, released)
    rows, pos, rec = calls[-1]
    assert w == ref.work_len
    assert rec[0] == w and rec[1] == scan, (what, "finish", rec, (w, scan))
    if ref.error is not None:
        assert text is not None and text in ref.error, (what, text, ref.error)
        assert isinstance(err, apt.InternalError) and str(err) == ref.error, (what, err, ref.error)
        assert rec[2] == 0
    else:
        assert err is None and text is None, (what, err, text)
        assert rec[2:4] == (n_rows, n_sync), (what, "finish", rec, (n_rows, n_sync))
        assert rec[3] == ref.n_sync and rec[5] == ref.rows.shape[0], (what, rec)
    all_rows = np.concatenate([c[0] for c in calls])
    all_pos = np.concatenate([c[1] for c in calls]).astype(np.int64)
    if ref.error is None:
        assert np.array_equal(all_pos, ref.positions), (what, all_pos, ref.positions)
        assert all_rows.shape == ref.rows.shape and np.array_equal(bits(all_rows), bits(ref.rows)), what
    return all_rows, all_pos


def check_same(calls_a, calls_b, what):
    """assertion 5: the same bits per push"""
    assert len(calls_a) == len(calls_b), what
    for k, (a, b) in enumerate(zip(calls_a, calls_b)):
        assert a[2] == b[2], (what, k, a[2], b[2])
        assert np.array_equal(a[1], b[1]) and a[0].shape == b[0].shape and np.array_equal(bits(a[0]), bits(b[0])), (what, k)
