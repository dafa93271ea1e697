"""Cases the flywheel sync tests share (test_track_cpu.py, test_gpu_track.py): the small signals of the bit-for-bit
comparisons with np_track_model.py, and the noisy recordings of the benefit checks with their truth."""
import functools

import numpy as np

import np_track_model as tm

from noaa_apt_amd.testing.synth import synth_apt

f32 = np.float32
PWS = (1, 3, 4, 5, 8)
SETTINGS = ((0, 0.0), (1, 0.1), (8, 0.1), (64, 0.0))
KINDS = ("noise", "nonfinite", "zeros", "constant")


def lengths(pw):
    L, G = 2080 * pw, 38 * pw
    return (L + G, L + G + 1, 3 * L + G + 17)


@functools.lru_cache(maxsize=None)
def signal(kind, pw, n):
    rng = np.random.default_rng(1000 * pw + n % 977)
    if kind == "zeros":
        x = np.zeros(n, f32)
    elif kind == "constant":
        x = np.full(n, 1234.5, f32)
    else:
        # an envelope-like signal: positive, with a planted sync frame per row so that the scores are not all alike
        x = (4000.0 + 1500.0 * rng.standard_normal(n)).astype(f32)
        g = np.where(tm.template_plus(pw), 3000.0, -3000.0).astype(f32)
        for p in range(37 * pw + 5, n - g.size, 2080 * pw + 3):
            x[p:p + g.size] += g
        if kind == "nonfinite":
            x[n // 3] = np.nan
            x[n // 2 + 7] = np.inf
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def model_score(kind, pw, n, gain=0):
    s = tm.score(scaled(kind, pw, n, gain), pw)
    s.setflags(write=False)
    return s


def scaled(kind, pw, n, gain):
    x = signal(kind, pw, n)
    return x if gain == 0 else (x * f32(2.0 ** gain)).astype(f32)


@functools.lru_cache(maxsize=None)
def model_track(kind, pw, n, w, lam, gain=0):
    x = scaled(kind, pw, n, gain)
    s = model_score(kind, pw, n, gain)
    pos = tm.track_scores(s, pw, w, lam)
    return pos, s[pos], tm.rows_of(x, pos, pw)


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def check_track(got, want, what):
    """positions, per-position scores and rows identical (scores and rows bit for bit)"""
    pos, sc, rows = got[:3]
    wpos, wsc, wrows = want
    assert np.array_equal(np.asarray(pos, np.int64), wpos), (what, pos, wpos)
    assert np.array_equal(bits(sc), bits(wsc)), what
    assert rows.shape == wrows.shape and np.array_equal(bits(rows), bits(wrows)), (what, rows.shape, wrows.shape)


def check_invariants(pos, pw, n, w, what):
    L, G, M = tm.geometry(n, pw)
    pos = np.asarray(pos, np.int64)
    assert pos.size >= 1 and pos[0] < L and pos[-1] >= M - L and pos[-1] < M, (what, pos)
    d = np.diff(pos)
    assert ((d >= L - w) & (d <= L + w)).all(), (what, d)


# ---------------------------------------------------------------- the table's recordings
RATE, SECONDS, SEED, START_PX = 11025, 40, 5, 700.0
WORK_RATE, PW = 12480, 3
# (noise_sigma, ppm, dropout, bound in work samples): rows 1..6 of the table in DESIGN.md §21
TABLE = ((400.0, 0.0, False, 3.0), (8000.0, 0.0, False, 3.0), (12000.0, 150.0, True, 8.0), (16000.0, -150.0, True, 8.0),
         (20000.0, 0.0, True, 3.0), (24000.0, 80.0, True, 8.0))


@functools.lru_cache(maxsize=None)
def recording(row):
    sigma, ppm, dropout, _ = TABLE[row]
    x = synth_apt(RATE, SECONDS, SEED, start_px=START_PX, noise_sigma=sigma, ppm=ppm)
    if dropout:
        x[15 * RATE:19 * RATE] = 0
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def filtered(row):
    """the oracle's "filter_result" step of the recording (the no-sync branch computes the same F and never refuses)"""
    from oracle import binding as oracle
    _, steps = oracle.decode(recording(row), RATE, False, want_steps=True)
    f = steps["filtered"]
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def truth_line(ppm):
    """least-squares line through the oracle's positions [1:-1] of the same recording without noise"""
    from oracle import binding as oracle
    x = synth_apt(RATE, SECONDS, SEED, start_px=START_PX, noise_sigma=0.0, ppm=ppm)
    _, steps = oracle.decode(x, RATE, True, want_steps=True)
    p = steps["sync_pos"].astype(np.float64)[1:-1]
    k = np.arange(p.size, dtype=np.float64)
    b, a = np.polyfit(k, p, 1)
    return a, b


def errors(pos, ppm):
    """distance of every position to the nearest point of the truth line, in work samples"""
    a, b = truth_line(ppm)
    p = np.asarray(pos, np.float64)
    k = np.rint((p - a) / b)
    return np.abs(p - (a + b * k))


@functools.lru_cache(maxsize=None)
def model_table(row):
    f = filtered(row)
    pos, sc, rows, _ = tm.track(f, PW, 8, 0.1)
    return pos, sc, rows


# ---------------------------------------------------------------- a recording decode() refuses
@functools.lru_cache(maxsize=None)
def weak_recording():
    """Six seconds at 11 025 Hz: three rows of APT, then the modulation stops and the bare carrier fades by half
    every 1.5 s.  The reference's correlation then rises sample after sample, its picker keeps replacing one peak to
    the end, and decode() fails with "less than 5 sync frames" (find_sync returns three positions)."""
    n = RATE * 6
    t = np.arange(n) / RATE
    x = synth_apt(RATE, 6.0, 11, noise_sigma=300.0, start_px=300.0).copy()
    cut = int(1.6 * RATE)
    fade = (12000.0 * 2.0 ** (-(t - 1.6) / 1.5) * np.cos(2 * np.pi * 2400.0 * t)).astype(f32)
    x[cut:] = fade[cut:]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def weak_model():
    """(F, positions, scores, rows) of the model on the oracle's filtered signal of weak_recording()"""
    from oracle import binding as oracle
    _, steps = oracle.decode(weak_recording(), RATE, False, want_steps=True)
    f = steps["filtered"]
    pos, sc, rows, _ = tm.track(f, PW, 8, 0.1)
    return f, pos, sc, rows


# ---------------------------------------------------------------- the table's recordings at another rate and profile
@functools.lru_cache(maxsize=None)
def recording_at(row, rate):
    if rate == RATE:
        return recording(row)
    sigma, ppm, dropout, _ = TABLE[row]
    x = synth_apt(rate, SECONDS, SEED, start_px=START_PX, noise_sigma=sigma, ppm=ppm)
    if dropout:
        x[15 * rate:19 * rate] = 0
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def model_at(row, rate, profile):
    """(positions, scores, rows) of the model on the oracle's filtered signal under the profile's settings"""
    from oracle import binding as oracle
    settings = {"standard": oracle.STANDARD, "fast": oracle.FAST}[profile]
    _, steps = oracle.decode(recording_at(row, rate), rate, False, settings=settings, want_steps=True)
    pos, sc, rows, _ = tm.track(steps["filtered"], settings["work_rate"] // 4160, 8, 0.1)
    return pos, sc, rows
