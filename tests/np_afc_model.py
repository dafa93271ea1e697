"""The AFC's definition (include/aptgpu.h §4b') in numpy: block sums in exact integers (F32: f64), the table in f64
with the adds in ascending block order, and an f64 model of the tracked demodulator (np_fm_model's, with the phase of
every frame taken from a table)."""
import numpy as np

import np_fm_model as fm

TWO32 = 1 << 32
RECORD = np.dtype([("pw", "<u4"), ("phase0", "<u4"), ("step_re", "<f4"), ("step_im", "<f4")])


def auto_lag(fs, max_offset_hz, deviation_hz):
    return int(min(max(np.floor(fs / (4.0 * (max_offset_hz + deviation_hz))), 1), 64))


def n_blocks(n, b):
    return -(-n // b)


def components(iq, fmt, swap=False):
    """(I, Q) as the sums take them: int64 (u8: 2 raw - 255) or, for F32, float64"""
    a = np.asarray(iq)
    assert a.dtype == fm.DTYPES[fmt]
    x = a.reshape(-1, 2).astype(np.float64 if fmt == fm.F32 else np.int64)
    if fmt == fm.U8:
        x = 2 * x - 255
    return (x[:, 1], x[:, 0]) if swap else (x[:, 0], x[:, 1])


def sums(iq, fmt, b, lag, swap=False):
    """(nb, 3) {re, im, en}: int64 (exact; object where a sum could pass 2^63, which no case here does) or f64"""
    i, q = components(iq, fmt, swap)
    n = i.size
    nb = n_blocks(n, b)
    out = np.zeros((nb, 3), i.dtype)
    m = max(n - lag, 0)  # frames with a partner
    re_t = i[lag:lag + m] * i[:m] + q[lag:lag + m] * q[:m]
    im_t = q[lag:lag + m] * i[:m] - i[lag:lag + m] * q[:m]
    en_t = i * i + q * q
    for k in range(nb):
        lo, hi = k * b, min((k + 1) * b, n)
        out[k, 0] = re_t[lo:min(hi, m)].sum() if lo < m else 0
        out[k, 1] = im_t[lo:min(hi, m)].sum() if lo < m else 0
        out[k, 2] = en_t[lo:hi].sum()
    return out


def llround(x):
    """halves away from zero"""
    return (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.int64)


def estimate(s, lag, w, pw_base, fs, max_offset_hz, min_coherence):
    """Stage B, steps 1-4 -> (coherence f64, est uint32-valued int64, good, rel, finite)"""
    s = np.asarray(s, dtype=np.float64)
    nb = s.shape[0]
    acc = np.zeros((nb, 3))
    idx = np.arange(nb)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(-(w // 2), w // 2 + 1):  # ascending block order for every b
            j = idx + k
            ok = (j >= 0) & (j < nb)
            acc[ok] += s[j[ok]]
        rre, rim, e = acc[:, 0], acc[:, 1], acc[:, 2]
        coh = np.zeros(nb)
        nz = e != 0
        coh[nz] = np.sqrt(rre[nz] * rre[nz] + rim[nz] * rim[nz]) / e[nz]
    finite = np.isfinite(rre) & np.isfinite(rim) & np.isfinite(e)
    turns = np.arctan2(np.where(finite, rim, 0.0), np.where(finite, rre, 0.0)) / (2.0 * np.pi)
    q = np.rint(turns * TWO32).astype(np.int64) % TWO32
    d = (q - (lag * pw_base) % TWO32) % TWO32
    d = np.where(d >= 1 << 31, d - TWO32, d)
    rel = llround(d.astype(np.float64) / float(lag))
    est = (pw_base + rel) % TWO32
    with np.errstate(invalid="ignore"):
        good = finite & (coh >= min_coherence) & (np.abs(rel).astype(np.float64) * float(fs) / TWO32 <= max_offset_hz)
    return coh, est, good, rel, finite


def hold(est, good, pw_base):
    """step 5"""
    nb = est.size
    pw = np.full(nb, pw_base, np.int64)
    g = np.flatnonzero(good)
    if g.size:
        last = np.maximum.accumulate(np.where(good, np.arange(nb), -1))
        j = np.where(last >= 0, last, g[0])
        pw = est[j]
    return pw


def records_of(pw, b):
    """steps 6 and 7 from a block's pw"""
    pw = np.asarray(pw, dtype=np.int64) % TWO32
    r = np.zeros(pw.size, RECORD)
    r["pw"] = pw
    inc = (b * pw) % TWO32
    r["phase0"] = (np.concatenate([[0], np.cumsum(inc)[:-1]]) % TWO32) if pw.size else 0
    t = np.where(pw >= 1 << 31, pw - TWO32, pw).astype(np.float64) * (np.pi / 2147483648.0)
    r["step_re"] = np.cos(t).astype(np.float32)
    r["step_im"] = (-np.sin(t)).astype(np.float32)
    return r


def coherence_f32(coh):
    c = coh.astype(np.float32)
    c[np.isnan(coh)] = np.uint32(0x7FC00000).view(np.float32)
    return c


def table(s, b, lag, w, pw_base, fs, max_offset_hz, min_coherence):
    """-> (records, coherence f32, good, rel, coherence f64)"""
    coh, est, good, rel, _ = estimate(s, lag, w, pw_base, fs, max_offset_hz, min_coherence)
    return records_of(hold(est, good, pw_base), b), coherence_f32(coh), good, rel, coh


def offset_hz(pw, fs):
    pw = np.asarray(pw, dtype=np.int64)
    return np.where(pw >= 1 << 31, pw - TWO32, pw) * fs / TWO32


def frame_phase(records, b, n):
    """the integer phase of frames 0 ... n - 1: phase0[k] + (uint32)(i - k b) * pw[k], k = i / b"""
    i = np.arange(n, dtype=np.int64)
    k = i // b
    return (records["phase0"].astype(np.int64)[k] + (i - k * b) * records["pw"].astype(np.int64)[k]) % TWO32


def filtered_tracked(iq, fmt, taps, d, records, b, swap=False):
    """np_fm_model.filtered with the table's phase: v[m], complex128 (always mixed)"""
    x = fm.convert(iq, fmt, swap)
    h = np.asarray(taps, dtype=np.float32).astype(np.float64)
    n, t = x.size, h.size
    if n < t:
        return np.zeros(0, np.complex128)
    m = (n - t) // d + 1
    with np.errstate(invalid="ignore"):
        u = x * np.exp(-2j * np.pi * (frame_phase(records, b, n).astype(np.float64) / TWO32))
        v = np.zeros(m, np.complex128)
        for k in range(t):
            j = t - 1 - k
            v += h[k] * u[j:j + (m - 1) * d + 1:d]
    return v


def demodulate_tracked(iq, fmt, fs, d, taps, records, b, deviation_hz=17000.0, swap=False):
    """-> (audio f64, v complex128)"""
    v = filtered_tracked(iq, fmt, taps, d, records, b, swap)
    return fm.discriminate(v, fm.gain(fs // d, deviation_hz)), v
