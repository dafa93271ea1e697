"""The FM demodulator's definition (include/aptgpu.h §4b) in numpy f64, and an FM modulator for building cases.

The model takes the same integer phase and the same f32 taps as the library and nothing else from it: every product and
sum is f64, the phasor of frame i is exp(-j theta_i) itself (no recurrence), atan2 is numpy's."""
import numpy as np

U8, S8, S16, F32 = 0, 1, 2, 3
DTYPES = {U8: np.dtype(np.uint8), S8: np.dtype(np.int8), S16: np.dtype("<i2"), F32: np.dtype("<f4")}
TWO32 = 1 << 32


def pw_of(shift_hz, fs):
    """(uint32) llround(shift_hz / fs * 2^32), two's complement"""
    v = shift_hz / fs * TWO32
    r = int(np.floor(abs(v) + 0.5))  # llround: halves away from zero
    return (r if v >= 0 else -r) % TWO32


def shift_used(pw, fs):
    return (pw - TWO32 if pw >= 1 << 31 else pw) * fs / TWO32


def phase(i, pw):
    """((uint32) i * pw) mod 2^32 for integer index arrays or ints of any size"""
    if isinstance(i, (int, np.integer)):
        return ((int(i) % TWO32) * pw) % TWO32
    lo = np.asarray(i, dtype=np.uint64) & np.uint64(TWO32 - 1)
    return (lo * np.uint64(pw)) & np.uint64(TWO32 - 1)  # < 2^64: no overflow before the mask


def theta(i, pw):
    return 2.0 * np.pi * (np.asarray(phase(i, pw), dtype=np.float64) / TWO32)


def convert(iq, fmt, swap=False):
    """interleaved components -> complex128, unscaled"""
    a = np.asarray(iq)
    assert a.dtype == DTYPES[fmt], (a.dtype, fmt)
    x = a.astype(np.float64).reshape(-1, 2)
    if fmt == U8:
        x = x - 127.5
    z = np.empty(x.shape[0], np.complex128)
    z.real, z.imag = (x[:, 1], x[:, 0]) if swap else (x[:, 0], x[:, 1])
    return z


def out_len(n, t, d):
    return max((n - t) // d + 1 - 1, 0) if n >= t else 0


def filtered(iq, fmt, taps, d, pw, swap=False):
    """v[m], complex128"""
    x = convert(iq, fmt, swap)
    h = np.asarray(taps, dtype=np.float32).astype(np.float64)
    n, t = x.size, h.size
    if n < t:
        return np.zeros(0, np.complex128)
    m = (n - t) // d + 1
    with np.errstate(invalid="ignore"):  # (non-finite frames)
        u = x * np.exp(-1j * theta(np.arange(n), pw)) if pw else x
        v = np.zeros(m, np.complex128)
        for k in range(t):  # v[m] = sum_k h[k] u[m d + t - 1 - k]
            j = t - 1 - k
            v += h[k] * u[j:j + (m - 1) * d + 1:d]
    return v


def gain(fs_out, deviation_hz):
    return fs_out / (2.0 * np.pi * deviation_hz)


def discriminate(v, g):
    if v.size < 2:
        return np.zeros(0, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        p = v[1:] * np.conj(v[:-1])
        a = g * np.arctan2(p.imag, p.real)
    a[(p.real == 0) & (p.imag == 0)] = 0.0
    bad = ~(np.isfinite(v.real) & np.isfinite(v.imag))
    a[bad[1:] | bad[:-1]] = np.nan
    return a


def demodulate(iq, fmt, fs, d, taps, shift_hz=0.0, deviation_hz=17000.0, swap=False):
    """-> (audio f64, v complex128, fs_out)"""
    assert fs % d == 0
    v = filtered(iq, fmt, taps, d, pw_of(shift_hz, fs), swap)
    return discriminate(v, gain(fs // d, deviation_hz)), v, fs // d


def bound(taps, x_max, v, a_model, g):
    """The issue's bound per output and the samples it lets a test skip: (bound, skip mask)."""
    h = np.abs(np.asarray(taps, dtype=np.float64))
    e = np.sqrt(2.0) * 2.0 * (h.size + 8) * 2.0 ** -24 * h.sum() * x_max
    with np.errstate(divide="ignore"):
        rel = e / np.abs(v[:-1]) + e / np.abs(v[1:])
    b = g * rel + 4.0 * 2.0 ** -24 * np.maximum(np.abs(a_model), 1e-3 * g)
    return b, rel > 0.01


# ---------------------------------------------------------------- building cases
def modulate(audio, fs, deviation_hz, offset_hz=0.0, phase0=0.0):
    """Constant-envelope FM of `audio` (in +-1, one value per frame at fs) around offset_hz: complex128, |z| = 1."""
    a = np.asarray(audio, dtype=np.float64)
    ph = 2.0 * np.pi * np.cumsum(deviation_hz * a + offset_hz) / fs + phase0
    return np.exp(1j * ph)


def quantize(z, fmt, amplitude=None):
    """complex128 -> interleaved components of the format (u8 / s8: amplitude 100, s16: 20000, f32: 1)"""
    amp = {U8: 100.0, S8: 100.0, S16: 20000.0, F32: 1.0}[fmt] if amplitude is None else amplitude
    x = np.empty(2 * z.size, np.float64)
    x[0::2], x[1::2] = amp * z.real, amp * z.imag
    if fmt == F32:
        return x.astype("<f4")
    if fmt == U8:
        return np.clip(np.rint(x + 127.5), 0, 255).astype(np.uint8)
    lim = 127 if fmt == S8 else 32767
    return np.clip(np.rint(x), -lim - 1, lim).astype(DTYPES[fmt])
