"""Float64 model of decode()'s front end (resampler -> AM envelope -> low-pass) and of the arithmetic the three
approximate front ends document, plus the one acceptance rule their tests share (test tooling, no GPU).

Written from the formulas, as np_model.py is — the polyphase closed form of fast_resampling (dsp.rs:186-289), the
envelope of demodulate (dsp.rs:350-383), filter() with its `i > j` start-up (dsp.rs:386-410) — but with every product
and sum in float64, so that what is left of a comparison against it is the rounding of whoever is compared: the strict
oracle's f32 chain, or a kernel's.  Every function takes the taps AS GIVEN (the oracle's `resample_filter` /
`filter_filter` steps, f32 values) and returns every work-rate sample.

The approximate modes (noaa_apt_amd/csrc/apt_kernels_fused_impl.hpp, apt_kernels_fused.hip):

  kModeFast     f32 with fused multiply-adds, native square root, a multiplication by RN(1 / sin phi): nothing is
                quantised, its prediction is the f64 chain itself;
  kModeMfma     stage 1 as five bf16 x bf16 products with f32 accumulation: taps h = h0 + h1 + h2 (`tap_pieces`, the
                host's split in mfma_fragments: upper 16 bits of the f32 pattern, of the remainder, of its remainder),
                samples x0 = upper 16 bits of x, x1 = upper 16 bits of x - x0, the rest of x dropped
                (`sample_planes`); R = sum of h2 x0, h1 x1, h1 x0, h0 x1, h0 x0 (`resample_mfma64`);
  kModeF16Taps  stage 1 on taps prescaled by a power of two (maximum in [1, 2)) and rounded to fp16
                (fused_f16_branch_taps), samples rounded to fp16, unscaled behind the sum (`resample_f16taps64`).

The work-rate stages behind are f32 (kModeFast's behind the matrix cores, the strict ones behind fp16 taps): the
prediction is `work_stages64` on that R.
"""
import numpy as np

import np_model

f64 = np.float64
f32 = np.float32

MFMA_TERMS = ((2, 0), (1, 1), (1, 0), (0, 1), (0, 0))  # (tap piece, sample plane) of the five products


def resample64(x, l, m, h):
    """fast_resampling: output k = sum_i x[x0 + i] h[p + i l], x0 = ceil(k m / l), p = x0 l - k m; x, h widened."""
    x = np.asarray(x, f64)
    h = np.asarray(h, f64)
    n, t_len = x.size, h.size
    off = (t_len - 1) // 2
    if n * l <= off:
        return np.zeros(0, f64)
    w = -(-(n * l - off) // m)
    k = np.arange(w, dtype=np.int64)
    x0 = -(-(k * m) // l)
    p = x0 * l - k * m
    tp = -(-t_len // l)
    xpad = np.concatenate([x, np.zeros(tp + 1, f64)])       # (samples behind the input's end: none, dsp.rs:258)
    hpad = np.concatenate([h, np.zeros(l + 1, f64)])
    s = np.zeros(w, f64)
    for i in range(tp):
        j = p + i * l
        s += hpad[np.minimum(j, t_len)] * xpad[np.minimum(x0 + i, n)]
    return s


def envelope_constants(work_rate):
    """The f32 constants 2 cos(phi) and sin(phi) of demodulate (dsp.rs:357-362), widened."""
    pi_rad = f32(f32(f32(2) * f32(2400)) / f32(work_rate))
    phi = f32(f32(2) * f32(pi_rad * np_model.PI))
    return f64(f32(np_model.cosf(phi) * f32(2))), f64(np_model.sinf(phi))


def envelope64(R, work_rate):
    """y[0] = 0, y[i] = sqrt(R[i-1]^2 + R[i]^2 - R[i-1] R[i] 2 cos(phi)) / sin(phi)."""
    R = np.asarray(R, f64)
    cosphi2, sinphi = envelope_constants(work_rate)
    y = np.zeros_like(R)
    y[1:] = np.sqrt(R[:-1] * R[:-1] + R[1:] * R[1:] - R[:-1] * R[1:] * cosphi2) / sinphi
    return y


def fir64(D, h2):
    """filter(): out[i] = sum over j < T with i > j of D[i - j] h2[j]."""
    D = np.asarray(D, f64)
    h2 = np.asarray(h2, f64)
    i = np.arange(D.size)
    s = np.zeros(D.size, f64)
    for j in range(h2.size):
        s += np.where(i > j, D[np.maximum(i - j, 0)], 0.0) * h2[j]
    return s


def work_stages64(R, work_rate, h2):
    return fir64(envelope64(R, work_rate), h2)


def chain64(x, l, m, h, work_rate, h2):
    return work_stages64(resample64(x, l, m, h), work_rate, h2)


# ---- kModeMfma

def _upper16(v):
    """f32 values whose bit patterns are those of v with the lower 16 bits cleared (a bf16, by truncation)."""
    v = np.ascontiguousarray(v, f32)
    return (v.view(np.uint32) & np.uint32(0xFFFF0000)).view(f32)


def tap_pieces(h):
    """mfma_fragments' split: p0 = upper(v), p1 = upper(v - p0), p2 = upper(v - p0 - p1), the subtractions in f32."""
    h = np.ascontiguousarray(h, f32)
    p0 = _upper16(h)
    r1 = (h - p0).astype(f32)
    p1 = _upper16(r1)
    r2 = (r1 - p1).astype(f32)
    p2 = _upper16(r2)
    return p0, p1, p2


def sample_planes(x):
    """planes_to_lds: x0 = upper(x), x1 = upper(x - x0) (f32 subtraction, exact); what is left of x is dropped."""
    x = np.ascontiguousarray(x, f32)
    x0 = _upper16(x)
    x1 = _upper16((x - x0).astype(f32))
    return x0, x1


def resample_mfma64(x, l, m, h, terms=MFMA_TERMS, planes=None):
    """Sum of the products `terms` (tap piece, sample plane) of the matrix-core stage 1, every one exact in f64."""
    hp = tap_pieces(h)
    xp = sample_planes(x) if planes is None else planes
    # (the resampler is linear in the taps: the products that share a sample plane go through it together)
    R = None
    for b in sorted({b for _, b in terms}):
        hsum = np.zeros(np.asarray(h).size, f64)
        for a, bb in terms:
            if bb == b:
                hsum += hp[a].astype(f64)
        r = resample64(xp[b], l, m, hsum)
        R = r if R is None else R + r
    return R


# ---- kModeF16Taps

def f16_tap_scale(h):
    """fused_f16_branch_taps' prescale: the power of two that puts max |h| into [1, 2)."""
    mx = float(np.max(np.abs(np.asarray(h, f32)))) if np.asarray(h).size else 0.0
    if mx <= 0.0:
        return 2.0
    _, e = np.frexp(f32(mx))
    return float(np.ldexp(1.0, -int(e) + 1))


def resample_f16taps64(x, l, m, h, prescale=True):
    """fp16(h * 2^s) against fp16(x), products and sums in f64, then * 2^-s.  prescale=False: the taps rounded as they
    are (a mutant for the tests: the small taps fall into fp16's subnormals)."""
    scale = f16_tap_scale(h) if prescale else 1.0
    with np.errstate(over="ignore"):
        h16 = (np.asarray(h, f32) * f32(scale)).astype(f32).astype(np.float16)
        x16 = np.asarray(x, f32).astype(np.float16)
    return resample64(x16.astype(f64), l, m, h16.astype(f64)) / scale


# ---- the acceptance rule

def error_figures(a, b):
    d = np.asarray(a, f64) - np.asarray(b, f64)
    return float(np.max(np.abs(d))), float(np.sqrt(np.mean(d * d)))


def accept(F_got, F_pred, F_oracle, F64, margin):
    """(passed, max ratio, rms ratio): max |F_got - F_pred| <= margin * max |F_oracle - F64|, and the same for the rms.
    The yardstick is the strict oracle's own f32 rounding on the same input against the all-f64 chain — never the code
    under test.  NaN anywhere fails."""
    F_got, F_pred, F_oracle, F64 = (np.asarray(v, f64) for v in (F_got, F_pred, F_oracle, F64))
    assert F_got.shape == F_pred.shape == F_oracle.shape == F64.shape, (F_got.shape, F_pred.shape, F_oracle.shape, F64.shape)
    emax, erms = error_figures(F_got, F_pred)
    omax, orms = error_figures(F_oracle, F64)
    assert omax > 0 and orms > 0
    rmax, rrms = emax / omax, erms / orms
    ok = bool(rmax <= margin and rrms <= margin)  # (a NaN compares false)
    return ok, rmax, rrms
