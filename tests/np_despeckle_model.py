"""numpy statement of the despeckle stage (aptgpu_despeckle; test tooling): a band-aware median of
the decoded f32 rows, in front of process().  The reference has no such stage (docs/development.md:139 only names
it), so this file is the definition the host code and the kernel are held to, bit for bit.

* Shape.  h = n // 2080 whole rows; the samples past h * 2080 are copied bit for bit.  h == 0: the output is the
  input, replaced = 0, no limits are computed.
* Bands.  Eight column bands per row, [0,39) [39,86) [86,995) [995,1040) and the same + 1040: sync, space, video
  and telemetry of channels A and B.  A window never leaves its band.
* Window.  Radius r in {1, 2}; the window of pixel (y, x) in band [b0, b1) is the (2r+1)^2 samples at rows
  clamp(y + dy, 0, h - 1) and columns clamp(x + dx, b0, b1 - 1): edges are replicated, the size is constant.
* Median.  Samples are ordered by IEEE totalOrder on their bits (key = bits ^ (0xFFFFFFFF if sign else 0x80000000)
  as u32, np_eqfloat_model.keys); med is the element of rank (2r+1)^2 // 2 (0-based), returned with its own bits.
* Decision.  out = med if med is not NaN and not (|x - med| <= t), else x: one f32 subtraction, one comparison.
* Threshold.  threshold == 0: t = 0 and no limits pass.  Otherwise (low, high) = misc::percent(signal, 0.98) of
  the whole unfiltered signal (misc.rs:119-175, what Contrast.Percent(0.98) reports) and t = threshold * (high - low)
  in f32.
* Count.  replaced = the samples for which the rule picked med (also where med's bits equal x's).
"""
import numpy as np

from np_eqfloat_model import keys

f32 = np.float32
PX = 2080
BANDS = tuple((lo + off, hi + off) for off in (0, 1040) for lo, hi in ((0, 39), (39, 86), (86, 995), (995, 1040)))


class LimitsError(Exception):
    """misc::percent found no low bucket (misc.rs:172 panics there): aptgpu_image_result reason 3."""


def unkeys(k):
    """The inverse of keys(): u32 keys -> f32 with the original bits."""
    k = np.ascontiguousarray(k, np.uint32)
    return (k ^ np.where(k >> np.uint32(31), np.uint32(0x80000000), np.uint32(0xFFFFFFFF)).astype(np.uint32)).view(f32)


def _extreme(x, want_max):
    """dsp::get_max / get_min (dsp.rs:20-54): best = x[0], replaced on a strict comparison only, so a NaN first
    element stays, later NaNs never win, and of equal values (+0 / -0) the first one is kept."""
    if np.isnan(x[0]):
        return x[0]
    best = (np.fmax if want_max else np.fmin).reduce(x)
    if best == 0:
        best = x[np.flatnonzero(x == 0)[0]]
    return f32(best)


def percent(signal, p=0.98):
    """misc::percent (misc.rs:119-175) in f32, every operation rounded on its own: (low, high)."""
    x = np.ascontiguousarray(signal, f32).ravel()
    assert x.size > 0
    remainder = (f32(1.0) - f32(p)) / f32(2.0)
    mn, mx = _extreme(x, False), _extreme(x, True)
    with np.errstate(all="ignore"):
        total_range = f32(mx - mn)
        t = np.trunc((x - mn) / total_range * f32(1000.0))
        b = np.where(t > 0, np.minimum(t, f32(999.0)), f32(0.0)).astype(np.int64)  # `as usize`, .min(999)
        frac = np.cumsum(np.bincount(b, minlength=1000)).astype(np.uint32).astype(f32) / f32(x.size)
        low_bucket = high_bucket = None
        for i in range(1000):
            if low_bucket is None and frac[i] > remainder:
                low_bucket = i
            elif high_bucket is None and frac[i] > f32(1.0) - remainder:
                high_bucket = i
        if high_bucket is None:
            high_bucket = 999
        if low_bucket is None:
            raise LimitsError("no low bucket")
        return (f32(f32(low_bucket) / f32(1000.0) * total_range + mn),
                f32(f32(high_bucket) / f32(1000.0) * total_range + mn))


def median(rows, r):
    """(h, 2080) f32 -> the band-aware window median of every pixel, with its own bits."""
    x = np.ascontiguousarray(rows, f32)
    h = x.shape[0]
    k = keys(x).reshape(h, PX)
    ys = np.arange(h)
    out = np.empty((h, PX), np.uint32)
    for b0, b1 in BANDS:
        xs = np.arange(b0, b1)
        win = [k[np.clip(ys + dy, 0, h - 1)][:, np.clip(xs + dx, b0, b1 - 1)]
               for dy in range(-r, r + 1) for dx in range(-r, r + 1)]
        out[:, b0:b1] = np.sort(np.stack(win, axis=-1), axis=-1)[..., len(win) // 2]
    return unkeys(out).reshape(h, PX)


def despeckle(signal, r, threshold):
    """The definition: (out, replaced, low, high, t).  Raises LimitsError where the limits cannot be computed."""
    assert r in (1, 2) and threshold >= 0
    x = np.ascontiguousarray(signal, f32).ravel()
    h = x.size // PX
    out = x.copy()
    low = high = t = f32(0.0)
    if h == 0:
        return out, 0, low, high, t
    if f32(threshold) != 0:
        low, high = percent(x, 0.98)
        with np.errstate(all="ignore"):
            t = f32(f32(threshold) * f32(high - low))
    img = x[:h * PX].reshape(h, PX)
    med = median(img, r)
    with np.errstate(all="ignore"):
        take = ~np.isnan(med) & ~(np.abs(img - med) <= t)
    out[:h * PX] = np.where(take, med, img).view(np.uint32).ravel().view(f32)
    return out, int(take.sum()), low, high, t


# ------------------------------------------------------------------ the input families of the tests
def noisy_image(h, seed, scale=80.0, sigma=160.0, impulses=0.01):
    """The project's synthetic frame (noaa_apt_amd.testing.synth.make_image) * scale + N(0, sigma), with a fraction
    of the samples set to 0 or 32767: (clean, noisy, mask)."""
    from noaa_apt_amd.testing.synth import make_image
    rng = np.random.default_rng([seed, h, 7])
    clean = (make_image(h, seed) * f32(scale)).astype(f32)
    noisy = (clean + rng.normal(0.0, sigma, clean.shape).astype(f32)).astype(f32)
    mask = rng.random(clean.shape) < impulses
    noisy[mask] = np.where(rng.random(int(mask.sum())) < 0.5, f32(0.0), f32(32767.0))
    return clean, noisy, mask


def family(name, h, seed=0, extra=0):
    """h * 2080 + extra f32 samples."""
    rng = np.random.default_rng([seed, h, sum(name.encode())])
    n = h * PX + extra
    if name == "normal":
        return rng.standard_normal(n).astype(f32)
    if name == "image":
        x = np.empty(n, f32)
        x[:h * PX] = noisy_image(h, seed)[1].ravel() if h else 0
        x[h * PX:] = 1e9
        return x
    if name == "special":  # +-NaN, +-Inf, +-0 sprinkled over noise
        bits = np.array([0x7FC00000, 0xFFC00000, 0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x00000000,
                         0x80000000], np.uint32)
        x = rng.standard_normal(n).astype(f32)
        m = rng.random(n) < 0.2
        x[m] = bits[rng.integers(0, bits.size, int(m.sum()))].view(f32)
        if n:
            x[0] = 0.25  # (a NaN first sample would make the limits NaN: that case has its own test)
        return x
    if name == "equal":
        return np.full(n, 1234.5, f32)
    raise KeyError(name)


FAMILIES = ("normal", "image", "special", "equal")
