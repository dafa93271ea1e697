"""numpy statement of Contrast.HISTOGRAM_FLOAT (APTGPU_CONTRAST_HISTOGRAM_FLOAT; test tooling): the
histogram equalisation of process()'s image on the f32 signal, before the pixel values become integers (the
reference's docs/development.md:105-106).

* The image is h = n // 2080 whole rows; its halves are columns [0, 1040) and [1040, 2080) (processing.rs:94-102),
  N = 1040 * h samples each.
* Samples are ordered by IEEE totalOrder on their bits: key = bits ^ (0xFFFFFFFF if sign else 0x80000000) as u32.
* cum(p) = samples of p's half with key <= key(p); out(p) = (255f32 * (cum as f32 / N as f32)) as u8
  (imageext.rs:33,38 with one bin per representable value).

`equalize` is the direct form (sort + searchsorted), `equalize_threshold` the form the kernels use: 255 order
statistics T_v per half and out(p) = #{v : key(p) >= T_v}.
"""
import numpy as np

f32 = np.float32
PX = 2080
HALF = 1040


def keys(x):
    """f32 -> u32 keys whose unsigned order is IEEE totalOrder."""
    b = np.ascontiguousarray(x, f32).view(np.uint32)
    return b ^ np.where(b >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000)).astype(np.uint32)


def level(c, n):
    """(255f32 * (c as f32 / n as f32)) as u8 for u32 c (array) and n."""
    c = np.asarray(c, np.uint32).astype(f32)
    return (f32(255.0) * (c / np.uint32(n).astype(f32))).astype(np.uint8)


def _rows(signal):
    x = np.ascontiguousarray(signal, f32).ravel()
    h = x.size // PX
    return x[:h * PX].reshape(h, PX), h


def equalize(signal):
    """The definition: (h, 2080) u8."""
    x, h = _rows(signal)
    out = np.zeros((h, PX), np.uint8)
    if h == 0:
        return out
    for lo in (0, HALF):
        k = keys(x[:, lo:lo + HALF])
        cum = np.searchsorted(np.sort(k.ravel()), k.ravel(), side="right").astype(np.uint32)
        out[:, lo:lo + HALF] = level(cum, k.size).reshape(h, HALF)
    return out


def ranks(n):
    """c_v for v = 1..255: the smallest c in [1, n] with level(c) >= v, by bisection over level() itself."""
    out = np.empty(255, np.uint32)
    for v in range(1, 256):
        lo, hi = 1, int(n)
        while lo < hi:
            mid = lo + (hi - lo) // 2
            if int(level(np.uint32(mid), n)) >= v:
                hi = mid
            else:
                lo = mid + 1
        out[v - 1] = lo
    return out


def thresholds(signal):
    """(2, 255) u32: T_v = the c_v-th smallest key of each half."""
    x, h = _rows(signal)
    assert h > 0
    c = ranks(HALF * h)
    return np.stack([np.sort(keys(x[:, lo:lo + HALF]).ravel())[c - 1] for lo in (0, HALF)])


def equalize_threshold(signal, t=None):
    """The threshold form: out(p) = #{v : key(p) >= T_v}."""
    x, h = _rows(signal)
    out = np.zeros((h, PX), np.uint8)
    if h == 0:
        return out
    t = thresholds(signal) if t is None else t
    for i, lo in enumerate((0, HALF)):
        k = keys(x[:, lo:lo + HALF])
        out[:, lo:lo + HALF] = np.searchsorted(t[i], k.ravel(), side="right").reshape(h, HALF).astype(np.uint8)
    return out


def process(signal, rotated=False, channels=1):
    """The model of aptgpu_process_image with the new contrast (no colour): equalise, RGBA, rotate."""
    import np_color_model as cm
    img = equalize(signal)
    if channels == 4:
        img = cm.rgba(img)
    return cm.rotate(img) if rotated else img


# ------------------------------------------------------------------ the input families of the tests
def family(name, h, seed=0, extra=0):
    """h * 2080 + extra f32 samples."""
    rng = np.random.default_rng([seed, h, sum(name.encode())])
    n = h * PX + extra
    if name == "normal":
        return rng.standard_normal(n).astype(f32)
    if name == "integers":  # 0 and 255 present in each half of the first row
        x = rng.integers(0, 256, n).astype(f32)
        x[[0, HALF]] = 0.0
        x[[1, HALF + 1]] = 255.0
        return x
    if name == "runs":  # runs of 52 equal samples
        return np.repeat(rng.standard_normal(n // 52 + 1).astype(f32), 52)[:n]
    if name == "special":
        bits = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7FC00001,
                         0xFFC12345, 0x7F800001, 0xFFFFFFFF, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,
                         0x3F800000, 0xBF800000, 0x3F800000, 0x7F7FFFFF, 0xFF7FFFFF], np.uint32)
        x = bits[rng.integers(0, bits.size, n)].view(f32).copy()
        m = rng.random(n) < 0.3
        x[m] = rng.standard_normal(int(m.sum())).astype(f32)
        return x
    if name == "ulps":  # 1.0f + k ulps, k < 1500: one level-1 bin, the last 10 bits decide
        return (np.uint32(0x3F800000) + rng.integers(0, 1500, n).astype(np.uint32)).view(f32).copy()
    raise KeyError(name)


FAMILIES = ("normal", "integers", "runs", "special", "ulps")
