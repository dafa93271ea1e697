"""numpy restatement of process()'s Histogram + false colour (test tooling): channel A equalised in CIE Lab.

Written from the reference (noaa_apt.rs:158-199, processing.rs:87-101, imageext.rs:50-95,124-143) and from the
published source of the `lab` crate 0.11.0 (Cargo.lock:991).  The crate is not built next to this project, so
this file restates it; it has not been checked against the crate itself.  Every operation is f32 and rounded on
its own; the powers are the C library's powf through ctypes (Rust's f32::powf calls the same function on
Linux), never np.power.

* limits: misc::percent(signal, 0.98) (after get_min / get_max, whose only error is the zero length);
* map_signal_u8 -> RGBA -> false colour over columns [86, 995) (np_color_model.false_color);
* channel A (columns 0..1040, every whole row, gray columns included): Lab::from_rgb of every pixel,
  bin = `l as usize` (saturating), 101-bin histogram, inclusive cumulative sum cum,
  l' = 100f32 * (cum[bin] as f32 / cum[100] as f32), Lab{l', a, b}.to_rgb(), alpha 255;
* channel B: equalize_histogram_grayscale (np_color_model.equalize_lut);
* then the rotation.
"""
import ctypes as C
import ctypes.util

import numpy as np

import np_color_model as cm

f32 = np.float32
f64 = np.float64

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.powf.restype = C.c_float
_libm.powf.argtypes = [C.c_float, C.c_float]

KAPPA = f32(24389.0) / f32(27.0)
EPSILON = f32(216.0) / f32(24389.0)
CBRT_EPSILON = f32(6.0) / f32(29.0)
WHITE_X = f32(0.9504492182750991)
WHITE_Z = f32(1.0889166484304715)
S_0 = f32(0.003130668442500564)
THIRD = f32(1.0) / f32(3.0)
INV_GAMMA = f32(1.0) / f32(2.4)

M_RGB_XYZ = [[f32(0.4124564390896921), f32(0.357576077643909), f32(0.18043748326639894)],
             [f32(0.21267285140562248), f32(0.715152155287818), f32(0.07217499330655958)],
             [f32(0.019333895582329317), f32(0.119192025881303), f32(0.9503040785363677)]]
M_XYZ_RGB = [[f32(3.2404541621141054), f32(1.5371385127977166), f32(0.4985314095560162)],
             [f32(-0.9692660305051868), f32(1.8760108454466942), f32(0.04155601753034984)],
             [f32(0.05564343095911469), f32(0.20402591351675387), f32(1.0572251882231791)]]


def powf(x, y):
    """Element-wise C powf of a float32 array and one float32 exponent."""
    x = np.asarray(x, f32)
    out = np.empty(x.shape, f32)
    flat, o = x.ravel(), out.reshape(-1)
    yy = float(y)
    for i in range(flat.size):
        o[i] = _libm.powf(float(flat[i]), yy)
    return out


def _lin_table():
    """rgb_to_xyz_map of the 256 channel values."""
    c = np.arange(256, dtype=f32)
    a, d, d_low = f32(0.055) * f32(255.0), f32(1.055) * f32(255.0), f32(12.92) * f32(255.0)
    hi = c > f32(10.0)
    out = c / d_low
    out[hi] = powf((c[hi] + a) / d, f32(2.4))
    return out


_LIN = None


def _f(t):
    """xyz_to_lab_map"""
    t = np.asarray(t, f32)
    out = (KAPPA * t + f32(16.0)) / f32(116.0)
    m = t > EPSILON
    out[m] = powf(t[m], THIRD)
    return out


def from_rgb(rgb):
    """Lab::from_rgb: (..., 3) uint8 -> (..., 3) float32."""
    global _LIN
    if _LIN is None:
        _LIN = _lin_table()
    rgb = np.asarray(rgb, np.uint8)
    r, g, b = (_LIN[rgb[..., k]] for k in range(3))
    (xr, xg, xb), (yr, yg, yb), (zr, zg, zb) = M_RGB_XYZ
    x = (r * xr + g * xg) + b * xb
    y = (r * yr + g * yg) + b * yb
    z = (r * zr + g * zg) + b * zb
    fx, fy, fz = _f(x / WHITE_X), _f(y), _f(z / WHITE_Z)
    return np.stack([f32(116.0) * fy - f32(16.0), f32(500.0) * (fx - fy), f32(200.0) * (fy - fz)], -1).astype(f32)


def to_linear(lab):
    """Lab::to_rgb up to xyz_to_rgb_map's argument: (..., 3) float32 -> linear r, g, b (..., 3) float32."""
    lab = np.asarray(lab, f32)
    l, a, b = lab[..., 0], lab[..., 1], lab[..., 2]
    with np.errstate(all="ignore"):
        fy = (l + f32(16.0)) / f32(116.0)
        fx = a / f32(500.0) + fy
        fz = fy - b / f32(200.0)
        xr = np.where(fx > CBRT_EPSILON, (fx * fx) * fx, (fx * f32(116.0) - f32(16.0)) / KAPPA)
        yr = np.where(l > EPSILON * KAPPA, (fy * fy) * fy, l / KAPPA)
        zr = np.where(fz > CBRT_EPSILON, (fz * fz) * fz, (fz * f32(116.0) - f32(16.0)) / KAPPA)
        x, y, z = xr * WHITE_X, yr, zr * WHITE_Z
        (rx, ry, rz), (gx, gy, gz), (bx, by, bz) = M_XYZ_RGB
        r = (x * rx - y * ry) - z * rz
        g = (x * gx + y * gy) + z * gz
        bb = (x * bx - y * by) + z * bz
    return np.stack([r, g, bb], -1).astype(f32)


def quantise(c):
    """xyz_to_rgb_map's companding, * 255, round (half away from zero), clamp, `as u8`; powf called directly."""
    c = np.asarray(c, f32)
    with np.errstate(all="ignore"):
        v = c * f32(12.92)
        m = c > S_0
        v[m] = f32(1.055) * powf(c[m], INV_GAMMA) - f32(0.055)
        s = (v * f32(255.0)).astype(f64)
        r = np.copysign(np.floor(np.abs(s) + 0.5), s)  # exact: |s| < 2^9 has spare bits in f64
        r = np.where(np.isnan(r), 0.0, np.clip(r, 0.0, 255.0))
    return r.astype(np.uint8)


def to_rgb(lab):
    """Lab::to_rgb: (..., 3) float32 -> (..., 3) uint8."""
    return quantise(to_linear(lab))


def l_bin(l):
    """`l as usize`: negative and NaN saturate to 0; the reference indexes a [u32; 101] with it."""
    l = np.asarray(l, f32)
    with np.errstate(invalid="ignore"):
        b = np.where(l > 0, np.floor(np.where(np.isnan(l), 0, l)), 0).astype(np.int64)
    assert b.size == 0 or b.max() <= 100, "the reference would panic: L > 100"
    return b


def equalize_color(rgba_half):
    """equalize_histogram_color of one (h, w, 4) RGBA sub-image (alpha kept)."""
    out = rgba_half.copy()
    if rgba_half.shape[0] == 0:
        return out
    rgb = rgba_half[..., :3].reshape(-1, 3)
    packed = rgb[:, 0].astype(np.uint32) | (rgb[:, 1].astype(np.uint32) << 8) | (rgb[:, 2].astype(np.uint32) << 16)
    uniq, first, inv = np.unique(packed, return_index=True, return_inverse=True)
    lab = from_rgb(rgb[first])  # per distinct colour: Lab::from_rgb depends on the colour only
    bins = l_bin(lab[:, 0])
    hist = np.bincount(bins[inv], minlength=101).astype(np.uint64)
    cum = np.cumsum(hist).astype(np.uint32)
    total = cum[100].astype(f32)
    with np.errstate(all="ignore"):
        lp = f32(100.0) * (cum.astype(f32) / total)
    new = to_rgb(np.stack([lp[bins], lab[:, 1], lab[:, 2]], -1).astype(f32))
    out[..., :3] = new[inv].reshape(rgba_half.shape[:2] + (3,))
    return out


def process(signal, rotated=False, palette=None, tune=(0.0, 0.0, 0.0, 0.0)):
    """The model of aptgpu_process_image with APTGPU_CONTRAST_HISTOGRAM, false colour and
    APTGPU_COLOR_EQUALIZE_LAB.  Returns (image (h, 2080, 4), low, high)."""
    from oracle import image_binding as oi
    signal = np.asarray(signal, f32)
    gray, lo, hi = oi.process_gray(signal, oi.CONTRAST_PERCENT, 0.98)
    h = signal.size // cm.PX
    gray = gray[:h * cm.PX].reshape(h, cm.PX)
    img = cm.false_color(gray, palette, *tune)
    if h:
        img[:, :cm.HALF] = equalize_color(img[:, :cm.HALF])
        gb = gray[:, cm.HALF:]
        img[:, cm.HALF:, :3] = cm.equalize_lut(gb)[gb][..., None]
    if rotated:
        img = cm.rotate(img)
    return img, lo, hi
