"""numpy restatement of process()'s colour layer (test tooling), written from the reference:

* histogram equalisation of a gray image, each channel half on its own (processing.rs:83-101,
  imageext.rs:21-45,121-145): 256-bin u32 histogram of columns 0..1040 / 1040..2080 over every row,
  inclusive cumulative sum, v -> (255f32 * (cum[v] as f32 / cum[255] as f32)) as u8;
* false colour (processing.rs:113-165): over columns [86, 995) of every row, a = gray[y][x],
  b = gray[y][x + 1040], pixel = palette[tune_b][tune_a] (palette.get_pixel(x = a', y = b')), A = 255;
  tune(in) = (in * ((1 + e') - s') - s' * 255).clamp(0, 255) as u32 with s' = start * 0.3f, e' = end * 0.3f,
  each operation rounded to f32, NaN -> 0;
* the order map -> false colour -> equalisation -> rotate (noaa_apt.rs:166-231), on the RgbaImage of
  n / 2080 whole rows.

The gray image comes from the CPU oracle's process_gray (MinMax / Percent / Telemetry limits and map_signal_u8).
"""
import numpy as np

f32 = np.float32
PX = 2080
HALF = 1040
COLOR_START, COLOR_END = 86, 995  # PX_SYNC_FRAME + PX_SPACE_DATA, + PX_CHANNEL_IMAGE_DATA


def equalize_lut(gray_half):
    """The 256-entry table equalize_histogram_grayscale applies to one half."""
    hist = np.bincount(np.asarray(gray_half, np.uint8).ravel(), minlength=256).astype(np.uint64)
    cum = np.cumsum(hist).astype(np.uint32)
    total = cum[255].astype(f32)
    fraction = cum.astype(f32) / total
    return (f32(255.0) * fraction).astype(np.uint8)


def equalize(gray):
    """(h, 2080) u8 -> (h, 2080) u8, both halves equalised on their own."""
    gray = np.asarray(gray, np.uint8)
    out = gray.copy()
    if gray.shape[0] == 0:
        return out
    for lo in (0, HALF):
        out[:, lo:lo + HALF] = equalize_lut(gray[:, lo:lo + HALF])[gray[:, lo:lo + HALF]]
    return out


def tune(values, start, end):
    """tune_input_values for one channel: u8 values -> u32 palette coordinates."""
    factor = f32(0.3)
    s = f32(start) * factor
    e = f32(end) * factor
    k = (f32(1.0) + e) - s
    o = s * f32(255.0)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.asarray(values).astype(f32) * k - o
        out = np.where(np.isnan(t), f32(0), np.clip(t, f32(0), f32(255)))
    return out.astype(np.uint32)


def rgba(gray):
    """DynamicImage::ImageLuma8(img).into_rgba8(): R = G = B = gray, A = 255."""
    gray = np.asarray(gray, np.uint8)
    out = np.empty(gray.shape + (4,), np.uint8)
    out[..., :3] = gray[..., None]
    out[..., 3] = 255
    return out


def false_color(gray, palette, a_start=0.0, a_end=0.0, b_start=0.0, b_end=0.0):
    """(h, 2080) u8 gray, (256, 256, 3) palette indexed [b, a] -> (h, 2080, 4) RGBA."""
    img = rgba(gray)
    a = gray[:, COLOR_START:COLOR_END]
    b = gray[:, COLOR_START + HALF:COLOR_END + HALF]
    ta, tb = tune(a, a_start, a_end), tune(b, b_start, b_end)
    img[:, COLOR_START:COLOR_END, :3] = np.asarray(palette, np.uint8)[tb, ta]
    return img


def rotate(img):
    """processing::rotate: both 909-px channel images turned by 180 degrees (gray or RGBA)."""
    out = img.copy()
    for base in (COLOR_START, COLOR_START + HALF):
        out[:, base:base + 909] = img[::-1, base:base + 909][:, ::-1]
    return out


CONTRAST_KIND = {"telemetry": 0, "percent": 1, "minmax": 2, "histogram": 2}


def process(signal, contrast, percent=0.98, rotated=False, color=None, channels=None):
    """The model of aptgpu_process_image.  contrast: "telemetry" | "percent" | "minmax" | "histogram";
    color: None or (palette, a_start, a_end, b_start, b_end).  Returns (image, low, high)."""
    from oracle import image_binding as oi
    assert not (color is not None and contrast == "histogram"), "refused: equalisation in CIE Lab"
    channels = channels or (4 if color is not None else 1)
    signal = np.asarray(signal, f32)
    gray, lo, hi = oi.process_gray(signal, CONTRAST_KIND[contrast], percent)
    h = signal.size // PX
    gray = gray[:h * PX].reshape(h, PX)
    if color is not None:
        img = false_color(gray, *color)
    elif contrast == "histogram":
        img = equalize(gray)
    else:
        img = gray
    if channels == 4 and img.ndim == 2:
        img = rgba(img)
    if rotated:
        img = rotate(img)
    return img, lo, hi
