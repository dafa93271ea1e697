"""A restatement of the reference's map overlay (src/map.rs:59-200) for the tests.

It restates map.rs, geo.rs (`distance`, `azimuth`), the `XiaolinWu<f64, i32>` iterator of line_drawing 1.0.0 and
`Rgba<u8>::blend` of image 0.24.7 (Cargo.lock:921,1026) from the crates' published source.  The crates are not
available here, so this model has not been run against the crates themselves.

Scalar f64 math uses Python's `math` module, i.e. the C library's libm, which is what Rust's f64::sin & co. call on
Linux.  The blend uses numpy float32 scalars, one rounding per operation, as the crate's f32 code.

The overlay takes any RGBA image as it stands before the overlay (process() with the same contrast and colour and
no rotation); the tests use the GPU's own pre-overlay image, which tests/test_gpu_process_image.py and
tests/test_gpu_lab_equalize.py pin to np_color_model.py / np_lab_model.py.

Margins.  The device evaluates sin/cos/tan/atan/asin/acos/atan2 with its own library, which may
differ from glibc by an ulp; that can only move a pixel where a rounding decision lies close to its boundary.  For
every segment the model returns the smallest distance, in pixels, of any such decision from its boundary: the
`round` of both walk ends, the i32 truncation / floor of y at every step inside the band, `(value * a) as u8`
(divided by a), the point-1 cull tests, `est_y`, and the steep / swap comparisons.  A segment with a vertex closer
than NEAR_START rad to the track's first point gets margin 0: `geo::distance` is an acos of a value near 1 there
(geo.rs:128, "less precise for small angles").
"""
import math

import numpy as np

PI = math.pi
PX_PER_ROW = 2080
MAX_WALK = 1 << 20          # APTGPU_MAP_MAX_WALK
MAX_FRAGMENTS = 1 << 21     # APTGPU_MAP_MAX_FRAGMENTS
MAX_PIXEL_FRAGMENTS = 1 << 16  # APTGPU_MAP_MAX_PIXEL_FRAGMENTS
TAU = 1e-6                  # the parity threshold in pixels
NEAR_START = 1e-3           # rad: vertices closer to sat_positions[0] get margin 0
DEFAULT_COLORS = {"states": (255, 255, 0, 150), "countries": (255, 255, 0, 255), "lakes": (50, 200, 200, 255)}
LAYER_ORDER = ("states", "countries", "lakes")


class WalkError(Exception):
    """A walk the device refuses (APTGPU_MAP_REASON_WALK): longer than MAX_WALK steps or with a non-finite end."""


def _div(a, b):
    """IEEE f64 division (Python raises on / 0)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(a) / np.float64(b))


def fmax(a, b):  # f64::max: NaN is ignored
    if math.isnan(a):
        return b
    if math.isnan(b):
        return a
    return a if a > b else b


def fmin(a, b):
    if math.isnan(a):
        return b
    if math.isnan(b):
        return a
    return a if a < b else b


def distance(p1, p2):
    """geo.rs:34-46"""
    (lat1, lon1), (lat2, lon2) = p1, p2
    delta_lon = lon2 - lon1
    c = math.sin(lat1) * math.sin(lat2) + math.cos(lat1) * math.cos(lat2) * math.cos(delta_lon)
    c = fmin(fmax(c, -1.0), 1.0)
    return math.acos(c)


def azimuth(p1, p2):
    """geo.rs:54-62"""
    (lat1, lon1), (lat2, lon2) = p1, p2
    delta_lon = lon2 - lon1
    return math.atan2(math.sin(delta_lon), math.cos(lat1) * math.tan(lat2) - math.sin(lat1) * math.cos(delta_lon))


class Scalars:
    """map.rs:59-69 from sat_positions (height pairs of lat, lon in rad)."""

    def __init__(self, positions, yaw=0.0, hscale=1.0, vscale=1.0):
        positions = [(float(a), float(b)) for a, b in positions]
        height = len(positions)
        self.start, self.end = positions[0], positions[-1]
        self.y_res = _div(distance(self.start, self.end) / float(height), vscale)
        self.x_res = _div(0.0005, hscale)
        self.ref_az = azimuth(self.start, self.end)
        self.yaw = yaw


def rel_px(sc, latlon):
    """latlon_to_rel_px, map.rs:71-100."""
    az = azimuth(sc.start, latlon)
    B = az - sc.ref_az
    c = fmin(fmax(distance(latlon, sc.start), -PI / 3.0), PI / 3.0)
    a = math.atan(math.cos(B) * math.tan(c))
    b = math.asin(math.sin(B) * math.sin(c))
    x = _div(-b, sc.x_res)
    y = _div(a, sc.y_res) + sc.yaw * x
    return x, y


def est_row(y, height):
    """(y.max(0.) as usize).min(height - 1): the cast saturates, NaN -> 0."""
    m = fmax(y, 0.0)
    if m >= height - 1:
        return height - 1
    return int(m)


def _trunc_i32(v):
    return int(v)  # toward zero, as NumCast


def xiaolin_wu(start, end, stop=None):
    """line_drawing 1.0.0's XiaolinWu<f64, i32>::new(start, end): yields ((x, y), value).

    stop: (steep-independent) callable major -> bool that ends the walk early once nothing later can be drawn
    (the device's early exit; it changes no yielded point before it).  Raises WalkError where the device does."""
    (sx, sy), (ex, ey) = start, end
    if not all(math.isfinite(v) for v in (sx, sy, ex, ey)):
        raise WalkError("non-finite end")
    steep = abs(ey - sy) > abs(ex - sx)
    if steep:
        sx, sy, ex, ey = sy, sx, ey, ex
    if sx > ex:
        sx, sy, ex, ey = ex, ey, sx, sy
    dx = ex - sx
    if not dx <= MAX_WALK:
        raise WalkError("walk longer than MAX_WALK")
    gradient = 1.0 if dx == 0.0 else (ey - sy) / dx
    x = _trunc_i32(_round(sx))
    end_x = _trunc_i32(_round(ex))
    y = sy
    lower = False
    while x <= end_x:
        if stop is not None and stop(steep, x):
            return
        ycur = y
        fpart = y - math.floor(y)
        yi = _trunc_i32(y)
        if lower:
            yi += 1
        point = (yi, x) if steep else (x, yi)
        if lower:
            lower = False
            x += 1
            y += gradient
            yield point, fpart, ycur, steep
        else:
            if fpart > 0.0:
                lower = True
            else:
                x += 1
                y += gradient
            yield point, 1.0 - fpart, ycur, steep


def _round(v):
    """f64::round: half away from zero."""
    r = math.floor(abs(v) + 0.5)
    # floor(|v| + 0.5) is exact for |v| < 2^52 except when |v| + 0.5 rounds up; fix that case
    if r - abs(v) > 0.5:
        r -= 1.0
    return math.copysign(r, v)


def xiaolin_points(start, end):
    """The plain iterator as a list of ((x, y), value) (tests)."""
    return [(p, v) for p, v, _, _ in xiaolin_wu(start, end)]


def alpha_u8(value, a):
    v = value * float(a)  # `as u8` saturates
    if not v > 0.0:
        return 0
    return 255 if v >= 255.0 else int(v)


_F255 = np.float32(255.0)


def blend(bg, fg):
    """image 0.24.7 Rgba<u8>::blend(&mut bg, &fg): f32 src-over with truncating casts and its alpha 0 / 255 fast
    paths.  bg, fg: 4 ints; returns 4 ints."""
    if fg[3] == 0:
        return tuple(bg)
    if fg[3] == 255:
        return tuple(fg)
    f32 = np.float32
    br, bgc, bb, ba = (f32(v) / _F255 for v in bg)
    fr, fgc, fb, fa = (f32(v) / _F255 for v in fg)
    af = ba + fa - ba * fa
    if af == f32(0.0):
        return tuple(bg)
    k = f32(1.0) - fa
    outs = [(fc * fa + (bc * ba) * k) / af for fc, bc in ((fr, br), (fgc, bgc), (fb, bb))]
    return tuple(int(_F255 * o) for o in outs) + (int(_F255 * af),)


def _near_int(v):
    return abs(v - round(v))


def _near_half(v):
    return abs(v - (math.floor(v) + 0.5))


class Segment:
    __slots__ = ("layer", "x1", "y1", "x2", "y2", "drawn", "margin", "pixels", "error")


def overlay(img, positions, layers, settings=None, colors=None, rotate=False):
    """map::draw_map on `img` ((h, 2080, 4) uint8, before the rotation; copied), then processing::rotate when
    `rotate`.  layers: {"states"|"countries"|"lakes": list of (n, 2) arrays of (lon°, lat°)}.  settings: dict with
    yaw / hscale / vscale.  colors: {layer: (r, g, b, a)} over DEFAULT_COLORS.  Returns (image, excused, info):
    excused is the (h, 2080) bool mask of the pixels that low-margin segments may change (dilated by one pixel), in
    the output's (rotated) coordinates; info holds the segments, the fragment count and the low-margin count.
    Raises WalkError or OverflowError where the device reports an error (reasons 6, and 5 or 8)."""
    settings = settings or {}
    colors = dict(DEFAULT_COLORS, **(colors or {}))
    img = np.array(img, dtype=np.uint8, copy=True)
    h = img.shape[0]
    sc = Scalars(positions, settings.get("yaw", 0.0), settings.get("hscale", 1.0), settings.get("vscale", 1.0))
    track = [(float(a), float(b)) for a, b in positions]
    xoff = [rel_px(sc, p)[0] for p in track]
    excused = np.zeros((h, PX_PER_ROW), bool)
    frags = []  # (x, y, alpha, color) in draw order
    segments = []
    stop = (lambda steep, major: major >= (h if steep else 456))
    for name in LAYER_ORDER:
        parts = layers.get(name)
        if parts is None:
            continue
        r, g, b, a = colors[name]
        for part in parts:
            part = np.asarray(part, np.float64).reshape(-1, 2)
            proj, near = [], []
            for lon, lat in part:
                ll = (float(lat) / 180.0 * PI, float(lon) / 180.0 * PI)
                proj.append(rel_px(sc, ll))
                near.append(distance(ll, sc.start) < NEAR_START)
            for j in range(len(part)):
                i2 = j - 1 if j > 0 else 0
                s = Segment()
                s.layer = name
                (x1, y1), (x2, y2) = proj[j], proj[i2]
                e1, e2 = est_row(y1, h), est_row(y2, h)
                x1 -= xoff[e1]
                x2 -= xoff[e2]
                s.x1, s.y1, s.x2, s.y2 = x1, y1, x2, y2
                m = math.inf
                for y, e in ((y1, e1), (y2, e2)):
                    if 0.0 <= y <= h - 1 and math.isfinite(y):
                        m = min(m, _near_int(y))
                    elif math.isfinite(y):
                        m = min(m, abs(y), abs(y - (h - 1)))
                for v in (x1 + 600.0, 600.0 - x1, y1, h - y1):
                    if math.isfinite(v):
                        m = min(m, abs(v))
                if near[j] or near[i2]:
                    m = 0.0
                s.drawn = x1 > -600.0 and x1 < 600.0 and y1 > 0.0 and y1 < float(h)
                s.pixels = []
                s.error = None
                if s.drawn or m < TAU:
                    if not (x1 == x2 and y1 == y2) and all(math.isfinite(v) for v in (x1, y1, x2, y2)):
                        m = min(m, abs(abs(y2 - y1) - abs(x2 - x1)), abs(x2 - x1), abs(y2 - y1))
                    try:
                        first = True
                        for (px, py), value, ycur, steep in xiaolin_wu((x1, y1), (x2, y2), stop):
                            if first:
                                st, en = ((y1, y2) if steep else (x1, x2))
                                m = min(m, _near_half(st), _near_half(en))
                                first = False
                            if px > -456 and px < 456 and py > 0 and py < h:
                                m = min(m, _near_int(ycur))
                                al = alpha_u8(value, a)
                                if a:
                                    m = min(m, _near_int(value * a) / a)
                                s.pixels.append((px, py))
                                if s.drawn:
                                    frags.append((px, py, al, (r, g, b)))
                    except WalkError as ex:
                        if s.drawn:
                            raise
                        s.error = ex
                s.margin = m
                segments.append(s)
    if len(frags) > MAX_FRAGMENTS:
        raise OverflowError("more than MAX_FRAGMENTS fragments")
    per_pixel = {}
    for px, py, _, _ in frags:
        per_pixel[(px, py)] = per_pixel.get((px, py), 0) + 1
    if per_pixel and max(per_pixel.values()) > MAX_PIXEL_FRAGMENTS:
        raise OverflowError("more than MAX_PIXEL_FRAGMENTS fragments on one pixel")
    for px, py, al, (r, g, b) in frags:
        for col in (px + 539, px + 1579):
            img[py, col] = blend(tuple(int(v) for v in img[py, col]), (r, g, b, al))
    for s in segments:
        if s.margin < TAU:
            for px, py in s.pixels:
                for col in (px + 539, px + 1579):
                    excused[max(py - 1, 0):py + 2, max(col - 1, 0):col + 2] = True
    if rotate:
        img = rotate_image(img)
        excused = rotate_image(excused)
    return img, excused, {"segments": segments, "fragments": len(frags),
                          "low_margin": sum(1 for s in segments if s.margin < TAU)}


def rotate_image(img):
    """processing::rotate (processing.rs:21-37): both channel sub-images [86, 995) and [1126, 2035) turn by 180°."""
    out = np.array(img, copy=True)
    for lo, hi in ((86, 995), (1126, 2035)):
        out[:, lo:hi] = img[::-1, lo:hi][:, ::-1]
    return out


def compare(gpu, model, excused):
    """The parity contract: every differing pixel must be excused.  Returns (n_diff_unexcused, n_diff_excused)."""
    diff = np.any(np.asarray(gpu) != np.asarray(model), axis=-1)
    return int(np.count_nonzero(diff & ~excused)), int(np.count_nonzero(diff & excused))


def great_circle_track(lat0_deg, lon0_deg, az_deg, rows, altitude_km=850.0, seconds_per_row=0.5):
    """A synthetic satellite ground track: rows positions along a great circle from (lat0, lon0) heading az, at the
    ground speed of a circular orbit of the given altitude (one row every 0.5 s).  Returns (rows, 2) lat, lon rad."""
    mu, re = 398600.4418, 6371.0
    rr = re + altitude_km
    omega = math.sqrt(mu / rr ** 3)  # rad/s of orbital angle = ground angle
    lat0, lon0, az = (math.radians(v) for v in (lat0_deg, lon0_deg, az_deg))
    out = np.empty((rows, 2))
    for i in range(rows):
        d = omega * seconds_per_row * i
        lat = math.asin(math.sin(lat0) * math.cos(d) + math.cos(lat0) * math.sin(d) * math.cos(az))
        lon = lon0 + math.atan2(math.sin(az) * math.sin(d) * math.cos(lat0),
                                math.cos(d) - math.sin(lat0) * math.sin(lat))
        out[i] = (lat, (lon + PI) % (2 * PI) - PI)
    return out
