"""A restatement of the reprojection for the tests: process()'s swath image resampled onto a north-up
equirectangular or Mercator grid through the reference's own latlon_to_rel_px (np_map_model.rel_px, map.rs:71-100).

Steps 1-5 of the contract, with Python's `math` (glibc's libm):
  1. grid -> (lat, lon): lon = (lon_west + j step) / 180 PI; lat = (lat_north - i step) / 180 PI, or for Mercator
     atan(sinh(Y_north - i step_rad)) with Y_north = asinh(tan(lat_north rad))
  2. (x, y) = rel_px(lat, lon); x -= xoff[est_row(y, h)]
  3. valid: finite, -456 < x < 456, 0 < y < h, and the unclamped distance(latlon, start) < PI / 3
  4. NEAREST at floor(x + 0.5), floor(y + 0.5) or BILINEAR in f64, neighbours clamped to x in [-455, 455],
     y in [0, h - 1]; channel A at x + 539, B at x + 1579
  5. the graticule, blended once with np_map_model.blend

Margins, as §12's model: for every output pixel the smallest distance of any rounding decision from its boundary --
the band edges, y against integers (est_row) and for NEAREST x + 0.5, y + 0.5 against integers, in px; the PI / 3
test in rad; for BILINEAR each channel's unrounded v against k + 0.5 in levels, divided by 2 * 255 (a coordinate
error of tau moves v by at most 2 * 255 * tau).  Pixels within NEAR_START of the track's first point get margin 0.
The GPU image must equal this model bit for bit on every pixel whose margin is >= TAU.
"""
import math

import numpy as np

from np_map_model import NEAR_START, PI, PX_PER_ROW, TAU, Scalars, blend, distance, est_row, rel_px  # noqa: F401

EQUIRECTANGULAR, MERCATOR = 0, 1
CHANNEL_A, CHANNEL_B = 0, 1
NEAREST, BILINEAR = 0, 1
MAX_PIXELS = 1 << 26


def rad(deg):
    return deg / 180.0 * PI


def y_north(lat_north):
    return math.asinh(math.tan(rad(lat_north)))


def row_lat(kind, lat_north, step, i):
    """Latitude in rad of output row i."""
    if kind == MERCATOR:
        return math.atan(math.sinh(y_north(lat_north) - i * rad(step)))
    return rad(lat_north - i * step)


def col_lon(lon_west, step, j):
    return rad(lon_west + j * step)


def graticule(kind, width, height, lat_north, lon_west, step, grid_deg):
    """(column flags, row flags) of the output columns / rows nearest to each multiple of grid_deg."""
    cols, rows = np.zeros(width, bool), np.zeros(height, bool)
    if not grid_deg > 0.0:
        return cols, rows
    lon_east = lon_west + float(width - 1) * step
    m = math.floor(lon_west / grid_deg) - 1.0
    while m <= math.ceil(lon_east / grid_deg) + 1.0:
        c = math.floor((m * grid_deg - lon_west) / step + 0.5)
        if 0.0 <= c < width:
            cols[int(c)] = True
        m += 1.0
    n1 = math.floor(90.0 / grid_deg)
    m = -n1
    while m <= n1:
        lat = m * grid_deg
        if abs(lat) < 90.0:
            if kind == MERCATOR:
                r = math.floor((y_north(lat_north) - math.asinh(math.tan(rad(lat)))) / rad(step) + 0.5)
            else:
                r = math.floor((lat_north - lat) / step + 0.5)
            if 0.0 <= r < height:
                rows[int(r)] = True
        m += 1.0
    return cols, rows


def _near_int(v):
    return abs(v - math.floor(v + 0.5))


def _near_half(v):
    return abs(v - (math.floor(v) + 0.5))


def locate(sc, xoff, h, lat, lon):
    """Steps 2 and 3 for one point: (x, y, valid, margin, dist)."""
    ll = (lat, lon)
    x, y = rel_px(sc, ll)
    d = distance(ll, sc.start)
    if not (math.isfinite(x) and math.isfinite(y)):
        return x, y, False, math.inf, d
    m = abs(d - PI / 3.0)
    if 0.0 <= y <= h - 1:
        m = min(m, _near_int(y))
    else:
        m = min(m, abs(y), abs(y - (h - 1)))
    x -= xoff[est_row(y, h)]
    if not math.isfinite(x):
        return x, y, False, m, d
    m = min(m, abs(x + 456.0), abs(456.0 - x), abs(y), abs(h - y))
    if d < NEAR_START:
        m = 0.0
    valid = -456.0 < x < 456.0 and 0.0 < y < float(h) and d < PI / 3.0
    return x, y, valid, m, d


def _rgba(img):
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:  # a gray source reads as (g, g, g, 255)
        img = np.concatenate([np.repeat(img[:, :, None], 3, axis=2), np.full(img.shape + (1,), 255, np.uint8)], axis=2)
    return img


def project(img, positions, kind, width, height, lat_north, lon_west, step, channel=CHANNEL_A, sampling=NEAREST,
            grid_deg=0.0, grid_color=(255, 255, 255, 255), yaw=0.0, hscale=1.0, vscale=1.0):
    """The projected (height, width, 4) image of the unrotated swath `img` ((h, 2080) gray or (h, 2080, 4) RGBA) with
    its track `positions` (h pairs lat, lon in rad).  Returns (image, margin, info): margin is the (height, width)
    f64 array of decision margins, info holds the valid mask, the source coordinates and the excused count."""
    src = _rgba(img)
    h = src.shape[0]
    track = [(float(a), float(b)) for a, b in positions]
    assert len(track) == h
    sc = Scalars(track, yaw, hscale, vscale)
    xoff = [rel_px(sc, p)[0] for p in track]
    base = 1579 if channel == CHANNEL_B else 539
    out = np.zeros((height, width, 4), np.uint8)
    margin = np.full((height, width), math.inf)
    valid = np.zeros((height, width), bool)
    xs = np.full((height, width), np.nan)
    ys = np.full((height, width), np.nan)
    lons = [col_lon(lon_west, step, float(j)) for j in range(width)]

    def px(xi, yi):
        xi = min(max(xi, -455), 455)
        yi = min(max(yi, 0), h - 1)
        return src[yi, xi + base]

    for i in range(height):
        lat = row_lat(kind, lat_north, step, float(i))
        for j in range(width):
            x, y, ok, m, _ = locate(sc, xoff, h, lat, lons[j])
            xs[i, j], ys[i, j] = x, y
            if ok:
                if sampling == BILINEAR:
                    x0, y0 = math.floor(x), math.floor(y)
                    fx, fy = x - x0, y - y0
                    p00, p10 = px(int(x0), int(y0)), px(int(x0) + 1, int(y0))
                    p01, p11 = px(int(x0), int(y0) + 1), px(int(x0) + 1, int(y0) + 1)
                    for c in range(4):
                        v = (float(p00[c]) * (1.0 - fx) + float(p10[c]) * fx) * (1.0 - fy) + \
                            (float(p01[c]) * (1.0 - fx) + float(p11[c]) * fx) * fy
                        out[i, j, c] = int(math.floor(v + 0.5))
                        m = min(m, _near_half(v) / (2.0 * 255.0))
                else:
                    m = min(m, _near_half(x), _near_half(y))
                    out[i, j] = px(int(math.floor(x + 0.5)), int(math.floor(y + 0.5)))
            valid[i, j] = ok
            margin[i, j] = m
    cols, rows = graticule(kind, width, height, lat_north, lon_west, step, grid_deg)
    if cols.any() or rows.any():
        fg = tuple(int(v) for v in grid_color)
        for i, j in zip(*np.nonzero(rows[:, None] | cols[None, :])):
            out[i, j] = blend(tuple(int(v) for v in out[i, j]), fg)
    excused = margin < TAU
    return out, margin, {"valid": valid, "x": xs, "y": ys, "excused": int(np.count_nonzero(excused)),
                         "n_valid": int(np.count_nonzero(valid)), "graticule": (cols, rows)}


def compare(gpu, model, margin):
    """The parity contract: (differing pixels with margin >= TAU, differing pixels below it)."""
    diff = np.any(np.asarray(gpu) != np.asarray(model), axis=-1)
    low = margin < TAU
    return int(np.count_nonzero(diff & ~low)), int(np.count_nonzero(diff & low))


def fit(positions, kind, step=None, max_width=None, hscale=1.0):
    """aptgpu_projection_fit restated: dict(kind, width, height, lat_north, lon_west, step)."""
    pos = [(float(a), float(b)) for a, b in positions]
    lat_min = lat_max = pos[0][0]
    lon = lon_min = lon_max = pos[0][1]
    abs_max = abs(pos[0][0])
    for r in range(1, len(pos)):
        d = math.fmod(pos[r][1] - pos[r - 1][1], 2.0 * PI)
        if d > PI:
            d -= 2.0 * PI
        if d < -PI:
            d += 2.0 * PI
        lon += d
        lat_min, lat_max = min(lat_min, pos[r][0]), max(lat_max, pos[r][0])
        lon_min, lon_max = min(lon_min, lon), max(lon_max, lon)
        abs_max = max(abs_max, abs(pos[r][0]))
    half = 456.0 * 0.0005 / hscale
    cap_deg = 85.0 if kind == MERCATOR else 90.0
    lat_cap = cap_deg / 180.0 * PI
    lat_min = max(lat_min - half, -lat_cap)
    lat_max = min(lat_max + half, lat_cap)
    if lat_min > lat_max:
        lat_min = lat_max
    c = math.cos(abs_max)
    grow = half / c if c > 0.0 else 2.0 * PI
    lon_min -= grow
    lon_max += grow
    if not lon_max - lon_min <= 2.0 * PI:
        mid = 0.5 * (lon_min + lon_max)
        lon_min, lon_max = mid - PI, mid + PI
    span = (lon_max - lon_min) * 180.0 / PI
    st = float(step) if step else span / float(max_width - 1)
    north, south = min(lat_max * 180.0 / PI, cap_deg), max(lat_min * 180.0 / PI, -cap_deg)
    width = math.floor(span / st + 0.5) + 1.0
    if kind == MERCATOR:
        rows = math.floor((math.asinh(math.tan(rad(north))) - math.asinh(math.tan(rad(south)))) / rad(st) + 0.5) + 1.0
    else:
        rows = math.floor((north - south) / st) + 1.0
    return {"kind": kind, "width": int(width), "height": int(rows), "lat_north": north,
            "lon_west": lon_min * 180.0 / PI, "step": st}
