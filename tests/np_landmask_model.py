"""The land / sea / lake mask and the map-coloured false colour in numpy (include/aptgpu.h, "land / sea / lake mask of
the swath"): the yardstick of test_landmask_cpu.py and test_gpu_landmask.py.

The library walks latitude bands.  This model has none: it sorts the points by latitude and, per edge, slices the points
with lo <= py < hi out of the sorted list (searchsorted), which is the straddle test, then applies the crossing rule to
the slice.  The count is an integer, so the two groupings must agree bit for bit.  brute() is the all-pairs evaluation
the sorted form was compared with."""
import numpy as np

DEG = 57.29577951308232
SEA, LAND, LAKE, INVALID = 0, 1, 2, 255
PX, VIDEO0, VIDEO_N, HALF = 2080, 86, 909, 1040
CHUNK = 1 << 22  # (point, edge) pairs evaluated at once
f32 = np.float32


def edges_of(parts):
    """(m, 4) x1, y1, x2, y2 of a layer given as a list of (n, 2) arrays of (lon, lat) degrees: consecutive pairs, and
    the closing edge of a part whose ends differ."""
    out = []
    for p in parts or ():
        p = np.asarray(p, np.float64).reshape(-1, 2)
        if len(p) >= 2:
            out.append(np.concatenate([p[:-1], p[1:]], axis=1))
        if len(p) and (p[0] != p[-1]).any():
            out.append(np.concatenate([p[-1:], p[:1]], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 4))


def _rule(e, px, py):
    """crossing of edges e (k, 4) at points (px, py) (k,), without the straddle test"""
    x1, y1, x2, y2 = e[:, 0], e[:, 1], e[:, 2], e[:, 3]
    d = (x2 - x1) * (py - y1) - (px - x1) * (y2 - y1)
    return np.where(y2 > y1, d > 0, d < 0)


def odd(edges, px, py):
    """parity of the crossing count of every point (px, py: finite or infinite, never NaN) against `edges`"""
    n = px.size
    if n == 0 or len(edges) == 0:
        return np.zeros(n, bool)
    order = np.argsort(py, kind="stable")
    ys, xs = py[order], px[order]
    lo, hi = np.minimum(edges[:, 1], edges[:, 3]), np.maximum(edges[:, 1], edges[:, 3])
    i0, i1 = np.searchsorted(ys, lo, "left"), np.searchsorted(ys, hi, "left")  # lo <= ys[i0:i1] < hi
    live = np.nonzero(i1 > i0)[0]
    count = np.zeros(n, np.int64)
    lens = (i1 - i0)[live]
    start = 0
    while start < live.size:
        stop = start + max(1, int(np.searchsorted(np.cumsum(lens[start:]), CHUNK, "right")))
        idx, ln = live[start:stop], lens[start:stop]
        e = np.repeat(idx, ln)
        first = np.repeat(np.cumsum(ln) - ln, ln)
        p = np.arange(e.size) - first + np.repeat(i0[idx], ln)
        hit = _rule(edges[e], xs[p], ys[p])
        count += np.bincount(p[hit], minlength=n)
        start = stop
    out = np.empty(n, bool)
    out[order] = (count & 1).astype(bool)
    return out


def brute(edges, px, py):
    """the same by all pairs, straddle test included (small inputs)"""
    x1, y1, x2, y2 = (edges[:, k][None, :] for k in range(4))
    px, py = px[:, None], py[:, None]
    straddle = (y1 > py) != (y2 > py)
    d = (x2 - x1) * (py - y1) - (px - x1) * (y2 - y1)
    cross = straddle & np.where(y2 > y1, d > 0, d < 0)
    return (cross.sum(axis=1) & 1).astype(bool)


def classify(latlon, countries, lakes, evaluate=odd):
    """(mask of latlon's shape without its last axis, (n_sea, n_land, n_lake, n_invalid)); countries / lakes: edge
    arrays from edges_of (None or empty: the layer is absent)"""
    ll = np.asarray(latlon, np.float64)
    lat, lon = ll[..., 0].ravel(), ll[..., 1].ravel()
    ok = ~(np.isnan(lat) | np.isnan(lon))
    py, px = lat[ok] * DEG, lon[ok] * DEG
    zero = np.zeros((0, 4))
    land = evaluate(countries if countries is not None else zero, px, py)
    lake = evaluate(lakes if lakes is not None else zero, px, py)
    mask = np.full(lat.size, INVALID, np.uint8)
    mask[ok] = np.where(lake, LAKE, np.where(land, LAND, SEA))
    return mask.reshape(ll.shape[:-1]), counts(mask)


def counts(mask):
    return tuple(int(np.count_nonzero(mask == c)) for c in (SEA, LAND, LAKE, INVALID))


def tune(v, start, end):
    """tune_input_values (processing.rs:126-140) in f32, one rounding per operation"""
    s, e = f32(start) * f32(0.3), f32(end) * f32(0.3)
    k, o = f32(f32(1) + e) - s, s * f32(255)
    t = (v.astype(f32) * k - o).astype(f32)
    return np.clip(t, f32(0), f32(255)).astype(np.uint32)


def false_color_masked(image, mask, palettes, tunes):
    """(h, 2080, 4) RGBA of an unrotated gray image (h, 2080) u8, a (h, 909) mask and three (256, 256, 3) palettes"""
    image = np.asarray(image, np.uint8)
    out = np.repeat(image[:, :, None], 4, axis=2)
    out[:, :, 3] = 255
    a = tune(image[:, VIDEO0:VIDEO0 + VIDEO_N], tunes[0], tunes[1])
    b = tune(image[:, HALF + VIDEO0:HALF + VIDEO0 + VIDEO_N], tunes[2], tunes[3])
    video = out[:, VIDEO0:VIDEO0 + VIDEO_N]
    for c in (SEA, LAND, LAKE):
        sel = mask == c
        video[sel, :3] = np.asarray(palettes[c], np.uint8)[b[sel], a[sel], :3]
    return out
