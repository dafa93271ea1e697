"""The overlay fit (include/aptgpu.h, "fitting the map overlay to the image") in numpy, for the tests.

The reference has no such stage, so the header's text is the definition and this file restates it: the sample points,
the edge planes, the per-shift frame, the per-point angles, the place of a point under a candidate, the integer score
and count, the grid of a round, and the winner by exact rationals with the lowest index on a tie.

Scalars (the frame, D, kx, ky, the axis values) use Python floats, i.e. IEEE f64 and the C library's libm; the per-point
transcendentals are numpy's.  Either may differ from the device's library by ulps, which matters only where a decision
lies within TAU pixels of its boundary: `floor(x + 0.5)`, `floor(y + 0.5)`, the row estimate, and the P.S > 0.5 test.
For every candidate the model returns the smallest such margin over the points near the image; a candidate whose margin
is below TAU is excused from the bit-for-bit comparison.
"""
import math
from fractions import Fraction

import numpy as np

import np_map_model as mm

TAU = mm.TAU
PX, HALF, VIDEO0, VIDEO_N, CENTRE = 2080, 1040, 86, 909, 453
MAX_POINTS = 1 << 22
REASON_NO_CANDIDATE, REASON_FLAT = 17, 18
SCORE_DTYPE = np.dtype([("score", np.uint64), ("count", np.uint32), ("zero", np.uint32)])
PS_NEAR = 1e-9   # |P.S - 0.5| below this: the validity test itself is within reach of an ulp
DEFAULT_LAYERS = ("countries", "lakes")


class Params:
    """aptgpu_fit_settings' numbers."""

    def __init__(self, channel=0, margin_rows=120, shift_step=8, n_shift=15, yaw_step=0.02, n_yaw=3, hscale_step=0.04,
                 n_hscale=3, vscale_step=0.04, n_vscale=3, rounds=4, radius=2, spacing_deg=0.05, min_points=64):
        self.channel, self.margin_rows, self.shift_step, self.n_shift = channel, margin_rows, shift_step, n_shift
        self.yaw_step, self.n_yaw, self.hscale_step, self.n_hscale = yaw_step, n_yaw, hscale_step, n_hscale
        self.vscale_step, self.n_vscale, self.rounds, self.radius = vscale_step, n_vscale, rounds, radius
        self.spacing_deg, self.min_points = spacing_deg, min_points

    def counts(self):
        return tuple(2 * n + 1 for n in (self.n_shift, self.n_yaw, self.n_hscale, self.n_vscale))

    def total(self):
        ns, ny, nh, nv = self.counts()
        return ns * ny * nh * nv

    def steps(self, rho):
        return (max(1, self.shift_step >> rho), self.yaw_step / 2.0 ** rho, self.hscale_step / 2.0 ** rho,
                self.vscale_step / 2.0 ** rho)

    def radius_of(self, rho):
        return self.radius << (self.rounds - 1 - rho)


def sample_points(layers, spacing_deg, names=DEFAULT_LAYERS):
    """layers: {"states"|"countries"|"lakes": list of (n, 2) arrays of (lon, lat) degrees}.  The masked layers in draw
    order, each part, each segment: n = max(1, ceil(max(|dlon|, |dlat|) / spacing)) points p0 + (p1 - p0) * (i / n)."""
    out = []
    total = 0
    for name in mm.LAYER_ORDER:
        if name not in names or layers.get(name) is None:
            continue
        for part in layers[name]:
            part = np.asarray(part, np.float64).reshape(-1, 2)
            if len(part) == 1:
                out.append(part.copy())
                total += 1
            for j in range(len(part) - 1):
                p0, d = part[j], part[j + 1] - part[j]
                steps = math.ceil(max(abs(float(d[0])), abs(float(d[1]))) / spacing_deg)
                n = int(steps) if steps >= 1 else 1
                total += n
                if total > MAX_POINTS:
                    raise OverflowError("more than 2^22 sample points")
                f = np.arange(n, dtype=np.float64) / float(n)
                out.append(np.stack([p0[0] + d[0] * f, p0[1] + d[1] * f], axis=1))
    if total > MAX_POINTS:
        raise OverflowError("more than 2^22 sample points")
    return np.concatenate(out) if out else np.zeros((0, 2))


def edge_plane(image, channel, radius):
    """E_R of the channel's 909 video columns: exact integers (int64)."""
    v = np.asarray(image, np.uint8)[:, HALF * channel + VIDEO0:HALF * channel + VIDEO0 + VIDEO_N].astype(np.int64)
    h = v.shape[0]
    right, left = np.minimum(np.arange(VIDEO_N) + 1, VIDEO_N - 1), np.maximum(np.arange(VIDEO_N) - 1, 0)
    down, up = np.minimum(np.arange(h) + 1, h - 1), np.maximum(np.arange(h) - 1, 0)
    g = np.abs(v[:, right] - v[:, left]) + np.abs(v[down, :] - v[up, :])
    c = np.zeros((h + 1, VIDEO_N + 1), np.int64)
    c[1:, 1:] = np.cumsum(np.cumsum(g, axis=0), axis=1)
    r0, r1 = np.maximum(np.arange(h) - radius, 0), np.minimum(np.arange(h) + radius, h - 1) + 1
    k0, k1 = np.maximum(np.arange(VIDEO_N) - radius, 0), np.minimum(np.arange(VIDEO_N) + radius, VIDEO_N - 1) + 1
    return c[r1][:, k1] - c[r0][:, k1] - c[r1][:, k0] + c[r0][:, k0]


def unit_of(lat, lon):
    cl = np.cos(lat)
    return np.stack([cl * np.cos(lon), cl * np.sin(lon), np.sin(lat)], axis=-1)


def unit_of_deg(points):
    points = np.asarray(points, np.float64).reshape(-1, 2)
    return unit_of(points[:, 1] / 180.0 * math.pi, points[:, 0] / 180.0 * math.pi)


def _dot(p, v):
    return (p[..., 0] * v[0] + p[..., 1] * v[1]) + p[..., 2] * v[2]


class Shift:
    """What a shift fixes: start, ref_az, D, the frame S, T, R and bx of the slice's rows."""

    def __init__(self, track, margin, s, h):
        t = np.asarray(track, np.float64)[margin + s:margin + s + h]
        start, end = (float(t[0, 0]), float(t[0, 1])), (float(t[-1, 0]), float(t[-1, 1]))
        self.start, self.ref_az, self.d = start, mm.azimuth(start, end), mm.distance(start, end)
        sp, cp, sl, cl = math.sin(start[0]), math.cos(start[0]), math.sin(start[1]), math.cos(start[1])
        sa, ca = math.sin(self.ref_az), math.cos(self.ref_az)
        n, e = (-sp * cl, -sp * sl, cp), (-sl, cl, 0.0)
        self.s = (cp * cl, cp * sl, sp)
        self.t = tuple(ca * n[i] + sa * e[i] for i in range(3))
        self.r = tuple(-sa * n[i] + ca * e[i] for i in range(3))
        _, self.bx, _ = self.angles(unit_of(t[:, 0], t[:, 1]))
        self.bx[0] = 0.0

    def angles(self, p):
        ps = _dot(p, self.s)
        a = np.arctan2(_dot(p, self.t), ps)
        b = np.arcsin(np.clip(_dot(p, self.r), -1.0, 1.0))
        return a, b, ps


def place(a, b, yaw, kx, ky, h, bx):
    """(x, y, col index, row index) of points under a candidate, all as floats (the indices are floors)."""
    x0 = -b * kx
    y = a * ky + yaw * x0
    m = np.maximum(y, 0.0)
    e = np.where(m >= h - 1, h - 1, np.minimum(m, h - 1).astype(np.int64))
    x = x0 - (-bx[e] * kx)
    return x, y, np.floor(x + 0.5), np.floor(y + 0.5)


def _near_int(v):
    return np.abs(v - np.round(v))


class Problem:
    """One image, channel, long track, point list and Params."""

    def __init__(self, image, track, points, params):
        self.image, self.track, self.params = np.asarray(image, np.uint8), np.asarray(track, np.float64), params
        self.h = self.image.shape[0]
        assert self.track.shape[0] == self.h + 2 * params.margin_rows
        self.p = unit_of_deg(points)
        self.planes = {}

    def plane(self, rho):
        if rho not in self.planes:
            self.planes[rho] = edge_plane(self.image, self.params.channel, self.params.radius_of(rho))
        return self.planes[rho]

    def axis(self, centre, rho):
        """the four axes' values of round rho around centre = (shift, yaw, hscale, vscale)"""
        pr = self.params
        steps = pr.steps(rho)
        ns = (pr.n_shift, pr.n_yaw, pr.n_hscale, pr.n_vscale)
        shifts = [int(centre[0]) + i * steps[0] for i in range(-ns[0], ns[0] + 1)]
        rest = [[float(centre[k]) + float(i) * steps[k] for i in range(-ns[k], ns[k] + 1)] for k in (1, 2, 3)]
        return shifts, rest[0], rest[1], rest[2]

    def round_scores(self, rho, centre):
        """Every candidate of round rho around `centre`, before min_points: (score, count, margin) arrays in index
        order.  Invalid candidates (|s| > M, hscale <= 0, vscale <= 0) have score 0, count 0 and margin inf."""
        pr, h = self.params, self.h
        shifts, yaws, hscales, vscales = self.axis(centre, rho)
        plane = self.plane(rho)
        total = pr.total()
        score, count = np.zeros(total, np.uint64), np.zeros(total, np.uint32)
        margin = np.full(total, np.inf)
        c = 0
        per_shift = len(yaws) * len(hscales) * len(vscales)
        for s in shifts:
            if abs(s) > pr.margin_rows:
                c += per_shift
                continue
            f = Shift(self.track, pr.margin_rows, s, h)
            a, b, ps = f.angles(self.p)
            keep = ps > 0.5 - PS_NEAR
            # a cull that drops only points no candidate of the round can bring within 2 px of the image
            kxs = [v / 0.0005 for v in hscales if v > 0]
            kys = [h * v / f.d for v in vscales if v > 0]
            if kxs and kys:
                reach = 458.0 + float(np.max(np.abs(f.bx))) * max(kxs)
                yreach = max(abs(v) for v in yaws) * reach + 2.5
                keep &= np.abs(b) * min(kxs) <= reach
                keep &= np.where(a >= 0, a * min(kys) <= h + yreach, -a * min(kys) <= yreach)
            a, b, ps = a[keep], b[keep], ps[keep]
            unsure = np.abs(ps - 0.5) < PS_NEAR
            sure = ps > 0.5
            for yaw in yaws:
                for hs in hscales:
                    for vs in vscales:
                        if hs > 0 and vs > 0:
                            kx, ky = hs / 0.0005, h * vs / f.d
                            x, y, fc, fr = place(a, b, yaw, kx, ky, h, f.bx)
                            inside = (fr >= 0) & (fr < h) & (fc >= -CENTRE) & (fc < VIDEO_N - CENTRE)
                            got = inside & sure
                            score[c] = int(plane[fr[got].astype(np.int64), fc[got].astype(np.int64) + CENTRE].sum())
                            count[c] = int(np.count_nonzero(got))
                            near = (fr >= -1) & (fr <= h) & (fc >= -CENTRE - 1) & (fc <= VIDEO_N - CENTRE)
                            if near.any():
                                m = np.minimum(np.minimum(_near_int(x[near] + 0.5), _near_int(y[near] + 0.5)),
                                               _near_int(y[near]))
                                m = np.where(unsure[near], 0.0, m)
                                margin[c] = float(m.min())
                        c += 1
        return score, count, margin

    def apply_min_points(self, score, count):
        ok = count >= self.params.min_points
        return np.where(ok, score, 0).astype(np.uint64), np.where(ok, count, 0).astype(np.uint32)

    def candidate(self, rho, centre, index):
        ns, ny, nh, nv = self.params.counts()
        shifts, yaws, hscales, vscales = self.axis(centre, rho)
        return (shifts[index // (nv * nh * ny)], yaws[index // (nv * nh) % ny], hscales[index // nv % nh],
                vscales[index % nv])

    def fit(self, initial=(0, 0.0, 1.0, 1.0)):
        """All rounds.  Returns (rounds, final, reason): rounds is a list of dicts (centre, winner, index, score,
        count, margin arrays), final = (shift, yaw, hscale, vscale)."""
        centre, out = tuple(initial), []
        final = tuple(initial)
        for rho in range(self.params.rounds):
            raw_s, raw_c, margin = self.round_scores(rho, centre)
            score, count = self.apply_min_points(raw_s, raw_c)
            best = pick(score, count)
            entry = {"centre": centre, "score": score, "count": count, "margin": margin, "index": best,
                     "raw_count": raw_c}
            out.append(entry)
            if best is None:
                return out, final, REASON_NO_CANDIDATE
            entry["winner"] = self.candidate(rho, centre, best)
            if int(score[best]) == 0:
                return out, tuple(initial), REASON_FLAT
            centre = final = entry["winner"]
        return out, final, 0


def pick(score, count):
    """The index of the greatest score / count over count > 0, as exact rationals; the lowest index on a tie."""
    best, best_q = None, None
    for i in np.flatnonzero(np.asarray(count) > 0):
        q = Fraction(int(score[i]), int(count[i]))
        if best is None or q > best_q:
            best, best_q = int(i), q
    return best
