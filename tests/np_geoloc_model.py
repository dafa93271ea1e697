"""The geolocation stage in numpy f64 (include/aptgpu.h, "geolocation of the swath"): the yardstick
of test_geoloc_cpu.py and test_gpu_geoloc.py.

The stage inverts latlon_to_rel_px (np_map_model.rel_px, map.rs:71-100): from swath pixel (row r, video column k) to
the point of the Earth it shows, then the cosine of the solar zenith angle there and the visible rows divided by it.
The scalars and the per-row x offsets are np_map_model's, the rest is stated here."""
import math

import numpy as np

import np_map_model as mm

PX = 2080
VIDEO0, VIDEO_N, CENTRE = 86, 909, 453
LINE_MS = 500
LIMIT = math.pi / 3.0      # beyond this arc from the start point rel_px clamps and has no inverse
EDGE = 1e-9                # rad: a pixel whose arc is this close to LIMIT may fall on either side
REASON_COUNT, REASON_SGP4, REASON_HEIGHT, REASON_DECODE = 7, 10, 15, 16
f32 = np.float32


def xoffs(track, sc):
    """xoff[r] = rel_px(track[r]).x, map.rs:110-114; xoff[0] = 0, the start point's own relative pixel (evaluated, it is
    0 or acos(1 - 2^-53) = 1.5e-8 rad times the sine of an arbitrary angle, whichever way one cosine rounds)"""
    out = np.array([mm.rel_px(sc, (float(a), float(b)))[0] for a, b in track])
    out[0] = 0.0
    return out


def frame(sc):
    """S, T, R: the start point's unit vector, the unit vector along the reference azimuth and the one to its right."""
    p0, l0 = sc.start
    s = np.array([math.cos(p0) * math.cos(l0), math.cos(p0) * math.sin(l0), math.sin(p0)])
    n = np.array([-math.sin(p0) * math.cos(l0), -math.sin(p0) * math.sin(l0), math.cos(p0)])
    e = np.array([-math.sin(l0), math.cos(l0), 0.0])
    t = math.cos(sc.ref_az) * n + math.sin(sc.ref_az) * e
    r = -math.sin(sc.ref_az) * n + math.cos(sc.ref_az) * e
    return s, t, r


class Forward:
    """The forward points of an h-row swath: p (h, 909, 3) unit vectors, arc (h, 909) their distance from the start
    point, valid = arc < LIMIT, edge = |arc - LIMIT| <= EDGE (validity undecided), xoff (h,), sc the scalars."""

    def __init__(self, track, yaw=0.0, hscale=1.0, vscale=1.0):
        track = np.asarray(track, np.float64).reshape(-1, 2)
        h = track.shape[0]
        self.sc = sc = mm.Scalars(track, yaw, hscale, vscale)
        self.xoff = xoffs(track, sc)
        x = (np.arange(VIDEO_N) - CENTRE)[None, :] + self.xoff[:, None]
        b = -x * sc.x_res
        a = (np.arange(h)[:, None] - yaw * x) * sc.y_res
        s, t, r = frame(sc)
        u, v, w = np.cos(b) * np.cos(a), np.cos(b) * np.sin(a), np.sin(b)
        self.p = u[..., None] * s + v[..., None] * t + w[..., None] * r
        self.arc = np.arccos(np.clip(np.cos(a) * np.cos(b), -1.0, 1.0))
        self.valid = self.arc < LIMIT
        self.edge = np.abs(self.arc - LIMIT) <= EDGE
        self.h = h

    def latlon(self):
        """(h, 909, 2) lat, lon in rad; NaN where invalid"""
        p = self.p
        out = np.stack([np.arctan2(p[..., 2], np.hypot(p[..., 0], p[..., 1])), np.arctan2(p[..., 1], p[..., 0])], -1)
        out[~self.valid] = np.nan
        return out

    def cos_sun(self, start_ms):
        """(h, 909) f64 cosine of the solar zenith angle, row r at start_ms + 500 r; NaN where invalid"""
        u = sun_vector(start_ms + LINE_MS * np.arange(self.h, dtype=np.int64))
        c = np.einsum("rkc,rc->rk", self.p, u)
        c[~self.valid] = np.nan
        return c


def unit(latlon):
    lat, lon = latlon[..., 0], latlon[..., 1]
    return np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], -1)


def separation(latlon, p):
    """angle between the points (lat, lon) and the unit vectors p, through the chord: exact at the pole and across
    the antimeridian"""
    d = np.linalg.norm(unit(latlon) - p, axis=-1)
    return 2.0 * np.arcsin(np.minimum(d / 2.0, 1.0))


def sun_angles(t_ms):
    """(declination, sub-solar longitude before wrapping) in rad: the Astronomical Almanac's low-precision series"""
    t = np.asarray(t_ms, np.float64)
    n = t / 86400000.0 + 2440587.5 - 2451545.0
    big_l = np.fmod(280.460 + 0.9856474 * n, 360.0)
    g = np.radians(np.fmod(357.528 + 0.9856003 * n, 360.0))
    lam = np.radians(big_l + 1.915 * np.sin(g) + 0.020 * np.sin(2.0 * g))
    eps = np.radians(23.439 - 0.0000004 * n)
    alpha = np.arctan2(np.cos(eps) * np.sin(lam), np.cos(lam))
    delta = np.arcsin(np.sin(eps) * np.sin(lam))
    theta = np.radians(15.0 * np.fmod(18.697374558 + 24.06570982441908 * n, 24.0))
    return delta, alpha - theta


def sun_position(t_ms):
    delta, lon = sun_angles(t_ms)
    return float(delta), float(np.arctan2(np.sin(lon), np.cos(lon)))


def sun_vector(t_ms):
    delta, lon = sun_angles(t_ms)
    return np.stack([np.cos(delta) * np.cos(lon), np.cos(delta) * np.sin(lon), np.sin(delta)], -1)


def start_ms(kind, unix_ms, h):
    return unix_ms - LINE_MS * h if kind == "end" else unix_ms


def cmin_of(max_zenith_deg):
    return f32(math.cos(float(f32(max_zenith_deg)) / 180.0 * math.pi))


def normalise(rows, cos32, channel, black, cmin):
    """The f32 mapping of the rows by a cos_sun plane (NaN = invalid: left alone), one rounding per operation."""
    h = cos32.shape[0]
    out = np.array(rows, f32).copy()
    img = out[:h * PX].reshape(h, PX)
    base = 1040 * channel + VIDEO0
    x = img[:, base:base + VIDEO_N]
    valid = ~np.isnan(cos32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.maximum(cos32.astype(f32), f32(cmin))
        y = (f32(black) + (x - f32(black)) / d).astype(f32)
    img[:, base:base + VIDEO_N] = np.where(valid, y, x)
    return out
