"""What test_geoloc_cpu.py and test_gpu_geoloc.py share: the tracks, and one call of the geolocation stage (the host twin
or the GPU forms) checked against np_geoloc_model.py with the bounds DESIGN.md §25 derives.

  position    angular separation from the model's point <= TAU px * x_res (TAU = 1e-6 px, the overlay's parity threshold)
  round trip  np_map_model.rel_px of the returned (lat, lon) gives back (x_rel + xoff[r], r) within TAU px
  cos_sun     within one f32 ulp at 1 (1.2e-7) of the model's f64 value
  rows        bit-exact against the model's f32 mapping of the returned cos_sun plane
  validity    the model's, except where the arc is within 1e-9 rad of pi / 3 (at most 16 pixels)
"""
import functools
import math

import numpy as np

import np_geoloc_model as gm
import np_map_model as mm

import noaa_apt_amd as apt

f32 = np.float32
TAU = mm.TAU
ULP1 = 1.2e-7
MAX_EDGE = 16
T_NOON_2024 = 1730635200000  # 2024-11-03 12:00 UTC


def rotating(track, seconds_per_row=0.5):
    """the Earth's rotation subtracted from a great-circle track's longitudes: x offsets of pixels, not of 1e-12 px"""
    out = np.array(track, np.float64)
    lon = out[:, 1] - 7.2921159e-5 * seconds_per_row * np.arange(out.shape[0])
    out[:, 1] = (lon + math.pi) % (2 * math.pi) - math.pi
    return out


EXTRA = {}  # cases a test defines from a computed track (define())


def define(name, track, geom, t_ms):
    EXTRA[name] = (np.asarray(track, np.float64).reshape(-1, 2), tuple(geom), int(t_ms))
    return name


# name -> (track, (yaw, hscale, vscale), reference time ms): heights 2, 5, 263 and 530, the settings' range, the pole,
# the antimeridian, x offsets that matter and the far limit
@functools.lru_cache(maxsize=None)
def case(name):
    if name in EXTRA:
        return EXTRA[name]
    gc = mm.great_circle_track
    return {
        "h2": (gc(10.0, 20.0, 15.0, 2), (0.0, 1.0, 1.0), T_NOON_2024),
        "h5": (gc(-30.0, 100.0, 195.0, 5), (0.03, 0.9, 1.1), T_NOON_2024 + 3 * 3600000),
        "h263": (gc(40.0, -75.0, 190.0, 263), (-0.03, 1.1, 0.9), T_NOON_2024 + 5 * 3600000),
        "h530_rotating": (rotating(gc(55.0, 10.0, 192.0, 530)), (0.01, 1.0, 1.0), T_NOON_2024 - 3600000),
        "pole": (gc(75.0, 30.0, 12.0, 400), (0.0, 1.0, 1.0), T_NOON_2024),
        "antimeridian": (gc(20.0, 179.2, 15.0, 300), (0.02, 1.05, 0.95), T_NOON_2024 + 11 * 3600000),
        "far": (gc(-20.0, -40.0, 10.0, 2100), (0.0, 1.0, 1.0), T_NOON_2024 + 2 * 3600000),
    }[name]


@functools.lru_cache(maxsize=None)
def model(name):
    track, (yaw, hscale, vscale), t = case(name)
    fw = gm.Forward(track, yaw, hscale, vscale)
    return fw, fw.latlon(), fw.cos_sun(t)


def rows_of(h, seed, extra=7):
    """h rows of plausible levels (and a few floats behind the last whole row)"""
    rng = np.random.default_rng(seed)
    return (rng.random(h * 2080 + extra) * 200.0 + 20.0).astype(f32)


def round_trip_sample(h):
    """(rows, columns) of the pixels the round trip visits: all of a small swath; of a large one, nine columns of every
    row and four whole rows"""
    if h * gm.VIDEO_N <= 5000:
        r, k = np.meshgrid(np.arange(h), np.arange(gm.VIDEO_N), indexing="ij")
        return r.ravel(), k.ravel()
    cols = np.array([0, 1, 226, 452, 453, 454, 680, 907, 908])
    r1, k1 = np.meshgrid(np.arange(h), cols, indexing="ij")
    r2, k2 = np.meshgrid(np.array([0, 1, h // 2, h - 1]), np.arange(gm.VIDEO_N), indexing="ij")
    return np.concatenate([r1.ravel(), r2.ravel()]), np.concatenate([k1.ravel(), k2.ravel()])


def check_planes(name, latlon, cos_sun, info, note=None):
    """the lat / lon and cos_sun planes and the record of one call against the model of case `name`"""
    fw, want_ll, want_c = model(name)
    h = fw.h
    note = note or name
    assert (info.status, info.reason, info.height) == (0, 0, h), note
    n_edge = int(fw.edge.sum())
    assert n_edge <= MAX_EDGE, (note, n_edge)
    sure = ~fw.edge
    got_valid = None
    if latlon is not None:
        assert latlon.dtype == np.float64 and latlon.shape == (h, gm.VIDEO_N, 2), note
        got_valid = ~np.isnan(latlon[..., 0])
        assert np.array_equal(np.isnan(latlon[..., 0]), np.isnan(latlon[..., 1])), note
        assert np.array_equal(got_valid[sure], fw.valid[sure]), note
        both = got_valid & fw.valid
        sep = gm.separation(latlon[both], fw.p[both])
        tol = TAU * fw.sc.x_res
        worst = float(sep.max()) if sep.size else 0.0
        print(f"geoloc {note}: {int(both.sum())} px, max separation {worst:.3g} rad (bound {tol:.3g}), "
              f"max |xoff| {np.abs(fw.xoff).max():.3g} px")
        assert worst <= tol, (note, worst, tol)
        lon = latlon[..., 1][both]
        assert np.all((lon > -math.pi - 1e-15) & (lon <= math.pi)), note
        # the round trip through the overlay's own projection
        start = np.array(fw.sc.start)
        worst_x = worst_y = 0.0
        for r, k in zip(*round_trip_sample(h)):
            if not both[r, k]:
                continue
            ll = (float(latlon[r, k, 0]), float(latlon[r, k, 1]))
            if mm.distance(ll, tuple(start)) < mm.NEAR_START:
                continue
            x, y = mm.rel_px(fw.sc, ll)
            worst_x = max(worst_x, abs(x - fw.xoff[r] - (k - gm.CENTRE)))
            worst_y = max(worst_y, abs(y - r))
        print(f"geoloc {note}: round trip max |dx| {worst_x:.3g} px, max |dy| {worst_y:.3g} px (bound {TAU:g})")
        assert worst_x <= TAU and worst_y <= TAU, (note, worst_x, worst_y)
    if cos_sun is not None:
        assert cos_sun.dtype == f32 and cos_sun.shape == (h, gm.VIDEO_N), note
        cv = ~np.isnan(cos_sun)
        if got_valid is not None:
            assert np.array_equal(cv, got_valid), note
        assert np.array_equal(cv[sure], fw.valid[sure]), note
        both = cv & fw.valid
        err = np.abs(cos_sun[both].astype(np.float64) - want_c[both])
        worst = float(err.max()) if err.size else 0.0
        print(f"geoloc {note}: max |cos_sun - model| {worst:.3g} (bound {ULP1:g})")
        assert worst <= ULP1, (note, worst)
        got_valid = cv
    if got_valid is not None:
        assert info.n_outside == int((~got_valid).sum()), (note, info.n_outside)
    if cos_sun is not None:
        fin = cos_sun[got_valid]
        if fin.size:
            assert f32(info.cos_min).tobytes() == fin.min().tobytes(), note
            assert f32(info.cos_max).tobytes() == fin.max().tobytes(), note
        else:
            assert np.isnan(info.cos_min) and np.isnan(info.cos_max), note


def check_rows(rows_in, rows_out, cos_sun, channel, black, max_zenith_deg, info, note=None):
    """normalised rows against the model's f32 mapping of the returned cos_sun plane, bit for bit; everything outside
    the channel's video untouched"""
    cmin = gm.cmin_of(max_zenith_deg)
    want = gm.normalise(rows_in, cos_sun, channel, black, cmin)
    assert rows_out.dtype == f32 and rows_out.size == rows_in.size, note
    assert rows_out.tobytes() == want.tobytes(), (note, np.argwhere(rows_out.view(np.uint32) != want.view(np.uint32))[:4])
    h = cos_sun.shape[0]
    base = 1040 * channel + gm.VIDEO0
    outside = np.ones(2080, bool)
    outside[base:base + gm.VIDEO_N] = False
    a = np.asarray(rows_in, f32)[:h * 2080].reshape(h, 2080)
    b = rows_out[:h * 2080].reshape(h, 2080)
    assert a[:, outside].tobytes() == b[:, outside].tobytes(), note
    assert np.asarray(rows_in, f32)[h * 2080:].tobytes() == rows_out[h * 2080:].tobytes(), note
    valid = ~np.isnan(cos_sun)
    with np.errstate(invalid="ignore"):
        assert info.n_capped == int((valid & (cos_sun < cmin)).sum()), (note, info.n_capped)
    assert info.n_outside == int((~valid).sum()), note


def record(r):
    return (r.status, r.reason, r.height, r.n_outside, r.n_capped, f32(r.cos_min).tobytes(), f32(r.cos_max).tobytes())


def settings_of(name, channel="A", black=0.0, kind="start", max_zenith_deg=80.0):
    _, _, t = case(name)
    h = case(name)[0].shape[0]
    ref = apt.RefTime.Start(t) if kind == "start" else apt.RefTime.End(t + gm.LINE_MS * h)
    return apt.GeolocSettings(channel=channel, ref_time=ref, black=black, max_zenith_deg=max_zenith_deg)


def map_settings_of(name):
    yaw, hscale, vscale = case(name)[1]
    return apt.MapSettings(yaw, hscale, vscale)
