"""What test_landmask_cpu.py and test_gpu_landmask.py share: the tracks, the layer sets and the assertions of the land /
sea / lake mask, each written against a `side`: the host twin or the GPU forms of the same calls.

  plane form   mask and counts equal np_landmask_model's bit for bit, no pixel excused, for n_bands 1, 7, 720 and 7200
  swath form   equals the plane form of the same side's geolocate() plane, bit for bit (track form and orbit form)
  end to end   against the model's own f64 geolocation: the library's points may differ from the model's by 5e-10 rad
               (§25), so a pixel is excused only if the model's class changes when its point moves by 1e-9 rad along one
               of the four axis directions; at most 8 per case
"""
import functools
import os
from collections import namedtuple

import numpy as np

import fit_cases as fc
import geoloc_cases as gc
import np_geoloc_model as gm
import np_landmask_model as lmm
import np_map_model as mm

import noaa_apt_amd as apt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PALETTES = os.path.join(ROOT, "tests", "golden", "palettes")
MAX_EXCUSED = 8
NUDGE = 1e-9
BANDS = (1, 7, 720, 7200)

# plane(latlon, layers, settings) / swath(h, track_or_orbit, layers, map_settings, settings) -> (mask, info);
# points(h, track_or_orbit, map_settings) -> the side's own lat / lon plane; color(image, mask, palettes, tunes) -> RGBA
Side = namedtuple("Side", "name plane swath points color")

HOST = Side(
    "host",
    lambda ll, layers, st=None: apt.land_mask_plane_host(ll, layers, st),
    lambda h, t, layers, ms=None, st=None: apt.land_mask_host(h, t, layers, ms, st),
    lambda h, t, ms=None: apt.geolocate_host(h, t, ms, None, latlon=True, sun=False)[0],
    lambda im, mask, pals, tunes: apt.false_color_masked_host(im, mask, pals, tunes))
GPU = Side(
    "gpu",
    lambda ll, layers, st=None: apt.land_mask_plane(ll, layers, st),
    lambda h, t, layers, ms=None, st=None: apt.land_mask(h, t, layers, ms, st),
    lambda h, t, ms=None: apt.geolocate(h, t, ms, None, latlon=True, sun=False)[0],
    lambda im, mask, pals, tunes: apt.false_color_masked(im, mask, pals, tunes))


def scene_track(k):
    """the scene's h rows from its start point, under its true geometry"""
    h, start, (_, yaw, hscale, vscale) = fc.SCENES[k]
    return mm.great_circle_track(*start, h), (yaw, hscale, vscale)


# name -> (track, (yaw, hscale, vscale)) over the fixture layers (South America)
@functools.lru_cache(maxsize=None)
def case(name):
    if name == "h2":  # the smallest with a direction: 1818 pixels, a partly filled last wave
        return mm.great_circle_track(-34.6, -58.4, 15.0, 2), (0.0, 1.0, 1.0)
    if name == "h5":  # waves that span two rows
        return mm.great_circle_track(-33.0, -71.5, 195.0, 5), (0.03, 0.9, 1.1)
    if name.startswith("scene"):
        return scene_track(int(name[5:]))
    track, geom, _ = gc.case(name)  # "far", "pole", "antimeridian"
    return track, geom


SMALL = ("h2", "h5")
FIXTURE_CASES = ("h2", "h5", "scene1", "scene2", "scene3", "far")
# sea / land / lake / invalid as the model gives them (the issue's table)
KNOWN_COUNTS = {"scene3": (89129, 19579, 372, 0), "scene1": (113005, 104992, 163, 0), "far": (1559652, 281662, 1435, 66151)}


def map_settings_of(name):
    return apt.MapSettings(*case(name)[1])


@functools.lru_cache(maxsize=None)
def fixture_edges():
    p = fc.parts()
    return lmm.edges_of(p["countries"]), lmm.edges_of(p["lakes"])


def fixture_layers():
    return fc.layers()


@functools.lru_cache(maxsize=None)
def model_points(name):
    track, (yaw, hscale, vscale) = case(name)
    ll = gm.Forward(track, yaw, hscale, vscale).latlon()
    ll.setflags(write=False)
    return ll


@functools.lru_cache(maxsize=None)
def model_mask(name):
    mask, cnt = lmm.classify(model_points(name), *fixture_edges())
    mask.setflags(write=False)
    return mask, cnt


def record(info):
    return (info.status, info.reason, info.height, info.n_sea, info.n_land, info.n_lake, info.n_invalid,
            tuple(info.n_edges), info.n_band_entries)


def counts_of(info):
    return (info.n_sea, info.n_land, info.n_lake, info.n_invalid)


def settings(nb):
    return apt.LandMaskSettings(n_bands=nb)


def check_plane(side, latlon, layers, edges, bands=BANDS, note=""):
    """the plane form against the model, bit for bit, under every band count; returns the mask"""
    want, cnt = lmm.classify(latlon, *edges)
    first = None
    for nb in bands:
        mask, info = side.plane(latlon, layers, settings(nb))
        assert mask.dtype == np.uint8 and mask.shape == want.shape, (note, nb)
        diff = np.argwhere(mask != want)
        assert diff.size == 0, (side.name, note, nb, len(diff), diff[:4])
        assert counts_of(info) == cnt and (info.status, info.reason, info.height) == (0, 0, 0), (note, nb)
        if first is None:
            first = info
        assert tuple(info.n_edges) == tuple(first.n_edges), (note, nb)  # (the band entries grow with the bands)
    return want


def swath_equals_plane(side, h, track_or_orbit, layers, ms, nb, note):
    mask, info = side.swath(h, track_or_orbit, layers, ms, settings(nb))
    ll = side.points(h, track_or_orbit, ms)
    want, winfo = side.plane(ll, layers, settings(nb))
    assert mask.shape == (h, 909) and mask.tobytes() == want.tobytes(), (side.name, note, np.argwhere(mask != want)[:4])
    assert counts_of(info) == counts_of(winfo) and (info.status, info.reason, info.height) == (0, 0, h), note
    assert info.n_invalid == int(np.isnan(ll[..., 0]).sum())
    assert (tuple(info.n_edges), info.n_band_entries) == (tuple(winfo.n_edges), winfo.n_band_entries)
    return mask, info


def excusable(ll, edges, want):
    """of the points ll (k, 2) whose model class is want (k,): whether the class changes under a nudge of 1e-9 rad along
    one of the four axis directions"""
    out = np.zeros(len(ll), bool)
    for dlat, dlon in ((NUDGE, 0), (-NUDGE, 0), (0, NUDGE), (0, -NUDGE)):
        moved, _ = lmm.classify(ll + np.array([dlat, dlon]), *edges)
        out |= moved != want
    return out


def check_end_to_end(side, name, layers, edges, mask=None):
    """the swath form against the model's own geolocation; returns the number of excused pixels"""
    if mask is None:
        mask, _ = side.swath(case(name)[0].shape[0], case(name)[0], layers, map_settings_of(name), settings(720))
    ll = model_points(name)
    want = model_mask(name)[0] if edges is fixture_edges() else lmm.classify(ll, *edges)[0]
    bad = np.argwhere(mask != want)
    n_bad = len(bad)
    print(f"landmask {side.name} {name}: {n_bad} of {mask.size} pixels differ from the model's end-to-end mask")
    assert n_bad <= MAX_EXCUSED, (side.name, name, n_bad)
    if n_bad:
        r, k = bad[:, 0], bad[:, 1]
        pts = ll[r, k]
        finite = ~np.isnan(pts[:, 0])
        ok = np.zeros(n_bad, bool)
        ok[finite] = excusable(pts[finite], edges, want[r, k][finite])  # (a pixel the model finds invalid is never excused)
        assert ok.all(), (side.name, name, bad[~ok][:4])
    return n_bad


# ---- synthetic layers: what the fixture files do not hold
def ring(lons, lats):
    return np.stack([np.asarray(lons, np.float64), np.asarray(lats, np.float64)], axis=1)


def box(w, s, e, n, close=True):
    pts = [(w, s), (e, s), (e, n), (w, n)] + ([(w, s)] if close else [])
    return np.array(pts, np.float64)


def synthetic_parts(name):
    """(countries, lakes) as lists of parts, placed under geoloc_cases' "pole" and "antimeridian" tracks"""
    if name == "pole":
        # a polar cap whose ring runs along lat 90 and back along lat 80; a ring with a hole and an island in the hole;
        # an unclosed part (the implicit closing edge); a lake over part of the cap
        cap = ring([-180, -90, 0, 90, 180, 180, 90, 0, -90, -180, -180], [80, 80, 80, 80, 80, 90, 90, 90, 90, 90, 80])
        outer, hole, island = box(20, 70, 60, 79), box(28, 72, 52, 77), box(35, 73.5, 45, 75.5)
        unclosed = box(-10, 71, 15, 78, close=False)
        return [cap, outer, hole, island, unclosed], [box(30, 82, 80, 86), box(38, 74, 42, 75)]
    if name == "antimeridian":
        # two polygons that abut lon +180 and -180, and a lake across one of them
        east, west = box(175, 15, 180, 32), box(-180, 18, -174, 30)
        return [east, west, box(170, 22, 173, 25, close=False)], [box(177, 20, 179, 24)]
    raise KeyError(name)


def layers_of(countries, lakes):
    return apt.MapLayers(countries=countries, lakes=lakes)


def synthetic(name):
    co, la = synthetic_parts(name)
    return layers_of(co, la), (lmm.edges_of(co), lmm.edges_of(la))


def degenerate(side, name="h5"):
    """Polygons whose vertices are the library's own points of chosen pixels, through the same multiply: py == y1 holds
    exactly there.  Returns (latlon plane, layers, edges, the chosen pixels)."""
    track = case(name)[0]
    h = track.shape[0]
    ll = side.points(h, track, map_settings_of(name))
    deg = ll * lmm.DEG  # (the multiply the library applies to a point)
    px = lambda r, k: (float(deg[r, k, 1]), float(deg[r, k, 0]))  # noqa: E731  (lon, lat) in degrees
    a, b, c, d = px(1, 100), px(1, 300), px(3, 300), px(3, 100)
    # a quadrilateral through four pixels: the points themselves lie exactly on its vertices, and the pixels of rows 1
    # and 3 between them lie (nearly) on its two long edges
    quad = np.array([a, b, c, d, a])
    # a triangle with a horizontal edge at exactly pixel (2, 500)'s latitude, through that pixel's own longitude
    m = px(2, 500)
    tri = np.array([(m[0] - 0.5, m[1]), (m[0] + 0.5, m[1]), (m[0], m[1] - 0.7), (m[0] - 0.5, m[1])])
    # a lake with a vertex on pixel (2, 200) and a horizontal edge through pixel (2, 260)'s latitude east of it
    v, w = px(2, 200), px(2, 260)
    lake = np.array([v, (w[0], w[1]), (w[0] + 0.3, w[1]), (v[0] + 0.2, v[1] + 0.4)])
    co, la = [quad, tri], [lake]
    return ll, layers_of(co, la), (lmm.edges_of(co), lmm.edges_of(la)), ((1, 100), (1, 300), (3, 300), (3, 100), (2, 500), (2, 200), (2, 260))


def nan_plane(ll, seed, n_nan=97, drop=5):
    """a flat plane from ll with NaNs at arbitrary places (either coordinate) and a length that is no multiple of 64"""
    flat = np.array(ll, np.float64).reshape(-1, 2)
    n = flat.shape[0] - drop
    if n % 64 == 0:
        n -= 1
    flat = flat[:n].copy()
    rng = np.random.default_rng(seed)
    idx = rng.choice(n, size=min(n_nan, n), replace=False)
    flat[idx, rng.integers(0, 2, size=idx.size)] = np.nan
    return flat


# ---- the colouriser
@functools.lru_cache(maxsize=None)
def palettes():
    from PIL import Image
    out = []
    for f in ("WXtoImg-NO.png", "noaa-apt-daylight.png"):
        with Image.open(os.path.join(PALETTES, f)) as im:
            out.append(np.ascontiguousarray(np.asarray(im.convert("RGB"), np.uint8)))
    out.append(np.random.default_rng(28).integers(0, 256, (256, 256, 3), dtype=np.uint8))
    assert all(p.shape == (256, 256, 3) for p in out)
    return tuple(out)


TUNES = (0.1, -0.2, 0.3, 0.15)


def gray_image(h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, 2080), dtype=np.uint8)


def random_mask(h, seed, invalid=True):
    rng = np.random.default_rng(seed)
    classes = np.array([0, 1, 2, 255] if invalid else [0, 1, 2], np.uint8)
    return classes[rng.integers(0, len(classes), (h, 909))]


def check_color_model(side, h):
    image, mask = gray_image(h, 100 + h), random_mask(h, 200 + h)
    got = side.color(image, mask, palettes(), TUNES)
    want = lmm.false_color_masked(image, mask, palettes(), TUNES)
    assert got.dtype == np.uint8 and got.shape == (h, 2080, 4)
    assert got.tobytes() == want.tobytes(), (side.name, h, np.argwhere(got != want)[:4])
    # class 255 and everything outside channel A's video columns stay gray
    gray = np.repeat(image[:, :, None], 3, axis=2)
    outside = np.ones(2080, bool)
    outside[86:995] = False
    assert np.array_equal(got[:, outside, :3], gray[:, outside]) and (got[..., 3] == 255).all()
    inv = mask == 255
    assert np.array_equal(got[:, 86:995][inv][:, :3], gray[:, 86:995][inv])
