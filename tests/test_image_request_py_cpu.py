"""The Python side of the image calls (process(), Plan.process_device_image, the composite calls, project_image), pinned
without a GPU.  Part 1: every refusal Python makes itself, as (exception class, exact message), and which one wins when
two apply.  A plan without a device is Plan.__new__(Plan) with _p = None: Python's checks run first, and once they pass
C answers the NULL plan with a bare APTGPU_ERR_INVALID (tests/test_capi_image_args_cpu.py).  Part 2: with the library
replaced by a stand-in that records its calls, which entry point the plan form chooses for every variant of
tests/test_gpu_image_request.py and what it hands over, argument by argument.  All expectations are literals."""
import ctypes as C
import os

import numpy as np
import pytest

import noaa_apt_amd as apt
from noaa_apt_amd import api
from test_gpu_image_request import variants

HERE = os.path.dirname(os.path.abspath(__file__))
TLE_2020 = open(os.path.join(HERE, "golden", "tle", "noaa_2020.txt")).read()

INVALID, UNSUPPORTED = apt.InvalidError, apt.UnsupportedError
COLOR = (UNSUPPORTED, "color must be a ColorSettings")
EXCLUDE = (INVALID, "map and orbit exclude each other")
PROJ_TYPE = (INVALID, "projection must be a ProjectionSettings")
PROJ_TUPLE = (INVALID, "projection: (settings, d_out, out_cap) with one entry per recording")
PROJ_TRACK_PLAN = (INVALID, "a projection needs the track: exactly one of map and orbit")
PROJ_TRACK = (INVALID, "a projection needs the track: orbit = a MapOverlay, an OrbitSettings or the sat_positions")
ORBIT_LIST = (INVALID, "orbit: an OrbitSettings or one per recording")
ORBIT_LIST_PASS = (INVALID, "orbit: an OrbitSettings or one per pass")
NEEDS_LAYERS = (INVALID, "OrbitSettings.draw_map needs layers=MapLayers")
PNG_PAIR = (INVALID, "png: (d_png, png_cap) with one entry per recording")
MAP_LIST = (INVALID, "map: a MapOverlay or one per recording")
MAP_SHARE = (INVALID, "map: every recording's MapOverlay must share settings and layers")
MAP_PLAIN = (INVALID, "map: one sat_positions array per recording")
ORBIT_KIND = (UNSUPPORTED, "orbit: only a MapOverlay (the map overlay) is served on the GPU path")
OVERLAY_ROWS = (INVALID, "MapOverlay: 3 positions for 2 rows")
PROJ_ROWS = (INVALID, "projection: 3 positions for 2 rows")
DESPECKLE = (INVALID, "despeckle must be a DespeckleSettings")
BARE = (INVALID, "aptgpu status 4")  # (every check of Python's passed: C's answer to a NULL plan, which has no text)
COMPOSITE_TRACKS = (INVALID, "a composite needs the tracks: exactly one of tracks and orbit")
COMPOSITE_COUNTS = (INVALID, "composite: one height and one channel count per image")
COMPOSITE_PLAIN = (INVALID, "tracks: one sat_positions array per pass")
COMPOSITE_ONE_TRACK = (INVALID, "composite: one track per image")
COMPOSITE_IMAGE = (INVALID, "composite: every image is a uint8 array of (height, 2080) or (height, 2080, 4)")
COMPOSITE_SETTINGS = (INVALID, "settings: a MapSettings, or one (or None) per pass")
PROJECT_IMAGE = (INVALID, "project_image: a uint8 array of (height, 2080) or (height, 2080, 4)")

ROWS_CAP = [250, 60]
D_ROWS, D_IMAGES, D_OUT, D_PNG = [0x1000, 0x2000], [0x3000, 0x4000], [0x5000, 0x6000], [0x7000, 0x8000]
OUT_CAP, PNG_CAP = [160, 216], [1111, 2222]


class Env:
    pass


@pytest.fixture(scope="module")
def env():
    e = Env()
    square = [np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 0.0]])]
    e.layers, e.other_layers = apt.MapLayers(countries=square), apt.MapLayers(lakes=square)
    e.settings = apt.MapSettings(yaw=0.02, hscale=1.1, vscale=0.9)
    e.tracks = [np.full((250, 2), 0.25), np.full((57, 2), 0.5)]
    e.overlays = [apt.MapOverlay(t, e.settings, e.layers) for t in e.tracks]
    ref = [apt.RefTime.Start(1580000000000), apt.RefTime.End(1580000600000)]
    e.orbits = {False: [apt.OrbitSettings("NOAA 19", TLE_2020, r) for r in ref],
                True: [apt.OrbitSettings("NOAA 19", TLE_2020, r, e.settings) for r in ref]}
    geometry = apt.MapSettings(yaw=0.03, hscale=1.2, vscale=0.8)
    e.grids = [apt.ProjectionSettings(apt.Projection.EQUIRECTANGULAR, 8, 5, 10.0, 20.0, 0.5, geometry=geometry),
               apt.ProjectionSettings(apt.Projection.MERCATOR, 9, 6, 11.0, 21.0, 0.25)]
    e.projection = (e.grids, D_OUT, OUT_CAP)
    e.png = (D_PNG, PNG_CAP)
    e.palette = np.zeros((256, 256, 3), np.uint8)
    e.colors = {"gray": None, "palette": apt.ColorSettings(e.palette, 0.5, -0.25, 0.75, 0.125),
                "lab": apt.ColorSettings(e.palette, 0.5, -0.25, 0.75, 0.125, equalize_lab=True)}
    e.plan = apt.Plan.__new__(apt.Plan)
    e.plan._p = None
    return e


def refused(expect, fn, *args, **kw):
    kind, text = expect
    with pytest.raises(apt.AptError) as info:
        fn(*args, **kw)
    assert (type(info.value), str(info.value)) == (kind, text)


# ------------------------------------------------------------------ part 1: refusals
def test_plan_refusals(env):
    e = env
    ov, o, drawn, grids = e.overlays, e.orbits[False], e.orbits[True], e.grids
    bad_png = ([1], [1, 2])
    other_settings = apt.MapOverlay(e.tracks[1], apt.MapSettings(yaw=0.5), e.layers)
    other_layers = apt.MapOverlay(e.tracks[1], e.settings, e.other_layers)
    rows = [
        # the colour type is checked first
        (COLOR, dict(color=3)),
        (COLOR, dict(color=3, map=ov, orbit=o)),
        (COLOR, dict(color=3, projection=(1, [1], [1]))),
        (COLOR, dict(color=3, orbit=drawn)),
        (COLOR, dict(color=3, png=bad_png)),
        # then: map and orbit exclude each other
        (EXCLUDE, dict(map=ov, orbit=o)),
        (EXCLUDE, dict(map=[ov[0]], orbit=[o[0]], png=bad_png)),
        (EXCLUDE, dict(map=ov, orbit=drawn)),
        # with a projection: its own triple first, then exactly one of map and orbit
        (PROJ_TUPLE, dict(projection=(grids[0], [1], [1, 2]), map=ov, orbit=o)),
        (PROJ_TUPLE, dict(projection=([grids[0]], [1, 2], [1, 2]), map=ov)),
        (PROJ_TUPLE, dict(projection=([grids[0], 3], [1, 2], [1, 2]), map=ov)),
        (PROJ_TUPLE, dict(projection=(grids, [1, 2], [1]))),
        (PROJ_TRACK_PLAN, dict(projection=e.projection)),
        (PROJ_TRACK_PLAN, dict(projection=e.projection, map=ov, orbit=o)),
        (PROJ_TRACK_PLAN, dict(projection=e.projection, png=bad_png)),
        # the swath with an orbit: the list, then draw_map's layers, then the png pair
        (ORBIT_LIST, dict(orbit=[o[0]])),
        (ORBIT_LIST, dict(orbit=[o[0], 3])),
        (ORBIT_LIST, dict(orbit=[o[0], ov[1]])),
        (ORBIT_LIST, dict(orbit=[drawn[0]], png=bad_png)),
        (NEEDS_LAYERS, dict(orbit=drawn)),
        (NEEDS_LAYERS, dict(orbit=drawn[0], layers=3)),
        (NEEDS_LAYERS, dict(orbit=drawn, png=bad_png)),
        (PNG_PAIR, dict(orbit=o, png=bad_png)),
        (PNG_PAIR, dict(orbit=drawn, layers=e.layers, png=([1, 2], [1]))),
        # the swath with a map or nothing: the png pair, then the list, then the shared settings and layers
        (PNG_PAIR, dict(png=bad_png)),
        (PNG_PAIR, dict(png=bad_png, map=[ov[0]])),
        (PNG_PAIR, dict(png=bad_png, map=[ov[0], other_settings])),
        (MAP_LIST, dict(map=[ov[0]])),
        (MAP_LIST, dict(map=[ov[0]], png=e.png)),
        (MAP_LIST, dict(map=[ov[0], e.tracks[1]])),
        (MAP_LIST, dict(map=e.tracks)),
        (MAP_LIST, dict(map=e.tracks, png=e.png)),
        (MAP_LIST, dict(map=[ov[0], o[1]])),
        (MAP_SHARE, dict(map=[ov[0], other_settings])),
        (MAP_SHARE, dict(map=[ov[0], other_layers])),
        (MAP_SHARE, dict(map=[ov[0], other_settings], png=e.png)),
        # the grid: the track's checks, then the png pair
        (ORBIT_LIST, dict(projection=e.projection, orbit=[o[0]])),
        (ORBIT_LIST, dict(projection=e.projection, orbit=[o[0], 3], png=bad_png)),
        (NEEDS_LAYERS, dict(projection=e.projection, orbit=drawn)),
        (NEEDS_LAYERS, dict(projection=e.projection, orbit=drawn, png=bad_png)),
        (MAP_LIST, dict(projection=e.projection, map=[ov[0]])),
        (MAP_LIST, dict(projection=e.projection, map=[ov[0]], png=bad_png)),
        (MAP_SHARE, dict(projection=e.projection, map=[ov[0], other_settings])),
        (MAP_SHARE, dict(projection=e.projection, map=[ov[0], other_layers], png=bad_png)),
        (MAP_PLAIN, dict(projection=e.projection, map=[e.tracks[0]])),
        (MAP_PLAIN, dict(projection=e.projection, map=e.tracks + e.tracks, png=bad_png)),
        (PNG_PAIR, dict(projection=e.projection, map=ov, png=bad_png)),
        (PNG_PAIR, dict(projection=e.projection, map=e.tracks, png=bad_png)),
        (PNG_PAIR, dict(projection=e.projection, orbit=o, png=bad_png)),
        (PNG_PAIR, dict(projection=e.projection, orbit=drawn, layers=e.layers, png=bad_png)),
        # every check of Python's passed, for each of the five entry points
        (BARE, dict()),
        (BARE, dict(color=e.colors["palette"], channels=4)),
        (BARE, dict(map=ov)),
        (BARE, dict(map=ov[0])),
        (BARE, dict(png=e.png)),
        (BARE, dict(png=e.png, map=ov)),
        (BARE, dict(orbit=o)),
        (BARE, dict(orbit=o[0], layers=e.layers)),
        (BARE, dict(orbit=drawn, layers=e.layers, png=e.png)),
        (BARE, dict(projection=e.projection, map=ov)),
        (BARE, dict(projection=e.projection, map=e.tracks, png=e.png)),
        (BARE, dict(projection=(grids[0], D_OUT, OUT_CAP), orbit=drawn[0], layers=e.layers)),
    ]
    for expect, kw in rows:
        refused(expect, e.plan.process_device_image, D_ROWS, ROWS_CAP, apt.Contrast.MINMAX, D_IMAGES, **kw)
    print(f"{len(rows)} plan calls refused as written down")


def test_one_shot_refusals(env):
    e = env
    sig = np.zeros(2 * 2080, np.float32)
    o, drawn, grid = e.orbits[False][0], e.orbits[True][0], e.grids[0]
    three = apt.MapOverlay(np.zeros((3, 2)), e.settings, e.layers)
    rows = [
        (DESPECKLE, dict(despeckle=3, projection=3, color=3)),
        # with a projection: its type, the colour's type, the track, then the track's own checks
        (PROJ_TYPE, dict(projection=3)),
        (PROJ_TYPE, dict(projection=3, color=3)),
        (PROJ_TYPE, dict(projection=(grid,), orbit=object(), png=True)),
        (COLOR, dict(projection=grid, color=3)),
        (COLOR, dict(projection=grid, color=3, orbit=drawn)),
        (COLOR, dict(projection=grid, color=3, orbit=three)),
        (PROJ_TRACK, dict(projection=grid)),
        (PROJ_TRACK, dict(projection=grid, png=True, layers=e.layers)),
        (NEEDS_LAYERS, dict(projection=grid, orbit=drawn)),
        (NEEDS_LAYERS, dict(projection=grid, orbit=drawn, layers=3, png=True)),
        (PROJ_ROWS, dict(projection=grid, orbit=three)),
        (PROJ_ROWS, dict(projection=grid, orbit=np.zeros((3, 2)), png=True)),
        (PROJ_ROWS, dict(projection=grid, orbit=[[0.0, 0.0]] * 3, color=e.colors["palette"])),
        # without: an orbit of another kind, then the colour's type, then the track's own checks
        (ORBIT_KIND, dict(orbit=object())),
        (ORBIT_KIND, dict(orbit=object(), png=True)),
        (ORBIT_KIND, dict(orbit=np.zeros((2, 2)), color=3)),
        (ORBIT_KIND, dict(orbit=3, color=3, png=True)),
        (COLOR, dict(color=3)),
        (COLOR, dict(color=3, png=True)),
        (COLOR, dict(color=e.palette, contrast=apt.Contrast.HISTOGRAM)),
        (COLOR, dict(color=3, orbit=drawn)),
        (COLOR, dict(color=3, orbit=three)),
        (COLOR, dict(color=3, orbit=three, png=True)),
        (NEEDS_LAYERS, dict(orbit=drawn)),
        (NEEDS_LAYERS, dict(orbit=drawn, layers=3, png=True)),
        (OVERLAY_ROWS, dict(orbit=three)),
        (OVERLAY_ROWS, dict(orbit=three, png=True)),
        (OVERLAY_ROWS, dict(orbit=three, color=e.colors["lab"], contrast=apt.Contrast.HISTOGRAM)),
    ]
    for expect, kw in rows:
        kw = dict(kw)
        refused(expect, apt.process, None, sig, kw.pop("contrast", apt.Contrast.MINMAX), **kw)
    print(f"{len(rows)} one-shot calls refused as written down")


def test_composite_and_project_image_refusals(env):
    e = env
    o, grid = e.orbits[False], e.grids[0]

    def device(**kw):
        args = dict(d_images=D_IMAGES, heights=ROWS_CAP, channels=[1, 4], projection=grid, d_out=D_OUT[0],
                    out_cap=OUT_CAP[0])
        args.update(kw)
        return e.plan.composite_device_images(**args)
    refused(PROJ_TYPE, device, projection=3, heights=[1])
    refused(COMPOSITE_COUNTS, device, heights=[1])
    refused(COMPOSITE_COUNTS, device, channels=[1, 4, 4], tracks=e.tracks, orbit=o)
    refused(COMPOSITE_TRACKS, device)
    refused(COMPOSITE_TRACKS, device, tracks=e.tracks, orbit=o)
    refused(ORBIT_LIST_PASS, device, orbit=[o[0]])
    refused(ORBIT_LIST_PASS, device, orbit=[o[0], 3])
    refused(ORBIT_LIST_PASS, device, orbit=[o[0], e.tracks[1]], settings=[None])
    refused(COMPOSITE_PLAIN, device, tracks=[e.tracks[0]])
    refused(COMPOSITE_PLAIN, device, tracks=e.tracks + e.tracks, settings=[None])
    refused(COMPOSITE_SETTINGS, device, tracks=e.tracks, settings=[None])
    refused(COMPOSITE_SETTINGS, device, orbit=o, settings=[e.settings, 3])
    refused(BARE, device, tracks=e.tracks)
    refused(BARE, device, orbit=o[0], settings=[e.settings, None], png=(D_PNG[0], PNG_CAP[0]))
    images = [np.zeros((4, 2080), np.uint8), np.zeros((3, 2080, 4), np.uint8)]
    tracks = [np.zeros((4, 2)), np.zeros((3, 2))]
    refused(PROJ_TYPE, apt.composite_images, images, tracks[:1], 3)
    refused(COMPOSITE_ONE_TRACK, apt.composite_images, images, tracks[:1], grid)
    refused(COMPOSITE_IMAGE, apt.composite_images, [images[0], np.zeros((3, 2080, 3), np.uint8)], tracks, grid)
    refused(COMPOSITE_IMAGE, apt.composite_images, [images[0].astype(np.float32)], tracks[:1], grid, settings=[None] * 2)
    refused(COMPOSITE_SETTINGS, apt.composite_images, images, tracks, grid, settings=[None])
    refused(COMPOSITE_SETTINGS, apt.composite_images, images, tracks, grid, settings=[e.settings, 3])
    refused(PROJECT_IMAGE, apt.project_image, np.zeros((4, 2079), np.uint8), tracks[0], 3)
    refused(PROJECT_IMAGE, apt.project_image, np.zeros((4, 2080, 3), np.uint8), tracks[0], grid)
    refused(PROJ_TYPE, apt.project_image, images[0], tracks[0], 3)
    refused(PROJ_TYPE, apt.project_image, images[1], tracks[1], (grid,), png=True)


# ------------------------------------------------------------------ part 2: dispatch and marshalling of the plan form
class Recorder:
    """Stands in for the loaded library: every function records (name, args) and returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


HEAD = ["plan", "count", "d_rows", "rows_cap", "contrast", "percent", "rotate", "color", "channels"]
TAILS = {
    "": ["d_images"],
    "_map": ["map", "layers", "positions", "n_positions", "d_images"],
    "_png": ["map", "layers", "positions", "n_positions", "d_images", "png", "d_png", "png_cap"],
    "_orbit": ["orbits", "layers", "d_images", "png", "d_png", "png_cap"],
    "_project": ["map", "layers", "positions", "n_positions", "orbits", "d_images", "proj", "d_out", "out_cap", "png",
                 "d_png", "png_cap"],
}
# (track, projected, png): (entry point, channels without colour, the trailing arguments that are NULL,
#                           (yaw, hscale, vscale) of the map settings handed over)
OVERLAY_MAP, GEOMETRY = (0.02, 1.1, 0.9), (0.03, 1.2, 0.8)
PLAN_CALLS = {
    ("none", False, False): ("", 1, [], None),
    ("none", False, True): ("_png", 1, ["map", "layers", "positions", "n_positions"], None),
    ("overlay", False, False): ("_map", 4, [], OVERLAY_MAP),
    ("overlay", False, True): ("_png", 4, [], OVERLAY_MAP),
    ("overlay", True, False): ("_project", 4, ["orbits", "d_png", "png_cap"], OVERLAY_MAP),
    ("overlay", True, True): ("_project", 4, ["orbits"], OVERLAY_MAP),
    ("orbit", False, False): ("_orbit", 1, ["layers", "d_png", "png_cap"], None),
    ("orbit", False, True): ("_orbit", 1, ["layers"], None),
    ("orbit", True, False): ("_project", 1, ["layers", "positions", "n_positions", "d_png", "png_cap"], GEOMETRY),
    ("orbit", True, True): ("_project", 1, ["layers", "positions", "n_positions"], GEOMETRY),
    ("orbit_map", False, False): ("_orbit", 4, ["d_png", "png_cap"], None),
    ("orbit_map", False, True): ("_orbit", 4, [], None),
    ("orbit_map", True, False): ("_project", 4, ["positions", "n_positions", "d_png", "png_cap"], OVERLAY_MAP),
    ("orbit_map", True, True): ("_project", 4, ["positions", "n_positions"], OVERLAY_MAP),
}
REF_TIMES = [(0, 1580000000000), (1, 1580000600000)]


def struct_of(arg):
    """The structure behind a byref() or pointer() argument."""
    return arg._obj if hasattr(arg, "_obj") else arg.contents


def addresses(pointers):
    return [C.cast(p, C.c_void_p).value for p in pointers]


def check_orbits(pointers, drawn):
    assert len(pointers) == 2
    for p, (kind, ms) in zip(pointers, REF_TIMES):
        c = p.contents
        assert (c.struct_size, c.flags, c.sat_name, c.ref_kind, c.ref_unix_ms) == (48, 0, b"NOAA 19", kind, ms)
        assert c.tle == TLE_2020.encode()
        assert bool(c.draw_map) == drawn
        if drawn:
            m = C.cast(c.draw_map, C.POINTER(api._CMapSettings)).contents
            assert (m.struct_size, m.yaw, m.hscale, m.vscale) == (32, 0.02, 1.1, 0.9)


def check_positions(e, pointers, counts):
    assert addresses(pointers) == [t.ctypes.data for t in e.tracks] and list(counts) == [250, 57]


def record(monkeypatch, fn, *args, **kw):
    """The calls fn makes into the library, with the stand-in in its place."""
    rec = Recorder()
    with monkeypatch.context() as m:
        m.setattr(api, "lib", lambda: rec)
        fn(*args, **kw)
    return rec.calls


def test_plan_dispatch_and_marshalling(env, monkeypatch):
    e = env
    seen = sorted({v[2:] for v in variants()})
    assert seen == sorted(PLAN_CALLS)
    for (track, projected, png), colour in [(v, c) for v in seen for c in ("gray", "palette", "lab")]:
        label = (track, projected, png, colour)
        entry, gray_channels, null, map_values = PLAN_CALLS[(track, projected, png)]
        kw = dict(color=e.colors[colour], rotate=apt.Rotate.YES)
        if track == "overlay":
            kw["map"] = e.overlays
        elif track != "none":
            kw.update(orbit=e.orbits[track == "orbit_map"], layers=e.layers if track == "orbit_map" else None)
        if projected:
            kw["projection"] = e.projection
        if png:
            kw["png"] = e.png
        calls = record(monkeypatch, e.plan.process_device_image, D_ROWS, ROWS_CAP, apt.Contrast.Percent(0.5),
                       D_IMAGES, **kw)
        # the layers get the settings' colours first (three layers), when a map is drawn; then the one entry point
        drawn = track in ("overlay", "orbit_map")
        assert [n for n, _ in calls] == ["aptgpu_map_layers_set_color"] * (3 if drawn else 0) + \
            ["aptgpu_plan_process_device_image" + entry], label
        for (_, (handle, index, rgba)), want in zip(calls[:-1], ((0, (255, 255, 0, 150)), (1, (255, 255, 0, 255)),
                                                                 (2, (50, 200, 200, 255)))):
            assert (handle.value, index, tuple(rgba)) == (e.layers._p.value, ) + want, label
        args = calls[-1][1]
        names = HEAD + TAILS[entry] + ["err", "err_cap"]
        assert len(args) == len(names), label
        a = dict(zip(names, args))
        assert a["plan"] is None and a["count"] == 2, label
        assert list(a["d_rows"]) == D_ROWS and list(a["rows_cap"]) == ROWS_CAP and list(a["d_images"]) == D_IMAGES, label
        assert (a["contrast"], a["percent"], a["rotate"]) == (1, 0.5, 1), label
        assert a["channels"] == (gray_channels if colour == "gray" else 4), label
        if colour == "gray":
            assert a["color"] is None, label
        else:
            c = struct_of(a["color"])
            assert (c.struct_size, c.flags) == (32, 1 if colour == "lab" else 0), label
            assert C.cast(c.palette_rgb, C.c_void_p).value == e.colors[colour].palette.ctypes.data, label
            assert (c.ch_a_tune_start, c.ch_a_tune_end, c.ch_b_tune_start, c.ch_b_tune_end) == (0.5, -0.25, 0.75, 0.125)
        assert [n for n in TAILS[entry] if a[n] is None] == [n for n in TAILS[entry] if n in null], label
        assert len(a["err"]) == a["err_cap"] > 0, label
        if a.get("map") is not None:
            m = struct_of(a["map"])
            assert (m.struct_size, m.reserved, m.yaw, m.hscale, m.vscale) == (32, 0) + map_values, label
        else:
            assert map_values is None, label
        if a.get("layers") is not None:
            assert a["layers"].value == e.layers._p.value, label
        if a.get("positions") is not None:
            check_positions(e, a["positions"], a["n_positions"])
        if a.get("orbits") is not None:
            check_orbits(a["orbits"], track == "orbit_map")
        if "png" in a:
            s = struct_of(a["png"])
            assert (s.struct_size, s.flags) == (8, 0), label
        if a.get("d_png") is not None:
            assert list(a["d_png"]) == D_PNG and list(a["png_cap"]) == PNG_CAP, label
        if projected:
            assert list(a["d_out"]) == D_OUT and list(a["out_cap"]) == OUT_CAP, label
            grids = [a["proj"][i] for i in range(2)]
            assert [(g.struct_size, g.kind, g.width, g.height, g.lat_north, g.lon_west, g.step, g.channel, g.sampling,
                     g.grid_deg, tuple(g.grid_color), g.reserved) for g in grids] == [
                (64, 0, 8, 5, 10.0, 20.0, 0.5, 0, 0, 0.0, (255, 255, 255, 255), 0),
                (64, 1, 9, 6, 11.0, 21.0, 0.25, 0, 0, 0.0, (255, 255, 255, 255), 0)], label
    print(f"{3 * len(seen)} plan calls recorded")


def test_plan_dispatch_of_the_other_argument_forms(env, monkeypatch):
    """One MapOverlay, one OrbitSettings and one ProjectionSettings for every recording; plain tracks under a
    projection; channels given."""
    e = env

    def call(**kw):
        calls = record(monkeypatch, e.plan.process_device_image, D_ROWS, ROWS_CAP, apt.Contrast.HISTOGRAM, D_IMAGES, **kw)
        name, args = calls[-1]
        entry = name[len("aptgpu_plan_process_device_image"):]
        a = dict(zip(HEAD + TAILS[entry] + ["err", "err_cap"], args))
        assert (a["contrast"], a["percent"], a["rotate"]) == (3, 0.0, 0)
        return entry, a, len(calls) - 1
    entry, a, colours = call(channels=4)
    assert (entry, a["channels"], a["color"], colours) == ("", 4, None, 0)
    entry, a, colours = call(channels=1, color=e.colors["lab"], png=e.png)
    assert (entry, a["channels"], colours) == ("_png", 1, 0) and a["color"] is not None
    entry, a, colours = call(map=e.overlays[1])
    assert (entry, a["channels"], colours) == ("_map", 4, 3)
    assert addresses(a["positions"]) == [e.tracks[1].ctypes.data] * 2 and list(a["n_positions"]) == [57, 57]
    entry, a, colours = call(orbit=e.orbits[True][1], layers=e.layers, channels=1)
    assert (entry, a["channels"], colours) == ("_orbit", 1, 3)
    assert [p.contents.ref_unix_ms for p in a["orbits"]] == [1580000600000] * 2
    entry, a, colours = call(map=e.tracks, projection=(e.grids[1], D_OUT, OUT_CAP), png=e.png)
    assert (entry, a["channels"], colours) == ("_project", 1, 0)
    assert a["layers"] is None and a["orbits"] is None
    check_positions(e, a["positions"], a["n_positions"])
    m = struct_of(a["map"])
    assert (m.yaw, m.hscale, m.vscale) == (0.0, 1.0, 1.0)  # (no overlay, no geometry: the defaults)
    assert [a["proj"][i].width for i in range(2)] == [9, 9]
    entry, a, colours = call(map=[list(map(list, t)) for t in e.tracks], projection=e.projection)
    assert (entry, colours) == ("_project", 0) and list(a["n_positions"]) == [250, 57]
    m = struct_of(a["map"])
    assert (m.yaw, m.hscale, m.vscale) == GEOMETRY  # (of the first recording's grid)


COMPOSITE = ["plan", "count", "d_images", "heights", "channels", "positions", "n_positions", "orbits", "maps", "proj",
             "composite", "d_out", "out_cap", "d_coverage", "png", "d_png", "png_cap", "err", "err_cap"]


def test_composite_dispatch_and_marshalling(env, monkeypatch):
    e = env

    def call(**kw):
        calls = record(monkeypatch, e.plan.composite_device_images, D_IMAGES, ROWS_CAP, [1, 4], e.grids[1], D_OUT[0],
                       OUT_CAP[0], **kw)
        assert [n for n, _ in calls] == ["aptgpu_plan_composite_device_images"] and len(calls[0][1]) == len(COMPOSITE)
        a = dict(zip(COMPOSITE, calls[0][1]))
        assert a["plan"] is None and a["count"] == 2 and list(a["d_images"]) == D_IMAGES
        assert list(a["heights"]) == ROWS_CAP and list(a["channels"]) == [1, 4]
        assert (a["d_out"], a["out_cap"]) == (D_OUT[0], OUT_CAP[0])
        g, c, s = struct_of(a["proj"]), struct_of(a["composite"]), struct_of(a["png"])
        assert (g.struct_size, g.kind, g.width, g.height) == (64, 1, 9, 6)
        assert (c.struct_size, c.reserved) == (12, 0) and (s.struct_size, s.flags) == (8, 0)
        return a, c.blend

    def maps(a):
        return [(m.contents.yaw, m.contents.hscale, m.contents.vscale) for m in a["maps"]]
    a, blend = call(tracks=e.tracks)
    check_positions(e, a["positions"], a["n_positions"])
    assert a["orbits"] is None and blend == 1 and maps(a) == [(0.0, 1.0, 1.0)] * 2
    assert (a["d_coverage"], a["d_png"], a["png_cap"]) == (None, None, 0)
    a, blend = call(tracks=e.tracks, settings=[None, e.settings], blend=apt.Composite.FEATHER, d_coverage=0x9000,
                    png=(D_PNG[0], PNG_CAP[0]))
    check_positions(e, a["positions"], a["n_positions"])
    assert blend == 2 and maps(a) == [(0.0, 1.0, 1.0), OVERLAY_MAP]
    assert (a["d_coverage"], a["d_png"], a["png_cap"]) == (0x9000, D_PNG[0], PNG_CAP[0])
    a, blend = call(orbit=e.orbits[True])
    assert a["positions"] is None and a["n_positions"] is None and a["maps"] is None
    check_orbits(a["orbits"], True)
    a, blend = call(orbit=e.orbits[False], settings=e.settings, blend=apt.Composite.FIRST)
    check_orbits(a["orbits"], False)
    assert blend == 0 and maps(a) == [OVERLAY_MAP] * 2
    a, blend = call(orbit=e.orbits[False][1])
    assert [p.contents.ref_unix_ms for p in a["orbits"]] == [1580000600000] * 2 and a["maps"] is None
