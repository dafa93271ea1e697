"""The argument checks of the image entry points of include/aptgpu.h, as (return code, err text), for every error that
is raised before the device is touched: which check each entry point makes, and which one wins when two fail.  The
expectations are literals; no GPU is needed.  The plan forms are called with plan = NULL: their own checks still run
and give text, and once those pass the result is a bare APTGPU_ERR_INVALID with an empty err."""
import ctypes as C
import os

import numpy as np
import pytest

import noaa_apt_amd as apt
from noaa_apt_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
TLE_2020 = open(os.path.join(HERE, "golden", "tle", "noaa_2020.txt")).read().encode()

INTERNAL, INVALID, UNSUPPORTED = 1, 4, 5

CONTRAST = (INVALID, "unknown contrast adjustment")
ROT_ORBIT = (UNSUPPORTED, "Rotate::Orbit needs the satellite and the time: aptgpu_orbit_settings, the *_orbit entry points")
CHANNELS = (INVALID, "channels must be 1 (gray) or 4 (RGBA)")
COLOR_SIZE = (INVALID, "aptgpu_color_settings: struct_size or palette_rgb not set")
COLOR_FLAGS = (INVALID, "aptgpu_color_settings: unknown flags")
FLOAT_COLOR = (UNSUPPORTED, "APTGPU_CONTRAST_HISTOGRAM_FLOAT equalises the gray image only: the reference has no "
               "float-domain equalisation of a false-colour image (pass color = NULL)")
LAB_FLAG = (UNSUPPORTED, "histogram equalisation of a false-colour image (CIE Lab, imageext.rs:51-64) needs "
            "APTGPU_COLOR_EQUALIZE_LAB in aptgpu_color_settings.flags")
COLOR_CH = (INVALID, "false colour needs channels = 4 (RGBA)")
MAP_SIZE = (INVALID, "aptgpu_map_settings: struct_size not set, or no layer set")
MAP_CH = (INVALID, "the map overlay needs channels = 4 (RGBA)")
MAPSET_SIZE = (INVALID, "aptgpu_map_settings: struct_size not set")
PNG_SIZE = (INVALID, "aptgpu_png_settings: struct_size not set")
PNG_FLAGS = (INVALID, "aptgpu_png_settings: unknown flags")
PNG_ZERO = (INVALID, "a PNG needs a width and a height of at least 1")
PNG_LARGE = (INVALID, "image too large for the PNG encoder (2^31 bytes)")
TOGETHER = (INVALID, "map, layers and sat_positions must be given together")
OUTPUT = (INVALID, "unknown output kind")
ORBIT_SIZE = (INVALID, "aptgpu_orbit_settings: struct_size not set")
ORBIT_FLAGS = (INVALID, "aptgpu_orbit_settings: unknown flags")
ORBIT_NAME = (INVALID, "aptgpu_orbit_settings: sat_name not set")
ORBIT_KIND = (INVALID, "aptgpu_orbit_settings: unknown ref_kind")
ORBIT_TLE = (UNSUPPORTED, "aptgpu_orbit_settings: tle is NULL (the reference then downloads the current TLE, "
             "misc::get_current_tle; pass the text)")
ORBIT_SAT = (INTERNAL, 'Satellite "NOAA 99" not found in TLE')
PROJ_ROT = (INVALID, "a projection takes rotate = APTGPU_ROTATE_NO only: it reads the unrotated image and north is up "
            "by construction")
EXACTLY = (INVALID, "a projection needs exactly one of sat_positions and aptgpu_orbit_settings")
PROJ_SIZE = (INVALID, "aptgpu_projection_settings: struct_size not set")
PROJ_KIND = (INVALID, "aptgpu_projection_settings: unknown kind")
PROJ_STEP = (INVALID, "aptgpu_projection_settings: step must be finite and > 0")
PROJ_PIXELS = (INVALID, "aptgpu_projection_settings: width * height exceeds APTGPU_PROJECTION_MAX_PIXELS (2^26)")
PROJ_RESERVED = (INVALID, "aptgpu_projection_settings: reserved must be 0")
PROJ_CHANNEL = (INVALID, "aptgpu_projection_settings: unknown channel")
PROJ_SAMPLING = (INVALID, "aptgpu_projection_settings: unknown sampling")
PROJ_EMPTY = (INVALID, "aptgpu_projection_settings: width and height must be at least 1")
PROJ_LAT = (INVALID, "aptgpu_projection_settings: lat_north must be within [-90, 90]")
PROJ_LON = (INVALID, "aptgpu_projection_settings: lon_west must be finite")
PROJ_LAST_ROW = (INVALID, "aptgpu_projection_settings: the last row's latitude must be within [-90, 90]")
PROJ_GRID = (INVALID, "aptgpu_projection_settings: grid_deg must be finite and >= 0")
PROJ_GRID_STEP = (INVALID, "aptgpu_projection_settings: grid_deg must be 0 or at least step")
NOROW_MAP = (INTERNAL, "map overlay: the image has no row to draw on")
NOROW_PNG = (INVALID, "PNG encoding: the image has no row")
NOROW_PROJ = (INTERNAL, "reprojection: the image has no row to read")
NOROW_PROJ_IMAGE = (INVALID, "reprojection: the image has no row to read")
NULL_POSITIONS = (INVALID, "null sat_positions")
BARE = (INVALID, "")

vp, sz = C.c_void_p, C.c_size_t
_keep = []  # (everything the structures below point to)


def _ptr(obj):
    _keep.append(obj)
    return C.pointer(obj)


def color(size=None, flags=0, palette=True):
    pal = np.zeros(256 * 256 * 3, np.uint8)
    _keep.append(pal)
    return _ptr(api._CColorSettings(C.sizeof(api._CColorSettings) if size is None else size, flags,
                                    pal.ctypes.data_as(api._u8p) if palette else None, 0, 0, 0, 0))


def mapset(size=None):
    return _ptr(api._CMapSettings(C.sizeof(api._CMapSettings) if size is None else size, 0, 0.0, 1.0, 1.0))


def png(size=None, flags=0):
    return _ptr(api._CPngSettings(C.sizeof(api._CPngSettings) if size is None else size, flags))


def orbit(size=None, flags=0, name=b"NOAA 19", tle=TLE_2020, kind=0, draw_map=None):
    o = api._COrbitSettings(C.sizeof(api._COrbitSettings) if size is None else size, flags, name, tle, kind, 0,
                            1580000000000, C.cast(draw_map, vp) if draw_map is not None else None)
    return _ptr(o)


def proj(size=None, kind=0, width=32, height=16, step=0.5, reserved=0, lat_north=40.0, lon_west=-10.0, channel=0,
         sampling=0, grid_deg=0.0):
    p = api._CProjectionSettings(C.sizeof(api._CProjectionSettings) if size is None else size, kind, width, height,
                                 lat_north, lon_west, step, channel, sampling, grid_deg, (C.c_uint8 * 4)(0, 0, 0, 255),
                                 reserved)
    return _ptr(p)


@pytest.fixture(scope="module")
def layers():
    h = vp()
    assert apt.lib().aptgpu_map_layers_create(C.byref(h)) == 0
    yield h
    apt.lib().aptgpu_map_layers_destroy(h)


SIGNAL = np.zeros(2 * 2080, np.float32)
TRACK = np.zeros(2 * 2, np.float64)
IMAGE = np.zeros(2 * 2080 * 4, np.uint8)
FAKE = 0x10000  # a device address no check dereferences (the plan is NULL)


def _arr(ctype, *values):
    a = (ctype * len(values))(*values)
    _keep.append(a)
    return a


# The arguments of each entry point in order (without err, err_cap), and what each key is when a case does not set it.
HEAD = ["ctx", "signal", "n", "contrast", "percent", "rotate", "color", "channels"]
PLAN = ["plan", "count", "d_rows", "rows_cap", "contrast", "percent", "rotate", "color", "channels"]
ARGS = {
    "aptgpu_process_gray": ["ctx", "signal", "n", "contrast", "percent", "rotate", "out", "n_out", "info"],
    "aptgpu_plan_process_device": ["plan", "count", "d_rows", "rows_cap", "contrast", "percent", "rotate", "d_images"],
    "aptgpu_process_image": HEAD + ["out", "n_out", "info"],
    "aptgpu_plan_process_device_image": PLAN + ["d_images"],
    "aptgpu_process_image_map": HEAD + ["map", "layers", "sat_positions", "out", "n_out", "info"],
    "aptgpu_plan_process_device_image_map": PLAN + ["map", "layers", "positions", "n_positions", "d_images"],
    "aptgpu_process_image_png": HEAD + ["map", "layers", "sat_positions", "png", "out", "n_out", "info"],
    "aptgpu_plan_process_device_image_png": PLAN + ["map", "layers", "positions", "n_positions", "d_images", "png",
                                                    "d_png", "png_cap"],
    "aptgpu_process_image_orbit": HEAD + ["orbit", "layers", "output", "png", "out", "n_out", "info"],
    "aptgpu_plan_process_device_image_orbit": PLAN + ["orbits", "layers", "d_images", "png", "d_png", "png_cap"],
    "aptgpu_process_image_project": HEAD + ["map", "layers", "sat_positions", "orbit", "proj", "output", "png", "out",
                                            "n_out", "info"],
    "aptgpu_plan_process_device_image_project": PLAN + ["map", "layers", "positions", "n_positions", "orbits",
                                                        "d_images", "proj", "d_out", "out_cap", "png", "d_png",
                                                        "png_cap"],
    "aptgpu_project_image": ["ctx", "image", "height", "channels", "sat_positions", "n_positions1", "map", "proj",
                             "output", "png", "out", "n_out"],
    "aptgpu_encode_png": ["ctx", "image", "width", "height", "channels", "png", "out", "n_out"],
}
SHORT = {name.replace("aptgpu_", "").replace("process_device_", "").replace("process_", ""): name for name in ARGS}
# keys that are NULL unless the entry point's defaults (below) or the case say otherwise
NULLS = ["ctx", "plan", "color", "map", "layers", "sat_positions", "positions", "n_positions", "png", "orbit", "orbits",
         "info", "d_png", "png_cap", "d_out", "out_cap", "proj"]


def defaults(name, layers):
    d = {k: None for k in NULLS}
    d.update(signal=SIGNAL.ctypes.data_as(api._f32p), n=SIGNAL.size, contrast=2, percent=0.98, rotate=0, channels=4,
             out=C.pointer(api._u8p()), n_out=C.pointer(sz()), output=0, count=1, d_rows=_arr(vp, FAKE),
             rows_cap=_arr(sz, 2), d_images=_arr(vp, FAKE), image=IMAGE.ctypes.data_as(api._u8p), height=2, width=2080,
             n_positions1=2)
    track = TRACK.ctypes.data_as(api._f64p)
    tracks = dict(positions=_arr(api._f64p, track), n_positions=_arr(sz, 2))
    if name.endswith("_map"):
        d.update(map=mapset(), layers=layers, sat_positions=track, **tracks)
    if name.endswith("_png") and "plan" in name:
        d.update(d_png=_arr(vp, FAKE), png_cap=_arr(sz, 1 << 20))
    if name.endswith("_orbit"):
        d.update(orbit=orbit(), orbits=_arr(C.POINTER(api._COrbitSettings), orbit()))
    if name.endswith("_project"):
        d.update(sat_positions=track, proj=proj(), d_out=_arr(vp, FAKE), out_cap=_arr(sz, 32 * 16 * 4), **tracks)
    if name == "aptgpu_project_image":
        d.update(sat_positions=track, proj=proj())
    return d


def call(name, layer_set, over):
    d = defaults(name, layer_set)
    for k, v in over.items():
        assert k in d, k
        d[k] = layer_set if isinstance(v, str) and v == "LAYERS" else v
    err = C.create_string_buffer(1024)
    rc = getattr(apt.lib(), name)(*[d[k] for k in ARGS[name]], err, len(err))
    return rc, err.value.decode()


MAP3 = dict(map=mapset(), layers="LAYERS", sat_positions=TRACK.ctypes.data_as(api._f64p))
PLAN_MAP3 = dict(map=mapset(), layers="LAYERS", positions=_arr(api._f64p, TRACK.ctypes.data_as(api._f64p)),
                 n_positions=_arr(sz, 2))
ORBITS = lambda *o: _arr(C.POINTER(api._COrbitSettings), *o)  # noqa: E731
BAD_COLOR = dict(color=color(flags=2))
# (plan_image and plan_image_orbit look at the plan, which is NULL here, before they reach color_args)
ALL_IMAGE = ["image", "image_map", "plan_image_map", "image_png", "plan_image_png", "image_project", "plan_image_project"]
ORBIT_FORMS = ["image_orbit"]

CASES = []


def case(short, expect, **over):
    for s in ([short] if isinstance(short, str) else short):
        CASES.append(pytest.param(SHORT[s], over, expect, id=f"{s}-{len(CASES)}"))


# ---- every single bad argument
# color_args, in every form that takes a colour (the orbit forms reach it too: their other arguments are valid)
for forms in (ALL_IMAGE, ORBIT_FORMS):
    case(forms, CONTRAST, contrast=5)
    case(forms, CONTRAST, contrast=-1)
    case(forms, CHANNELS, channels=3)
    case(forms, COLOR_SIZE, color=color(size=8))
    case(forms, COLOR_SIZE, color=color(palette=False))
    case(forms, COLOR_FLAGS, color=color(flags=2))
    case(forms, FLOAT_COLOR, contrast=4, color=color())
    case(forms, LAB_FLAG, contrast=3, color=color())
case(["image", "image_png", "plan_image_png", "image_project", "plan_image_project"] + ORBIT_FORMS, COLOR_CH,
     color=color(), channels=1)
case(["image", "image_map", "plan_image_map", "image_png", "plan_image_png"], ROT_ORBIT, rotate=2)
case("image", ROT_ORBIT, rotate=7)
case("gray", CONTRAST, contrast=3)
case("gray", CONTRAST, contrast=-1)
case("gray", ROT_ORBIT, rotate=2)
case("plan_device", BARE, contrast=3, rotate=2)  # (the plan, NULL here, is looked at first)
# map_args
case(["image_map", "plan_image_map"], MAP_SIZE, map=mapset(size=8))
case(["image_map", "plan_image_map"], MAP_SIZE, map=None)
case(["image_map", "plan_image_map"], MAP_SIZE, layers=None)
case(["image_map", "plan_image_map"], MAP_CH, channels=1)
case("image_png", MAP_SIZE, **dict(MAP3, map=mapset(size=8)))
case("image_png", MAP_CH, channels=1, **MAP3)
case("plan_image_png", MAP_SIZE, **dict(PLAN_MAP3, map=mapset(size=8)))
case("plan_image_png", MAP_CH, channels=1, **PLAN_MAP3)
case("image_orbit", MAP_SIZE, orbit=orbit(draw_map=mapset()))  # (no layer set)
case("image_orbit", MAP_CH, orbit=orbit(draw_map=mapset()), layers="LAYERS", channels=1)
case(["image_project", "plan_image_project"], MAP_CH, layers="LAYERS", channels=1)
case(["image_project", "plan_image_project"], MAPSET_SIZE, map=mapset(size=8))
# png_args
for bad, want in ((png(size=4), PNG_SIZE), (png(flags=1), PNG_FLAGS)):
    case(["image_png", "plan_image_png", "encode_png"], want, png=bad)
    case(["image_orbit", "image_project", "project_image"], want, png=bad, output=1)
    case(["plan_image_orbit", "plan_image_project"], want, png=bad, d_png=_arr(vp, FAKE), png_cap=_arr(sz, 1 << 20))
# given together
case("image_png", TOGETHER, map=mapset())
case("image_png", TOGETHER, layers="LAYERS")
case("image_png", TOGETHER, sat_positions=TRACK.ctypes.data_as(api._f64p))
case("image_png", TOGETHER, map=mapset(), layers="LAYERS")  # (n >= 2080: the positions are needed)
case("plan_image_png", TOGETHER, map=mapset(), layers="LAYERS")
case("plan_image_png", TOGETHER, positions=PLAN_MAP3["positions"])
# output kind
case(["image_orbit", "image_project", "project_image"], OUTPUT, output=2)
case(["image_orbit", "image_project", "project_image"], OUTPUT, output=-1)
# orbit_args
for bad, want in ((orbit(size=8), ORBIT_SIZE), (orbit(flags=1), ORBIT_FLAGS), (orbit(name=None), ORBIT_NAME),
                  (orbit(kind=2), ORBIT_KIND), (orbit(tle=None), ORBIT_TLE), (orbit(name=b"NOAA 99"), ORBIT_SAT),
                  (orbit(draw_map=mapset(size=8)), MAPSET_SIZE)):
    case("image_orbit", want, orbit=bad)
    case("image_project", want, orbit=bad, sat_positions=None)
case("image_orbit", ORBIT_SIZE, orbit=None)
case(ORBIT_FORMS[:1], CONTRAST, rotate=2, contrast=5)  # ROTATE_ORBIT is accepted: the next error is the contrast's
case("image_orbit", CONTRAST, output=0, png=png(flags=1), contrast=5)  # (the png settings are read for a PNG only)
# the projection
case(["image_project", "plan_image_project"], PROJ_ROT, rotate=1)
case(["image_project", "plan_image_project"], PROJ_ROT, rotate=2)
case("image_project", EXACTLY, orbit=orbit())
case("image_project", EXACTLY, sat_positions=None)
case("plan_image_project", EXACTLY, orbits=ORBITS(orbit()))
case("plan_image_project", EXACTLY, positions=None)
case("plan_image_project", EXACTLY, n_positions=None)
for bad, want in ((proj(size=8), PROJ_SIZE), (proj(kind=2), PROJ_KIND), (proj(step=0.0), PROJ_STEP),
                  (proj(width=1 << 14, height=1 << 13), PROJ_PIXELS), (proj(reserved=1), PROJ_RESERVED),
                  (proj(channel=2), PROJ_CHANNEL), (proj(sampling=2), PROJ_SAMPLING), (proj(width=0), PROJ_EMPTY),
                  (proj(height=0), PROJ_EMPTY), (proj(step=float("nan")), PROJ_STEP), (proj(lat_north=91.0), PROJ_LAT),
                  (proj(lat_north=float("nan")), PROJ_LAT), (proj(lon_west=float("inf")), PROJ_LON),
                  (proj(height=400), PROJ_LAST_ROW), (proj(grid_deg=-1.0), PROJ_GRID),
                  (proj(grid_deg=float("nan")), PROJ_GRID), (proj(grid_deg=0.25), PROJ_GRID_STEP),
                  (proj(kind=2, channel=2), PROJ_KIND), (proj(channel=2, sampling=2), PROJ_CHANNEL),
                  (proj(grid_deg=0.25, reserved=1), PROJ_GRID_STEP)):
    case(["image_project", "plan_image_project", "project_image"], want, proj=bad)
case(["image_project", "project_image"], PROJ_SIZE, proj=None)
case("plan_image_project", ORBIT_SIZE, positions=None, n_positions=None, orbits=ORBITS(None))
case("project_image", CHANNELS, channels=3)
case("project_image", NOROW_PROJ_IMAGE, height=0)
case("project_image", NOROW_PROJ_IMAGE, image=None)
case("project_image", NULL_POSITIONS, sat_positions=None)
# the PNG's size (a projection's grid cannot reach it: APTGPU_PROJECTION_MAX_PIXELS is refused first)
case("encode_png", PNG_LARGE, width=30000, height=30000)
case("encode_png", PNG_ZERO, width=0)
case("encode_png", CHANNELS, channels=2)
case("encode_png", (INVALID, "null image"), image=None)
# n = 1000: no row
case("image_map", NOROW_MAP, n=1000)
case("image_png", NOROW_PNG, n=1000)
case("image_orbit", NOROW_MAP, n=1000, orbit=orbit(draw_map=mapset()), layers="LAYERS")
case("image_orbit", NOROW_PNG, n=1000, output=1)
case("image_project", NOROW_PROJ, n=1000)

# ---- pairs: who wins
case(ALL_IMAGE[:5], CONTRAST, contrast=5, rotate=2, channels=3)
case(ALL_IMAGE[:5], ROT_ORBIT, rotate=2, channels=3)
case("gray", CONTRAST, contrast=5, rotate=2)
case(ALL_IMAGE + ORBIT_FORMS, CHANNELS, channels=3, color=color(size=8))
case(ALL_IMAGE + ORBIT_FORMS, COLOR_SIZE, color=color(size=8, flags=2))
case(ALL_IMAGE + ORBIT_FORMS, COLOR_FLAGS, contrast=4, color=color(flags=2))
case(ALL_IMAGE + ORBIT_FORMS, FLOAT_COLOR, contrast=4, color=color(), channels=1)
case(ALL_IMAGE + ORBIT_FORMS, LAB_FLAG, contrast=3, color=color(), channels=1)
# _map: a bare INVALID for the missing positions, then color_args, then map_args
case("image_map", BARE, sat_positions=None, contrast=5, map=None)
case("image_map", CONTRAST, sat_positions=None, n=1000, contrast=5, map=None)  # (n < 2080: no positions needed)
case(["image_map", "plan_image_map"], COLOR_FLAGS, map=None, **BAD_COLOR)
case(["image_map", "plan_image_map"], COLOR_CH, color=color(), channels=1, layers=None)
case(["image_map", "plan_image_map"], MAP_SIZE, map=mapset(size=8), channels=1)
case("plan_image_map", BARE, positions=None)
case("plan_image_map", BARE, n_positions=None)
case("plan_image_map", MAP_SIZE, positions=None, layers=None)
# _png: color_args, png_args, given together, map_args
case(["image_png", "plan_image_png"], COLOR_FLAGS, png=png(flags=1), map=mapset(), **BAD_COLOR)
case(["image_png", "plan_image_png"], PNG_FLAGS, png=png(flags=1), map=mapset())
case("image_png", TOGETHER, **dict(MAP3, map=mapset(size=8), sat_positions=None))
case("plan_image_png", TOGETHER, **dict(PLAN_MAP3, map=mapset(size=8), positions=None))
case("plan_image_png", BARE, d_png=None, contrast=5)
case("plan_image_png", BARE, png_cap=None, contrast=5)
case("plan_image_png", BARE, **dict(PLAN_MAP3, n_positions=None))
# _orbit: output kind, orbit_args, png_args, map_args, and only then color_args
case("image_orbit", OUTPUT, output=2, orbit=orbit(flags=1))
case("image_orbit", ORBIT_FLAGS, output=1, orbit=orbit(flags=1), png=png(flags=1))
case("image_orbit", PNG_FLAGS, output=1, png=png(flags=1), orbit=orbit(draw_map=mapset()))
case("image_orbit", MAP_SIZE, orbit=orbit(draw_map=mapset()), contrast=5)
case("image_orbit", ORBIT_KIND, orbit=orbit(kind=2), contrast=5)
case("image_orbit", ORBIT_TLE, orbit=orbit(tle=None), contrast=5, channels=3)
case("plan_image_orbit", BARE, orbits=None, contrast=5)
case("plan_image_orbit", BARE, d_png=_arr(vp, FAKE), contrast=5)  # (no png_cap)
case("plan_image_orbit", PNG_FLAGS, d_png=_arr(vp, FAKE), png_cap=_arr(sz, 1), png=png(flags=1), contrast=5)
case("plan_image_orbit", BARE, orbits=ORBITS(orbit(flags=1)), contrast=5)  # (the plan is NULL before orbit_args)
# _project: output kind, rotate, exactly one, color_args, orbit_args, png_args, the settings, map_args
case("image_project", OUTPUT, output=2, rotate=1)
case(["image_project", "plan_image_project"], PROJ_ROT, rotate=1, sat_positions=None, positions=None, contrast=5)
case("image_project", EXACTLY, sat_positions=None, contrast=5)
case("plan_image_project", EXACTLY, positions=None, contrast=5)
case("image_project", CONTRAST, contrast=5, sat_positions=None, orbit=orbit(flags=1))
case("image_project", ORBIT_FLAGS, sat_positions=None, orbit=orbit(flags=1), output=1, png=png(flags=1))
case(["image_project"], PNG_FLAGS, output=1, png=png(flags=1), proj=proj(kind=2))
case("plan_image_project", PNG_FLAGS, d_png=_arr(vp, FAKE), png_cap=_arr(sz, 1), png=png(flags=1), proj=proj(kind=2))
case(["image_project", "plan_image_project"], PROJ_KIND, proj=proj(kind=2), layers="LAYERS", channels=1)
case(["image_project", "plan_image_project"], COLOR_FLAGS, proj=proj(kind=2), **BAD_COLOR)
case("plan_image_project", BARE, count=-1, rotate=1)
case("plan_image_project", BARE, proj=None, rotate=1)
case("plan_image_project", BARE, d_out=None, rotate=1)
case("plan_image_project", BARE, out_cap=None, rotate=1)
case("plan_image_project", BARE, d_png=_arr(vp, FAKE), rotate=1)
# the no-row errors: map, png, projection
case("image_png", NOROW_MAP, n=1000, **MAP3)
case("image_project", NOROW_MAP, n=1000, layers="LAYERS", output=1)
case("image_project", NOROW_PNG, n=1000, output=1)
case("image_map", CONTRAST, n=1000, contrast=5)

# ---- NULL outputs: a bare INVALID where the entry point looks at them
case(["gray", "image"], BARE, out=None, contrast=5)
case(["gray", "image"], BARE, n_out=None, contrast=5)
case(["gray", "image"], BARE, signal=None, contrast=5)
case(["image_map", "image_png", "image_project"], CONTRAST, out=None, contrast=5)  # (behind their own checks)
case(["image_map", "image_png", "image_orbit", "image_project"], BARE, out=None)
case(["image_map", "image_png", "image_orbit", "image_project"], BARE, n_out=None)
case(["image_map", "image_png", "image_orbit", "image_project"], BARE, signal=None)
case("image_orbit", BARE, out=None, contrast=5)  # (before color_args there)
case("image_orbit", ORBIT_FLAGS, out=None, orbit=orbit(flags=1))
case(["project_image", "encode_png"], BARE, out=None, channels=3)
case(["project_image", "encode_png"], BARE, n_out=None, channels=3)
# ---- the plan forms with plan = NULL once their own checks pass
PLAN_FORMS = ["plan_device", "plan_image", "plan_image_map", "plan_image_png", "plan_image_orbit", "plan_image_project"]
case(PLAN_FORMS, BARE)
case(PLAN_FORMS, BARE, count=-1)
case(PLAN_FORMS, BARE, d_rows=None)
case(PLAN_FORMS, BARE, rows_cap=None)
case(PLAN_FORMS, BARE, d_images=None)
case(["plan_device", "plan_image", "plan_image_orbit"], BARE, contrast=5)  # (the plan is looked at first)
case(["plan_image_map", "plan_image_png", "plan_image_project"], CONTRAST, contrast=5, d_images=None)



@pytest.mark.parametrize("name,over,expect", CASES)
def test_argument_error(layers, name, over, expect):
    assert call(name, layers, over) == expect


@pytest.mark.parametrize("short", ["image", "image_map", "image_png", "image_orbit", "image_project"])
def test_a_call_without_one_output_touches_neither(layers, short):
    held = api._u8p()
    C.cast(C.pointer(held), C.POINTER(vp))[0] = FAKE
    assert call(SHORT[short], layers, dict(out=C.pointer(held), n_out=None)) == BARE
    assert C.cast(held, vp).value == FAKE
    size = sz(77)
    assert call(SHORT[short], layers, dict(out=None, n_out=C.pointer(size))) == BARE
    assert size.value == 77
