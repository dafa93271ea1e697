"""CPU-side checks of the composite: tests/np_composite_model.py pinned against
tests/np_project_model.py and a hand-computed pixel, the conditions every case of tests/composite_cases.py has to
meet on the model alone (so that the GPU test's allowance is a property of the inputs, not of the code under test),
the argument checks of the C entry points that return before the device is touched, and the ABI.

The composite's entry points take no rotation (the images are unrotated by contract), so there is no rotate check to
test here; a projection that takes one keeps its own (tests/test_project_cpu.py)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import composite_cases as cc
import noaa_apt_amd as apt
import np_composite_model as cm
import np_project_model as pm
from noaa_apt_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTERNAL, INVALID = 1, 4
BLENDS = (cm.FIRST, cm.NADIR, cm.FEATHER)


def _parts(c):
    return ([p["image"] for p in c["passes"]], [p["track"] for p in c["passes"]], [p["geom"] for p in c["passes"]])


def _single(p, grid):
    g = p["geom"] or {}
    return pm.project(p["image"], p["track"], grid["kind"], grid["width"], grid["height"], grid["lat_north"],
                      grid["lon_west"], grid["step"], grid["channel"], grid["sampling"], grid.get("grid_deg", 0.0),
                      grid.get("grid_color", (255, 255, 255, 255)), g.get("yaw", 0.0), g.get("hscale", 1.0),
                      g.get("vscale", 1.0))


@pytest.fixture(scope="module")
def small():
    """Three passes on a 48 x 24 grid, bilinear, with their single-pass model outputs."""
    c = cc.case("three", cc.MERCATOR, cc.BILINEAR)
    c["grid"].update(width=48, height=24, step=0.8, lon_west=-63.9)
    singles = [_single(p, c["grid"]) for p in c["passes"]]
    return c, cm.locate_passes(*_parts(c)[:2], c["grid"], _parts(c)[2]), singles


# ---------------------------------------------------------------- the model, pinned
@pytest.mark.parametrize("blend", BLENDS)
def test_one_pass_is_the_projection(blend):
    c = cc.case("two", cc.EQUIRECTANGULAR, cc.BILINEAR)
    grid = dict(c["grid"], width=40, height=20, step=0.7, grid_deg=5.0, grid_color=(255, 0, 0, 128))
    p = c["passes"][1]
    want, margin, info = _single(p, grid)
    got, cov, m, _ = cm.composite([p["image"]], [p["track"]], grid, blend, [p["geom"]])
    assert info["n_valid"] > 100 and np.array_equal(got, want)
    assert np.array_equal(cov, info["valid"].astype(np.uint8)) and np.array_equal(m, margin)


def test_first_paints_in_reverse_order(small):
    c, located, singles = small
    got, cov, _, info = cm.combine(located, c["grid"], cm.FIRST)
    want = np.zeros_like(got)
    for img, _, one in reversed(singles):
        want[one["valid"]] = img[one["valid"]]
    assert np.array_equal(got, want)
    assert all(np.count_nonzero(info["winner"] == p) > 0 for p in range(3))


@pytest.mark.parametrize("blend", BLENDS)
def test_coverage_is_the_sum_of_the_valid_masks(small, blend):
    c, located, singles = small
    _, cov, _, _ = cm.combine(located, c["grid"], blend)
    assert np.array_equal(cov, sum(one["valid"].astype(np.uint8) for _, _, one in singles)) and cov.max() >= 2


def test_nadir_takes_the_smallest_abs_x_and_the_lower_index_on_a_tie(small):
    c, located, _ = small
    got, cov, margin, info = cm.combine(located, c["grid"], cm.NADIR)
    key = np.where(info["valid"], np.abs(info["x"]), math.inf)
    for i, j in np.argwhere(cov > 0):
        assert info["winner"][i, j] == int(np.argmin(key[:, i, j]))
        assert tuple(got[i, j]) == tuple(located[info["winner"][i, j]]["c"][i, j])
    tie = [{"x": np.array([[-7.5]]), "valid": np.array([[True]]), "margin": np.array([[0.3]]),
            "located": np.array([[0.3]]), "c": np.array([[[p, 0, 0, 255]]], np.uint8)} for p in (1, 2)]
    img, _, m, info = cm.combine(tie, dict(kind=0, width=1, height=1, lat_north=0.0, lon_west=0.0, step=1.0), cm.NADIR)
    assert info["winner"][0, 0] == 0 and img[0, 0, 0] == 1 and m[0, 0] == 0.0


def test_feather_pixel_by_hand():
    # x = 100 and -300: w = 356 and 156, sum 512 (a power of two, so every quotient below is exact)
    #   r (3560 + 31200) / 512 = 67.890625 -> 68      g (7120 + 15600) / 512 = 44.375 -> 44
    #   b (10680 + 7800) / 512 = 36.09375 -> 36       a 255
    # margin: r |67.890625 - 67.5| * 512 / (57.890625 + 132.109375) = 200 / 190, g 0.125 * 512 / (24.375 + 55.625)
    # = 0.8, b 0.40625 * 512 / (6.09375 + 13.90625) = 10.4, a infinite; the passes' own margins are 5
    def one(x, c):
        return {"x": np.array([[x]]), "valid": np.array([[True]]), "margin": np.array([[5.0]]),
                "located": np.array([[5.0]]), "c": np.array([[c]], np.uint8)}
    grid = dict(kind=0, width=1, height=1, lat_north=0.0, lon_west=0.0, step=1.0)
    img, cov, m, _ = cm.combine([one(100.0, (10, 20, 30, 255)), one(-300.0, (200, 100, 50, 255))], grid, cm.FEATHER)
    assert tuple(img[0, 0]) == (68, 44, 36, 255) and cov[0, 0] == 2
    assert m[0, 0] == 0.8
    # equal samples have no rounding decision of their own
    img, _, m, _ = cm.combine([one(100.0, (9, 9, 9, 255)), one(-300.0, (9, 9, 9, 255))], grid, cm.FEATHER)
    assert tuple(img[0, 0]) == (9, 9, 9, 255) and m[0, 0] == 5.0


def test_no_pass_is_transparent_and_the_graticule_is_blended_once(small):
    c, located, _ = small
    grid = dict(c["grid"], grid_deg=4.0, grid_color=(0, 255, 0, 128))
    plain, cov, _, _ = cm.combine(located, c["grid"], cm.NADIR)
    assert (cov == 0).any() and not plain[cov == 0].any()
    lined, _, _, _ = cm.combine(located, grid, cm.NADIR)
    cols, rows = pm.graticule(grid["kind"], grid["width"], grid["height"], grid["lat_north"], grid["lon_west"],
                              grid["step"], 4.0)
    on = rows[:, None] | cols[None, :]
    assert on.any() and np.array_equal(lined[~on], plain[~on])
    for i, j in np.argwhere(on):
        assert tuple(lined[i, j]) == tuple(pm.blend(tuple(int(v) for v in plain[i, j]), (0, 255, 0, 128)))


# ---------------------------------------------------------------- the cases' conditions
@pytest.mark.parametrize("sampling", [cc.NEAREST, cc.BILINEAR])
@pytest.mark.parametrize("kind", [cc.EQUIRECTANGULAR, cc.MERCATOR])
@pytest.mark.parametrize("name", cc.CASES)
def test_case_conditions(name, kind, sampling):
    c = cc.case(name, kind, sampling)
    assert c["grid"]["width"] <= 160 and c["grid"]["height"] <= 80
    located = cm.locate_passes(*_parts(c)[:2], c["grid"], _parts(c)[2])
    for blend in BLENDS:
        _, cov, margin, info = cm.combine(located, c["grid"], blend)
        wins = [int(np.count_nonzero(info["winner"] == p)) for p in range(len(c["passes"]))]
        print(f"{name} kind {kind} sampling {sampling} blend {blend}: {info['n_covered']} covered, "
              f"{info['excused']} excused, wins {wins}, {int(np.count_nonzero(cov >= 2))} with coverage >= 2")
        assert info["excused"] <= min(16, int(0.001 * info["n_covered"]))
        assert min(wins) >= 50
        assert np.count_nonzero(cov >= 2) >= 500
        assert np.all(info["coverage_margin"] >= margin) or blend == cm.FIRST


def test_shapes_are_what_they_say():
    for name in cc.SHAPES:
        c = cc.shape(name)
        _, cov, _, info = cm.composite(*_parts(c)[:2], c["grid"], cm.NADIR, _parts(c)[2])
        per_pass = info["valid"].sum(axis=(1, 2))
        if name == "sixteen":
            assert len(c["passes"]) == cm.MAX_PASSES == apt.COMPOSITE_MAX_PASSES and cov.max() == 16
            assert per_pass.min() > 0
        elif name == "miss":
            assert per_pass[2] == 0 and per_pass[0] > 0 and per_pass[1] > 0
        else:
            assert cov.max() == 3


# ---------------------------------------------------------------- argument checks, before the device is touched
_u8p, _f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_double)
COUNT = (INVALID, "a composite takes 1 to APTGPU_COMPOSITE_MAX_PASSES (16) passes")


def _call(count=2, images="ok", tracks="ok", settings=None, proj=None, maps=None, output=0, png=None, plan=False):
    """(rc, err text) of aptgpu_composite_images (or the plan form with plan = NULL) on `count` tiny passes."""
    k = max(count, 1)
    imgs = [np.zeros((2, 2080), np.uint8) for _ in range(k)]
    pos = [np.zeros((2, 2)) for _ in range(k)]
    ip = (_u8p * k)(*[(None if images == "null" and i == k - 1 else x.ctypes.data_as(_u8p)) for i, x in enumerate(imgs)])
    tp = (_f64p * k)(*[(None if tracks == "null" and i == k - 1 else x.ctypes.data_as(_f64p)) for i, x in enumerate(pos)])
    heights, chans = (C.c_uint32 * k)(*[2] * k), (C.c_int32 * k)(*[1] * k)
    npos = (C.c_size_t * k)(*[2] * k)
    cco = settings if settings is not None else api._CCompositeSettings(C.sizeof(api._CCompositeSettings), 1, 0)
    cpr = proj if proj is not None else apt.ProjectionSettings(0, 8, 8, 10.0, -60.0, 0.5)._c()
    out, n = _u8p(), C.c_size_t()
    err = C.create_string_buffer(512)
    L = apt.lib()
    if plan:
        rc = L.aptgpu_plan_composite_device_images(None, count, C.cast(ip, C.POINTER(C.c_void_p)), heights, chans,
                                                   None if tracks == "none" else tp, npos, None, maps, C.byref(cpr),
                                                   C.byref(cco) if settings != "none" else None, None, 0, None, png,
                                                   None, 0, err, 512)
    else:
        rc = L.aptgpu_composite_images(None, count, None if images == "none" else ip, heights, chans,
                                       None if tracks == "none" else tp, npos, maps, C.byref(cpr),
                                       C.byref(cco) if settings != "none" else None, output, png, C.byref(out),
                                       C.byref(n), None, err, 512)
    assert not out and n.value == 0
    return rc, err.value.decode()


@pytest.mark.parametrize("plan", [False, True])
def test_refusals_before_the_device(plan):
    cs = api._CCompositeSettings
    size = C.sizeof(cs)
    assert _call(0, plan=plan) == COUNT and _call(17, plan=plan) == COUNT and _call(-1, plan=plan) == COUNT
    assert _call(images="null", plan=plan) == (INVALID, "composite: a pass has no image or no row")
    assert _call(tracks="null", plan=plan) == (INVALID, "null sat_positions")
    assert _call(settings=cs(0, 1, 0), plan=plan) == (INVALID, "aptgpu_composite_settings: struct_size not set")
    assert _call(settings="none", plan=plan) == (INVALID, "aptgpu_composite_settings: struct_size not set")
    assert _call(settings=cs(size, 3, 0), plan=plan) == (INVALID, "aptgpu_composite_settings: unknown blend")
    assert _call(settings=cs(size, -1, 0), plan=plan) == (INVALID, "aptgpu_composite_settings: unknown blend")
    assert _call(settings=cs(size, 2, 7), plan=plan) == (INVALID, "aptgpu_composite_settings: reserved must be 0")
    bad = apt.ProjectionSettings(0, 8, 8, 10.0, -60.0, 0.5)._c()
    bad.reserved = 1
    assert _call(proj=bad, plan=plan) == (INVALID, "aptgpu_projection_settings: reserved must be 0")
    bad = apt.ProjectionSettings(0, 0, 8, 10.0, -60.0, 0.5)._c()
    assert _call(proj=bad, plan=plan) == (INVALID, "aptgpu_projection_settings: width and height must be at least 1")
    ms = api._CMapSettings(0, 0, 0.0, 1.0, 1.0)
    maps = (C.POINTER(api._CMapSettings) * 2)(None, C.pointer(ms))
    assert _call(maps=maps, plan=plan) == (INVALID, "aptgpu_map_settings: struct_size not set")
    # every check passed: the plan form stops at its null plan with a bare code
    if plan:
        assert _call(plan=True) == (INVALID, "")
        assert _call(tracks="none", plan=True) == (INVALID, "a composite needs exactly one of sat_positions and "
                                                   "aptgpu_orbit_settings")


def test_png_and_output_refusals():
    ps = api._CPngSettings
    assert _call(output=2) == (INVALID, "unknown output kind")
    assert _call(output=1, png=C.byref(ps(0, 0))) == (INVALID, "aptgpu_png_settings: struct_size not set")
    assert _call(output=1, png=C.byref(ps(C.sizeof(ps), 1))) == (INVALID, "aptgpu_png_settings: unknown flags")
    assert _call(tracks="none") == (INVALID, "null sat_positions")
    assert _call(images="none") == (INVALID, "composite: null images, heights or channels")
    # (a grid without a pixel never reaches the encoder's own shape check: the projection settings refuse it first)
    assert _call(output=1, proj=apt.ProjectionSettings(0, 8, 0, 10.0, -60.0, 0.5)._c())[1].endswith("at least 1")


def test_python_refusals():
    ps = apt.ProjectionSettings(0, 8, 8, 10.0, -60.0, 0.5)
    img, pos = np.zeros((2, 2080), np.uint8), np.zeros((2, 2))
    with pytest.raises(apt.InvalidError, match="1 to APTGPU_COMPOSITE_MAX_PASSES"):
        apt.composite_images([], [], ps)
    with pytest.raises(apt.InvalidError, match="1 to APTGPU_COMPOSITE_MAX_PASSES"):
        apt.composite_images([img] * 17, [pos] * 17, ps)
    with pytest.raises(apt.InvalidError, match="one track per image"):
        apt.composite_images([img, img], [pos], ps)
    with pytest.raises(apt.InvalidError, match="unknown blend"):
        apt.composite_images([img], [pos], ps, blend=5)
    with pytest.raises(apt.InvalidError, match=r"\(height, 2080\)"):
        apt.composite_images([np.zeros((2, 100), np.uint8)], [pos], ps)
    with pytest.raises(apt.InvalidError, match="one \\(or None\\) per pass"):
        apt.composite_images([img, img], [pos, pos], ps, settings=[apt.MapSettings()])


# ---------------------------------------------------------------- projection_fit over several tracks
def test_projection_fit_of_one_track_is_unchanged_and_of_several_is_their_union():
    tracks = [cc.track(160, 0.0), cc.track(96, cc.SHIFT), cc.track(160, 2 * cc.SHIFT)]
    for kind in (0, 1):
        one = apt.projection_fit(tracks[0], kind, step=0.25)
        assert vars(apt.projection_fit([tracks[0]], kind, step=0.25)) == vars(one)
        assert {k: getattr(one, k) for k in pm.fit(tracks[0], kind, step=0.25)} == pm.fit(tracks[0], kind, step=0.25)
        fits = [apt.projection_fit(t, kind, step=0.25) for t in tracks]
        union = apt.projection_fit(tracks, kind, step=0.25)
        assert union.lon_west == min(f.lon_west for f in fits) and union.lat_north == max(f.lat_north for f in fits)
        east = max(f.lon_west + (f.width - 1) * f.step for f in fits)
        assert abs(union.lon_west + (union.width - 1) * union.step - east) <= union.step
        assert union.height >= max(f.height for f in fits)
    # passes on both sides of the antimeridian share the first track's axis
    a, b = cc.mm.great_circle_track(5.0, 176.0, 14.0, 100), cc.mm.great_circle_track(5.0, -172.0, 14.0, 100)
    u = apt.projection_fit([a, b], 0, step=0.25)
    fa, fb = apt.projection_fit(a, 0, step=0.25), apt.projection_fit(b, 0, step=0.25)
    assert u.lon_west == fa.lon_west and abs(u.lon_west + (u.width - 1) * 0.25 - (fb.lon_west + 360.0 + (fb.width - 1) * 0.25)) <= 0.25
    with pytest.raises(apt.InvalidError, match="the track is empty"):
        apt.projection_fit([a, np.zeros((0, 2))], 0, step=0.25)


# ---------------------------------------------------------------- the ABI
def test_header_declares_what_api_binds():
    hdr = open(os.path.join(ROOT, "include", "aptgpu.h")).read()
    L = apt.lib()
    for name in ("aptgpu_composite_images", "aptgpu_plan_composite_device_images", "aptgpu_projection_fit_many"):
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert getattr(L, name).argtypes is not None
    for name, value in (("APTGPU_COMPOSITE_FIRST", 0), ("APTGPU_COMPOSITE_NADIR", 1), ("APTGPU_COMPOSITE_FEATHER", 2),
                        ("APTGPU_COMPOSITE_MAX_PASSES", 16), ("APTGPU_COMPOSITE_REASON_PASS", 12)):
        assert re.search(rf"#define {name} {value}\b", hdr), name
    assert (apt.Composite.FIRST, apt.Composite.NADIR, apt.Composite.FEATHER) == (0, 1, 2)
    assert apt.COMPOSITE_REASON_PASS == 12 and apt.COMPOSITE_MAX_PASSES == 16
    assert "#define APTGPU_ABI_VERSION 2" in hdr and apt.abi_version() == 2
    m = re.search(r"typedef struct aptgpu_composite_settings \{(.*?)\} aptgpu_composite_settings;", hdr, re.S)
    assert [f for f in re.findall(r"\b(\w+);", m.group(1))] == [f for f, _ in api._CCompositeSettings._fields_]
    assert C.sizeof(api._CCompositeSettings) == 12
    for name in ("Composite", "composite_images", "COMPOSITE_REASON_PASS"):
        assert hasattr(apt, name)
    assert hasattr(apt.Plan, "composite_device_images")
