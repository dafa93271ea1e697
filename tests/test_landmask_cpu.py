"""The land / sea / lake mask without a GPU: the plain C++ twin (aptgpu_land_mask_host, aptgpu_land_mask_plane_host,
aptgpu_false_color_masked_host) against np_landmask_model.py with the assertions landmask_cases.py states, the model's
sorted form against its brute-force form, the refusals, which all come before a device is touched, and the ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import landmask_cases as lc
import np_landmask_model as lmm
from test_sat_cpu import TLE_2020, orbit

import noaa_apt_amd as apt

SIDE = lc.HOST
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = apt.InvalidError.code


def test_model_sorted_form_equals_brute_force():
    co, la = lc.fixture_edges()
    for name, step in (("h2", 3), ("h5", 9)):  # (a few hundred points against every edge)
        ll = lc.model_points(name).reshape(-1, 2)[::step]
        a = lmm.classify(ll, co, la)
        b = lmm.classify(ll, co, la, evaluate=lmm.brute)
        assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1], name
    assert len(co) > 10000 and len(la) > 5000


def test_model_counts_of_the_fixture_cases():
    for name, want in lc.KNOWN_COUNTS.items():
        if name != "far":
            assert lc.model_mask(name)[1] == want, name


@pytest.mark.parametrize("name", lc.SMALL)
def test_plane_small_cases_every_band_count(name):
    ll = lc.model_points(name)
    lc.check_plane(SIDE, ll, lc.fixture_layers(), lc.fixture_edges(), note=name)
    lc.check_plane(SIDE, lc.nan_plane(ll, seed=len(name)), lc.fixture_layers(), lc.fixture_edges(), note=name + " nan")


def test_plane_scene_240_rows():
    lc.check_plane(SIDE, lc.model_points("scene1"), lc.fixture_layers(), lc.fixture_edges(), bands=(720, 7200), note="scene1")
    lc.check_plane(SIDE, lc.nan_plane(lc.model_points("scene1"), seed=1, n_nan=1500), lc.fixture_layers(),
                   lc.fixture_edges(), bands=(720,), note="scene1 nan")


def test_plane_takes_any_shape_and_infinities():
    ll = lc.model_points("h5")
    flat = np.ascontiguousarray(ll.reshape(-1, 2)[:1000]).copy()
    flat[3] = (np.inf, 0.1)
    flat[4] = (-0.5, -np.inf)
    flat[5] = (-np.inf, np.inf)
    lc.check_plane(SIDE, flat.reshape(10, 100, 2), lc.fixture_layers(), lc.fixture_edges(), bands=(1, 720), note="3-d")
    mask, info = SIDE.plane(np.zeros((0, 2)), lc.fixture_layers())
    assert mask.shape == (0,) and lc.counts_of(info) == (0, 0, 0, 0)


@pytest.mark.parametrize("name", ("pole", "antimeridian"))
def test_plane_synthetic_layers(name):
    layers, edges = lc.synthetic(name)
    ll = lc.model_points(name)[::7]  # every seventh row: the classes of all the shapes, a seventh of the points
    want = lc.check_plane(SIDE, ll, layers, edges, bands=(1, 7, 720, 7200), note=name)
    assert {0, 1, 2} <= set(np.unique(want)), name
    # one layer alone: the other counts 0
    co, la = lc.synthetic_parts(name)
    lc.check_plane(SIDE, ll, lc.layers_of(co, None), (edges[0], None), bands=(720,), note=name + " countries")
    lc.check_plane(SIDE, ll, lc.layers_of(None, la), (None, edges[1]), bands=(720,), note=name + " lakes")


def test_degenerate_polygons_pin_the_half_open_rule():
    ll, layers, edges, chosen = lc.degenerate(SIDE)
    want = lc.check_plane(SIDE, ll, layers, edges, note="degenerate")
    deg = ll * lmm.DEG
    co = edges[0]
    # the chosen pixels lie exactly on vertices, and one on a horizontal edge's latitude
    for r, k in chosen[:4]:
        assert ((co[:, 0] == deg[r, k, 1]) & (co[:, 1] == deg[r, k, 0])).any(), (r, k)
    assert (co[:, 1] == co[:, 3]).any() and (co[co[:, 1] == co[:, 3]][:, 1] == deg[2, 500, 0]).any()
    assert {0, 1, 2} <= set(np.unique(want))


@pytest.mark.parametrize("name", ("h2", "h5", "scene3", "antimeridian"))
def test_swath_equals_plane_of_own_points(name):
    layers = lc.fixture_layers() if name != "antimeridian" else lc.synthetic(name)[0]
    h = lc.case(name)[0].shape[0]
    lc.swath_equals_plane(SIDE, h, lc.case(name)[0], layers, lc.map_settings_of(name), 720, name)


def test_swath_orbit_form():
    o = orbit(TLE_2020, "NOAA 19", "start", 1580246771392)
    mask, info = lc.swath_equals_plane(SIDE, 40, o, lc.fixture_layers(), None, 720, "orbit")
    track = apt.sat_track_host(o, 40)
    again, _ = SIDE.swath(40, track, lc.fixture_layers())
    assert again.tobytes() == mask.tobytes()


@pytest.mark.parametrize("name", lc.FIXTURE_CASES)
def test_end_to_end_against_the_models_geolocation(name):
    mask, info = SIDE.swath(lc.case(name)[0].shape[0], lc.case(name)[0], lc.fixture_layers(), lc.map_settings_of(name))
    n_bad = lc.check_end_to_end(SIDE, name, lc.fixture_layers(), lc.fixture_edges(), mask)
    if name in lc.KNOWN_COUNTS:
        assert lc.model_mask(name)[1] == lc.KNOWN_COUNTS[name]
        assert sum(abs(a - b) for a, b in zip(lc.counts_of(info), lc.KNOWN_COUNTS[name])) <= 2 * n_bad
    if name == "far":
        assert info.n_invalid > 60000


def test_end_to_end_synthetic_antimeridian():
    layers, edges = lc.synthetic("antimeridian")
    lc.check_end_to_end(SIDE, "antimeridian", layers, edges)


def test_record_reasons_and_table_size():
    track = lc.case("h5")[0]
    layers = lc.fixture_layers()
    with pytest.raises(apt.InternalError, match="fewer than two rows") as e:
        apt.land_mask_host(1, track[:1], layers)
    assert (e.value.info.status, e.value.info.reason, e.value.info.height) == (1, apt.GEOLOC_REASON_HEIGHT, 1)
    with pytest.raises(apt.InternalError, match="differs from the image height") as e:
        apt.land_mask_host(5, track[:4], layers)
    assert (e.value.info.status, e.value.info.reason, e.value.info.height) == (1, 7, 5)
    # the table: non-horizontal edges per layer, and for one band one entry per edge
    co, la = lc.fixture_edges()
    want = tuple(int((e[:, 1] != e[:, 3]).sum()) for e in (co, la))
    _, info = apt.land_mask_host(5, track, layers, None, apt.LandMaskSettings(n_bands=1))
    assert tuple(info.n_edges) == want and info.n_band_entries == sum(want)
    # 720 bands: 16 249 and 11 905 entries with the 26 and 157 horizontal edges still listed, which the table drops
    _, info = apt.land_mask_host(5, track, layers)
    assert info.n_band_entries == (16249 - 26) + (11905 - 157)
    # the signal's length gives the height, as geolocate() takes it
    a, _ = apt.land_mask_host(np.zeros(5 * 2080 + 7, np.float32), track, layers)
    assert a.shape == (5, 909)


def test_layer_set_changes_rebuild_the_table():
    co, la = lc.synthetic_parts("pole")
    layers = lc.layers_of(co, la)
    ll = lc.model_points("pole")[::40]
    a, ia = apt.land_mask_plane_host(ll, layers)
    layers._set(apt.MAP_LAKES, [])  # the lakes go: their class goes with them
    b, ib = apt.land_mask_plane_host(ll, layers)
    assert ia.n_lake > 0 and ib.n_lake == 0 and ib.n_edges[1] == 0 and ib.n_land > ia.n_land
    want, _ = lmm.classify(ll, lmm.edges_of(co), None)
    assert b.tobytes() == want.tobytes()


@pytest.mark.parametrize("h", (1, 2, 120))
def test_colouriser_equals_model(h):
    lc.check_color_model(SIDE, h)


# ---- refusals: every one before a device is touched, so every one on a machine without a GPU, in the GPU forms too
def _raw():
    return apt.lib()


def _call_swath(gpu, layers_p, settings=None, h=5, track=None):
    track = np.ascontiguousarray(lc.case("h5")[0] if track is None else track)
    mask, err = C.POINTER(C.c_uint8)(), C.create_string_buffer(512)
    info = apt.LandMaskResult()
    info.struct_size = C.sizeof(info)
    cctx = apt.Context()._c()
    head = (C.byref(cctx),) if gpu else ()
    fn = _raw().aptgpu_land_mask if gpu else _raw().aptgpu_land_mask_host
    rc = fn(*head, h, track.ctypes.data_as(C.POINTER(C.c_double)), len(track), None, None, layers_p,
            C.byref(settings) if settings is not None else None, C.byref(mask), C.byref(info), err, 512)
    assert not mask
    return rc, err.value.decode()


def _call_plane(gpu, addr, n, layers_p, settings=None):
    mask, err = C.POINTER(C.c_uint8)(), C.create_string_buffer(512)
    cctx = apt.Context()._c()
    head = (C.byref(cctx),) if gpu else ()
    fn = _raw().aptgpu_land_mask_plane if gpu else _raw().aptgpu_land_mask_plane_host
    rc = fn(*head, C.c_void_p(addr), n, layers_p, C.byref(settings) if settings is not None else None, C.byref(mask),
            None, err, 512)
    assert not mask
    return rc, err.value.decode()


@pytest.mark.parametrize("gpu", (False, True))
def test_refusals_layers_and_settings(gpu):
    layers = lc.fixture_layers()
    rc, msg = _call_swath(gpu, None)
    assert rc == INVALID and "layer set is required" in msg
    empty = apt.MapLayers()
    rc, msg = _call_swath(gpu, empty._p)
    assert rc == INVALID and "neither countries nor lakes" in msg
    states_only = apt.MapLayers(states=[lc.box(0, 0, 1, 1)])
    rc, msg = _call_swath(gpu, states_only._p)
    assert rc == INVALID and "neither countries nor lakes" in msg
    ok = apt.LandMaskSettings()._c()
    small = apt.LandMaskSettings()._c(struct_size=C.sizeof(ok) - 4)
    rc, msg = _call_swath(gpu, layers._p, small)
    assert rc == INVALID and "struct_size" in msg
    for nb in (0, -1, 7201):
        rc, msg = _call_swath(gpu, layers._p, apt.LandMaskSettings(n_bands=nb)._c())
        assert rc == INVALID and "n_bands" in msg, nb
    rc, msg = _call_swath(gpu, layers._p, apt.LandMaskSettings(flags=1)._c())
    assert rc == INVALID and "flag" in msg
    ll = np.ascontiguousarray(lc.model_points("h2").reshape(-1, 2))
    rc, msg = _call_plane(gpu, ll.ctypes.data, len(ll), None)
    assert rc == INVALID and "layer set is required" in msg
    rc, msg = _call_plane(gpu, ll.ctypes.data, len(ll), layers._p, apt.LandMaskSettings(n_bands=7201)._c())
    assert rc == INVALID and "n_bands" in msg
    rc, msg = _call_plane(gpu, ll.ctypes.data, len(ll), layers._p, small)
    assert rc == INVALID and "struct_size" in msg


@pytest.mark.parametrize("gpu", (False, True))
def test_refusals_plane_pointer(gpu):
    layers = lc.fixture_layers()
    rc, msg = _call_plane(gpu, 0, 10, layers._p)
    assert rc == INVALID and "plane is required" in msg
    buf = np.zeros(2 * 10 + 1, np.float64)
    rc, msg = _call_plane(gpu, buf.ctypes.data + 4, 10, layers._p)
    assert rc == INVALID and "8-byte aligned" in msg
    # through the binding: a misaligned float64 view goes to the library as it is
    raw = np.zeros(16 * 10 + 8, np.uint8)
    view = raw[4:4 + 160].view(np.float64).reshape(10, 2)
    assert view.ctypes.data % 8 == 4
    fn = apt.land_mask_plane if gpu else apt.land_mask_plane_host
    with pytest.raises(apt.InvalidError, match="8-byte aligned"):
        fn(view, layers)
    with pytest.raises(apt.InvalidError, match="MapLayers"):
        fn(np.zeros((4, 2)), None)
    with pytest.raises(apt.InvalidError, match="last axis"):
        fn(np.zeros((4, 3)), layers)


@pytest.mark.parametrize("gpu", (False, True))
def test_refusals_track_and_non_finite_vertices(gpu):
    layers = lc.fixture_layers()
    fn = apt.land_mask if gpu else apt.land_mask_host
    with pytest.raises(apt.InvalidError, match="exactly one"):
        fn(5, None, layers)
    with pytest.raises(apt.InvalidError, match="2\\^22 rows"):
        fn((1 << 22) + 1, lc.case("h5")[0], layers)
    for bad in (np.nan, np.inf):
        part = lc.box(0, 0, 1, 1)
        part[2, 0] = bad
        with pytest.raises(apt.InvalidError, match="not finite"):
            fn(5, lc.case("h5")[0], lc.layers_of([part], None))


@pytest.mark.parametrize("gpu", (False, True))
def test_refusals_colouriser(gpu):
    fn = apt.false_color_masked if gpu else apt.false_color_masked_host
    image, mask = lc.gray_image(2, 1), lc.random_mask(2, 2)
    pals = lc.palettes()
    with pytest.raises(apt.InvalidError, match="256 x 256 x 3"):
        fn(image, mask, (pals[0], pals[1][:255], pals[2]))
    with pytest.raises(apt.InvalidError, match="256 x 256 x 3"):
        fn(image, mask, (pals[0], pals[1], np.zeros((256, 256, 4), np.uint8)))
    with pytest.raises(apt.InvalidError, match="height differs"):
        fn(image, lc.random_mask(3, 2), pals)
    with pytest.raises(apt.InvalidError, match="three palettes"):
        fn(image, mask, pals[:2])
    with pytest.raises(apt.InvalidError, match="2080"):
        fn(image[:, :2000], mask, pals)
    with pytest.raises(apt.InvalidError, match="909"):
        fn(image, mask[:, :900], pals)


def test_plan_refusals_need_no_plan():
    L = _raw()
    layers = lc.fixture_layers()
    track = np.ascontiguousarray(lc.case("h5")[0])
    rows_base, far = 1 << 20, 1 << 30
    err = C.create_string_buffer(512)

    def call(layers_p=layers._p, settings=None, d_mask=far, positions=True, cap=5):
        pos = (C.POINTER(C.c_double) * 1)(track.ctypes.data_as(C.POINTER(C.c_double)))
        rc = L.aptgpu_plan_land_mask_device(None, 1, (C.c_void_p * 1)(rows_base), (C.c_size_t * 1)(cap),
                                            pos if positions else None, (C.c_size_t * 1)(len(track)), None, None,
                                            layers_p, C.byref(settings) if settings is not None else None,
                                            (C.c_void_p * 1)(d_mask), err, 512)
        return rc, err.value.decode()
    rc, msg = call(layers_p=None)
    assert rc == INVALID and "layer set is required" in msg
    rc, msg = call(settings=apt.LandMaskSettings(n_bands=0)._c())
    assert rc == INVALID and "n_bands" in msg
    rc, msg = call(positions=False)
    assert rc == INVALID and "exactly one" in msg
    rc, msg = call(d_mask=rows_base + 2080 * 4)
    assert rc == INVALID and "overlaps" in msg
    rc, msg = call(cap=(1 << 22) + 1)
    assert rc == INVALID and "2^22" in msg
    rc, msg = call()  # nothing left to refuse but the missing plan
    assert rc == INVALID and "no plan" in msg
    assert L.aptgpu_plan_land_mask_results(None, 1, None) == INVALID


def test_abi():
    hdr = open(os.path.join(ROOT, "include", "aptgpu.h")).read()
    raw = C.CDLL(apt.lib_path())
    for name in ("aptgpu_land_mask", "aptgpu_land_mask_host", "aptgpu_land_mask_plane", "aptgpu_land_mask_plane_host",
                 "aptgpu_plan_land_mask_device", "aptgpu_plan_land_mask_results", "aptgpu_false_color_masked",
                 "aptgpu_false_color_masked_host"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and hasattr(raw, name), name
    assert C.sizeof(apt.api._CLandMaskSettings) == 16 and C.sizeof(apt.LandMaskResult) == 64
    assert apt.LandMaskResult.n_sea.offset == 16 and apt.LandMaskResult.n_edges.offset == 48
    assert apt.LandMaskResult.n_band_entries.offset == 56
    assert apt.abi_version() == 2
    for name, value in (("APTGPU_LAND_SEA", apt.LAND_SEA), ("APTGPU_LAND_LAND", apt.LAND_LAND),
                        ("APTGPU_LAND_LAKE", apt.LAND_LAKE), ("APTGPU_LAND_INVALID", apt.LAND_INVALID)):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == value
    # a caller built against a shorter record gets its own size back and nothing beyond it
    info = apt.LandMaskResult()
    info.struct_size = 16
    info.n_sea = 77
    ll = np.ascontiguousarray(lc.model_points("h2").reshape(-1, 2))
    mask, err = C.POINTER(C.c_uint8)(), C.create_string_buffer(512)
    rc = apt.lib().aptgpu_land_mask_plane_host(C.c_void_p(ll.ctypes.data), len(ll), lc.fixture_layers()._p, None,
                                               C.byref(mask), C.byref(info), err, 512)
    assert rc == 0 and info.struct_size == 16 and info.n_sea == 77
    apt.lib().aptgpu_free(mask)
