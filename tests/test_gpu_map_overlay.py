"""The map overlay on the GPU (process(orbit=MapOverlay(...)), aptgpu_process_image_map and the plan chain) against
np_map_model.py under the parity contract of DESIGN.md §12: the image equals the model's bit for bit, except on
pixels that a segment with a decision margin below np_map_model.TAU may change.  Such exceptions are counted and
printed; on these fixtures and seeds there are none, and the tests assert that."""
import ctypes as C
import math
import os
import time

import numpy as np
import pytest

import noaa_apt_amd as apt
import np_map_model as mm
from noaa_apt_amd.testing.synth import synth_apt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHP = os.path.join(ROOT, "tests", "golden", "shapefiles")
PALETTES = os.path.join(ROOT, "tests", "golden", "palettes")


@pytest.fixture(scope="module")
def fixture_layers():
    parts = {"countries": apt.read_shapefile(os.path.join(SHP, "countries.shp"), 5),
             "lakes": apt.read_shapefile(os.path.join(SHP, "lakes.shp"), 5)}
    return parts, apt.MapLayers(countries=parts["countries"], lakes=parts["lakes"])


def _signal(rows, seed):
    return np.random.default_rng(seed).random(rows * 2080).astype(np.float32)


def _pre(signal, contrast, color):
    """process()'s RGBA image before the overlay and the rotation (gray: Luma8 -> RGBA, A = 255)."""
    img = apt.process(None, signal, contrast, rotate=apt.Rotate.NO, color=color)
    if img.ndim == 2:
        img = np.concatenate([np.repeat(img[:, :, None], 3, axis=2), np.full(img.shape + (1,), 255, np.uint8)],
                             axis=2)
    return img


def _check(signal, positions, parts, layers, contrast=apt.Contrast.MINMAX, color=None, rotate=False,
           settings=None, colors=None, label=""):
    settings = settings or {}
    colors = colors or {}
    ms = apt.MapSettings(**settings, **{f"{k}_color": v for k, v in colors.items()})
    got = apt.process(None, signal, contrast, rotate=apt.Rotate.YES if rotate else apt.Rotate.NO, color=color,
                      orbit=apt.MapOverlay(positions, ms, layers))
    want, excused, info = mm.overlay(_pre(signal, contrast, color), positions, parts, settings, colors, rotate)
    assert got.shape == want.shape
    unexcused, exceptions = mm.compare(got, want, excused)
    print(f"{label}: {info['fragments']} fragments, {info['low_margin']} low-margin segments, "
          f"{exceptions} excused differing pixels")
    assert unexcused == 0, label
    assert exceptions == 0, label
    return got, want, info


TRACKS = {"south_north": (-52.0, -68.0, 8.0), "north_south": (8.0, -58.0, 192.0)}


@pytest.mark.parametrize("rows", [360, 1198])
@pytest.mark.parametrize("track", sorted(TRACKS))
def test_fixture_gray(fixture_layers, rows, track):
    parts, layers = fixture_layers
    pos = mm.great_circle_track(*TRACKS[track], rows)
    _, _, info = _check(_signal(rows, rows), pos, parts, layers, label=f"{track} {rows}")
    assert info["fragments"] > 1000


@pytest.mark.parametrize("kind", ["palette", "lab"])
def test_fixture_colour(fixture_layers, kind):
    parts, layers = fixture_layers
    rows = 600
    pos = mm.great_circle_track(*TRACKS["south_north"], rows)
    color = apt.ColorSettings(os.path.join(PALETTES, "noaa-apt-daylight.png"), 0.1, -0.2, 0.3, 0.0,
                              equalize_lab=kind == "lab")
    contrast = apt.Contrast.HISTOGRAM if kind == "lab" else apt.Contrast.Percent(0.98)
    _check(_signal(rows, 5), pos, parts, layers, contrast=contrast, color=color, rotate=True, label=kind)


def test_fixture_settings(fixture_layers):
    parts, layers = fixture_layers
    pos = mm.great_circle_track(*TRACKS["north_south"], 500)
    _check(_signal(500, 9), pos, parts, layers, settings={"yaw": 0.07, "hscale": 1.6, "vscale": 0.7},
           colors={"lakes": (10, 20, 250, 0), "countries": (200, 30, 40, 120)}, label="settings + alpha 0")


def _edge_layers():
    # north-south lines 13.00-13.08 degrees east of a northbound equator track: x near -455, columns 84 / 85 and
    # 1124 / 1125, which the rotation leaves in place
    lines = [np.array([[13.0 + 0.01 * k, 0.2], [13.0 + 0.01 * k, 1.5], [13.0 + 0.01 * k, 2.7]]) for k in range(9)]
    return {"states": lines}


def test_rotation_edge_columns():
    parts = _edge_layers()
    layers = apt.MapLayers(states=parts["states"])
    rows = 360
    pos = mm.great_circle_track(0.0, 0.0, 0.0, rows)
    sig = _signal(rows, 3)
    got, want, _ = _check(sig, pos, parts, layers, rotate=True, label="rotate edges")
    flat, _, _ = mm.overlay(_pre(sig, apt.Contrast.MINMAX, None), pos, parts)
    pre = _pre(sig, apt.Contrast.MINMAX, None)
    changed = np.any(flat != pre, axis=-1)
    for col in (84, 85, 1124, 1125):
        assert changed[:, col].any(), col
    assert changed[:, 86].any() and changed[:, 1126].any()


def test_shared_borders_blend_order():
    # two polygons sharing an edge, a polyline over it and repeated vertices: pixels with many fragments whose
    # order matters
    a = np.array([[-60.0, -30.0], [-58.0, -30.0], [-58.0, -28.0], [-58.0, -28.0], [-60.0, -28.0], [-60.0, -30.0]])
    b = np.array([[-58.0, -30.0], [-56.0, -30.0], [-56.0, -28.0], [-58.0, -28.0], [-58.0, -30.0]])
    line = np.array([[-58.0, -31.0], [-58.0, -29.0], [-58.0, -29.0], [-58.0, -27.0]])
    parts = {"states": [line, line[::-1]], "countries": [a, b], "lakes": [b, a]}
    layers = apt.MapLayers(states=parts["states"], countries=parts["countries"], lakes=parts["lakes"])
    pos = mm.great_circle_track(-34.0, -58.5, 3.0, 300)
    colors = {"states": (255, 0, 0, 90), "countries": (0, 255, 0, 170), "lakes": (0, 0, 255, 60)}
    _check(_signal(300, 4), pos, parts, layers, colors=colors, label="shared borders")


@pytest.mark.parametrize("kind", ["single_row", "identical"])
def test_degenerate_tracks(fixture_layers, kind):
    parts, layers = fixture_layers
    rows = 1 if kind == "single_row" else 40
    pos = np.tile([[math.radians(-30.0), math.radians(-60.0)]], (rows, 1))
    sig = _signal(rows, 8)
    got = apt.process(None, sig, apt.Contrast.MINMAX, orbit=apt.MapOverlay(pos, apt.MapSettings(), layers))
    assert np.array_equal(got, _pre(sig, apt.Contrast.MINMAX, None))


def test_refusals(fixture_layers):
    parts, layers = fixture_layers
    rows = 100
    sig = _signal(rows, 1)
    ov = apt.MapOverlay(mm.great_circle_track(-30.0, -60.0, 0.0, rows), apt.MapSettings(), layers)
    # channels = 1 through the public C boundary
    cctx, cms = apt.Context()._c(), ov.settings._c()
    img, n, info = C.POINTER(C.c_uint8)(), C.c_size_t(), apt.ImageResult()
    err = C.create_string_buffer(1024)
    rc = apt.lib().aptgpu_process_image_map(C.byref(cctx), sig.ctypes.data_as(C.POINTER(C.c_float)), sig.size, 2,
                                            0.0, 0, None, 1, C.byref(cms), layers._p,
                                            ov.sat_positions.ctypes.data_as(C.POINTER(C.c_double)), C.byref(img),
                                            C.byref(n), C.byref(info), err, 1024)
    assert rc == 4 and b"channels = 4" in err.value and not img
    with pytest.raises(apt.UnsupportedError):
        apt.process(None, sig, apt.Contrast.MINMAX, rotate=apt.Rotate.ORBIT, orbit=ov)
    with pytest.raises(apt.UnsupportedError):
        apt.process(None, sig, apt.Contrast.MINMAX, orbit=object())
    # a segment from a vertex inside the band to one millions of pixels away (vscale 1e4): over the walk cap
    far = apt.MapLayers(countries=[np.array([[0.0, 9.0], [0.0, 0.0002]])])
    ov = apt.MapOverlay(mm.great_circle_track(0.0, 0.0, 0.0, rows), apt.MapSettings(vscale=1e4), far)
    with pytest.raises(mm.WalkError):
        mm.overlay(_pre(sig, apt.Contrast.MINMAX, None), ov.sat_positions,
                   {"countries": [np.array([[0.0, 9.0], [0.0, 0.0002]])]}, {"vscale": 1e4})
    with pytest.raises(apt.InternalError, match="walk"):
        apt.process(None, sig, apt.Contrast.MINMAX, orbit=ov)


def test_plan_chain(oracle, fixture_layers):
    torch = pytest.importorskip("torch")
    parts, layers = fixture_layers
    dev = torch.device("cuda:0")
    k = 4
    recs = [synth_apt(48000, 40 + 5 * i, 700 + i) for i in range(k)]
    rows = [oracle.decode(r, 48000, True) for r in recs]
    heights = [r.size // 2080 for r in rows]
    maps = [apt.MapOverlay(mm.great_circle_track(-45.0 + 3 * i, -66.0, 10.0, heights[i]), apt.MapSettings(), layers)
            for i in range(k)]
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        plan = apt.Plan(apt.Settings(), apt.Rate.hz(48000), True, max_samples=max(r.size for r in recs), max_batch=k,
                        stream=stream.cuda_stream)
        plan.enable_timing(2)
        cap = int(plan.info.max_rows)
        d_in = [torch.from_numpy(r).to(dev) for r in recs]
        d_rows = [torch.empty(cap * 2080, dtype=torch.float32, device=dev) for _ in recs]
        d_rgba = [torch.zeros(cap * 2080 * 4, dtype=torch.uint8, device=dev) for _ in recs]
        ptr = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
        plan.decode_device(ptr(d_in), [r.size for r in recs], ptr(d_rows), [cap] * k)
        for rotate in (False, True, False):
            plan.process_device_image(ptr(d_rows), [cap] * k, apt.Contrast.MINMAX, ptr(d_rgba),
                                      rotate=apt.Rotate.YES if rotate else apt.Rotate.NO, map=maps)
            ires = plan.image_results(k)
            for i in range(k):
                h = heights[i]
                assert ires[i].status == 0 and ires[i].height == h
                got = d_rgba[i][:h * 2080 * 4].cpu().numpy().reshape(h, 2080, 4)
                want, excused, _ = mm.overlay(_pre(rows[i], apt.Contrast.MINMAX, None), maps[i].sat_positions, parts,
                                              rotate=rotate)
                assert mm.compare(got, want, excused) == (0, 0), (rotate, i)
        assert "image_map_overlay" in plan.collect_timing()
        # a position count that differs from the height: an error in the record, not a host round trip
        bad = list(maps)
        bad[1] = apt.MapOverlay(maps[1].sat_positions[:-1], apt.MapSettings(), layers)
        plan.process_device_image(ptr(d_rows), [cap] * k, apt.Contrast.MINMAX, ptr(d_rgba), map=bad)
        ires = plan.image_results(k)
        assert ires[1].status == 1 and ires[1].reason == 7
        assert all(ires[i].status == 0 for i in (0, 2, 3))
        with pytest.raises(apt.InvalidError):  # the overlay is colour
            plan.process_device_image(ptr(d_rows), [cap] * k, apt.Contrast.MINMAX, ptr(d_rgba), map=maps, channels=1)
    plan.close()


def test_tiny_scales_end_quickly(fixture_layers):
    # hscale = vscale = 0.01 squeezes the map: about 1 650 fragments land on the busiest pixel, whose run is sorted
    # (heapsort) before it is blended
    parts, layers = fixture_layers
    rows = 1198
    pos = mm.great_circle_track(*TRACKS["south_north"], rows)
    t0 = time.perf_counter()
    _check(_signal(rows, 12), pos, parts, layers, settings={"hscale": 0.01, "vscale": 0.01}, rotate=True,
           label="hscale = vscale = 0.01")
    assert time.perf_counter() - t0 < 60.0


def _stack(n, lon=-58.0, lat=-34.0):
    # n zero-length segments on one point: every one of them draws the same one or two pixels
    return [np.tile([[lon + 0.001, lat + 0.004]], (n, 1))]


def test_stacked_pixel_runs():
    # 3 x 15 000 fragments on the same pixels, in three colours: the long-run sort must keep the draw order
    rows = 200
    pos = mm.great_circle_track(-35.0, -58.0, 3.0, rows)
    parts = {"states": _stack(15000), "countries": _stack(15000), "lakes": _stack(15000)}
    layers = apt.MapLayers(**parts)
    colors = {"states": (255, 0, 0, 90), "countries": (0, 255, 0, 170), "lakes": (0, 0, 255, 60)}
    _, _, info = _check(_signal(rows, 6), pos, parts, layers, colors=colors, label="stacked runs")
    assert info["fragments"] >= 45000


def test_pixel_bound_reported():
    # more than APTGPU_MAP_MAX_PIXEL_FRAGMENTS on one pixel: an error in the record, the image without the overlay
    rows = 200
    pos = mm.great_circle_track(-35.0, -58.0, 3.0, rows)
    layers = apt.MapLayers(countries=_stack(mm.MAX_PIXEL_FRAGMENTS + 10))
    sig = _signal(rows, 7)
    with pytest.raises(apt.InternalError, match="one pixel"):
        apt.process(None, sig, apt.Contrast.MINMAX, orbit=apt.MapOverlay(pos, apt.MapSettings(), layers))
    # and the next call on a fresh target is unaffected
    parts = {"countries": _stack(3)}
    _check(sig, pos, parts, apt.MapLayers(**parts), label="after the bound")


def _random_layers(rng, pos):
    lat0, lon0 = (math.degrees(v) for v in pos[len(pos) // 2])
    out = {}
    for name in mm.LAYER_ORDER:
        if rng.random() < 0.25:
            continue
        parts = []
        for _ in range(int(rng.integers(1, 5))):
            n = int(rng.integers(1, 30))
            start = np.array([lon0 + rng.normal(0, 4), lat0 + rng.normal(0, 4)])
            steps = rng.normal(0, 0.4, (n, 2))
            steps[rng.random(n) < 0.1] = 0.0  # repeated vertices
            parts.append(start + np.cumsum(steps, axis=0))
        out[name] = parts
    return out


def test_soak_random(fixture_layers):
    rng = np.random.default_rng(4242)
    total_exc = 0
    for case in range(200):
        rows = int(rng.integers(2, 160))
        pos = mm.great_circle_track(rng.uniform(-70, 70), rng.uniform(-180, 180), rng.uniform(0, 360), rows)
        parts = _random_layers(rng, pos)
        layers = apt.MapLayers(**parts)
        settings = {"yaw": float(rng.uniform(-0.1, 0.1)), "hscale": float(rng.uniform(0.5, 2.0)),
                    "vscale": float(rng.uniform(0.5, 2.0))}
        colors = {n: tuple(int(v) for v in rng.integers(0, 256, 4)) for n in mm.LAYER_ORDER}
        if rng.random() < 0.2:
            colors["countries"] = colors["countries"][:3] + (255,)
        sig = _signal(rows, case)
        rotate = bool(rng.random() < 0.5)
        ms = apt.MapSettings(**settings, **{f"{k}_color": v for k, v in colors.items()})
        got = apt.process(None, sig, apt.Contrast.MINMAX, rotate=apt.Rotate.YES if rotate else apt.Rotate.NO,
                          orbit=apt.MapOverlay(pos, ms, layers))
        want, excused, _ = mm.overlay(_pre(sig, apt.Contrast.MINMAX, None), pos, parts, settings, colors, rotate)
        unexcused, exc = mm.compare(got, want, excused)
        assert unexcused == 0, case
        total_exc += exc
    print(f"soak: {total_exc} excused differing pixels")
    assert total_exc == 0
