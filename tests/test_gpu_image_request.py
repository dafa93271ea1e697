"""One image request, two ways to run it: every variant of process()'s image stage gives the same bytes and the same
ImageResult through the one-shot entry points (rows on the host) and through the plan (rows on the device), the plan
launches exactly the kernels written down here, the one-shot status callbacks are the lists written down here, and the
checks that need a live plan give the codes and texts written down here.  Two recordings, decoded once: 250 rows
(enough for Telemetry) and 60 rows (too short for it)."""
import ctypes
import itertools
import os

import numpy as np
import pytest

import noaa_apt_amd as apt
import np_map_model as mm
from noaa_apt_amd.testing.synth import synth_apt
from test_gpu_sat_track import PASSES
from test_sat_cpu import orbit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHP = os.path.join(ROOT, "tests", "golden", "shapefiles")
PALETTE = os.path.join(ROOT, "tests", "golden", "palettes", "noaa-apt-daylight.png")
C = apt.Contrast
CONTRASTS = {"telemetry": C.TELEMETRY, "percent": C.Percent(0.98), "minmax": C.MINMAX, "histogram": C.HISTOGRAM,
             "histfloat": C.HISTOGRAM_FLOAT}
TOO_SHORT = "Recording too short for telemetry decoding"


def variants():
    """(contrast, colour, track, projected, png) for every legal combination."""
    out = []
    for contrast, colour in itertools.product(CONTRASTS, ("gray", "palette", "lab")):
        if (colour == "lab") != (contrast == "histogram" and colour != "gray") or \
                (colour == "palette" and contrast in ("histogram", "histfloat")):
            continue
        for track, projected, png in itertools.product(("none", "overlay", "orbit", "orbit_map"), (False, True),
                                                       (False, True)):
            if projected and track == "none":
                continue
            out.append((contrast, colour, track, projected, png))
    return out


def variant_id(v):
    return "-".join([v[0], v[1], v[2], "grid" if v[3] else "swath", "png" if v[4] else "px"])


# The kernels the plan launches for each variant, as collect_timing() names them (without "image_"), in the order of
# their first launch.  Each is launched once per recording.
KERNELS = {
    "telemetry-gray-none-swath-px": "telemetry color",
    "telemetry-gray-none-swath-png": "telemetry color png_filter png_deflate png_place",
    "telemetry-gray-overlay-swath-px": "telemetry color map_overlay",
    "telemetry-gray-overlay-swath-png": "telemetry color map_overlay png_filter png_deflate png_place",
    "telemetry-gray-overlay-grid-px": "telemetry color map_overlay project",
    "telemetry-gray-overlay-grid-png": "telemetry color map_overlay project project_png",
    "telemetry-gray-orbit-swath-px": "telemetry color",
    "telemetry-gray-orbit-swath-png": "telemetry color png_filter png_deflate png_place",
    "telemetry-gray-orbit-grid-px": "telemetry color project_track project",
    "telemetry-gray-orbit-grid-png": "telemetry color project_track project project_png",
    "telemetry-gray-orbit_map-swath-px": "telemetry color map_overlay_sat",
    "telemetry-gray-orbit_map-swath-png": "telemetry color map_overlay_sat png_filter png_deflate png_place",
    "telemetry-gray-orbit_map-grid-px": "telemetry color map_overlay_sat project",
    "telemetry-gray-orbit_map-grid-png": "telemetry color map_overlay_sat project project_png",
    "telemetry-palette-none-swath-px": "telemetry color",
    "telemetry-palette-none-swath-png": "telemetry color png_filter png_deflate png_place",
    "telemetry-palette-overlay-swath-px": "telemetry color map_overlay",
    "telemetry-palette-overlay-swath-png": "telemetry color map_overlay png_filter png_deflate png_place",
    "telemetry-palette-overlay-grid-px": "telemetry color map_overlay project",
    "telemetry-palette-overlay-grid-png": "telemetry color map_overlay project project_png",
    "telemetry-palette-orbit-swath-px": "telemetry color",
    "telemetry-palette-orbit-swath-png": "telemetry color png_filter png_deflate png_place",
    "telemetry-palette-orbit-grid-px": "telemetry color project_track project",
    "telemetry-palette-orbit-grid-png": "telemetry color project_track project project_png",
    "telemetry-palette-orbit_map-swath-px": "telemetry color map_overlay_sat",
    "telemetry-palette-orbit_map-swath-png": "telemetry color map_overlay_sat png_filter png_deflate png_place",
    "telemetry-palette-orbit_map-grid-px": "telemetry color map_overlay_sat project",
    "telemetry-palette-orbit_map-grid-png": "telemetry color map_overlay_sat project project_png",
    "percent-gray-none-swath-px": "percent color",
    "percent-gray-none-swath-png": "percent color png_filter png_deflate png_place",
    "percent-gray-overlay-swath-px": "percent color map_overlay",
    "percent-gray-overlay-swath-png": "percent color map_overlay png_filter png_deflate png_place",
    "percent-gray-overlay-grid-px": "percent color map_overlay project",
    "percent-gray-overlay-grid-png": "percent color map_overlay project project_png",
    "percent-gray-orbit-swath-px": "percent color",
    "percent-gray-orbit-swath-png": "percent color png_filter png_deflate png_place",
    "percent-gray-orbit-grid-px": "percent color project_track project",
    "percent-gray-orbit-grid-png": "percent color project_track project project_png",
    "percent-gray-orbit_map-swath-px": "percent color map_overlay_sat",
    "percent-gray-orbit_map-swath-png": "percent color map_overlay_sat png_filter png_deflate png_place",
    "percent-gray-orbit_map-grid-px": "percent color map_overlay_sat project",
    "percent-gray-orbit_map-grid-png": "percent color map_overlay_sat project project_png",
    "percent-palette-none-swath-px": "percent color",
    "percent-palette-none-swath-png": "percent color png_filter png_deflate png_place",
    "percent-palette-overlay-swath-px": "percent color map_overlay",
    "percent-palette-overlay-swath-png": "percent color map_overlay png_filter png_deflate png_place",
    "percent-palette-overlay-grid-px": "percent color map_overlay project",
    "percent-palette-overlay-grid-png": "percent color map_overlay project project_png",
    "percent-palette-orbit-swath-px": "percent color",
    "percent-palette-orbit-swath-png": "percent color png_filter png_deflate png_place",
    "percent-palette-orbit-grid-px": "percent color project_track project",
    "percent-palette-orbit-grid-png": "percent color project_track project project_png",
    "percent-palette-orbit_map-swath-px": "percent color map_overlay_sat",
    "percent-palette-orbit_map-swath-png": "percent color map_overlay_sat png_filter png_deflate png_place",
    "percent-palette-orbit_map-grid-px": "percent color map_overlay_sat project",
    "percent-palette-orbit_map-grid-png": "percent color map_overlay_sat project project_png",
    "minmax-gray-none-swath-px": "minmax color",
    "minmax-gray-none-swath-png": "minmax color png_filter png_deflate png_place",
    "minmax-gray-overlay-swath-px": "minmax color map_overlay",
    "minmax-gray-overlay-swath-png": "minmax color map_overlay png_filter png_deflate png_place",
    "minmax-gray-overlay-grid-px": "minmax color map_overlay project",
    "minmax-gray-overlay-grid-png": "minmax color map_overlay project project_png",
    "minmax-gray-orbit-swath-px": "minmax color",
    "minmax-gray-orbit-swath-png": "minmax color png_filter png_deflate png_place",
    "minmax-gray-orbit-grid-px": "minmax color project_track project",
    "minmax-gray-orbit-grid-png": "minmax color project_track project project_png",
    "minmax-gray-orbit_map-swath-px": "minmax color map_overlay_sat",
    "minmax-gray-orbit_map-swath-png": "minmax color map_overlay_sat png_filter png_deflate png_place",
    "minmax-gray-orbit_map-grid-px": "minmax color map_overlay_sat project",
    "minmax-gray-orbit_map-grid-png": "minmax color map_overlay_sat project project_png",
    "minmax-palette-none-swath-px": "minmax color",
    "minmax-palette-none-swath-png": "minmax color png_filter png_deflate png_place",
    "minmax-palette-overlay-swath-px": "minmax color map_overlay",
    "minmax-palette-overlay-swath-png": "minmax color map_overlay png_filter png_deflate png_place",
    "minmax-palette-overlay-grid-px": "minmax color map_overlay project",
    "minmax-palette-overlay-grid-png": "minmax color map_overlay project project_png",
    "minmax-palette-orbit-swath-px": "minmax color",
    "minmax-palette-orbit-swath-png": "minmax color png_filter png_deflate png_place",
    "minmax-palette-orbit-grid-px": "minmax color project_track project",
    "minmax-palette-orbit-grid-png": "minmax color project_track project project_png",
    "minmax-palette-orbit_map-swath-px": "minmax color map_overlay_sat",
    "minmax-palette-orbit_map-swath-png": "minmax color map_overlay_sat png_filter png_deflate png_place",
    "minmax-palette-orbit_map-grid-px": "minmax color map_overlay_sat project",
    "minmax-palette-orbit_map-grid-png": "minmax color map_overlay_sat project project_png",
    "histogram-gray-none-swath-px": "minmax equalize color",
    "histogram-gray-none-swath-png": "minmax equalize color png_filter png_deflate png_place",
    "histogram-gray-overlay-swath-px": "minmax equalize color map_overlay",
    "histogram-gray-overlay-swath-png": "minmax equalize color map_overlay png_filter png_deflate png_place",
    "histogram-gray-overlay-grid-px": "minmax equalize color map_overlay project",
    "histogram-gray-overlay-grid-png": "minmax equalize color map_overlay project project_png",
    "histogram-gray-orbit-swath-px": "minmax equalize color",
    "histogram-gray-orbit-swath-png": "minmax equalize color png_filter png_deflate png_place",
    "histogram-gray-orbit-grid-px": "minmax equalize color project_track project",
    "histogram-gray-orbit-grid-png": "minmax equalize color project_track project project_png",
    "histogram-gray-orbit_map-swath-px": "minmax equalize color map_overlay_sat",
    "histogram-gray-orbit_map-swath-png": "minmax equalize color map_overlay_sat png_filter png_deflate png_place",
    "histogram-gray-orbit_map-grid-px": "minmax equalize color map_overlay_sat project",
    "histogram-gray-orbit_map-grid-png": "minmax equalize color map_overlay_sat project project_png",
    "histogram-lab-none-swath-px": "percent equalize_lab color",
    "histogram-lab-none-swath-png": "percent equalize_lab color png_filter png_deflate png_place",
    "histogram-lab-overlay-swath-px": "percent equalize_lab color map_overlay",
    "histogram-lab-overlay-swath-png": "percent equalize_lab color map_overlay png_filter png_deflate png_place",
    "histogram-lab-overlay-grid-px": "percent equalize_lab color map_overlay project",
    "histogram-lab-overlay-grid-png": "percent equalize_lab color map_overlay project project_png",
    "histogram-lab-orbit-swath-px": "percent equalize_lab color",
    "histogram-lab-orbit-swath-png": "percent equalize_lab color png_filter png_deflate png_place",
    "histogram-lab-orbit-grid-px": "percent equalize_lab color project_track project",
    "histogram-lab-orbit-grid-png": "percent equalize_lab color project_track project project_png",
    "histogram-lab-orbit_map-swath-px": "percent equalize_lab color map_overlay_sat",
    "histogram-lab-orbit_map-swath-png": "percent equalize_lab color map_overlay_sat png_filter png_deflate png_place",
    "histogram-lab-orbit_map-grid-px": "percent equalize_lab color map_overlay_sat project",
    "histogram-lab-orbit_map-grid-png": "percent equalize_lab color map_overlay_sat project project_png",
    "histfloat-gray-none-swath-px": "minmax equalize_float color_float",
    "histfloat-gray-none-swath-png": "minmax equalize_float color_float png_filter png_deflate png_place",
    "histfloat-gray-overlay-swath-px": "minmax equalize_float color_float map_overlay",
    "histfloat-gray-overlay-swath-png": "minmax equalize_float color_float map_overlay png_filter png_deflate png_place",
    "histfloat-gray-overlay-grid-px": "minmax equalize_float color_float map_overlay project",
    "histfloat-gray-overlay-grid-png": "minmax equalize_float color_float map_overlay project project_png",
    "histfloat-gray-orbit-swath-px": "minmax equalize_float color_float",
    "histfloat-gray-orbit-swath-png": "minmax equalize_float color_float png_filter png_deflate png_place",
    "histfloat-gray-orbit-grid-px": "minmax equalize_float color_float project_track project",
    "histfloat-gray-orbit-grid-png": "minmax equalize_float color_float project_track project project_png",
    "histfloat-gray-orbit_map-swath-px": "minmax equalize_float color_float map_overlay_sat",
    "histfloat-gray-orbit_map-swath-png": "minmax equalize_float color_float map_overlay_sat png_filter png_deflate png_place",
    "histfloat-gray-orbit_map-grid-px": "minmax equalize_float color_float map_overlay_sat project",
    "histfloat-gray-orbit_map-grid-png": "minmax equalize_float color_float map_overlay_sat project project_png",
}


class Env:
    pass


@pytest.fixture(scope="module")
def env():
    torch = pytest.importorskip("torch")
    e = Env()
    dev = torch.device("cuda:0")
    recs = [synth_apt(48000, 125, 300), synth_apt(48000, 30, 310)]
    e.k = len(recs)
    e.plan = apt.Plan(apt.Settings(), apt.Rate.hz(48000), True, max_samples=max(r.size for r in recs), max_batch=e.k)
    e.cap = int(e.plan.info.max_rows)
    e.d_in = [torch.from_numpy(r).to(dev) for r in recs]
    e.d_rows = [torch.empty(e.cap * 2080, dtype=torch.float32, device=dev) for _ in recs]
    e.d_img = [torch.zeros(e.cap * 2080 * 4, dtype=torch.uint8, device=dev) for _ in recs]
    e.plan.decode_device([t.data_ptr() for t in e.d_in], [r.size for r in recs], [t.data_ptr() for t in e.d_rows],
                         [e.cap] * e.k)
    e.plan.synchronize()
    e.heights = [int(r.n_rows) for r in e.plan.results(e.k)]
    assert e.heights[0] >= 200 > e.heights[1] > 0, e.heights
    e.rows = [e.d_rows[i][:e.heights[i] * 2080].cpu().numpy() for i in range(e.k)]
    e.layers = apt.MapLayers(countries=apt.read_shapefile(os.path.join(SHP, "countries.shp"), 5),
                             lakes=apt.read_shapefile(os.path.join(SHP, "lakes.shp"), 5))
    e.settings = apt.MapSettings(hscale=1.1, vscale=0.9, yaw=0.02)
    e.tracks = [mm.great_circle_track(-34.0, -62.0, 11.0, h) for h in e.heights]
    tle, name, ms, _ = PASSES["noaa19_north"]
    e.orbits = {False: [orbit(tle, name, "start", ms) for _ in recs],
                True: [orbit(tle, name, "start", ms, e.settings) for _ in recs]}
    sat_tracks = [apt.sat_track(e.orbits[False][i], e.heights[i]) for i in range(e.k)]
    fit = lambda t: apt.projection_fit(t, apt.Projection.EQUIRECTANGULAR, max_width=64)  # noqa: E731
    e.grids = {"pos": [fit(t) for t in e.tracks], "sat": [fit(t) for t in sat_tracks]}
    assert all(g.width <= 64 for gs in e.grids.values() for g in gs)
    e.d_out = [torch.zeros(64 * 4096 * 4, dtype=torch.uint8, device=dev) for _ in recs]
    e.d_png = [torch.zeros(apt.png_bound(2080, e.cap, 4), dtype=torch.uint8, device=dev) for _ in recs]
    e.colors = {"gray": None, "palette": apt.ColorSettings(PALETTE, 0.1, -0.2, 0.3, 0.0),
                "lab": apt.ColorSettings(PALETTE, 0.1, -0.2, 0.3, 0.0, equalize_lab=True)}
    e.plan.enable_timing(2)
    e.plan.collect_timing()
    yield e
    e.plan.close()


def ptr(ts):
    return [t.data_ptr() for t in ts]


def run_plan(e, v):
    """The plan call of variant v: ([(kernel name, launches)] in launch order, [(record, output bytes)] per recording)."""
    contrast, colour, track, projected, png = v
    kw = dict(color=e.colors[colour])
    grids = e.grids["pos" if track == "overlay" else "sat"]
    if track == "overlay":
        kw["map"] = [apt.MapOverlay(t, e.settings, e.layers) for t in e.tracks]
    elif track != "none":
        kw.update(orbit=e.orbits[track == "orbit_map"], layers=e.layers if track == "orbit_map" else None)
    if not projected and track in ("orbit", "orbit_map"):
        kw["rotate"] = apt.Rotate.ORBIT
    if not projected and track == "none" and colour == "palette":
        kw["rotate"] = apt.Rotate.YES
    if projected:
        for g, t in zip(grids, e.d_out):
            assert g.width * g.height * 4 <= t.numel()
        kw["projection"] = (grids, ptr(e.d_out), [g.width * g.height * 4 for g in grids])
    if png:
        kw["png"] = (ptr(e.d_png), [t.numel() for t in e.d_png])
    e.plan.process_device_image(ptr(e.d_rows), [e.cap] * e.k, CONTRASTS[contrast], ptr(e.d_img), **kw)
    recs = e.plan.image_results(e.k)
    names = [(n, launches) for n, (_, launches) in e.plan.collect_timing().items()]
    channels = 4 if colour != "gray" or track in ("overlay", "orbit_map") else 1
    out = []
    for i, r in enumerate(recs):
        if r.status != 0:
            data = None
        elif png:
            data = e.d_png[i][:r.png_bytes].cpu().numpy().tobytes()
        elif projected:
            data = e.d_out[i][:grids[i].width * grids[i].height * 4].cpu().numpy().tobytes()
        else:
            data = e.d_img[i][:e.heights[i] * 2080 * channels].cpu().numpy().tobytes()
        out.append((r, data))
    return names, out


def run_one_shot(e, v, i, ctx=None):
    """The one-shot call of variant v on recording i's downloaded rows: (record, output bytes)."""
    contrast, colour, track, projected, png = v
    kw = dict(color=e.colors[colour], png=png, return_info=True)
    if track == "overlay":
        kw["orbit"] = apt.MapOverlay(e.tracks[i], e.settings, e.layers)
    elif track != "none":
        kw.update(orbit=e.orbits[track == "orbit_map"][i], layers=e.layers if track == "orbit_map" else None)
    if not projected and track in ("orbit", "orbit_map"):
        kw["rotate"] = apt.Rotate.ORBIT
    if not projected and track == "none" and colour == "palette":
        kw["rotate"] = apt.Rotate.YES
    if projected:
        kw["projection"] = e.grids["pos" if track == "overlay" else "sat"][i]
    out, info = apt.process(ctx, e.rows[i], CONTRASTS[contrast], **kw)
    return info, out if png else out.tobytes()


def test_one_shot_and_plan_agree(env):
    e = env
    checked = 0
    assert [variant_id(v) for v in variants()] == list(KERNELS)
    for v in variants():
        names, plan_out = run_plan(e, v)
        assert names == [("image_" + k, e.k) for k in KERNELS[variant_id(v)].split()], variant_id(v)
        for i, (rec, data) in enumerate(plan_out):
            label = (variant_id(v), i)
            if v[0] == "telemetry" and i == 1:  # 60 rows: reported in the record, raised by the one-shot call
                assert (rec.status, rec.reason) == (1, 2), label
                with pytest.raises(apt.InternalError, match=TOO_SHORT):
                    run_one_shot(e, v, i)
                continue
            assert rec.status == 0 and rec.height == e.heights[i], label
            info, one = run_one_shot(e, v, i)
            assert bytes(info) == bytes(rec), label
            assert one == data, label
            checked += 1
    assert checked == 2 * len(variants()) - sum(v[0] == "telemetry" for v in variants())
    print(f"{len(variants())} variants, {checked} one-shot / plan pairs equal")


def _callbacks():
    seen, steps = [], []
    ctx = apt.Context.decode(ui_callback=lambda p, t: seen.append((round(p, 2), t)),
                             step_callback=lambda step_id, *a: steps.append(step_id))
    return seen, steps, ctx


def test_one_shot_status_callbacks(env):
    e = env
    seen, steps, ctx = _callbacks()
    run_one_shot(e, ("minmax", "gray", "none", False, False), 0, ctx)
    assert seen == [(0.1, "Mapping values"), (0.3, "Generating image")] and steps == []
    seen, steps, ctx = _callbacks()
    apt.process(ctx, e.rows[0], C.Percent(0.98), rotate=apt.Rotate.YES,
                orbit=apt.MapOverlay(e.tracks[0], e.settings, e.layers))
    assert seen == [(0.1, "Adjusting contrast using 98 percent"), (0.3, "Generating image"), (0.5, "Drawing map"),
                    (0.9, "Rotating output image")] and steps == []
    seen, steps, ctx = _callbacks()
    run_one_shot(e, ("telemetry", "gray", "none", False, False), 0, ctx)
    assert seen == [(0.1, "Adjusting contrast from telemetry"), (0.3, "Generating image")]
    assert steps == ["telemetry_a", "telemetry_b", "telemetry_correlation", "telemetry_variance", "telemetry_quality"]
    seen, steps, ctx = _callbacks()
    with pytest.raises(apt.InternalError, match="^Percent given should be between 0 and 1$"):
        apt.process(ctx, e.rows[0], C.Percent(1.5), color=e.colors["palette"])
    assert seen == [(0.1, "Adjusting contrast using 150 percent")] and steps == []


def test_live_plan_checks(env):
    e = env
    k, caps, img = e.k, [e.cap] * e.k, ptr(e.d_img)

    def refused(kind, text, *args, **kw):
        with pytest.raises(kind) as info:
            e.plan.process_device_image(*args, **kw)
        assert str(info.value) == text

    refused(apt.InvalidError, "count exceeds the recordings of the last decode call", ptr(e.d_rows) * 2, caps * 2,
            C.MINMAX, img * 2)
    refused(apt.InvalidError, "null device pointer", [ptr(e.d_rows)[0], 0], caps, C.MINMAX, img)
    refused(apt.InvalidError, "null device pointer", ptr(e.d_rows), caps, C.MINMAX, [img[0], 0])
    refused(apt.InvalidError, "d_images must be 4-byte aligned", ptr(e.d_rows), caps, C.MINMAX, [img[0], img[1] + 2])
    refused(apt.InvalidError, "d_images must be 16-byte aligned for channels = 4", ptr(e.d_rows), caps, C.MINMAX,
            [img[0], img[1] + 4], channels=4)
    grids = e.grids["pos"]
    sizes = [g.width * g.height * 4 for g in grids]
    out = ptr(e.d_out)
    refused(apt.InvalidError, "d_out must be non-null and 4-byte aligned", ptr(e.d_rows), caps, C.MINMAX, img,
            map=e.tracks, projection=(grids, [out[0], out[1] + 2], sizes))
    refused(apt.InvalidError, "d_out must be non-null and 4-byte aligned", ptr(e.d_rows), caps, C.MINMAX, img,
            map=e.tracks, projection=(grids, [0, out[1]], sizes))
    refused(apt.InvalidError, "draw_map must be set for every recording of the call or for none", ptr(e.d_rows), caps,
            C.MINMAX, img, orbit=[e.orbits[True][0], e.orbits[False][1]], layers=e.layers)
    refused(apt.InvalidError, "null device pointer (d_png)", ptr(e.d_rows), caps, C.MINMAX, img,
            png=([ptr(e.d_png)[0], 0], [e.d_png[0].numel()] * 2))
    for p in (1.5, -0.25):
        refused(apt.InternalError, "Percent given should be between 0 and 1", ptr(e.d_rows), caps, C.Percent(p), img)
        with pytest.raises(apt.InternalError, match="^Percent given should be between 0 and 1$"):
            e.plan.process_device(ptr(e.d_rows), caps, C.Percent(p), img)
    # the plan still serves the next call
    names, out = run_plan(e, ("minmax", "gray", "none", False, False))
    assert all(r.status == 0 for r, _ in out)


ZERO = "^Can't get minimum of a zero length vector$"


def test_zero_length_one_shot(env):
    e = env
    empty = np.zeros(0, np.float32)
    pos = np.zeros((0, 2))
    grid = e.grids["pos"][0]
    o = e.orbits[False][0]
    calls = {
        "gray": dict(),
        "image": dict(color=e.colors["palette"]),
        "map": dict(orbit=apt.MapOverlay(pos, e.settings, e.layers)),
        "png": dict(png=True),
        "orbit": dict(orbit=o),
        "project": dict(orbit=o, projection=grid),
    }
    for name, kw in calls.items():
        for contrast in (C.MINMAX, C.Percent(0.5)) + ((C.HISTOGRAM,) if name != "image" else ()):
            with pytest.raises(apt.InternalError, match=ZERO):
                apt.process(None, empty, contrast, **kw)
        with pytest.raises(apt.InternalError, match="^" + TOO_SHORT + "$"):  # (from the record)
            apt.process(None, empty, C.TELEMETRY, **kw)


# ------------------------------------------------------------------ the plan's record readbacks
READBACKS = ("despeckle_results", "thermal_results", "geoloc_results", "track_results", "image_results")


def test_plan_result_readbacks():
    """aptgpu_plan_{despeckle,thermal,geoloc,track,image}_results on a plan of its own: refused until their stage has
    run on the recordings asked for, refused beyond the recordings of the last decode call, empty for count 0, and
    record i the same whatever the count; the struct_size of the two records that carry one."""
    import torch
    import np_thermal_model as tm
    dev = torch.device("cuda:0")
    recs = [synth_apt(48000, s, 700 + i) for i, s in enumerate((6, 8, 11))]
    plan = apt.Plan(apt.Settings(), apt.Rate.hz(48000), True, max_samples=max(r.size for r in recs), max_batch=3)
    cap = int(plan.info.max_rows)
    k = 2  # (of the three the plan has room for)
    d_in = [torch.from_numpy(r).to(dev) for r in recs[:k]]
    new = lambda n, dtype=torch.float32: [torch.zeros(n, dtype=dtype, device=dev) for _ in range(k)]  # noqa: E731
    d_rows, d_out, d_trk, d_kelvin = new(cap * 2080), new(cap * 2080), new(cap * 2080), new(cap * 909)
    d_cos, d_img = new(cap * 909), new(cap * 2080, torch.uint8)
    caps = [cap] * k
    plan.decode_device(ptr(d_in), [r.size for r in recs[:k]], ptr(d_rows), caps)
    heights = [int(r.n_rows) for r in plan.results(k)]
    assert min(heights) >= 2
    # before any stage has run (image_results has no records at all then, whatever the count)
    for name in READBACKS:
        for count in (1, 2):
            with pytest.raises(apt.InvalidError):
                getattr(plan, name)(count)
        if name == "image_results":
            with pytest.raises(apt.InvalidError):
                plan.image_results(0)
        else:
            assert getattr(plan, name)(0) == []
    tracks = [mm.great_circle_track(35.0, -80.0, 191.0, h) for h in heights]
    stages = {
        "despeckle_results": lambda: plan.despeckle_device(ptr(d_rows), caps, ptr(d_out), apt.DespeckleSettings(1, 0.1)),
        "thermal_results": lambda: plan.calibrate_thermal_device(
            ptr(d_rows), caps, ptr(d_kelvin), apt.ThermalCoefficients(tm.PRT, tm.CH3B, tm.CH4, tm.CH5),
            apt.ThermalSettings("B", "4", t_low=180, t_high=320, image_channels=0)),
        "geoloc_results": lambda: plan.geolocate_device(
            ptr(d_rows), caps, tracks, apt.GeolocSettings("A", apt.RefTime.Start(1730635200000), 0.0), None, None,
            ptr(d_cos), None),
        "track_results": lambda: plan.track_device(ptr(d_trk), caps),
        "image_results": lambda: plan.process_device_image(ptr(d_rows), caps, CONTRASTS["minmax"], ptr(d_img)),
    }
    plan.enable_timing(2)
    plan.collect_timing()
    for name in READBACKS:
        stages[name]()
        read = getattr(plan, name)
        both = read(2)
        assert len(both) == 2, name
        if name != "track_results":  # (the tracker finds its own rows)
            assert [r.height for r in both] == heights, name
        with pytest.raises(apt.InvalidError):
            read(3)
        assert read(0) == []
        one = read(1)
        assert len(one) == 1 and bytes(one[0]) == bytes(both[0]), name
    # the launches of the five stages under the plan's timer, in the order of their first appearance
    assert list(plan.collect_timing()) == [
        "image_percent", "image_despeckle", "image_telemetry", "image_thermal_space", "image_thermal_setup",
        "image_thermal_map", "image_geoloc_track", "image_geoloc_rows", "image_geoloc", "track_score", "track_dp",
        "track_rows", "image_minmax", "image_color"]
    # a caller built against a shorter geolocation record gets its own size back and nothing beyond it
    arr = (apt.GeolocResult * 2)()
    ctypes.memset(arr, 0xAB, ctypes.sizeof(arr))
    for r in arr:
        r.struct_size = 16
    assert apt.lib().aptgpu_plan_geoloc_results(plan._p, 2, arr) == 0
    full = plan.geoloc_results(2)
    for r, want in zip(arr, full):
        assert bytes(r)[:16] == bytes(apt.GeolocResult(16, want.status, want.reason, want.height))[:16]
        assert bytes(r)[16:] == b"\xab" * 24
    # the tracker's record is refused when shorter (nothing written), and a longer one keeps its size and its tail
    size = ctypes.sizeof(apt.TrackResult)
    arr = (apt.TrackResult * 2)()
    ctypes.memset(arr, 0xAB, ctypes.sizeof(arr))
    arr[0].struct_size = size
    arr[1].struct_size = size - 4
    assert apt.lib().aptgpu_plan_track_results(plan._p, 2, arr) == apt.InvalidError.code
    assert bytes(arr)[4:size] == b"\xab" * (size - 4) and bytes(arr[1])[4:] == b"\xab" * (size - 4)

    class Longer(ctypes.Structure):
        _fields_ = [("r", apt.TrackResult), ("tail", ctypes.c_uint8 * 8)]
    longer = Longer()
    ctypes.memset(ctypes.byref(longer), 0xAB, ctypes.sizeof(longer))
    longer.r.struct_size = size + 8
    assert apt.lib().aptgpu_plan_track_results(plan._p, 1, ctypes.cast(ctypes.byref(longer),
                                                                       ctypes.POINTER(apt.TrackResult))) == 0
    want = plan.track_results(1)[0]
    assert longer.r.struct_size == size + 8 and bytes(longer.r)[4:] == bytes(want)[4:]
    assert bytes(longer.tail) == b"\xab" * 8
    plan.close()
