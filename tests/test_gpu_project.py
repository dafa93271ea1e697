"""The reprojection on the GPU (process(projection=...), project_image and the plan chain) against
np_project_model.py under the parity contract of DESIGN.md §15: the image equals the model's bit for bit on every
pixel whose decision margin is at least np_project_model.TAU.  The model alone decides which pixels are left out;
they are counted and printed, and a test may leave out at most 16 pixels and at most 0.1 % of its valid pixels.

Swath images come from seeded signals through the existing process(); the GPU's own pre-projection image feeds the
model (tests/test_gpu_process_image.py and its siblings pin that image).  The signals are constant over blocks of
4 rows x 8 pixels: a bilinear sample rounds within TAU of k + 0.5 with probability 2 * 255 * TAU * 2 ~ 1e-3 per
distinct channel wherever its four neighbours differ, which alone would spend the 0.1 % allowance; with the blocks
only the samples that straddle a block edge (about one in three) can.  False colour has three distinct channels,
so its signals use blocks of 16 rows x 52 pixels (about one sample in twelve)."""
import math
import os

import numpy as np
import pytest

import noaa_apt_amd as apt
import np_map_model as mm
import np_project_model as pm
from test_gpu_sat_track import PASSES, _decode_png
from test_sat_cpu import orbit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHP = os.path.join(ROOT, "tests", "golden", "shapefiles")
PALETTES = os.path.join(ROOT, "tests", "golden", "palettes")
P = apt.Projection


@pytest.fixture(scope="module")
def fixture_layers():
    parts = {"countries": apt.read_shapefile(os.path.join(SHP, "countries.shp"), 5),
             "lakes": apt.read_shapefile(os.path.join(SHP, "lakes.shp"), 5)}
    return parts, apt.MapLayers(countries=parts["countries"], lakes=parts["lakes"])


def _signal(rows, seed, block=(4, 8)):
    rng = np.random.default_rng(seed)
    bh, bw = block
    blocks = rng.random(((rows + bh - 1) // bh, 2080 // bw)).astype(np.float32)
    return np.ascontiguousarray(np.repeat(np.repeat(blocks, bh, axis=0), bw, axis=1)[:rows]).reshape(-1)


def _color(kind):
    if kind == "gray":
        return None, apt.Contrast.MINMAX
    return (apt.ColorSettings(os.path.join(PALETTES, "noaa-apt-daylight.png"), 0.1, -0.2, 0.3, 0.0,
                              equalize_lab=kind == "lab"),
            apt.Contrast.HISTOGRAM if kind == "lab" else apt.Contrast.Percent(0.98))


def _model(pre, pos, ps, ms=None):
    ms = ms or apt.MapSettings()
    return pm.project(pre, pos, ps.kind, ps.width, ps.height, ps.lat_north, ps.lon_west, ps.step, ps.channel,
                      ps.sampling, ps.grid_deg, ps.grid_color, ms.yaw, ms.hscale, ms.vscale)


def _compare(got, pre, pos, ps, label, ms=None, allow=None):
    """The contract; returns the model's (image, margin, info)."""
    want, margin, info = _model(pre, pos, ps, ms)
    assert got.shape == want.shape == (ps.height, ps.width, 4) and got.dtype == np.uint8
    bad, low = pm.compare(got, want, margin)
    print(f"{label}: {info['n_valid']} valid of {ps.width * ps.height} pixels, {info['excused']} left out "
          f"(margin < {pm.TAU}), {low} of them differ, {bad} differ outside")
    assert bad == 0, label
    cap = min(16, int(0.001 * info["n_valid"])) if allow is None else allow
    assert info["excused"] <= cap, (label, info["excused"], cap)
    return want, margin, info


def _grid(pos, kind, width, height, step, at=0.5, **kw):
    """A width x height grid centred on the track's position at fraction `at`."""
    lat, lon = (math.degrees(v) for v in pos[int(at * (len(pos) - 1))])
    if kind == P.MERCATOR:
        lat_north = math.degrees(math.atan(math.sinh(pm.y_north(lat) + 0.5 * (height - 1) * pm.rad(step))))
    else:
        lat_north = lat + 0.5 * (height - 1) * step
    return apt.ProjectionSettings(kind, width, height, lat_north, lon - 0.5 * (width - 1) * step, step, **kw)


ROWS = 160
TRACK = mm.great_circle_track(-34.0, -62.0, 11.0, ROWS)


@pytest.fixture(scope="module")
def gray():
    sig = _signal(ROWS, 7)
    return sig, apt.process(None, sig, apt.Contrast.MINMAX)


# ---------------------------------------------------------------- parity with the model
@pytest.mark.parametrize("channel", [P.CHANNEL_A, P.CHANNEL_B])
@pytest.mark.parametrize("sampling", [P.NEAREST, P.BILINEAR])
@pytest.mark.parametrize("kind", [P.EQUIRECTANGULAR, P.MERCATOR])
def test_parity_131x77(gray, kind, sampling, channel):
    sig, pre = gray
    ps = _grid(TRACK, kind, 131, 77, 0.043, channel=channel, sampling=sampling)
    got = apt.process(None, sig, apt.Contrast.MINMAX, orbit=TRACK, projection=ps)
    _, _, info = _compare(got, pre, TRACK, ps, f"131x77 kind {kind} sampling {sampling} channel {channel}")
    assert info["n_valid"] > 3000
    if channel == P.CHANNEL_B:  # the two channels are different pictures
        a = apt.process(None, sig, apt.Contrast.MINMAX, orbit=TRACK,
                        projection=_grid(TRACK, kind, 131, 77, 0.043, sampling=sampling))
        assert np.any(a != got)


@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1)])
@pytest.mark.parametrize("kind", [P.EQUIRECTANGULAR, P.MERCATOR])
def test_parity_thin_grids(gray, kind, shape):
    sig, pre = gray
    ps = _grid(TRACK, kind, shape[0], shape[1], 0.031, at=0.4, sampling=P.BILINEAR)
    got = apt.process(None, sig, apt.Contrast.MINMAX, orbit=TRACK, projection=ps)
    _, _, info = _compare(got, pre, TRACK, ps, f"{shape} kind {kind}", allow=0)
    assert info["n_valid"] > 0


@pytest.mark.parametrize("kind", [P.EQUIRECTANGULAR, P.MERCATOR])
def test_parity_fitted_256(gray, kind):
    sig, pre = gray
    fit = apt.projection_fit(TRACK, kind, max_width=256)
    ps = apt.ProjectionSettings(kind, 256, 256, fit.lat_north, fit.lon_west, fit.step, sampling=P.BILINEAR)
    got = apt.process(None, sig, apt.Contrast.MINMAX, orbit=TRACK, projection=ps)
    # the fitted grid holds the track's first point: the pixels within NEAR_START of it are left out too
    _, margin, info = _compare(got, pre, TRACK, ps, f"fitted 256 kind {kind}")
    assert 0 < info["n_valid"] < 256 * 256 and not info["valid"][0, 0]


# ---------------------------------------------------------------- input kinds
@pytest.mark.parametrize("kind", ["palette", "lab"])
def test_colour_sources(kind):
    color, contrast = _color(kind)
    sig = _signal(ROWS, 21, block=(16, 52))
    pre = apt.process(None, sig, contrast, color=color)
    for sampling in (P.NEAREST, P.BILINEAR):
        ps = _grid(TRACK, P.MERCATOR, 90, 70, 0.05, sampling=sampling)
        got = apt.process(None, sig, contrast, color=color, orbit=TRACK, projection=ps)
        _compare(got, pre, TRACK, ps, f"{kind} sampling {sampling}")
        assert np.any(got[..., 0] != got[..., 1])


def test_overlay_is_drawn_first(fixture_layers):
    _, layers = fixture_layers
    rows = 200
    pos = mm.great_circle_track(-45.0, -66.0, 8.0, rows)
    sig = _signal(rows, 5)
    ov = apt.MapOverlay(pos, apt.MapSettings(hscale=1.2, vscale=0.9, yaw=0.03), layers)
    pre = apt.process(None, sig, apt.Contrast.MINMAX, orbit=ov)
    plain = apt.process(None, sig, apt.Contrast.MINMAX)
    assert np.any(pre[..., :3] != plain[..., None])  # something was drawn
    ps = _grid(pos, P.EQUIRECTANGULAR, 150, 100, 0.05, sampling=P.BILINEAR)
    got = apt.process(None, sig, apt.Contrast.MINMAX, orbit=ov, projection=ps)
    _compare(got, pre, pos, ps, "overlay", ms=ov.settings)
    assert np.any(got[..., 0] != got[..., 2])  # the yellow coastline came through


# ---------------------------------------------------------------- special geometry
def test_antimeridian(gray):
    pos = mm.great_circle_track(5.0, 179.2, 14.0, ROWS)
    sig, pre = gray
    ps = _grid(pos, P.EQUIRECTANGULAR, 120, 60, 0.05)
    assert ps.lon_west < 180.0 < ps.lon_west + (ps.width - 1) * ps.step
    got = apt.process(None, sig, apt.Contrast.MINMAX, orbit=pos, projection=ps)
    _, _, info = _compare(got, pre, pos, ps, "antimeridian")
    assert info["valid"][:, 0].any() and info["valid"][:, -1].any()


def test_near_start_pixels_are_the_only_ones_left_out(gray):
    sig, pre = gray
    ps = _grid(TRACK, P.EQUIRECTANGULAR, 200, 200, 0.06, at=0.0)
    got = apt.process(None, sig, apt.Contrast.MINMAX, orbit=TRACK, projection=ps)
    _, margin, info = _compare(got, pre, TRACK, ps, "near start")
    low = np.argwhere(margin < pm.TAU)
    assert len(low) > 0
    for i, j in low:
        ll = (pm.row_lat(ps.kind, ps.lat_north, ps.step, float(i)), pm.col_lon(ps.lon_west, ps.step, float(j)))
        assert mm.distance(ll, tuple(TRACK[0])) < pm.NEAR_START


def test_off_swath_is_transparent(gray):
    sig, _ = gray
    ps = apt.ProjectionSettings(P.MERCATOR, 70, 50, 60.0, 100.0, 0.1)
    got = apt.process(None, sig, apt.Contrast.MINMAX, orbit=TRACK, projection=ps)
    assert got.shape == (50, 70, 4) and not got.any()


def test_pi_3_rule_paints_nothing_beyond_60_degrees():
    rows = 100
    pos = mm.great_circle_track(-40.0, -60.0, 0.0, rows, seconds_per_row=12.0)
    assert mm.distance(tuple(pos[0]), tuple(pos[-1])) > math.pi / 3
    sig = _signal(rows, 3)
    ms = apt.MapSettings(vscale=0.5)
    ps = apt.ProjectionSettings(P.EQUIRECTANGULAR, 60, 180, 45.0, -75.0, 0.5, geometry=ms)
    got = apt.process(None, sig, apt.Contrast.MINMAX, orbit=pos, projection=ps)
    pre = apt.process(None, sig, apt.Contrast.MINMAX)
    _, _, info = _compare(got, pre, pos, ps, "pi/3", ms=ms)
    painted = got[..., 3] != 0
    assert painted.any()
    for i, j in np.argwhere(painted):
        ll = (pm.row_lat(ps.kind, ps.lat_north, ps.step, float(i)), pm.col_lon(ps.lon_west, ps.step, float(j)))
        assert mm.distance(ll, tuple(pos[0])) < math.pi / 3
    # without the rule the rows beyond it would have been painted: the clamped projection lands inside the band
    sc = mm.Scalars(pos, vscale=0.5)
    x, y = mm.rel_px(sc, (math.radians(28.0), math.radians(-60.0)))
    assert -456 < x < 456 and 0 < y < rows and not painted[int(round((45.0 - 28.0) / 0.5)), 30]


def test_degenerate_track_is_transparent(gray):
    sig, _ = gray
    pos = np.repeat(TRACK[:1], ROWS, axis=0)
    ps = _grid(TRACK, P.EQUIRECTANGULAR, 40, 30, 0.1)
    got, info = apt.process(None, sig, apt.Contrast.MINMAX, orbit=pos, projection=ps, return_info=True)
    assert info.status == 0 and info.height == ROWS and not got.any()


# ---------------------------------------------------------------- graticule
@pytest.mark.parametrize("kind", [P.EQUIRECTANGULAR, P.MERCATOR])
@pytest.mark.parametrize("color", [(255, 0, 0, 255), (10, 200, 90, 120)])
def test_graticule(gray, kind, color):
    sig, pre = gray
    ps = _grid(TRACK, kind, 140, 90, 0.05, grid_deg=1.0, grid_color=color)
    got = apt.process(None, sig, apt.Contrast.MINMAX, orbit=TRACK, projection=ps)
    _, _, info = _compare(got, pre, TRACK, ps, f"graticule kind {kind} {color}")
    cols, rows = info["graticule"]
    assert cols.sum() >= 6 and rows.sum() >= 3  # rows and columns cross, on and off the swath
    off = _grid(TRACK, kind, 140, 90, 0.05)
    plain = apt.process(None, sig, apt.Contrast.MINMAX, orbit=TRACK, projection=off)
    lines = rows[:, None] | cols[None, :]
    assert np.array_equal(got[~lines], plain[~lines]) and np.any(got[lines] != plain[lines])
    i, j = np.nonzero(rows)[0][0], np.nonzero(cols)[0][0]
    assert tuple(got[i, j]) == mm.blend(tuple(int(v) for v in plain[i, j]), color)  # blended once


# ---------------------------------------------------------------- a check that does not use rel_px
def test_rows_land_where_the_track_says():
    rows = 180
    pos = mm.great_circle_track(-20.0, -64.0, 13.0, rows)
    img = np.zeros((rows, 2080, 4), np.uint8)  # every pixel encodes its own (row, column)
    r, c = np.meshgrid(np.arange(rows), np.arange(2080), indexing="ij")
    img[..., 0], img[..., 1], img[..., 2], img[..., 3] = r & 255, c & 255, c >> 8, 255
    ps = apt.projection_fit(pos, P.EQUIRECTANGULAR, step=0.02)
    got = apt.project_image(img, pos, ps)
    for k in range(1, rows - 1):
        i = int(round((ps.lat_north - math.degrees(pos[k, 0])) / ps.step))
        j = int(round((math.degrees(pos[k, 1]) - ps.lon_west) / ps.step))
        px = got[i, j]
        assert px[3] == 255, k
        assert abs(int(px[0]) - k) <= 1 and abs((int(px[1]) | int(px[2]) << 8) - 539) <= 1, (k, px)


# ---------------------------------------------------------------- both track sources, PNG, standalone
def test_orbit_settings_track(fixture_layers):
    _, layers = fixture_layers
    tle, name, ms, _ = PASSES["noaa19_north"]
    rows = 120
    sig = _signal(rows, 34)
    o = orbit(tle, name, "end", ms + 500 * rows)
    pos = apt.sat_track(o, rows)
    ps = _grid(pos, P.MERCATOR, 110, 80, 0.05, sampling=P.BILINEAR)
    got = apt.process(None, sig, apt.Contrast.MINMAX, orbit=o, projection=ps)
    pre = apt.process(None, sig, apt.Contrast.MINMAX)
    _compare(got, pre, pos, ps, "OrbitSettings, RefTime.End")
    # the caller's track gives the same picture
    assert np.array_equal(got, apt.process(None, sig, apt.Contrast.MINMAX, orbit=pos, projection=ps))
    # with draw_map the overlay is drawn first
    od = orbit(tle, name, "end", ms + 500 * rows, apt.MapSettings())
    drawn = apt.process(None, sig, apt.Contrast.MINMAX, orbit=od, layers=layers, projection=ps)
    _compare(drawn, apt.process(None, sig, apt.Contrast.MINMAX, orbit=od, layers=layers), pos, ps, "OrbitSettings + map")


def test_png_and_standalone(gray):
    sig, pre = gray
    ps = _grid(TRACK, P.EQUIRECTANGULAR, 131, 77, 0.043, sampling=P.BILINEAR, grid_deg=2.0)
    want = apt.process(None, sig, apt.Contrast.MINMAX, orbit=TRACK, projection=ps)
    data, info = apt.process(None, sig, apt.Contrast.MINMAX, orbit=TRACK, projection=ps, png=True, return_info=True)
    assert info.png_bytes == len(data) and info.height == ROWS
    assert np.array_equal(_decode_png(data), want)
    # project_image on the same pixels: the same grid, from a gray and from an RGBA source
    assert np.array_equal(apt.project_image(pre, TRACK, ps), want)
    rgba = np.concatenate([np.repeat(pre[:, :, None], 3, axis=2), np.full(pre.shape + (1,), 255, np.uint8)], axis=2)
    assert np.array_equal(apt.project_image(rgba, TRACK, ps), want)
    assert np.array_equal(_decode_png(apt.project_image(pre, TRACK, ps, png=True)), want)
    with pytest.raises(apt.InternalError, match="differs from the image height"):
        apt.project_image(pre, TRACK[:-1], ps)


def test_refusals():
    sig = _signal(8, 1)
    pos = mm.great_circle_track(0.0, 0.0, 10.0, 8)
    ps = apt.ProjectionSettings(P.EQUIRECTANGULAR, 8, 8, 1.0, -1.0, 0.1)
    for rot in (apt.Rotate.YES, apt.Rotate.ORBIT):
        with pytest.raises(apt.InvalidError, match="rotate"):
            apt.process(None, sig, apt.Contrast.MINMAX, rotate=rot, orbit=pos, projection=ps)
    with pytest.raises(apt.InvalidError, match="step must be finite and > 0"):
        apt.process(None, sig, apt.Contrast.MINMAX, orbit=pos,
                    projection=apt.ProjectionSettings(P.EQUIRECTANGULAR, 8, 8, 1.0, -1.0, 0.0))
    assert apt.process(None, sig, apt.Contrast.MINMAX, orbit=pos, projection=ps).shape == (8, 8, 4)


# ---------------------------------------------------------------- the plan chain
def test_plan_chain(oracle):
    torch = pytest.importorskip("torch")
    from noaa_apt_amd.testing.synth import synth_apt
    dev = torch.device("cuda:0")
    k = 4
    recs = [synth_apt(48000, 30 + 4 * i, 700 + i) for i in range(k)]
    rows = [oracle.decode(r, 48000, True) for r in recs]
    heights = [r.size // 2080 for r in rows]
    tracks = [mm.great_circle_track(-30.0 + 5 * i, -60.0 + 3 * i, 10.0 + i, heights[i]) for i in range(k)]
    grids = [_grid(tracks[0], P.EQUIRECTANGULAR, 131, 77, 0.02, sampling=P.BILINEAR),
             _grid(tracks[1], P.MERCATOR, 64, 200, 0.01, grid_deg=0.5, grid_color=(0, 255, 0, 128)),
             _grid(tracks[2], P.MERCATOR, 1, 1, 0.02, channel=P.CHANNEL_B),
             _grid(tracks[3], P.EQUIRECTANGULAR, 200, 33, 0.015, channel=P.CHANNEL_B, sampling=P.BILINEAR)]
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        plan = apt.Plan(apt.Settings(), apt.Rate.hz(48000), True, max_samples=max(r.size for r in recs), max_batch=k,
                        stream=stream.cuda_stream)
        cap = int(plan.info.max_rows)
        d_in = [torch.from_numpy(r).to(dev) for r in recs]
        d_rows = [torch.empty(cap * 2080, dtype=torch.float32, device=dev) for _ in recs]
        d_img = [torch.zeros(cap * 2080, dtype=torch.uint8, device=dev) for _ in recs]
        d_out = [torch.full((g.width * g.height * 4,), 7, dtype=torch.uint8, device=dev) for g in grids]
        d_png = [torch.zeros(apt.png_bound(g.width, g.height, 4), dtype=torch.uint8, device=dev) for g in grids]
        ptr = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
        sizes = [t.numel() for t in d_out]
        plan.decode_device(ptr(d_in), [r.size for r in recs], ptr(d_rows), [cap] * k)
        plan.process_device_image(ptr(d_rows), [cap] * k, apt.Contrast.MINMAX, ptr(d_img), map=tracks,
                                  projection=(grids, ptr(d_out), sizes), png=(ptr(d_png), [t.numel() for t in d_png]))
        ires = plan.image_results(k)
        ones = []
        for i in range(k):
            assert ires[i].status == 0 and ires[i].height == heights[i], (i, ires[i].reason)
            one = apt.process(None, rows[i], apt.Contrast.MINMAX, orbit=tracks[i], projection=grids[i])
            ones.append(one)
            assert np.array_equal(d_out[i].cpu().numpy().reshape(one.shape), one), i
            assert np.array_equal(_decode_png(d_png[i][:ires[i].png_bytes].cpu().numpy().tobytes()), one), i
        assert ones[0][..., 3].any() and ones[1][..., 3].any()
        # a buffer that is too small and a count that differs are reported; the neighbours are unaffected
        for t in d_out:
            t.fill_(7)
        sizes[1] -= 4
        short = list(tracks)
        short[3] = tracks[3][:-1]
        plan.process_device_image(ptr(d_rows), [cap] * k, apt.Contrast.MINMAX, ptr(d_img), map=short,
                                  projection=(grids, ptr(d_out), sizes))
        ires = plan.image_results(k)
        assert (ires[1].status, ires[1].reason) == (1, apt.PROJECT_REASON_CAPACITY)
        assert (ires[3].status, ires[3].reason) == (1, 7)
        for i in (1, 3):
            assert bool((d_out[i] == 7).all()), i  # nothing written, never truncated
        for i in (0, 2):
            assert ires[i].status == 0 and np.array_equal(d_out[i].cpu().numpy().reshape(ones[i].shape), ones[i]), i
    plan.close()


# ---------------------------------------------------------------- soak
def test_soak_100_cases():
    rng = np.random.default_rng(2024)
    rows = 200  # (grids stay clear of the track's first point: its NEAR_START pixels would spend the allowance)
    sigs = [_signal(rows, 100 + s) for s in range(3)]
    pres = [apt.process(None, s, apt.Contrast.MINMAX) for s in sigs]
    left = valid = 0
    for case in range(100):
        pos = mm.great_circle_track(rng.uniform(-60, 60), rng.uniform(-180, 180), rng.uniform(0, 360), rows)
        big = case % 50 == 0
        w, h = (int(rng.integers(100, 201)), int(rng.integers(100, 201))) if big else \
            (int(rng.integers(1, 32)), int(rng.integers(1, 32)))
        ms = apt.MapSettings(yaw=rng.uniform(-0.1, 0.1), hscale=rng.uniform(0.6, 1.6), vscale=rng.uniform(0.6, 1.6))
        ps = _grid(pos, int(rng.integers(0, 2)), w, h, rng.uniform(0.01, 0.025 if big else 0.1), at=rng.uniform(0.65, 0.9),
                   channel=int(rng.integers(0, 2)), sampling=int(rng.integers(0, 2)),
                   grid_deg=float(rng.choice([0.0, 0.5, 2.0])), grid_color=tuple(int(v) for v in rng.integers(0, 256, 4)),
                   geometry=ms)
        s = case % 3
        got = apt.process(None, sigs[s], apt.Contrast.MINMAX, orbit=pos, projection=ps)
        want, margin, info = _model(pres[s], pos, ps, ms)
        bad, low = pm.compare(got, want, margin)
        assert bad == 0, (case, bad)
        left += info["excused"]
        valid += info["n_valid"]
    print(f"soak: {valid} valid pixels in 100 cases, {left} left out (margin < {pm.TAU})")
    assert valid > 5000 and left <= 16 and left <= 0.001 * valid
