"""CPU-side checks of the reprojection: the settings' refusals (all raised before the device is
touched), aptgpu_projection_fit against its Python restatement, hand cases of tests/np_project_model.py and the ABI."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import noaa_apt_amd as apt
import np_map_model as mm
import np_project_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _settings(**kw):
    f = dict(kind=apt.Projection.EQUIRECTANGULAR, width=8, height=8, lat_north=10.0, lon_west=-60.0, step=0.5)
    f.update(kw)
    return apt.ProjectionSettings(**f)


def _refused(ps, settings=None):
    img = np.zeros((4, 2080), np.uint8)
    pos = mm.great_circle_track(0.0, -58.0, 10.0, 4)
    with pytest.raises(apt.InvalidError) as e:
        apt.project_image(img, pos, ps, settings=settings)
    return str(e.value)


@pytest.mark.parametrize("kw, text", [
    (dict(width=0), "width and height must be at least 1"),
    (dict(height=0), "width and height must be at least 1"),
    (dict(width=8193, height=8192), "width * height exceeds APTGPU_PROJECTION_MAX_PIXELS (2^26)"),
    (dict(step=0.0), "step must be finite and > 0"),
    (dict(step=-1.0), "step must be finite and > 0"),
    (dict(step=math.inf), "step must be finite and > 0"),
    (dict(step=math.nan), "step must be finite and > 0"),
    (dict(lat_north=90.5), "lat_north must be within [-90, 90]"),
    (dict(lat_north=-91.0), "lat_north must be within [-90, 90]"),
    (dict(lat_north=math.nan), "lat_north must be within [-90, 90]"),
    (dict(lat_north=-80.0, height=30), "the last row's latitude must be within [-90, 90]"),
    (dict(lon_west=math.inf), "lon_west must be finite"),
    (dict(kind=2), "unknown kind"),
    (dict(kind=-1), "unknown kind"),
    (dict(channel=2), "unknown channel"),
    (dict(sampling=7), "unknown sampling"),
    (dict(grid_deg=-1.0), "grid_deg must be finite and >= 0"),
    (dict(grid_deg=0.1), "grid_deg must be 0 or at least step"),
])
def test_settings_refusals(kw, text):
    msg = _refused(_settings(**kw))
    assert msg == "aptgpu_projection_settings: " + text


def test_mercator_has_no_last_row_rule():
    # a Mercator grid's rows never reach the pole: only lat_north is bounded; the largest grid is accepted as far as
    # the checks go (the refusal below is the next check, raised for the image)
    ps = _settings(kind=apt.Projection.MERCATOR, lat_north=-80.0, height=30, width=8192 * 8192 // 30)
    with pytest.raises(apt.InvalidError, match="no row to read"):
        apt.project_image(np.zeros((0, 2080), np.uint8), np.zeros((0, 2)), ps)


def test_struct_size_zero_and_other_refusals():
    L = apt.lib()
    c = _settings()._c()
    c.struct_size = 0
    out, n = C.POINTER(C.c_uint8)(), C.c_size_t()
    err = C.create_string_buffer(512)
    img = np.zeros((4, 2080), np.uint8)
    pos = np.ascontiguousarray(mm.great_circle_track(0.0, -58.0, 10.0, 4))
    args = (None, img.ctypes.data_as(C.POINTER(C.c_uint8)), 4, 1, pos.ctypes.data_as(C.POINTER(C.c_double)), 4, None)
    rc = L.aptgpu_project_image(*args, C.byref(c), 0, None, C.byref(out), C.byref(n), err, 512)
    assert rc == apt.InvalidError.code and err.value == b"aptgpu_projection_settings: struct_size not set"
    rc = L.aptgpu_project_image(*args, None, 0, None, C.byref(out), C.byref(n), err, 512)
    assert rc == apt.InvalidError.code and err.value == b"aptgpu_projection_settings: struct_size not set"
    c = _settings()._c()
    rc = L.aptgpu_project_image(*args, C.byref(c), 2, None, C.byref(out), C.byref(n), err, 512)
    assert rc == apt.InvalidError.code and err.value == b"unknown output kind"
    c.reserved = 1
    rc = L.aptgpu_project_image(*args, C.byref(c), 0, None, C.byref(out), C.byref(n), err, 512)
    assert rc == apt.InvalidError.code and err.value == b"aptgpu_projection_settings: reserved must be 0"
    ms = apt.api._CMapSettings(0, 0, 0.0, 1.0, 1.0)
    c.reserved = 0
    bad = args[:6] + (C.byref(ms),)
    rc = L.aptgpu_project_image(*bad, C.byref(c), 0, None, C.byref(out), C.byref(n), err, 512)
    assert rc == apt.InvalidError.code and err.value == b"aptgpu_map_settings: struct_size not set"


def test_process_refusals_before_the_device():
    sig = np.zeros(4 * 2080, np.float32)
    pos = mm.great_circle_track(0.0, -58.0, 10.0, 4)
    for rot in (apt.Rotate.YES, apt.Rotate.ORBIT):
        with pytest.raises(apt.InvalidError, match="rotate = APTGPU_ROTATE_NO only"):
            apt.process(None, sig, apt.Contrast.MINMAX, rotate=rot, orbit=pos, projection=_settings())
    with pytest.raises(apt.InvalidError, match="unknown kind"):
        apt.process(None, sig, apt.Contrast.MINMAX, orbit=pos, projection=_settings(kind=5))
    with pytest.raises(apt.InvalidError, match="needs the track"):
        apt.process(None, sig, apt.Contrast.MINMAX, projection=_settings())
    with pytest.raises(apt.InvalidError, match="3 positions for 4 rows"):
        apt.process(None, sig, apt.Contrast.MINMAX, orbit=pos[:3], projection=_settings())


TRACKS = {
    "northbound": mm.great_circle_track(-30.0, -60.0, 10.0, 900),
    "southbound": mm.great_circle_track(40.0, 20.0, 192.0, 900),
    "antimeridian": mm.great_circle_track(10.0, 178.5, 60.0, 900),
    "polar81": mm.great_circle_track(60.0, 10.0, 9.0, 1500),
}


@pytest.mark.parametrize("name", sorted(TRACKS))
@pytest.mark.parametrize("kind", [pm.EQUIRECTANGULAR, pm.MERCATOR])
@pytest.mark.parametrize("how", [dict(step=0.05), dict(max_width=300), dict(step=0.11, hscale=1.7)])
def test_projection_fit(name, kind, how):
    pos = TRACKS[name]
    got = apt.projection_fit(pos, kind, **how)
    want = pm.fit(pos, kind, **how)
    assert (got.kind, got.width, got.height) == (want["kind"], want["width"], want["height"])
    assert (got.lat_north, got.lon_west, got.step) == (want["lat_north"], want["lon_west"], want["step"])
    assert (got.channel, got.sampling, got.grid_deg) == (0, 0, 0.0)
    if "max_width" in how:
        assert got.width == how["max_width"]
    # it covers the track: every position lies inside the grid, at least the swath's half angle from its edges
    half = math.degrees(456 * 0.0005 / how.get("hscale", 1.0))
    lat = np.degrees(pos[:, 0])
    lon = np.degrees(np.unwrap(pos[:, 1]))
    lon += 360.0 * round((got.lon_west + 0.5 * got.width * got.step - lon.mean()) / 360.0)
    cap = 85.0 if kind == pm.MERCATOR else 90.0
    assert got.lat_north >= min(lat.max() + half, cap) - 1e-9
    south = math.degrees(pm.row_lat(kind, got.lat_north, got.step, float(got.height - 1)))
    assert south <= max(lat.min() - half, -cap) + got.step
    assert got.lon_west <= lon.min() - half + 1e-9 and got.lon_west + (got.width - 1) * got.step >= lon.max() + half - got.step
    if name == "antimeridian":
        assert got.lon_west + (got.width - 1) * got.step > 180.0
    if name == "polar81":
        assert lat.max() > 81.0 - 1.0 and got.lat_north == (85.0 if kind == pm.MERCATOR else min(lat.max() + half, 90.0))
    # and the settings it returns pass the checks (the refusal is the image's)
    with pytest.raises(apt.InvalidError, match="no row to read"):
        apt.project_image(np.zeros((0, 2080), np.uint8), np.zeros((0, 2)), got)


def test_projection_fit_refusals():
    pos = TRACKS["northbound"]
    for kw, text in ((dict(), "give a step > 0 or a maximum width of at least 2"),
                     (dict(max_width=1), "give a step > 0 or a maximum width of at least 2"),
                     (dict(step=0.05, hscale=0.0), "hscale must be finite and > 0"),
                     (dict(step=1e-4), "the fitted grid exceeds APTGPU_PROJECTION_MAX_PIXELS (2^26)")):
        with pytest.raises(apt.InvalidError) as e:
            apt.projection_fit(pos, pm.EQUIRECTANGULAR, **kw)
        assert str(e.value) == "aptgpu_projection_fit: " + text
    with pytest.raises(apt.InvalidError, match="unknown kind"):
        apt.projection_fit(pos, 3, step=0.1)
    with pytest.raises(apt.InvalidError, match="the track is empty"):
        apt.projection_fit(np.zeros((0, 2)), 0, step=0.1)


def test_model_track_position_samples_the_centre_column():
    # the output pixel at the track's row-r position samples x ~ 0, y ~ r
    rows = 300
    pos = mm.great_circle_track(-20.0, -65.0, 12.0, rows)
    sc = mm.Scalars(pos)
    xoff = [mm.rel_px(sc, (float(a), float(b)))[0] for a, b in pos]
    for r in (1, 37, 150, 298):
        x, y, valid, _, _ = pm.locate(sc, xoff, rows, float(pos[r, 0]), float(pos[r, 1]))
        assert valid and abs(x) < 1e-6 and abs(y - r * rows / (rows - 1)) < 1e-6 and abs(y - r) <= 1.0, (r, x, y)


def test_model_pi_3_rule():
    # 100 rows whose arc exceeds PI / 3: a point 70 degrees down-track would alias onto the row of 60 degrees
    rows = 100
    pos = mm.great_circle_track(-40.0, -60.0, 0.0, rows, seconds_per_row=12.0)
    sc = mm.Scalars(pos, vscale=0.5)
    assert mm.distance(sc.start, sc.end) > mm.PI / 3
    xoff = [mm.rel_px(sc, (float(a), float(b)))[0] for a, b in pos]
    lat70, lon = math.radians(-40.0 + 70.0), math.radians(-60.0)
    x, y, valid, margin, d = pm.locate(sc, xoff, rows, lat70, lon)
    assert abs(d - math.radians(70.0)) < 1e-9 and not valid and margin > 0.1
    # it is the PI / 3 rule alone that refuses it: the clamped projection lands inside the band
    assert -456.0 < x < 456.0 and 0.0 < y < rows
    x, y, valid, _, _ = pm.locate(sc, xoff, rows, math.radians(-40.0 + 50.0), lon)
    assert valid


def test_model_mercator_rows_round_trip():
    for lat_north, step in ((60.0, 0.04), (-10.0, 0.25), (85.0, 0.01)):
        y0 = pm.y_north(lat_north)
        for i in (0, 1, 77, 1000):
            lat = pm.row_lat(pm.MERCATOR, lat_north, step, float(i))
            assert abs(math.asinh(math.tan(lat)) - (y0 - i * pm.rad(step))) < 1e-12
        assert abs(pm.row_lat(pm.MERCATOR, lat_north, step, 0.0) - pm.rad(lat_north)) < 1e-15


def test_model_graticule_rows_and_columns():
    cols, rows = pm.graticule(pm.EQUIRECTANGULAR, 101, 61, 30.0, -70.0, 0.1, 5.0)
    assert list(np.nonzero(cols)[0]) == [0, 50, 100] and list(np.nonzero(rows)[0]) == [0, 50]
    cols, rows = pm.graticule(pm.MERCATOR, 20, 300, 60.0, 1.0, 0.1, 10.0)
    assert not cols.any()
    r50 = (pm.y_north(60.0) - pm.y_north(50.0)) / pm.rad(0.1)
    assert list(np.nonzero(rows)[0]) == [0, int(math.floor(r50 + 0.5))]


def test_abi():
    L = apt.lib()
    hdr = open(os.path.join(ROOT, "include", "aptgpu.h")).read()
    for name in ("aptgpu_projection_fit", "aptgpu_project_image", "aptgpu_process_image_project",
                 "aptgpu_plan_process_device_image_project"):
        assert name + "(" in hdr and hasattr(L, name)
    assert re.search(r"#define APTGPU_ABI_VERSION 2\b", hdr) and apt.abi_version() == 2
    S = apt.api._CProjectionSettings
    assert C.sizeof(S) == 64 and S.struct_size.offset == 0
    assert (S.kind.offset, S.width.offset, S.height.offset, S.lat_north.offset, S.lon_west.offset, S.step.offset,
            S.channel.offset, S.sampling.offset, S.grid_deg.offset, S.grid_color.offset, S.reserved.offset) == \
        (4, 8, 12, 16, 24, 32, 40, 44, 48, 56, 60)
    # the library fills the struct it was compiled with: its struct_size is the mirror's
    out = S()
    pos = np.ascontiguousarray(TRACKS["northbound"])
    assert L.aptgpu_projection_fit(pos.ctypes.data_as(C.POINTER(C.c_double)), len(pos), 1.0, 0, 0.1, 0, C.byref(out),
                                   None, 0) == 0
    assert out.struct_size == C.sizeof(S)
    assert apt.PROJECT_REASON_CAPACITY == 11 and "#define APTGPU_PROJECT_REASON_CAPACITY 11" in hdr
    assert C.sizeof(apt.ImageResult) == 176
    for name in ("Projection", "ProjectionSettings", "projection_fit", "project_image"):
        assert hasattr(apt, name)
