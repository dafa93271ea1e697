"""The geolocation stage without a GPU: the plain C++ twin (aptgpu_geolocate_host) against the numpy model
(np_geoloc_model.py) with the bounds geoloc_cases.py states, the sun series against almanac values, the refusals of
every entry point before a device is touched, the record's reasons and the ABI."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import geoloc_cases as gc
import np_geoloc_model as gm

import noaa_apt_amd as apt
from test_sat_cpu import TLE_2020, orbit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAMES = ("h2", "h5", "h263", "h530_rotating", "pole", "antimeridian", "far")


def host(name, x=None, latlon=True, sun=True, rows=False, **kw):
    track = gc.case(name)[0]
    sig = x if x is not None else track.shape[0]
    return apt.geolocate_host(sig, track, gc.map_settings_of(name), gc.settings_of(name, **kw), latlon=latlon, sun=sun,
                              rows=rows)


@pytest.mark.parametrize("name", NAMES)
def test_twin_equals_model(name):
    h = gc.case(name)[0].shape[0]
    x = gc.rows_of(h, seed=h)
    latlon, cos_sun, rows, info = host(name, x, rows=True, channel="B", black=33.5)
    gc.check_planes(name, latlon, cos_sun, info)
    gc.check_rows(x, rows, cos_sun, 1, 33.5, 80.0, info, note=name)


def test_cases_cover_what_they_are_for():
    fw = gc.model("h530_rotating")[0]
    assert np.abs(fw.xoff).max() > 0.5  # the x offsets matter (1.95 px here)
    assert np.degrees(gc.model("pole")[1][..., 0][gc.model("pole")[0].valid].max()) > 87.0
    lon = gc.model("antimeridian")[1][..., 1]
    assert np.nanmax(lon) > 3.1 and np.nanmin(lon) < -3.1
    far = gc.model("far")[0]
    assert far.valid[0].all() and (~far.valid).sum() > 10000 and int(far.edge.sum()) == 0
    assert far.sc.y_res * far.h > math.pi / 3  # the track itself runs past the limit


def test_far_limit_is_nan_everywhere_and_counted():
    h = 2100
    x = gc.rows_of(h, seed=1)
    latlon, cos_sun, rows, info = host("far", x, rows=True)
    out = np.isnan(cos_sun)
    assert info.n_outside == int(out.sum()) > 10000
    assert np.isnan(latlon[out]).all() and not np.isnan(latlon[~out]).any()
    video = rows[:h * 2080].reshape(h, 2080)[:, 86:995]
    assert video[out].tobytes() == x[:h * 2080].reshape(h, 2080)[:, 86:995][out].tobytes()


def test_orbit_form_equals_positions_form():
    # NOAA 19 northbound over South America: SGP4's track bends against a great circle, max |xoff| = 0.58 px
    ms, h = 1580246771392, 300
    o = orbit(TLE_2020, "NOAA 19", "start", ms)
    track = apt.sat_track_host(o, h)
    name = gc.define("noaa19", track, (0.0, 1.0, 1.0), ms)
    assert np.abs(gc.model(name)[0].xoff).max() > 0.5
    a = apt.geolocate_host(h, o, None, apt.GeolocSettings(), latlon=True, sun=True)
    b = apt.geolocate_host(h, track, None, apt.GeolocSettings(ref_time=apt.RefTime.Start(ms)), latlon=True, sun=True)
    gc.check_planes(name, *a)
    # (on the CPU both forms run the same library: equal bits)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and gc.record(a[2]) == gc.record(b[2])
    # RefTime::End names the same image
    e = apt.geolocate_host(h, orbit(TLE_2020, "NOAA 19", "end", ms + 500 * h), None, apt.GeolocSettings(), sun=True)
    assert e[0].tobytes() == a[0].tobytes() and e[1].tobytes() == a[1].tobytes()


@pytest.mark.parametrize("ms,delta_deg,lon_deg", [(946728000000, -23.0334, 0.8252), (1730635200000, -15.2987, -4.1111),
                                                  (1710903960000, 0.0015, None)])
def test_sun_anchors(ms, delta_deg, lon_deg):
    delta, lon = apt.sun_position(ms)
    assert abs(math.degrees(delta) - delta_deg) <= 1e-3
    if lon_deg is not None:
        assert abs(math.degrees(lon) - lon_deg) <= 1e-3
    md, ml = gm.sun_position(ms)
    assert abs(delta - md) <= 1e-12 and abs(lon - ml) <= 1e-9 and -math.pi < lon <= math.pi


def test_pixel_at_the_sub_solar_point():
    t = gc.T_NOON_2024
    delta, lon = apt.sun_position(t)
    from np_map_model import great_circle_track
    track = great_circle_track(math.degrees(delta), math.degrees(lon), 190.0, 5)
    _, cos_sun, info = apt.geolocate_host(5, track, None, apt.GeolocSettings(ref_time=apt.RefTime.Start(t)), latlon=False,
                                          sun=True)
    assert abs(float(cos_sun[0, gm.CENTRE]) - 1.0) <= 1e-7  # row 0's centre is the track's first point
    assert info.n_capped == 0 and info.cos_max == cos_sun.max()


def test_start_and_end_name_the_same_image():
    x = gc.rows_of(263, seed=2)
    a = host("h263", x, rows=True, kind="start")
    b = host("h263", x, rows=True, kind="end")
    assert all(p.tobytes() == q.tobytes() for p, q in zip(a[:3], b[:3])) and gc.record(a[3]) == gc.record(b[3])


def test_night_pass_is_capped():
    h = 263
    x = gc.rows_of(h, seed=3)
    track, _, t = gc.case("h263")
    st = apt.GeolocSettings(channel="A", ref_time=apt.RefTime.Start(t + 12 * 3600000), black=30.0, max_zenith_deg=75.0)
    _, cos_sun, rows, info = apt.geolocate_host(x, track, gc.map_settings_of("h263"), st, latlon=False, sun=True, rows=True)
    assert cos_sun.max() < 0 and info.n_outside == 0 and info.n_capped == h * 909
    cmin = gm.cmin_of(75.0)
    v = x[:h * 2080].reshape(h, 2080)[:, 86:995]
    want = (f32(30.0) + (v - f32(30.0)) / cmin).astype(f32)
    assert rows[:h * 2080].reshape(h, 2080)[:, 86:995].tobytes() == want.tobytes()
    gc.check_rows(x, rows, cos_sun, 0, 30.0, 75.0, info)


def test_non_finite_video():
    h = 5
    x = gc.rows_of(h, seed=4)
    x[86], x[2080 + 994], x[2 * 2080 + 500], x[3 * 2080 + 85], x[4 * 2080 + 1040 + 86] = np.nan, np.inf, -np.inf, np.nan, np.nan
    _, cos_sun, rows, info = host("h5", x, latlon=False, rows=True, black=25.0)
    gc.check_rows(x, rows, cos_sun, 0, 25.0, 80.0, info)
    assert np.isnan(rows[86]) and rows[2080 + 994] == np.inf and rows[2 * 2080 + 500] == -np.inf


def test_output_masks():
    x = gc.rows_of(263, seed=5)
    full = host("h263", x, rows=True)
    only = host("h263", x, latlon=False, sun=False, rows=True)
    assert only[0] is None and only[1] is None and only[2].tobytes() == full[2].tobytes()
    assert gc.record(only[3]) == gc.record(full[3])
    ll = host("h263", latlon=True, sun=False)
    assert ll[1] is None and ll[0].tobytes() == full[0].tobytes() and gc.record(ll[2]) == gc.record(full[3])
    again = host("h263", x, rows=True)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(full[:3], again[:3]))


def test_record_reasons():
    track = gc.case("h5")[0]
    with pytest.raises(apt.InternalError, match="fewer than two rows") as e:
        apt.geolocate_host(1, track[:1])
    assert (e.value.info.status, e.value.info.reason, e.value.info.height) == (1, apt.GEOLOC_REASON_HEIGHT, 1)
    with pytest.raises(apt.InternalError, match="differs from the image height") as e:
        apt.geolocate_host(5, track[:4])
    assert (e.value.info.status, e.value.info.reason, e.value.info.height) == (1, 7, 5)
    with pytest.raises(apt.InternalError) as e:
        apt.geolocate_host(0, track[:0].reshape(0, 2))
    assert e.value.info.reason == apt.GEOLOC_REASON_HEIGHT


# ---- refusals: every one before a device is touched, so they read the same on a machine without a GPU

def _raw(fn, head, n, pos, count, orb, cms, cs, want_rows=False, signal=None):
    err = C.create_string_buffer(512)
    ll, cosp, rows = apt.api._f64p(), apt.api._f32p(), apt.api._f32p()
    info = apt.GeolocResult()
    info.struct_size = C.sizeof(apt.GeolocResult)
    rc = fn(*head, signal, n, pos, count, orb, cms, C.byref(cs) if cs is not None else None, C.byref(ll), C.byref(cosp),
            C.byref(rows) if want_rows else None, C.byref(info), err, 512)
    assert not ll and not cosp and not rows
    return rc, err.value.decode()


def _forms():
    L = apt.lib()
    cctx = apt.Context()._c()
    return (("gpu", L.aptgpu_geolocate, (C.byref(cctx),)), ("host", L.aptgpu_geolocate_host, ()))


@pytest.mark.parametrize("form", [0, 1])
def test_refusals(form):
    _, fn, head = _forms()[form]
    track = np.ascontiguousarray(gc.case("h5")[0])
    pos = track.ctypes.data_as(apt.api._f64p)
    n = 5 * 2080
    good = apt.GeolocSettings()
    INVALID = apt.InvalidError.code

    def refused(cs, match, pos=pos, count=5, orb=None, cms=None, **kw):
        rc, msg = _raw(fn, head, n, pos, count, orb, cms, cs, **kw)
        assert rc == INVALID and match in msg, (rc, msg)

    refused(good._c(struct_size=8), "struct_size")
    refused(None, "settings are required")
    refused(apt.GeolocSettings(flags=2)._c(), "flag")
    refused(apt.GeolocSettings(channel=2)._c(), "channel")
    for z in (0.0, 90.0, -5.0, 120.0, float("nan")):
        refused(apt.GeolocSettings(max_zenith_deg=z)._c(), "max_zenith_deg")
    for b in (float("nan"), float("inf")):
        refused(apt.GeolocSettings(black=b)._c(), "black_level")
    cs = good._c()
    cs.time_kind = 2
    refused(cs, "time_kind")
    co, keep = orbit(TLE_2020, "NOAA 19", "start", 1580246771392)._c()
    refused(good._c(), "exactly one", orb=C.byref(co))          # both
    refused(good._c(), "exactly one", pos=None, count=0)        # neither
    refused(good._c(), "need the signal", want_rows=True)       # rows without a signal
    cms = apt.MapSettings()._c()
    cms.struct_size = 4
    refused(good._c(), "aptgpu_map_settings", cms=C.byref(cms))
    del keep


def test_plan_form_refuses_bad_buffers_before_it_looks_at_the_plan():
    L = apt.lib()
    track = np.ascontiguousarray(gc.case("h5")[0])
    cs = apt.GeolocSettings()._c()
    rows_base = 1 << 20
    rows_bytes = 5 * 2080 * 4

    def call(d_latlon=None, d_cos=None, d_out=None, positions=True):
        err = C.create_string_buffer(512)
        pos = (apt.api._f64p * 1)(track.ctypes.data_as(apt.api._f64p)) if positions else None
        cnt = (C.c_size_t * 1)(5) if positions else None

        def arr(v):
            return (C.c_void_p * 1)(v) if v is not None else None
        rc = L.aptgpu_plan_geolocate_device(None, 1, (C.c_void_p * 1)(rows_base), (C.c_size_t * 1)(5), pos, cnt, None, None,
                                            C.byref(cs), arr(d_latlon), arr(d_cos), arr(d_out), err, 512)
        return rc, err.value.decode()

    far = rows_base + (1 << 24)
    INVALID = apt.InvalidError.code
    rc, msg = call(d_latlon=far + 8)
    assert rc == INVALID and "16-byte" in msg
    rc, msg = call(d_cos=far + 2)
    assert rc == INVALID and "4-byte" in msg
    rc, msg = call(d_out=far + 1)
    assert rc == INVALID and "4-byte" in msg
    rc, msg = call(d_out=rows_base + 2080 * 4)  # partly overlapping the rows
    assert rc == INVALID and "overlaps" in msg
    rc, msg = call(d_cos=rows_base + rows_bytes - 4)
    assert rc == INVALID and "overlaps" in msg
    rc, msg = call(d_latlon=far, d_cos=far + 16)
    assert rc == INVALID and "overlaps" in msg
    rc, msg = call(d_latlon=far, positions=False)
    assert rc == INVALID and "exactly one" in msg
    rc, msg = call(d_out=rows_base)  # in place is allowed: the next refusal is the missing plan
    assert rc == INVALID and "no plan" in msg
    assert L.aptgpu_plan_geoloc_results(None, 1, None) == INVALID


def test_abi():
    hdr = open(os.path.join(ROOT, "include", "aptgpu.h")).read()
    raw = C.CDLL(apt.lib_path())
    for name in ("aptgpu_geolocate", "aptgpu_geolocate_host", "aptgpu_sun_position", "aptgpu_plan_geolocate_device",
                 "aptgpu_plan_geoloc_results"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and hasattr(raw, name), name
    assert C.sizeof(apt.api._CGeolocSettings) == 32 and C.sizeof(apt.GeolocResult) == 40
    assert apt.GeolocResult.n_outside.offset == 16 and apt.GeolocResult.cos_min.offset == 32
    assert apt.abi_version() == 2
    for name, value in (("APTGPU_GEOLOC_PX", apt.GEOLOC_PX), ("APTGPU_GEOLOC_REASON_HEIGHT", apt.GEOLOC_REASON_HEIGHT),
                        ("APTGPU_GEOLOC_REASON_DECODE", apt.GEOLOC_REASON_DECODE)):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == value
    # a caller built against a shorter record gets its own size back and nothing beyond it
    info = apt.GeolocResult()
    info.struct_size = 16
    info.n_outside = 77
    track = np.ascontiguousarray(gc.case("h2")[0])
    cs = apt.GeolocSettings()._c()
    err = C.create_string_buffer(512)
    rc = apt.lib().aptgpu_geolocate_host(None, 2 * 2080, track.ctypes.data_as(apt.api._f64p), 2, None, None, C.byref(cs),
                                         None, None, None, C.byref(info), err, 512)
    assert rc == 0 and (info.struct_size, info.height, info.n_outside) == (16, 2, 77)
