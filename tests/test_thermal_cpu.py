"""The thermal calibration stage without a GPU: the host twin (aptgpu_calibrate_thermal_host) against the numpy model
(np_thermal_model.py), two closed-form anchors that depend on neither, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import np_thermal_model as tm
import thermal_cases as tc

import noaa_apt_amd as apt
from noaa_apt_amd import api

f32 = np.float32
host = apt.calibrate_thermal_host


@pytest.mark.parametrize("channel", [0, 1])
@pytest.mark.parametrize("identity", ["4", "5", "3b"])
def test_host_equals_model(channel, identity):
    x = tm.scene(200, 0, seed=3 + channel, space_noise=0.8)
    tc.check(host, x, channel, identity, image_channels=4, pal=tc.palette(), note=("host", channel, identity))


def test_host_frame_row_identity_from_telemetry_and_images():
    x = tm.scene(263, 37, seed=5, identities=(5, 3), space_noise=0.8)
    _, _, info, _ = tc.check(host, x, 0, None, image_channels=1, cold_white=False, note="A auto")
    assert (info.telemetry_row, info.channel_id) == (37, 5)
    _, _, info, _ = tc.check(host, x, 1, None, image_channels=4, note="B auto")
    assert (info.telemetry_row, info.channel_id) == (37, 3)
    tc.check(host, x, 1, None, image_channels=0, note="no image")


def test_host_failures():
    with pytest.raises(apt.InternalError, match="too short") as e:
        host(tm.scene(199, 0, seed=1), tc.coeffs(), apt.ThermalSettings("A", "4", t_low=180, t_high=320))
    assert (e.value.info.status, e.value.info.reason, e.value.info.height) == (1, 2, 199)
    # a visible channel: reason 13 from the telemetry's identity, fine when the caller forces one
    x = tm.scene(200, 0, seed=2, identities=(1, 3))
    info = tc.check(host, x, 0, None, note="identity 2")
    assert (info.reason, info.channel_id) == (13, 1)
    tc.check(host, x, 0, "4", note="identity 2 forced to 4")
    info = tc.check(host, x, 0, 2, note="forced 3a")
    assert info.reason == 13
    # a flat count scale (sxx == 0), and space == back scan (c_space == c_bb): reason 14
    y = x.reshape(200, 2080).copy()
    y[:, 994:1040] = y[0, 995]  # (the telemetry band is columns 994 .. 1037 of a channel, as the reference reads it)
    y[:, 2034:2080] = y[0, 995]
    info = tc.check(host, y.ravel(), 0, "4", note="flat wedges")
    assert info.reason == 14
    y = _anchor_scene(f32(6000.0)).reshape(200, 2080).copy()
    y[:, 39:86] = f32(4950.0)  # the space view equal to wedge 15, both exact
    info = tc.check(host, y.ravel(), 0, "4", note="space == back scan")
    assert info.reason == 14 and info.c_space == info.c_bb


def test_host_non_finite_samples():
    x = tm.scene(200, 0, seed=8, space_noise=0.0)
    _, _, clean, _ = tc.check(host, x, 1, "5", note="clean")
    y = x.reshape(200, 2080).copy()
    y[5, 1040 + 100], y[6, 1040 + 101], y[7, 1040 + 993], y[199, 1040 + 86] = np.nan, np.inf, -np.inf, np.nan
    kelvin, _, info, _ = tc.check(host, y.ravel(), 1, "5", image_channels=4, note="video")
    assert np.isnan(kelvin[5, 14]) and np.isnan(kelvin[6, 15]) and np.isnan(kelvin[7, 907]) and np.isnan(kelvin[199, 0])
    y = x.reshape(200, 2080).copy()
    y[3, 1040 + 50], y[90, 1040 + 60], y[91, 1040 + 44] = np.nan, np.inf, -np.inf
    _, _, info, _ = tc.check(host, y.ravel(), 1, "5", note="space band")
    assert tc.bits64(info.space) == tc.bits64(clean.space)
    y = x.reshape(200, 2080).copy()
    y[83, 1040 + 1000] = np.nan  # wedge 11, a PRT
    info = tc.check(host, y.ravel(), 1, "5", note="wedge")
    assert info.reason == 14


def test_minute_markers_leave_space_alone():
    x = tm.scene(263, 37, seed=4)
    y = tm.scene(263, 37, seed=4, markers=(20, 21, 80, 81))
    assert not np.array_equal(x, y)
    _, _, a, _ = tc.check(host, x, 1, "4", note="no markers")
    _, _, b, _ = tc.check(host, y, 1, "4", note="markers")
    assert tc.bits64(a.space) == tc.bits64(b.space) and tc.bits64(a.c_space) == tc.bits64(b.c_space)


def _anchor_scene(value):
    """noise-free rows (a frame at row 0 of 200: no search); pixel (0, 0) of channel A's video holds `value`"""
    g, o = 37.5, 1200.0
    y = np.full((200, 2080), f32(g * 128.0 + o), f32)
    y[:, 39:86] = f32(g * 248.0 + o)
    y[:, 1079:1126] = f32(g * 248.0 + o)
    wedges = np.array(list(tm.WEDGE_COUNTS) + [104.0, 105.0, 106.0, 105.5, 120.0, 100.0, 127.0])
    w = (g * wedges[(np.arange(200) // 8) % 16] + o).astype(f32)
    y[:, 994:1040] = w[:, None]  # (the telemetry band is columns 994 .. 1037 of a channel, as the reference reads it)
    y[:, 2034:2080] = w[:, None]
    y[0, 86] = value
    return y.ravel()


@pytest.mark.parametrize("name", ["4", "3b"])
def test_closed_form_anchors(name):
    """With b0 = b1 = b2 = 0 the radiance is linear in the count between two known points, whatever the count scale is:
    a sample equal to wedge 15 has C_e = c_bb, so N_e = n_bb and the inverse Planck function gives (t_bb* - A) / B = t_bb;
    a sample equal to the space view has C_e = c_space, so N_e = N_s (taken positive here so that it has a temperature).
    Neither statement uses the model or the slope.  The sums of equal values are exact here: wedge 15 is 4950 and the
    space view 10500 exactly."""
    ch = {"4": (928.0, 0.55, 0.99850, 2.0, 0.0, 0.0, 0.0), "3b": (2670.0, 1.70, 0.99750, 0.002, 0.0, 0.0, 0.0)}[name]
    co = apt.ThermalCoefficients(tm.PRT, ch, ch, ch)
    st = apt.ThermalSettings("A", name, t_low=180, t_high=320)
    kelvin, _, info = host(_anchor_scene(f32(4950.0)), co, st)
    assert info.space == 10500.0 and 290.0 < info.t_bb < 310.0
    # f32: a handful of roundings of values near 300 K and of a logarithm near 5 .. 13, each 2^-24 relative
    assert abs(float(kelvin[0, 0]) - info.t_bb) <= 1e-3, (kelvin[0, 0], info.t_bb)
    kelvin, _, info = host(_anchor_scene(f32(10500.0)), co, st)
    want = (tm.C2 * ch[0] / np.log(1.0 + tm.C1 * ch[0] ** 3 / ch[3]) - ch[1]) / ch[2]
    assert abs(float(kelvin[0, 0]) - want) <= 1e-3, (kelvin[0, 0], want)
    assert abs(tm.radiance_of_kelvin(float(kelvin[0, 0]), ch) - ch[3]) <= 1e-5 * info.n_bb


def _c_call(coeffs, settings, x=None, kelvin=True, image=False):
    x = tm.scene(200, 0, seed=1) if x is None else x
    k, img, info = api._f32p(), api._u8p(), apt.ThermalResult()
    err = C.create_string_buffer(512)
    rc = apt.lib().aptgpu_calibrate_thermal_host(x.ctypes.data_as(api._f32p), x.size, coeffs, settings,
                                                 C.byref(k) if kelvin else None, C.byref(img) if image else None,
                                                 C.byref(info), err, 512)
    for p in (k, img):
        if p:
            apt.lib().aptgpu_free(C.cast(p, C.c_void_p))
    return rc, err.value.decode()


def test_refusals():
    ok = apt.ThermalSettings("A", "4", t_low=180, t_high=320)
    cs, _ = ok._c()
    cc = tc.coeffs()._c()
    assert _c_call(C.byref(cc), C.byref(cs))[0] == 0
    assert _c_call(None, C.byref(cs))[0] == 4 and _c_call(C.byref(cc), None)[0] == 4
    assert _c_call(C.byref(cc), C.byref(cs), kelvin=False)[0] == 4
    assert _c_call(C.byref(tc.coeffs()._c(struct_size=8)), C.byref(cs))[0] == 4
    assert _c_call(C.byref(cc), C.byref(ok._c(struct_size=12)[0]))[0] == 4
    for bad in (dict(t_low=300, t_high=300), dict(t_low=320, t_high=180), dict(t_low=float("nan"), t_high=320),
                dict(t_low=180, t_high=float("inf")), dict(t_low=180, t_high=320, flags=2),
                dict(t_low=180, t_high=320, flags=1 << 31), dict(t_low=180, t_high=320, image_channels=3),
                dict(t_low=180, t_high=320, image_channels=1, palette=tc.palette())):
        st, keep = apt.ThermalSettings("A", "4", **bad)._c()
        assert _c_call(C.byref(cc), C.byref(st), image=bool(st.image_channels))[0] == 4, bad
    st, _ = apt.ThermalSettings(2, "4", t_low=180, t_high=320)._c()
    assert _c_call(C.byref(cc), C.byref(st))[0] == 4
    # an image exactly when image_channels asks for one
    st, _ = apt.ThermalSettings("A", "4", t_low=180, t_high=320, image_channels=1)._c()
    assert _c_call(C.byref(cc), C.byref(st), image=False)[0] == 4
    assert _c_call(C.byref(cc), C.byref(cs), image=True)[0] == 4
    for i, k, v in ((0, 0, np.nan), (3, 2, np.inf)):
        prt = np.array(tm.PRT)
        prt[i, k] = v
        assert _c_call(C.byref(apt.ThermalCoefficients(prt, tm.CH3B, tm.CH4, tm.CH5)._c()), C.byref(cs))[0] == 4
    for k, v in ((0, np.nan), (2, 0.0), (6, -np.inf)):
        ch = list(tm.CH5)
        ch[k] = v
        rc, msg = _c_call(C.byref(apt.ThermalCoefficients(tm.PRT, tm.CH3B, tm.CH4, ch)._c()), C.byref(cs))
        assert rc == 4 and "thermal" in msg
    with pytest.raises(apt.InvalidError):
        host(tm.scene(200, 0, seed=1), tc.coeffs(), apt.DespeckleSettings())
    with pytest.raises(apt.InvalidError):
        host(tm.scene(200, 0, seed=1), tc.coeffs(), apt.ThermalSettings("A", "6", t_low=180, t_high=320))
