"""What test_thermal_cpu.py and test_gpu_thermal.py share: one call of the thermal calibration (the host twin or the
GPU form) checked against np_thermal_model.py with the bounds DESIGN.md §19 states."""
import struct

import numpy as np
import pytest

import np_thermal_model as tm

import noaa_apt_amd as apt

f32 = np.float32
T_LOW, T_HIGH = 180.0, 320.0
SCALARS = ("slope", "icpt", "space", "c_space", "c_bb", "t_bb")


def coeffs():
    return apt.ThermalCoefficients(tm.PRT, tm.CH3B, tm.CH4, tm.CH5)


def palette():
    lv = np.arange(256)
    return np.stack([(lv * 7 + 3) % 256, 255 - lv, (lv * lv) % 251], axis=1).astype(np.uint8)


def telemetry(x):
    """(frame row, values_a, values_b, index_a, index_b) from the CPU oracle"""
    from oracle import image_binding as oi
    tel = oi.read_telemetry(x)
    a, b = tel._arrs()
    idx = [oi.lib().apt_oracle_telemetry_channel_index(a, b, ch) for ch in (0, 1)]
    return tel.row, tel.values_a, tel.values_b, idx[0], idx[1]


def bits64(v):
    return struct.pack("<d", float(v))


def check(call, x, channel, channel_id=None, image_channels=0, pal=None, cold_white=True, note=None):
    """call: apt.calibrate_thermal or apt.calibrate_thermal_host.  -> (kelvin, image, info, model scalars), or the failed
    record where the model says the calibration fails."""
    row, va, vb, ia, ib = telemetry(x)
    forced = None if channel_id is None else {"4": 3, "5": 4, "3b": 5}.get(channel_id, channel_id)
    ident = (ia, ib)[channel] if forced is None else forced
    reason, s, n_model, t_model = tm.calibrate(x, row, (va, vb)[channel], channel, ident)
    settings = apt.ThermalSettings("AB"[channel], channel_id, t_low=T_LOW, t_high=T_HIGH, cold_white=cold_white,
                                   palette=pal, image_channels=image_channels)
    if reason:
        with pytest.raises(apt.InternalError) as e:
            call(x, coeffs(), settings)
        info = e.value.info
        assert (info.status, info.reason, info.telemetry_row, info.channel_id) == (1, reason, row, ident), note
        return info
    kelvin, image, info = call(x, coeffs(), settings)
    h = x.size // 2080
    assert kelvin.dtype == f32 and kelvin.shape == (h, 909), note
    assert (info.status, info.reason, info.height, info.telemetry_row, info.channel_id) == (0, 0, h, row, ident), note
    for name in SCALARS:
        assert bits64(getattr(info, name)) == bits64(s[name]), (note, name, getattr(info, name), s[name])
    assert abs(info.n_bb - s["n_bb"]) <= 1e-12 * abs(s["n_bb"]), (note, info.n_bb, s["n_bb"])

    # the Kelvin plane: 0.01 K from 200 K up; below, by radiance; NaNs in the same places except at N_e = 0
    ch = tm.CHANNELS[tm.SET_OF_IDENTITY[ident]]
    tol_n = 1e-5 * s["n_bb"]
    got = kelvin.astype(np.float64)
    hot = t_model >= 200.0  # (False where the model is NaN)
    dt = np.abs(got[hot] - t_model[hot])
    worst_t = float(dt.max()) if dt.size else 0.0
    cold = ~hot & ~np.isnan(t_model) & ~np.isnan(got)
    dn = np.abs(tm.radiance_of_kelvin(got[cold], ch) - n_model[cold])
    worst_n = float(dn.max()) if dn.size else 0.0
    print(f"thermal {note}: identity {ident}, hot {int(hot.sum())} px max |dT| {worst_t:.3g} K; "
          f"cold {int(cold.sum())} px max |dN| / n_bb {worst_n / s['n_bb']:.3g}")
    assert not np.isnan(got[hot]).any() and worst_t <= 0.01, (note, worst_t)
    assert worst_n <= tol_n, (note, worst_n, tol_n)
    with np.errstate(invalid="ignore"):
        near_zero = np.abs(n_model) < tol_n
    assert near_zero.sum() <= 0.001 * near_zero.size, note
    differ = np.isnan(got) != np.isnan(t_model)
    assert not (differ & ~near_zero).any(), (note, int((differ & ~near_zero).sum()))

    # the record's view of the plane
    finite = kelvin[np.isfinite(kelvin)]
    assert info.n_nan == int(np.isnan(kelvin).sum()), note
    if finite.size:
        assert f32(info.t_min).tobytes() == finite.min().tobytes() and f32(info.t_max).tobytes() == finite.max().tobytes()
    else:
        assert np.isnan(info.t_min) and np.isnan(info.t_max)

    # the scale image: the f32 mapping of the plane the call returned, bit for bit; zero outside the video
    if image_channels == 0:
        assert image is None
    else:
        want = tm.scale_image(kelvin, channel, image_channels, T_LOW, T_HIGH, cold_white, pal)
        assert image.dtype == np.uint8 and image.shape == want.shape, note
        bad = np.argwhere(image != want)
        assert bad.size == 0, (note, bad[:4])
        base = 1040 * channel + 86
        outside = np.ones(2080, bool)
        outside[base:base + 909] = False
        if image_channels == 1:
            assert not image[:, outside].any()
        else:
            assert not image[:, outside, :3].any() and (image[:, outside, 3] == 255).all()
    return kelvin, image, info, s
