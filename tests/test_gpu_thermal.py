"""The thermal calibration stage on the GPU (k_thermal_space, k_thermal_setup, k_thermal_map) against the numpy model
(np_thermal_model.py) on row images built directly, and the plan form against the host-array form.

What thermal_cases.check asserts: slope, icpt, space, c_space, c_bb and t_bb bit-identical to the model, n_bb within
1e-12 relative (one exp); |T - T_model| <= 0.01 K wherever T_model >= 200 K (a tenth of what a 10-bit count resolves),
below that |N_e - N_e_model| <= 1e-5 * n_bb, NaNs in the same places except where the model has |N_e| < 1e-5 * n_bb (at
most 0.1 % of the video); the scale image bit-exact against the model's f32 mapping of the returned plane; n_nan, t_min
and t_max equal to numpy's over the returned plane."""
import numpy as np
import pytest

import np_thermal_model as tm
import thermal_cases as tc

import noaa_apt_amd as apt
from noaa_apt_amd.testing.synth import synth_apt

pytestmark = pytest.mark.gpu

f32 = np.float32
gpu = apt.calibrate_thermal


@pytest.mark.parametrize("channel", [0, 1])
@pytest.mark.parametrize("identity", ["4", "5", "3b"])
def test_equals_model(channel, identity):
    x = tm.scene(200, 0, seed=3 + channel, space_noise=0.8)  # h = 200: the frame search's loop is empty, row 0
    _, _, info, _ = tc.check(gpu, x, channel, identity, image_channels=4, pal=tc.palette(), note=(channel, identity))
    assert info.telemetry_row == 0


def test_frame_row_identity_from_telemetry_and_image_forms():
    x = tm.scene(263, 37, seed=5, identities=(5, 3), space_noise=0.8)
    _, _, info, _ = tc.check(gpu, x, 0, None, image_channels=1, cold_white=False, note="A auto, gray")
    assert (info.telemetry_row, info.channel_id) == (37, 5)
    _, _, info, _ = tc.check(gpu, x, 1, None, image_channels=4, note="B auto, RGBA")
    assert (info.telemetry_row, info.channel_id) == (37, 3)
    tc.check(gpu, x, 1, None, image_channels=1, note="B gray, cold white")
    tc.check(gpu, x, 0, "5", image_channels=4, pal=tc.palette(), cold_white=False, note="A palette, warm white")
    tc.check(gpu, x, 1, None, image_channels=0, note="no image")


def test_more_rows_than_workgroups():
    # the map kernel's grid stops at 512 workgroups: rows beyond are walked with a stride
    x = tm.scene(530, 45, seed=6, identities=(4, 4), space_noise=0.8)
    _, _, info, _ = tc.check(gpu, x, 1, None, image_channels=4, note="530 rows")
    assert info.telemetry_row % 128 == 45 and info.channel_id == 4  # (the scene repeats its frame every 128 rows)
    tc.check(gpu, x, 0, None, image_channels=1, note="530 rows gray")


def test_failures():
    with pytest.raises(apt.InternalError, match="too short") as e:
        gpu(tm.scene(199, 0, seed=1), tc.coeffs(), apt.ThermalSettings("A", "4", t_low=180, t_high=320))
    assert (e.value.info.status, e.value.info.reason, e.value.info.height) == (1, 2, 199)
    x = tm.scene(200, 0, seed=2, identities=(1, 3))  # channel A sends "2"
    info = tc.check(gpu, x, 0, None, note="identity 2")
    assert (info.reason, info.channel_id) == (13, 1)
    tc.check(gpu, x, 0, "4", image_channels=1, note="identity 2 forced to 4")
    assert tc.check(gpu, x, 0, 2, note="forced 3a").reason == 13
    y = x.reshape(200, 2080).copy()
    y[:, 994:1040] = y[0, 995]
    y[:, 2034:2080] = y[0, 995]
    assert tc.check(gpu, y.ravel(), 0, "4", note="flat wedges").reason == 14


def test_minute_markers_leave_space_alone():
    x = tm.scene(263, 37, seed=4)
    y = tm.scene(263, 37, seed=4, markers=(20, 21, 80, 81))
    _, _, a, _ = tc.check(gpu, x, 1, "4", note="no markers")
    _, _, b, _ = tc.check(gpu, y, 1, "4", note="markers")
    assert a.telemetry_row == b.telemetry_row == 37
    assert tc.bits64(a.space) == tc.bits64(b.space) and tc.bits64(a.c_space) == tc.bits64(b.c_space)


def test_non_finite_samples():
    x = tm.scene(200, 0, seed=8)
    _, _, clean, _ = tc.check(gpu, x, 1, "5", note="clean")
    y = x.reshape(200, 2080).copy()
    y[5, 1040 + 100], y[6, 1040 + 101], y[7, 1040 + 993], y[199, 1040 + 86] = np.nan, np.inf, -np.inf, np.nan
    kelvin, image, info, _ = tc.check(gpu, y.ravel(), 1, "5", image_channels=4, note="video")
    assert np.isnan(kelvin[5, 14]) and np.isnan(kelvin[6, 15]) and np.isnan(kelvin[7, 907]) and np.isnan(kelvin[199, 0])
    assert not image[5, 1040 + 100].any() and image[5, 1040 + 99, 3] == 255
    y = x.reshape(200, 2080).copy()
    y[3, 1040 + 50], y[90, 1040 + 60], y[91, 1040 + 44] = np.nan, np.inf, -np.inf
    _, _, info, _ = tc.check(gpu, y.ravel(), 1, "5", note="space band")
    assert tc.bits64(info.space) == tc.bits64(clean.space)
    y = x.reshape(200, 2080).copy()
    y[83, 1040 + 1000] = np.nan  # wedge 11, a thermometer
    assert tc.check(gpu, y.ravel(), 1, "5", note="wedge").reason == 14


def test_host_twin_has_the_same_scalars():
    x = tm.scene(263, 37, seed=9, space_noise=0.8)
    st = apt.ThermalSettings("B", "3b", t_low=180, t_high=320, image_channels=1)
    kg, ig, a = gpu(x, tc.coeffs(), st)
    kh, ih, b = apt.calibrate_thermal_host(x, tc.coeffs(), st)
    for name in tc.SCALARS:
        assert tc.bits64(getattr(a, name)) == tc.bits64(getattr(b, name)), name
    assert abs(a.n_bb - b.n_bb) <= 1e-12 * b.n_bb
    # (two logf implementations, each within the bound against the f64 model)
    both = np.isfinite(kg) & np.isfinite(kh) & (kh >= 201)
    assert np.abs(kg[both] - kh[both]).max() <= 0.02


def _record(r):
    return (r.status, r.reason, r.height, r.telemetry_row, r.channel_id, r.n_nan) + tuple(
        tc.bits64(getattr(r, n)) for n in tc.SCALARS + ("n_bb",)) + (f32(r.t_min).tobytes(), f32(r.t_max).tobytes())


def test_plan_path():
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    rec = synth_apt(11025, 110, 41)
    stream = torch.cuda.Stream(device=dev)
    co = tc.coeffs()
    with torch.cuda.stream(stream):
        plan = apt.Plan(apt.Settings(), apt.Rate.hz(11025), True, max_samples=rec.size, max_batch=1,
                        stream=stream.cuda_stream)
        plan.enable_timing(2)
        cap = int(plan.info.max_rows)
        d_in = torch.from_numpy(rec).to(dev)
        d_rows = torch.zeros(cap * 2080, dtype=torch.float32, device=dev)
        d_kelvin = torch.empty(cap * 909 + 1, dtype=torch.float32, device=dev)
        d_image = torch.empty(cap * 2080 * 4 + 8, dtype=torch.uint8, device=dev)
        st = apt.ThermalSettings("B", "4", t_low=180, t_high=320, image_channels=4)
        with pytest.raises(apt.InvalidError):
            plan.calibrate_thermal_device([d_rows.data_ptr()], [cap], [d_kelvin.data_ptr()], co, st, [d_image.data_ptr()])
        plan.decode_device([d_in.data_ptr()], [rec.size], [d_rows.data_ptr()], [cap])
        res = plan.results(1)
        assert res[0].status == 0
        decoded = int(res[0].n_out) // 2080
        assert decoded >= 206
        for rows_cap, ch, k_off, i_off, ident in ((cap, 4, 0, 0, "4"), (decoded - 5, 1, 1, 1, "4"), (cap, 4, 1, 4, 1),
                                                  (cap, 0, 0, 0, "3b")):
            h = min(decoded, rows_cap)
            d_kelvin.fill_(-7.0)
            d_image.fill_(77)
            st = apt.ThermalSettings("B", ident, t_low=180, t_high=320, image_channels=ch)
            kp, ip = d_kelvin.data_ptr() + 4 * k_off, d_image.data_ptr() + i_off
            plan.calibrate_thermal_device([d_rows.data_ptr()], [rows_cap], [kp], co, st, [ip] if ch else None)
            got = plan.thermal_results(1)[0]
            kelvin = d_kelvin.cpu().numpy()
            image = d_image.cpu().numpy()
            rows = d_rows[:h * 2080].cpu().numpy()
            assert np.all(kelvin[:k_off] == f32(-7.0)) and np.all(kelvin[k_off + h * 909:] == f32(-7.0))  # nothing past the rows
            plane = kelvin[k_off:k_off + h * 909].reshape(h, 909)
            if ch:
                assert np.all(image[:i_off] == 77) and np.all(image[i_off + h * 2080 * ch:] == 77)
                img = image[i_off:i_off + h * 2080 * ch].reshape((h, 2080) if ch == 1 else (h, 2080, 4))
            if ident == 1:  # not a thermal channel: recorded, the planes all NaN / level 0 with alpha 0
                assert (got.status, got.reason, got.height, got.channel_id) == (1, 13, h, 1)
                assert np.isnan(plane).all() and got.n_nan == h * 909 and np.isnan(got.t_min) and np.isnan(got.t_max)
                assert np.array_equal(img, tm.scale_image(plane, 1, 4, 180, 320, True))
                continue
            want_k, want_i, want = apt.calibrate_thermal(rows, co, st)
            assert plane.tobytes() == want_k.tobytes(), (rows_cap, ch)
            assert _record(got) == _record(want) and got.status == 0 and got.height == h
            if ch:
                assert np.array_equal(img, want_i), (rows_cap, ch)
        timing = plan.collect_timing()
        for name in ("image_telemetry", "image_thermal_space", "image_thermal_setup", "image_thermal_map"):
            assert name in timing
        st = apt.ThermalSettings("B", "4", t_low=180, t_high=320, image_channels=4)
        with pytest.raises(apt.InvalidError, match="overlaps"):
            plan.calibrate_thermal_device([d_rows.data_ptr()], [cap], [d_rows.data_ptr() + 64], co, st, [d_image.data_ptr()])
        with pytest.raises(apt.InvalidError, match="overlaps"):
            plan.calibrate_thermal_device([d_rows.data_ptr()], [cap], [d_kelvin.data_ptr()], co, st, [d_rows.data_ptr()])
        with pytest.raises(apt.InvalidError, match="aligned"):
            plan.calibrate_thermal_device([d_rows.data_ptr()], [cap], [d_kelvin.data_ptr()], co, st, [d_image.data_ptr() + 2])
        plan.synchronize()
    plan.close()


def test_plan_buffer_edges():
    """What the plan form accepts and refuses at the edges of its "overlaps d_rows" checks: d_rows[0] and the outputs
    are carved from one tensor, so the addresses are exact.  (The recordings are too short for a telemetry frame: the
    record says so and the planes are NaN / level 0, written all the same.)"""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    recs = [synth_apt(48000, s, 700 + i) for i, s in enumerate((6, 8, 11))]
    k = len(recs)
    co = tc.coeffs()
    plan = apt.Plan(apt.Settings(), apt.Rate.hz(48000), True, max_samples=max(r.size for r in recs), max_batch=k)
    cap = int(plan.info.max_rows)
    floats = cap * 2080
    d_in = [torch.from_numpy(r).to(dev) for r in recs]
    both = torch.full((2 * floats,), -7.0, dtype=torch.float32, device=dev)  # d_rows[0], then room for an output
    d_rows = [both[:floats]] + [torch.zeros(floats, dtype=torch.float32, device=dev) for _ in recs[1:]]
    d_kelvin = [torch.full((cap * 909,), -7.0, dtype=torch.float32, device=dev) for _ in recs]
    d_image = [torch.full((floats,), 77, dtype=torch.uint8, device=dev) for _ in recs]
    rows_p, kelvin_p, image_p = ([t.data_ptr() for t in ts] for ts in (d_rows, d_kelvin, d_image))
    end = rows_p[0] + 4 * floats
    assert rows_p[0] == both.data_ptr()
    plan.decode_device([t.data_ptr() for t in d_in], [r.size for r in recs], rows_p, [cap] * k)
    res = plan.results(k)
    assert all(r.status == 0 for r in res)
    heights = [int(r.n_out) // 2080 for r in res]
    st = apt.ThermalSettings("B", "4", t_low=180, t_high=320, image_channels=1)
    plan.calibrate_thermal_device(rows_p, [cap] * k, kelvin_p, co, st, image_p)
    apart = plan.thermal_results(k)
    assert [(r.status, r.reason, r.height) for r in apart] == [(1, 2, h) for h in heights]
    # an output that begins exactly where d_rows[0] ends: accepted, and the separate buffer's bits
    h = heights[0]
    plan.calibrate_thermal_device(rows_p, [cap] * k, [end] + kelvin_p[1:], co, st, image_p)
    assert [_record(r) for r in plan.thermal_results(k)] == [_record(r) for r in apart]
    assert both[floats:floats + h * 909].cpu().numpy().tobytes() == d_kelvin[0][:h * 909].cpu().numpy().tobytes()
    want_image = d_image[0].clone()
    d_image[0].fill_(77)
    plan.calibrate_thermal_device(rows_p, [cap] * k, kelvin_p, co, st, [end] + image_p[1:])
    assert [_record(r) for r in plan.thermal_results(k)] == [_record(r) for r in apart]
    assert torch.equal(both.view(torch.uint8)[4 * floats:4 * floats + h * 2080], want_image[:h * 2080])
    assert torch.all(want_image[h * 2080:] == 77) and torch.all(d_image[0] == 77)
    # one float (one byte) earlier: refused
    with pytest.raises(apt.InvalidError, match="d_kelvin overlaps"):
        plan.calibrate_thermal_device(rows_p, [cap] * k, [end - 4] + kelvin_p[1:], co, st, image_p)
    with pytest.raises(apt.InvalidError, match="d_images overlaps"):
        plan.calibrate_thermal_device(rows_p, [cap] * k, kelvin_p, co, st, [end - 1] + image_p[1:])
    # equal starts overlap even where the rows buffer is empty
    with pytest.raises(apt.InvalidError, match="d_kelvin overlaps"):
        plan.calibrate_thermal_device(rows_p, [cap, 0, cap], [rows_p[1]] + kelvin_p[1:], co, st, image_p)
    with pytest.raises(apt.InvalidError, match="d_images overlaps"):
        plan.calibrate_thermal_device(rows_p, [cap, 0, cap], kelvin_p, co, st, [rows_p[1]] + image_p[1:])
    plan.synchronize()
    plan.close()
