"""The geolocation stage on the GPU (k_geoloc_head, k_geoloc_rows, k_geoloc behind the track's launches) against the
numpy model (np_geoloc_model.py) with the bounds geoloc_cases.py states, the orbit form against the positions form, and
the plan form against the host-array forms.

Heights 2 (the smallest with a direction), 5 (4545 pixels: a partly filled last wave, waves spanning two rows), 263 and
530; yaw +-0.03, hscale / vscale 0.9 to 1.1; a swath over 87 degrees of latitude; one across the antimeridian; x offsets
above half a pixel; 2100 rows, whose last rows lie beyond the 60 degrees of arc the geometry can invert."""
import math

import numpy as np
import pytest

import geoloc_cases as gc
import np_geoloc_model as gm

import noaa_apt_amd as apt
from noaa_apt_amd.testing.synth import synth_apt
from test_sat_cpu import TLE_2020, orbit

pytestmark = pytest.mark.gpu

f32 = np.float32
NAMES = ("h2", "h5", "h263", "h530_rotating", "pole", "antimeridian", "far")


def planes(name, **kw):
    track = gc.case(name)[0]
    return apt.geolocate(track.shape[0], track, gc.map_settings_of(name), gc.settings_of(name, **kw), latlon=True, sun=True)


def normalised(name, x, channel, black, max_zenith_deg=80.0, kind="start"):
    track, _, t = gc.case(name)
    ref = gc.settings_of(name, kind=kind).ref_time
    return apt.normalize_sun(x, track, channel, black=black, ref_time=ref, max_zenith_deg=max_zenith_deg,
                             map_settings=gc.map_settings_of(name), return_info=True)


@pytest.mark.parametrize("name", NAMES)
def test_equals_model(name):
    h = gc.case(name)[0].shape[0]
    latlon, cos_sun, info = planes(name)
    gc.check_planes(name, latlon, cos_sun, info)
    x = gc.rows_of(h, seed=h)
    rows, rinfo = normalised(name, x, "B", 33.5)
    gc.check_rows(x, rows, cos_sun, 1, 33.5, 80.0, rinfo, note=name)  # (rows asked for alone: the same cos_sun bits)
    assert gc.record(rinfo) == gc.record(info)
    if name == "far":
        assert info.n_outside > 10000 and np.isnan(latlon[np.isnan(cos_sun)]).all()
    if name == "h530_rotating":
        assert np.abs(gc.model(name)[0].xoff).max() > 0.5


def test_repeat_start_end_and_host_twin():
    a = planes("h263")
    b = planes("h263")
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and gc.record(a[2]) == gc.record(b[2])
    e = planes("h263", kind="end")
    assert a[0].tobytes() == e[0].tobytes() and a[1].tobytes() == e[1].tobytes() and gc.record(a[2]) == gc.record(e[2])
    # the plain C++ twin: another libm, the same bounds against the model, so twice the bound between the two
    track = gc.case("h263")[0]
    hl, hc, _ = apt.geolocate_host(263, track, gc.map_settings_of("h263"), gc.settings_of("h263"), latlon=True, sun=True)
    assert np.array_equal(np.isnan(hc), np.isnan(a[1]))
    assert gm.separation(hl, gm.unit(a[0])).max() <= 2 * gc.TAU * gc.model("h263")[0].sc.x_res
    assert np.abs(hc.astype(np.float64) - a[1]).max() <= 2 * gc.ULP1


def test_orbit_form_against_positions_form():
    ms, h = 1580246771392, 300
    o = orbit(TLE_2020, "NOAA 19", "start", ms)
    track = apt.sat_track(o, h)
    name = gc.define("noaa19_gpu", track, (0.0, 1.0, 1.0), ms)
    assert np.abs(gc.model(name)[0].xoff).max() > 0.5
    a = apt.geolocate(h, o, None, apt.GeolocSettings(), latlon=True, sun=True)
    b = apt.geolocate(h, track, None, apt.GeolocSettings(ref_time=apt.RefTime.Start(ms)), latlon=True, sun=True)
    gc.check_planes(name, *a, note="orbit form")
    gc.check_planes(name, *b, note="positions form")
    e = apt.geolocate(h, orbit(TLE_2020, "NOAA 19", "end", ms + 500 * h), None, apt.GeolocSettings(), latlon=True, sun=True)
    assert e[0].tobytes() == a[0].tobytes() and e[1].tobytes() == a[1].tobytes()
    x = gc.rows_of(h, seed=7)
    rows, info = apt.normalize_sun(x, o, "A", black=20.0, return_info=True)
    gc.check_rows(x, rows, a[1], 0, 20.0, 80.0, info, note="orbit rows")


def test_sun_night_and_non_finite_video():
    t = gc.T_NOON_2024
    delta, lon = apt.sun_position(t)
    track = gc.mm.great_circle_track(math.degrees(delta), math.degrees(lon), 190.0, 5)
    _, cos_sun, info = apt.geolocate(5, track, None, apt.GeolocSettings(ref_time=apt.RefTime.Start(t)), latlon=False, sun=True)
    assert abs(float(cos_sun[0, gm.CENTRE]) - 1.0) <= 1e-7 and info.n_capped == 0
    # twelve hours later the same swath is in the dark: every pixel capped, gain 1 / cmin
    h = 263
    x = gc.rows_of(h, seed=3)
    x[86], x[2080 + 994], x[2 * 2080 + 500] = np.nan, np.inf, -np.inf
    track, _, t = gc.case("h263")
    night = apt.RefTime.Start(t + 12 * 3600000)
    ms = gc.map_settings_of("h263")
    _, cos_sun, _ = apt.geolocate(h, track, ms, apt.GeolocSettings(ref_time=night), latlon=False, sun=True)
    rows, info = apt.normalize_sun(x, track, "A", black=30.0, ref_time=night, max_zenith_deg=75.0, map_settings=ms,
                                   return_info=True)
    assert cos_sun.max() < 0 and info.n_outside == 0 and info.n_capped == h * 909
    gc.check_rows(x, rows, cos_sun, 0, 30.0, 75.0, info, note="night")
    v = x[:h * 2080].reshape(h, 2080)[:, 86:995]
    with np.errstate(invalid="ignore"):
        want = (f32(30.0) + (v - f32(30.0)) / gm.cmin_of(75.0)).astype(f32)
    assert rows[:h * 2080].reshape(h, 2080)[:, 86:995].tobytes() == want.tobytes()
    assert np.isnan(rows[86]) and rows[2080 + 994] == np.inf and rows[2 * 2080 + 500] == -np.inf


def test_record_reasons():
    track = gc.case("h5")[0]
    with pytest.raises(apt.InternalError, match="fewer than two rows") as e:
        apt.geolocate(1, track[:1])
    assert (e.value.info.status, e.value.info.reason, e.value.info.height) == (1, apt.GEOLOC_REASON_HEIGHT, 1)
    with pytest.raises(apt.InternalError, match="differs from the image height") as e:
        apt.geolocate(5, track[:4])
    assert (e.value.info.status, e.value.info.reason, e.value.info.height) == (1, 7, 5)
    with pytest.raises(apt.InternalError, match="differs from the image height"):
        apt.geolocate(5, gc.case("h263")[0])
    with pytest.raises(apt.InternalError):
        apt.normalize_sun(gc.rows_of(1, 1), track[:1], "A", black=0.0)


def test_normalize_sun_takes_black_from_the_telemetry():
    x = synth_apt(11025, 110, 41)
    rows = apt.decode(apt.Context(device=0), apt.Settings(), x, apt.Rate.hz(11025), True)
    h = rows.size // 2080
    track = gc.mm.great_circle_track(30.0, -60.0, 190.0, h)
    ref = apt.RefTime.Start(gc.T_NOON_2024 + 4 * 3600000)
    black = float(apt.read_telemetry(None, rows).get_wedge_value(9, "A"))
    got = apt.normalize_sun(rows, track, "A", ref_time=ref)
    want = apt.normalize_sun(rows, track, "A", black=black, ref_time=ref)
    assert got.tobytes() == want.tobytes() and got.tobytes() != rows.tobytes()


def test_plan_path():
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    recs = [synth_apt(11025, 110, 41), synth_apt(11025, 80, 42)]
    k = len(recs)
    stream = torch.cuda.Stream(device=dev)
    st = apt.GeolocSettings(channel="B", ref_time=apt.RefTime.End(gc.T_NOON_2024 + 3 * 3600000), black=12.0)
    ms = apt.MapSettings(0.02, 0.95, 1.05)
    ptr = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
    with torch.cuda.stream(stream):
        plan = apt.Plan(apt.Settings(), apt.Rate.hz(11025), True, max_samples=max(r.size for r in recs), max_batch=k,
                        stream=stream.cuda_stream)
        plan.enable_timing(2)
        cap = int(plan.info.max_rows)
        d_in = [torch.from_numpy(r).to(dev) for r in recs]
        d_rows = [torch.zeros(cap * 2080, dtype=torch.float32, device=dev) for _ in recs]
        d_ll = [torch.full((cap * 909 * 2 + 2,), -7.0, dtype=torch.float64, device=dev) for _ in recs]
        d_cos = [torch.full((cap * 909 + 1,), -7.0, dtype=torch.float32, device=dev) for _ in recs]
        d_out = [torch.full((cap * 2080,), -7.0, dtype=torch.float32, device=dev) for _ in recs]
        tracks0 = [gc.mm.great_circle_track(10.0, 20.0, 12.0, 10)] * k
        with pytest.raises(apt.InvalidError):
            plan.geolocate_device(ptr(d_rows), [cap] * k, tracks0, st, ms, ptr(d_ll), ptr(d_cos), ptr(d_out))  # nothing decoded
        plan.decode_device(ptr(d_in), [r.size for r in recs], ptr(d_rows), [cap] * k)
        res = plan.results(k)
        assert all(r.status == 0 for r in res)
        decoded = [int(r.n_out) // 2080 for r in res]
        assert decoded[0] != decoded[1] and min(decoded) >= 100
        originals = [t.clone() for t in d_rows]
        caps = [cap, decoded[1] - 5]  # the second recording's buffers hold fewer rows than were decoded
        hs = [min(d, c) for d, c in zip(decoded, caps)]
        tracks = [gc.mm.great_circle_track(35.0 + 5 * i, -80.0, 191.0, hs[i]) for i in range(k)]
        ll_p = [d_ll[0].data_ptr(), d_ll[1].data_ptr() + 16]
        cos_p = [d_cos[0].data_ptr(), d_cos[1].data_ptr() + 4]
        plan.geolocate_device(ptr(d_rows), caps, tracks, st, ms, ll_p, cos_p, ptr(d_out))
        got = plan.geoloc_results(k)
        for i in range(k):
            h = hs[i]
            rows = originals[i][:h * 2080].cpu().numpy()
            off = i  # (the offsets above, in elements of 16 and 4 bytes)
            ll = d_ll[i].cpu().numpy()
            cs = d_cos[i].cpu().numpy()
            assert np.all(ll[:2 * off] == -7.0) and np.all(ll[2 * off + h * 909 * 2:] == -7.0)  # nothing past the rows
            assert np.all(cs[:off] == f32(-7.0)) and np.all(cs[off + h * 909:] == f32(-7.0))
            want_ll, want_cos, want = apt.geolocate(h, tracks[i], ms, st, latlon=True, sun=True)
            want_rows, want_r = apt.normalize_sun(rows, tracks[i], "B", black=12.0, ref_time=st.ref_time, map_settings=ms,
                                                  return_info=True)
            assert ll[2 * off:2 * off + h * 909 * 2].tobytes() == want_ll.tobytes(), i
            assert cs[off:off + h * 909].tobytes() == want_cos.tobytes(), i
            out = d_out[i].cpu().numpy()
            assert out[:h * 2080].tobytes() == want_rows.tobytes(), i  # rows with both planes == rows alone
            assert gc.record(got[i]) == gc.record(want) == gc.record(want_r) and got[i].height == h
            assert torch.equal(d_rows[i], originals[i])  # out of place: the input is untouched
        timing = plan.collect_timing()
        for name in ("image_geoloc_track", "image_geoloc_rows", "image_geoloc"):
            assert name in timing
        # in place, rows alone: the same bits
        out_of_place = [t.clone() for t in d_out]
        plan.geolocate_device(ptr(d_rows), caps, tracks, st, ms, None, None, ptr(d_rows))
        again = plan.geoloc_results(k)
        for i in range(k):
            assert torch.equal(d_rows[i][:hs[i] * 2080], out_of_place[i][:hs[i] * 2080]), i
            assert torch.equal(d_rows[i][hs[i] * 2080:], originals[i][hs[i] * 2080:]), i
            assert gc.record(again[i]) == gc.record(got[i])
            d_rows[i].copy_(originals[i])
        # the orbit form, chained likewise: against the host-array orbit form
        o = orbit(TLE_2020, "NOAA 19", "end", 1580246771392 + 500 * hs[0])
        plan.geolocate_device(ptr(d_rows)[:1], caps[:1], [o], st, None, ll_p[:1], cos_p[:1], None)
        want_ll, want_cos, want = apt.geolocate(hs[0], o, None, st, latlon=True, sun=True)
        rec = plan.geoloc_results(1)[0]
        assert d_ll[0][:hs[0] * 909 * 2].cpu().numpy().tobytes() == want_ll.tobytes()
        assert d_cos[0][:hs[0] * 909].cpu().numpy().tobytes() == want_cos.tobytes() and gc.record(rec) == gc.record(want)
        # a failed record: the planes of the rows NaN, the rows copied unchanged
        for t in d_out:
            t.fill_(-7.0)
        bad = [tracks[0][:-1], tracks[1]]
        plan.geolocate_device(ptr(d_rows), caps, bad, st, ms, ptr(d_ll), ptr(d_cos), ptr(d_out))
        rec = plan.geoloc_results(k)
        assert (rec[0].status, rec[0].reason, rec[0].height, rec[0].n_outside) == (1, 7, hs[0], 0)
        assert rec[1].status == 0
        assert torch.isnan(d_ll[0][:hs[0] * 909 * 2]).all() and torch.isnan(d_cos[0][:hs[0] * 909]).all()
        assert torch.equal(d_out[0][:hs[0] * 2080], originals[0][:hs[0] * 2080])
        # refusals that need the buffers
        with pytest.raises(apt.InvalidError, match="overlaps"):
            plan.geolocate_device(ptr(d_rows), caps, tracks, st, ms, None, None, [d_rows[0].data_ptr() + 2080 * 4, d_out[1].data_ptr()])
        with pytest.raises(apt.InvalidError, match="overlaps"):
            plan.geolocate_device(ptr(d_rows), caps, tracks, st, ms, None, [d_out[0].data_ptr(), d_cos[1].data_ptr()], ptr(d_out))
        with pytest.raises(apt.InvalidError, match="16-byte"):
            plan.geolocate_device(ptr(d_rows), caps, tracks, st, ms, [d_ll[0].data_ptr() + 8, d_ll[1].data_ptr()], None, None)
        plan.synchronize()
    plan.close()
