"""The land / sea / lake mask on the GPU (k_land_mask<Plane>, k_land_mask<Swath> behind the geolocation stage's track and
row launches, k_false_color_masked) against np_landmask_model.py with the assertions landmask_cases.py states, which
test_landmask_cpu.py applies to the host twin: the plane form bit for bit under every band count, the swath form against
the plane form of the GPU's own points, end to end against the model's geolocation, the plan form against the host-array
form, and the colouriser against process() and against the model.

Heights 2 (1818 pixels: a partly filled last wave) and 5 (waves that span two rows), the scenes of the overlay fit
(120 to 240 rows), 2100 rows whose last are invalid, planes whose length is no multiple of 64 with NaNs at arbitrary
places, a wave with no valid lane, synthetic layers at the pole and across the antimeridian."""
import numpy as np
import pytest

import landmask_cases as lc
import np_landmask_model as lmm
from test_sat_cpu import TLE_2020, orbit

import noaa_apt_amd as apt
from noaa_apt_amd.testing.synth import synth_apt

pytestmark = pytest.mark.gpu

SIDE = lc.GPU


@pytest.mark.parametrize("name", lc.SMALL)
def test_plane_small_cases_every_band_count(name):
    ll = lc.model_points(name)
    lc.check_plane(SIDE, ll, lc.fixture_layers(), lc.fixture_edges(), note=name)
    lc.check_plane(SIDE, lc.nan_plane(ll, seed=len(name)), lc.fixture_layers(), lc.fixture_edges(), note=name + " nan")


def test_plane_scene_240_rows():
    lc.check_plane(SIDE, lc.model_points("scene1"), lc.fixture_layers(), lc.fixture_edges(), bands=(720, 7200), note="scene1")
    lc.check_plane(SIDE, lc.nan_plane(lc.model_points("scene1"), seed=1, n_nan=1500), lc.fixture_layers(),
                   lc.fixture_edges(), bands=(720,), note="scene1 nan")


def test_plane_takes_any_shape_infinities_and_a_wave_without_a_valid_lane():
    ll = lc.model_points("h5")
    flat = np.ascontiguousarray(ll.reshape(-1, 2)[:1000]).copy()
    flat[3] = (np.inf, 0.1)
    flat[4] = (-0.5, -np.inf)
    flat[5] = (-np.inf, np.inf)
    flat[128:192] = np.nan  # one whole wave
    flat[256:320, 0] = np.nan
    lc.check_plane(SIDE, flat.reshape(10, 100, 2), lc.fixture_layers(), lc.fixture_edges(), bands=(1, 720), note="3-d")
    lc.check_plane(SIDE, np.full((70, 2), np.nan), lc.fixture_layers(), lc.fixture_edges(), bands=(720,), note="all nan")
    mask, info = SIDE.plane(np.zeros((0, 2)), lc.fixture_layers())
    assert mask.shape == (0,) and lc.counts_of(info) == (0, 0, 0, 0)


@pytest.mark.parametrize("name", ("pole", "antimeridian"))
def test_plane_synthetic_layers(name):
    layers, edges = lc.synthetic(name)
    ll = lc.model_points(name)[::7]
    want = lc.check_plane(SIDE, ll, layers, edges, bands=(1, 7, 720, 7200), note=name)
    assert {0, 1, 2} <= set(np.unique(want)), name
    co, la = lc.synthetic_parts(name)
    lc.check_plane(SIDE, ll, lc.layers_of(co, None), (edges[0], None), bands=(720,), note=name + " countries")
    lc.check_plane(SIDE, ll, lc.layers_of(None, la), (None, edges[1]), bands=(720,), note=name + " lakes")


def test_degenerate_polygons_pin_the_half_open_rule():
    ll, layers, edges, chosen = lc.degenerate(SIDE)
    want = lc.check_plane(SIDE, ll, layers, edges, note="degenerate")
    deg = ll * lmm.DEG
    co = edges[0]
    for r, k in chosen[:4]:
        assert ((co[:, 0] == deg[r, k, 1]) & (co[:, 1] == deg[r, k, 0])).any(), (r, k)
    assert {0, 1, 2} <= set(np.unique(want))
    # the twin on the same plane: the same bits
    host, _ = apt.land_mask_plane_host(ll, layers)
    assert host.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", ("h2", "h5", "scene3", "antimeridian"))
def test_swath_equals_plane_of_own_points(name):
    layers = lc.fixture_layers() if name != "antimeridian" else lc.synthetic(name)[0]
    h = lc.case(name)[0].shape[0]
    a, ia = lc.swath_equals_plane(SIDE, h, lc.case(name)[0], layers, lc.map_settings_of(name), 720, name)
    b, ib = SIDE.swath(h, lc.case(name)[0], layers, lc.map_settings_of(name), lc.settings(7))
    assert a.tobytes() == b.tobytes() and lc.counts_of(ia) == lc.counts_of(ib)  # again, under another band count


def test_swath_orbit_form():
    o = orbit(TLE_2020, "NOAA 19", "start", 1580246771392)
    mask, info = lc.swath_equals_plane(SIDE, 40, o, lc.fixture_layers(), None, 720, "orbit")
    track = apt.sat_track(o, 40)
    again, _ = SIDE.swath(40, track, lc.fixture_layers())
    assert again.tobytes() == mask.tobytes()


@pytest.mark.parametrize("name", lc.FIXTURE_CASES)
def test_end_to_end_against_the_models_geolocation(name):
    mask, info = SIDE.swath(lc.case(name)[0].shape[0], lc.case(name)[0], lc.fixture_layers(), lc.map_settings_of(name))
    n_bad = lc.check_end_to_end(SIDE, name, lc.fixture_layers(), lc.fixture_edges(), mask)
    assert lc.counts_of(info) == lmm.counts(mask)
    if name in lc.KNOWN_COUNTS:
        assert lc.model_mask(name)[1] == lc.KNOWN_COUNTS[name]
        assert sum(abs(a - b) for a, b in zip(lc.counts_of(info), lc.KNOWN_COUNTS[name])) <= 2 * n_bad
    if name == "far":
        assert info.n_invalid > 60000


def test_end_to_end_synthetic_antimeridian():
    layers, edges = lc.synthetic("antimeridian")
    lc.check_end_to_end(SIDE, "antimeridian", layers, edges)


def test_record_reasons():
    track = lc.case("h5")[0]
    layers = lc.fixture_layers()
    with pytest.raises(apt.InternalError, match="fewer than two rows") as e:
        apt.land_mask(1, track[:1], layers)
    assert (e.value.info.status, e.value.info.reason, e.value.info.height) == (1, apt.GEOLOC_REASON_HEIGHT, 1)
    with pytest.raises(apt.InternalError, match="differs from the image height") as e:
        apt.land_mask(5, track[:4], layers)
    assert (e.value.info.status, e.value.info.reason, e.value.info.height) == (1, 7, 5)
    a, ia = apt.land_mask(5, track, layers)
    b, ib = apt.land_mask(5, track, layers)
    assert a.tobytes() == b.tobytes() and lc.record(ia) == lc.record(ib)


def test_plan_path():
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    recs = [synth_apt(11025, 30, 41), synth_apt(11025, 22, 42), synth_apt(11025, 3, 43)]  # the last: too short to decode
    k = len(recs)
    stream = torch.cuda.Stream(device=dev)
    layers = lc.fixture_layers()
    ms = apt.MapSettings(0.02, 0.95, 1.05)
    ptr = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
    with torch.cuda.stream(stream):
        plan = apt.Plan(apt.Settings(), apt.Rate.hz(11025), True, max_samples=max(r.size for r in recs), max_batch=k,
                        stream=stream.cuda_stream)
        plan.enable_timing(2)
        cap = int(plan.info.max_rows)
        d_in = [torch.from_numpy(r).to(dev) for r in recs]
        d_rows = [torch.zeros(cap * 2080, dtype=torch.float32, device=dev) for _ in recs]
        d_mask = [torch.full((cap * 909 + 8,), 7, dtype=torch.uint8, device=dev) for _ in recs]
        tracks0 = [lc.mm.great_circle_track(-30.0, -60.0, 12.0, 10)] * k
        with pytest.raises(apt.InvalidError):
            plan.land_mask_device(ptr(d_rows), [cap] * k, tracks0, layers, ptr(d_mask))  # nothing decoded
        plan.decode_device(ptr(d_in), [r.size for r in recs], ptr(d_rows), [cap] * k)
        res = plan.results(k)
        assert res[0].status == 0 and res[1].status == 0 and res[2].status != 0  # fewer than 10 rows of samples
        decoded = [int(r.n_out) // 2080 for r in res[:2]]
        originals = [t.clone() for t in d_rows]
        caps = [cap, decoded[1] - 5, cap]  # the second recording's buffers hold fewer rows than were decoded
        hs = [decoded[0], decoded[1] - 5]
        tracks = [lc.mm.great_circle_track(-25.0 - 8 * i, -62.0, 191.0, hs[i]) for i in range(2)] + [tracks0[0]]
        mask_p = [d_mask[0].data_ptr(), d_mask[1].data_ptr() + 3, d_mask[2].data_ptr()]
        plan.land_mask_device(ptr(d_rows), caps, tracks, layers, mask_p, None, ms)
        got = plan.land_mask_results(k)
        first = []
        for i in range(2):
            h, off = hs[i], 3 * i
            m = d_mask[i].cpu().numpy()
            assert np.all(m[:off] == 7) and np.all(m[off + h * 909:] == 7)  # nothing past the rows
            want, winfo = apt.land_mask(h, tracks[i], layers, ms)
            assert m[off:off + h * 909].tobytes() == want.tobytes(), i
            assert lc.record(got[i]) == lc.record(winfo) and got[i].height == h
            assert len(np.unique(want)) >= 2
            first.append(m.copy())
        # behind the decode that failed: refused as geolocate_device refuses it, nothing written
        assert (got[2].status, got[2].reason, got[2].height) == (1, apt.GEOLOC_REASON_DECODE, 0)
        assert lc.counts_of(got[2]) == (0, 0, 0, 0) and torch.all(d_mask[2] == 7)
        for t, o in zip(d_rows, originals):
            assert torch.equal(t, o)  # the rows are only read
        timing = plan.collect_timing()
        for name in ("image_geoloc_track", "image_geoloc_rows", "image_land_mask"):
            assert name in timing
        # a repeated call: bit for bit, and the table is not built or uploaded again
        plan.land_mask_device(ptr(d_rows), caps, tracks, layers, mask_p, None, ms)
        again = plan.land_mask_results(k)
        for i in range(2):
            assert d_mask[i].cpu().numpy().tobytes() == first[i].tobytes() and lc.record(again[i]) == lc.record(got[i])
        # fewer than two rows, and a track of another length: the record says so, the rows' pixels are invalid
        plan.land_mask_device(ptr(d_rows)[:2], [1, caps[1]], [tracks[0][:1], tracks[1][:-1]], layers, mask_p[:2], None, ms)
        rec = plan.land_mask_results(2)
        assert (rec[0].status, rec[0].reason, rec[0].height) == (1, apt.GEOLOC_REASON_HEIGHT, 1)
        assert (rec[1].status, rec[1].reason, rec[1].height) == (1, 7, hs[1])
        assert lc.counts_of(rec[0]) == (0, 0, 0, 909) and lc.counts_of(rec[1]) == (0, 0, 0, hs[1] * 909)
        assert torch.all(d_mask[0][:909] == 255) and torch.all(d_mask[1][3:3 + hs[1] * 909] == 255)
        # the orbit form, chained likewise: against the host-array orbit form
        o = orbit(TLE_2020, "NOAA 19", "end", 1580246771392 + 500 * hs[0])
        plan.land_mask_device(ptr(d_rows)[:1], caps[:1], [o], layers, mask_p[:1], lc.settings(7))
        want, winfo = apt.land_mask(hs[0], o, layers, None, lc.settings(7))
        rec = plan.land_mask_results(1)[0]
        assert d_mask[0][:hs[0] * 909].cpu().numpy().tobytes() == want.tobytes() and lc.record(rec) == lc.record(winfo)
        # refusals that need the buffers
        with pytest.raises(apt.InvalidError, match="overlaps"):
            plan.land_mask_device(ptr(d_rows)[:2], caps[:2], tracks[:2], layers, [d_rows[1].data_ptr() + 64, mask_p[1]])
        with pytest.raises(apt.InvalidError, match="overlaps"):
            plan.land_mask_device(ptr(d_rows)[:2], caps[:2], tracks[:2], layers, [mask_p[0], mask_p[0] + 909])
        plan.synchronize()
    plan.close()


@pytest.mark.parametrize("h", (1, 2, 120))
def test_colouriser(h):
    lc.check_color_model(SIDE, h)
    # three identical palettes and a mask without 255: process()'s false colour of the same rows, bit for bit
    rows = (np.random.default_rng(h).random(h * 2080) * 3000.0 + 500.0).astype(np.float32)
    pal = lc.palettes()[0]
    ctx = apt.Context(device=0)
    contrast = apt.Contrast.Percent(0.98)
    gray = apt.process(ctx, rows, contrast, rotate=apt.Rotate.NO)
    want = apt.process(ctx, rows, contrast, rotate=apt.Rotate.NO, color=apt.ColorSettings(pal, *lc.TUNES))
    mask = lc.random_mask(h, 300 + h, invalid=False)
    got = apt.false_color_masked(gray, mask, (pal, pal, pal), lc.TUNES)
    assert gray.shape == (h, 2080) and want.shape == (h, 2080, 4)
    assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:4]
    host = apt.false_color_masked_host(gray, mask, (pal, pal, pal), lc.TUNES)
    assert host.tobytes() == got.tobytes()
