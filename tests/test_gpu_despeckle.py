"""The despeckle stage on the GPU (k_despeckle<1>, k_despeckle<2>) against the numpy model (np_despeckle_model.py):
every case exact, in the bits of the rows and in the count of replaced samples."""
import os

import numpy as np
import pytest

import np_despeckle_model as dm

import noaa_apt_amd as apt
from noaa_apt_amd.testing.synth import synth_apt

pytestmark = pytest.mark.gpu

f32 = np.float32
PALETTES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "palettes")


def _check(x, r, threshold, note=None):
    want, replaced, low, high, t = dm.despeckle(x, r, threshold)
    got, info = apt.despeckle(x, apt.DespeckleSettings(r, threshold), return_info=True)
    assert got.dtype == f32 and got.size == x.size, note
    diff = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert diff.size == 0, (note, diff.size, diff[:8] // 2080, diff[:8] % 2080)
    assert (info.status, info.reason, info.height, info.replaced) == (0, 0, x.size // 2080, replaced), note
    for a, b in ((info.low, low), (info.high, high), (info.t, t)):
        assert f32(a).tobytes() == f32(b).tobytes(), note
    return got, info


@pytest.mark.parametrize("threshold", [0.0, 0.05])
@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("h", [1, 2, 3, 5, 17, 64])
def test_equals_model(h, r, threshold):
    for name in dm.FAMILIES:
        _check(dm.family(name, h, seed=h + 100 * r), r, threshold, name)


@pytest.mark.parametrize("r", [1, 2])
def test_band_isolation(r):
    h = 11
    x = np.empty((h, 2080), f32)
    for i, (b0, b1) in enumerate(dm.BANDS):
        x[:, b0:b1] = 100.0 * (i + 1)
    got, info = _check(x.ravel(), r, 0.0)
    assert got.tobytes() == x.tobytes() and info.replaced == 0
    cols = (0, 38, 39, 85, 86, 994, 995, 1039, 1040, 1078, 1079, 2079)
    for row in (0, h - 1):
        y = x.copy()
        y[row, cols] = 1e6  # one impulse per column, all at once: they are at least 2 r + 1 apart or in other bands
        _check(y.ravel(), r, 0.0, ("impulses", row))
        for c in cols:      # and each on its own, wide enough to win a window's median if it leaked across a band
            y = x.copy()
            y[max(0, row - 2):row + 3, max(0, c - 2):c + 3] = 1e6
            _check(y.ravel(), r, 0.0, ("block", row, c))


def test_partial_last_row_and_short_inputs():
    x = dm.family("image", 9, seed=2, extra=517)
    assert np.all(x[9 * 2080:] == f32(1e9))
    for r, threshold in ((1, 0.0), (1, 0.05), (2, 0.05)):
        got, info = _check(x, r, threshold)
        assert got[9 * 2080:].tobytes() == x[9 * 2080:].tobytes()
        if threshold:  # the limits are those of the whole signal, tail included
            assert info.high > 1e8
    for n in (0, 1, 2079):
        x = dm.family("special", 0, seed=n, extra=n)
        got, info = _check(x, 2, 0.05)
        assert got.tobytes() == x.tobytes() and (info.low, info.high, info.t) == (0.0, 0.0, 0.0)


@pytest.mark.parametrize("r", [1, 2])
def test_nan_heavy_and_nan_limits(r):
    rng = np.random.default_rng(5)
    x = rng.standard_normal(19 * 2080).astype(f32)
    x[rng.random(x.size) < 0.55] = np.nan
    x[0] = 1.0
    med = dm.median(x.reshape(19, 2080), r)
    assert np.isnan(med).any() and (~np.isnan(med)).any()
    _check(x, r, 0.0)
    _check(x, r, 0.05)
    x = dm.family("normal", 7, seed=9)
    x[0] = np.nan  # get_min / get_max keep a NaN first sample: NaN limits, NaN t
    got, info = _check(x, r, 0.05)
    assert np.isnan(info.low) and np.isnan(info.high) and np.isnan(info.t) and info.replaced == 7 * 2080


def test_limits_are_percent_98s():
    for name, threshold in (("normal", 0.05), ("image", 0.1), ("image", 0.37)):
        x = dm.family(name, 17, seed=4)
        _, info = apt.despeckle(x, apt.DespeckleSettings(1, threshold), return_info=True)
        _, pinfo = apt.process(None, x, apt.Contrast.Percent(0.98), return_info=True)
        assert f32(info.low).tobytes() == f32(pinfo.low).tobytes()
        assert f32(info.high).tobytes() == f32(pinfo.high).tobytes()
        assert f32(info.t).tobytes() == f32(f32(threshold) * f32(f32(info.high) - f32(info.low))).tobytes()


def test_process_with_despeckle():
    x = dm.family("image", 33, seed=6)
    ds = apt.DespeckleSettings(1, 0.1)
    filtered = dm.despeckle(x, 1, 0.1)[0]
    got = apt.process(None, x, apt.Contrast.MINMAX, despeckle=ds)
    assert np.array_equal(got, apt.process(None, filtered, apt.Contrast.MINMAX))
    assert not np.array_equal(got, apt.process(None, x, apt.Contrast.MINMAX))
    color = apt.ColorSettings(os.path.join(PALETTES, "noaa-apt-daylight.png"))
    got = apt.process(None, x, apt.Contrast.Percent(0.98), apt.Rotate.YES, color=color, despeckle=ds)
    assert got.shape == (33, 2080, 4)
    assert np.array_equal(got, apt.process(None, filtered, apt.Contrast.Percent(0.98), apt.Rotate.YES, color=color))


def test_plan_path():
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    recs = [synth_apt(48000, s, 700 + i) for i, s in enumerate((6, 8, 11))]
    k = len(recs)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        plan = apt.Plan(apt.Settings(), apt.Rate.hz(48000), True, max_samples=max(r.size for r in recs), max_batch=k,
                        stream=stream.cuda_stream)
        plan.enable_timing(2)
        cap = int(plan.info.max_rows)
        d_in = [torch.from_numpy(r).to(dev) for r in recs]
        d_rows = [torch.zeros(cap * 2080, dtype=torch.float32, device=dev) for _ in recs]
        d_out = [torch.full((cap * 2080,), -7.0, dtype=torch.float32, device=dev) for _ in recs]
        rows_p, out_p = [t.data_ptr() for t in d_rows], [t.data_ptr() for t in d_out]
        with pytest.raises(apt.InvalidError):
            plan.despeckle_device(rows_p, [cap] * k, out_p)  # nothing decoded yet
        plan.decode_device([t.data_ptr() for t in d_in], [r.size for r in recs], rows_p, [cap] * k)
        res = plan.results(k)
        assert all(r.status == 0 for r in res)
        decoded = [int(r.n_out) // 2080 for r in res]
        for caps, (r, threshold) in (([cap] * k, (1, 0.1)), ([5, cap, 3], (2, 0.0)), ([cap, 1, cap], (1, 0.05))):
            heights = [min(d, c) for d, c in zip(decoded, caps)]
            for t in d_out:
                t.fill_(-7.0)
            plan.despeckle_device(rows_p, caps, out_p, apt.DespeckleSettings(r, threshold))
            d_img = [torch.zeros(cap * 2080, dtype=torch.uint8, device=dev) for _ in range(k)]
            plan.process_device_image(out_p, caps, apt.Contrast.MINMAX, [t.data_ptr() for t in d_img])
            dres = plan.despeckle_results(k)
            ires = plan.image_results(k)
            for i, h in enumerate(heights):
                src = d_rows[i][:h * 2080].cpu().numpy()
                want, replaced, low, high, t = dm.despeckle(src, r, threshold)
                got = d_out[i].cpu().numpy()
                assert got[:h * 2080].tobytes() == want.tobytes(), (caps, i)
                assert np.all(got[h * 2080:] == f32(-7.0)), (caps, i)  # nothing written past the rows
                assert (dres[i].status, dres[i].height, dres[i].replaced) == (0, h, replaced), (caps, i)
                assert f32(dres[i].t).tobytes() == f32(t).tobytes() and f32(dres[i].low).tobytes() == f32(low).tobytes()
                assert ires[i].status == 0 and ires[i].height == h
                img = d_img[i].cpu().numpy()[:h * 2080].reshape(h, 2080)
                assert np.array_equal(img, apt.process(None, want, apt.Contrast.MINMAX)), (caps, i)
        timing = plan.collect_timing()
        assert "image_despeckle" in timing and "image_percent" in timing
        # overlapping and identical buffers are refused
        with pytest.raises(apt.InvalidError, match="overlaps"):
            plan.despeckle_device(rows_p, [cap] * k, rows_p)
        with pytest.raises(apt.InvalidError, match="overlaps"):
            plan.despeckle_device(rows_p, [cap] * k, [rows_p[1] + 4 * 2080 * (cap - 1)] + out_p[1:])
        with pytest.raises(apt.InvalidError):
            plan.despeckle_device(rows_p, [cap] * k, out_p, apt.DespeckleSettings(3, 0.0))
        plan.synchronize()
    plan.close()


def test_plan_buffer_edges():
    """What the plan form accepts and refuses at the edges of the "d_out overlaps d_rows" check: d_rows[0] and the
    output are carved from one tensor, so the addresses are exact."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    recs = [synth_apt(48000, s, 700 + i) for i, s in enumerate((6, 8, 11))]
    k = len(recs)
    plan = apt.Plan(apt.Settings(), apt.Rate.hz(48000), True, max_samples=max(r.size for r in recs), max_batch=k)
    cap = int(plan.info.max_rows)
    floats = cap * 2080
    d_in = [torch.from_numpy(r).to(dev) for r in recs]
    both = torch.full((2 * floats,), -7.0, dtype=torch.float32, device=dev)  # d_rows[0], then room for an output
    d_rows = [both[:floats]] + [torch.zeros(floats, dtype=torch.float32, device=dev) for _ in recs[1:]]
    d_out = [torch.full((floats,), -7.0, dtype=torch.float32, device=dev) for _ in recs]
    rows_p, out_p = [t.data_ptr() for t in d_rows], [t.data_ptr() for t in d_out]
    assert rows_p[0] == both.data_ptr()
    plan.decode_device([t.data_ptr() for t in d_in], [r.size for r in recs], rows_p, [cap] * k)
    assert all(r.status == 0 for r in plan.results(k))
    ds = apt.DespeckleSettings(1, 0.1)
    plan.despeckle_device(rows_p, [cap] * k, out_p, ds)
    apart = plan.despeckle_results(k)
    assert all(r.status == 0 and r.height > 0 for r in apart)
    # an output that begins exactly where d_rows[0] ends: accepted, and the separate buffer's bits
    plan.despeckle_device(rows_p, [cap] * k, [rows_p[0] + 4 * floats] + out_p[1:], ds)
    adjacent = plan.despeckle_results(k)
    assert [bytes(r) for r in adjacent] == [bytes(r) for r in apart]
    assert torch.equal(both[floats:], d_out[0])
    # one float earlier: refused
    with pytest.raises(apt.InvalidError, match="overlaps"):
        plan.despeckle_device(rows_p, [cap] * k, [rows_p[0] + 4 * (floats - 1)] + out_p[1:], ds)
    # equal starts overlap even where the rows buffer is empty
    with pytest.raises(apt.InvalidError, match="overlaps"):
        plan.despeckle_device(rows_p, [cap, 0, cap], [rows_p[1]] + out_p[1:], ds)
    # two recordings may share one d_out (outputs are compared with rows only)
    plan.despeckle_device(rows_p, [cap] * k, [out_p[0], out_p[0], out_p[2]], ds)
    plan.synchronize()
    plan.close()


@pytest.mark.parametrize("n", [0, 2079])
def test_one_shot_below_one_row(n):
    """No whole row: status 0 and the input's bits, with a threshold too (the one-shot form leaves the limits launch
    out), and the host twin likewise."""
    x = dm.family("special", 0, seed=n, extra=n)
    assert x.size == n
    for fn in (apt.despeckle, apt.despeckle_host):
        got, info = fn(x, apt.DespeckleSettings(1, 0.1), return_info=True)
        assert (info.status, info.reason, info.height, info.replaced) == (0, 0, 0, 0), fn.__name__
        assert got.dtype == f32 and got.tobytes() == x.tobytes(), fn.__name__


@pytest.fixture(scope="module")
def recording(oracle):
    rows = oracle.decode(synth_apt(48000, 600, seed=7), 48000, True)
    assert rows.size // 2080 >= 1190
    rng = np.random.default_rng(3)
    rows = rows.copy()
    pops = rng.random(rows.size) < 0.005  # FM pops over the decoded rows
    rows[pops] = np.where(rng.random(int(pops.sum())) < 0.5, f32(0.0), f32(4.0) * rows.max())
    return rows


@pytest.mark.parametrize("r", [1, 2])
def test_realistic_1198_rows(recording, r):
    _, info = _check(recording, r, 0.1)
    assert 0 < info.replaced < 0.05 * recording.size
