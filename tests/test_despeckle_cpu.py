"""The despeckle stage without a GPU: the host restatement (aptgpu_despeckle_host) against the numpy model
(np_despeckle_model.py) bit for bit, the model against scipy's median filter and the oracle's percent, the refusals,
and what the stage is for: impulses go, the picture stays."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import np_despeckle_model as dm

import noaa_apt_amd as apt
from noaa_apt_amd import api

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_bits(a, b):
    return a.dtype == b.dtype == f32 and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("threshold", [0.0, 0.1])
@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("h", [1, 2, 3, 5, 17])
@pytest.mark.parametrize("name", dm.FAMILIES)
def test_host_equals_model(name, h, r, threshold):
    x = dm.family(name, h, seed=h + 10 * r)
    want, replaced, low, high, t = dm.despeckle(x, r, threshold)
    got, info = apt.despeckle_host(x, apt.DespeckleSettings(r, threshold), return_info=True)
    assert _same_bits(got, want)
    assert (info.status, info.reason, info.height, info.replaced) == (0, 0, h, replaced)
    assert f32(info.low).tobytes() == f32(low).tobytes() and f32(info.high).tobytes() == f32(high).tobytes()
    assert f32(info.t).tobytes() == f32(t).tobytes()


def test_host_partial_row_and_short_inputs():
    x = dm.family("image", 3, seed=2, extra=517)
    assert np.all(x[3 * 2080:] == f32(1e9))
    for r, threshold in ((1, 0.0), (2, 0.1)):
        want, replaced, *_ = dm.despeckle(x, r, threshold)
        got, info = apt.despeckle_host(x, apt.DespeckleSettings(r, threshold), return_info=True)
        assert _same_bits(got, want) and info.replaced == replaced and info.height == 3
        assert got[3 * 2080:].tobytes() == x[3 * 2080:].tobytes()
    for n in (0, 1, 2079):
        x = dm.family("special", 0, seed=n, extra=n)
        got, info = apt.despeckle_host(x, apt.DespeckleSettings(2, 0.1), return_info=True)
        assert _same_bits(got, x)
        assert (info.status, info.height, info.replaced, info.low, info.high, info.t) == (0, 0, 0, 0.0, 0.0, 0.0)


def test_host_nan_cases():
    # windows whose median is NaN are kept; a NaN among finite neighbours goes
    rng = np.random.default_rng(5)
    x = rng.standard_normal(9 * 2080).astype(f32)
    x[rng.random(x.size) < 0.55] = np.nan
    x[0] = 1.0
    x[4 * 2080 + 500] = np.nan
    x[4 * 2080 + 1500:4 * 2080 + 1530] = 2.0
    x[4 * 2080 + 1515] = np.nan
    for r in (1, 2):
        want, replaced, *_ = dm.despeckle(x, r, 0.0)
        med = dm.median(x.reshape(9, 2080), r)
        assert np.isnan(med).any() and (~np.isnan(med)).any()
        assert want[4 * 2080 + 1515] == 2.0
        got, info = apt.despeckle_host(x, apt.DespeckleSettings(r, 0.0), return_info=True)
        assert _same_bits(got, want) and info.replaced == replaced
    # NaN limits (a NaN first sample): t is NaN and every sample with a non-NaN median takes it
    x = dm.family("normal", 5, seed=9)
    x[0] = np.nan
    want, replaced, low, high, t = dm.despeckle(x, 1, 0.1)
    assert np.isnan(low) and np.isnan(high) and np.isnan(t) and replaced == 5 * 2080
    got, info = apt.despeckle_host(x, apt.DespeckleSettings(1, 0.1), return_info=True)
    assert _same_bits(got, want) and info.replaced == replaced and np.isnan(info.t)


def test_zero_threshold_keeps_signed_zeros_and_counts_equal_bits():
    x = np.zeros(3 * 2080, f32)
    x[::2] = -0.0
    got, info = apt.despeckle_host(x, apt.DespeckleSettings(1, 0.0), return_info=True)
    assert _same_bits(got, x) and info.replaced == 0
    x = np.full(3 * 2080, np.inf, f32)  # Inf - Inf is NaN: the rule picks med, whose bits equal x's
    want, replaced, *_ = dm.despeckle(x, 1, 0.0)
    got, info = apt.despeckle_host(x, apt.DespeckleSettings(1, 0.0), return_info=True)
    assert replaced == x.size and info.replaced == replaced and _same_bits(got, x) and _same_bits(want, x)


@pytest.mark.parametrize("r", [1, 2])
def test_model_equals_scipy_band_by_band(r):
    ndimage = pytest.importorskip("scipy.ndimage")
    x = dm.family("normal", 17, seed=4).reshape(17, 2080)
    want = np.empty_like(x)
    for b0, b1 in dm.BANDS:
        want[:, b0:b1] = ndimage.median_filter(x[:, b0:b1], size=2 * r + 1, mode="nearest")
    got, replaced, *_ = dm.despeckle(x, r, 0.0)
    assert np.array_equal(got.reshape(17, 2080), want)
    assert replaced == int((x != want).sum())


def test_model_percent_equals_the_oracle():
    from oracle import image_binding as oi
    for name in ("normal", "image", "special"):
        x = dm.family(name, 5, seed=3, extra=100)
        lo, hi = dm.percent(x, 0.98)
        olo, ohi = oi.percent(x, 0.98)[:2]
        assert f32(lo).tobytes() == f32(olo).tobytes() and f32(hi).tobytes() == f32(ohi).tobytes()


def test_bands_match_the_decoded_layout():
    assert dm.BANDS[0] == (0, 39) and dm.BANDS[2] == (86, 995) and dm.BANDS[6] == (1126, 2035)
    assert all(a[1] == b[0] for a, b in zip(dm.BANDS, dm.BANDS[1:])) and dm.BANDS[-1][1] == 2080
    with open(os.path.join(ROOT, "include", "aptgpu.h")) as f:
        header = f.read()
    assert "[0,39) [39,86) [86,995) [995,1040)" in header
    assert re.search(r"^#define APTGPU_ABI_VERSION 2\b", header, re.M)


@pytest.mark.parametrize("settings", [apt.DespeckleSettings(0), apt.DespeckleSettings(3), apt.DespeckleSettings(1, -1.0),
                                      apt.DespeckleSettings(1, float("nan")), apt.DespeckleSettings(-1, 0.5)])
def test_refusals(settings):
    x = dm.family("normal", 2)
    with pytest.raises(apt.InvalidError):
        apt.despeckle_host(x, settings)
    with pytest.raises(apt.InvalidError):
        apt.despeckle(x, settings)  # refused before anything touches a device


def test_short_struct_size_is_refused():
    x = dm.family("normal", 2)
    xp = x.ctypes.data_as(api._f32p)
    out, info = api._f32p(), api.DespeckleResult()
    err = C.create_string_buffer(256)
    for size in (0, 8, C.sizeof(api._CDespeckleSettings) - 1):
        cs = apt.DespeckleSettings(1, 0.0)._c(struct_size=size)
        assert apt.lib().aptgpu_despeckle_host(xp, x.size, C.byref(cs), C.byref(out), C.byref(info), err, 256) == 4
        assert apt.lib().aptgpu_despeckle(None, xp, x.size, C.byref(cs), C.byref(out), C.byref(info), err, 256) == 4
        assert not out
    assert C.sizeof(api._CDespeckleSettings) == 12 and C.sizeof(api.DespeckleResult) == 40


# ------------------------------------------------------------------ what the stage is for
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_impulses_go_and_the_picture_stays(seed):
    clean, noisy, mask = dm.noisy_image(64, seed)
    n_imp = int(mask.sum())
    assert 0.008 * mask.size < n_imp < 0.012 * mask.size
    before = np.abs(noisy - clean)
    out, replaced, *_ = dm.despeckle(noisy, 1, 0.1)
    after = np.abs(out.reshape(clean.shape) - clean)
    gain = before[mask].mean(dtype=np.float64) / after[mask].mean(dtype=np.float64)
    print(f"seed {seed}: impulse error falls {gain:.1f} x, replaced / impulses = {replaced / n_imp:.3f}")
    assert gain > 50.0
    assert replaced <= 1.3 * n_imp
    out0, _, *_ = dm.despeckle(noisy, 1, 0.0)
    ratio = np.abs(out0.reshape(clean.shape) - clean).mean(dtype=np.float64) / before.mean(dtype=np.float64)
    print(f"seed {seed}: plain median, whole-image error ratio {ratio:.3f}")
    assert ratio < 0.35


def test_public_surface():
    assert apt.DespeckleSettings().radius == 1 and apt.DespeckleSettings().threshold == 0.0
    for name in ("despeckle", "despeckle_host", "DespeckleSettings", "DespeckleResult"):
        assert hasattr(apt, name)
    assert hasattr(apt.Plan, "despeckle_device") and hasattr(apt.Plan, "despeckle_results")
    import inspect
    assert inspect.signature(apt.process).parameters["despeckle"].default is None
    with pytest.raises(apt.InvalidError):
        apt.process(None, dm.family("normal", 2), apt.Contrast.MINMAX, despeckle=(1, 0.0))
