"""Contrast.HISTOGRAM_FLOAT without a GPU: the numpy model (np_eqfloat_model.py) against a brute-force count of
its definition, its two forms against each other, its anchor to the reference-pinned HISTOGRAM model, the
properties of level() the threshold form rests on, and the public surface."""
import os
import re

import numpy as np
import pytest

import np_eqfloat_model as em

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_model_against_brute_force_count():
    x = em.family("special", 1, seed=3)
    x[:8] = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1.0, 1.0], f32)  # +-0, +-Inf, subnormals, a tie
    x[8:12] = np.array([0x7FC00000, 0xFFC00000, 0x7FC00001, 0xFFC00002], np.uint32).view(f32)  # NaNs, both signs
    x[em.HALF:em.HALF + 12] = x[:12]
    got = em.equalize(x)
    assert got.shape == (1, 2080)
    for lo in (0, em.HALF):
        k = em.keys(x[lo:lo + em.HALF]).astype(np.uint64)
        cum = (k[None, :] <= k[:, None]).sum(axis=1).astype(np.uint32)  # O(N^2): samples with key <= key(p)
        want = (f32(255) * (cum.astype(f32) / f32(em.HALF))).astype(np.uint8)
        assert np.array_equal(got[0, lo:lo + em.HALF], want)
    # the order itself: -NaN < -Inf < -1 < -0 < +0 < 1 < +Inf < +NaN, payloads distinct
    order = np.array([0xFFC00002, 0xFFC00000, 0xFF800000, 0xBF800000, 0x80000000, 0x00000000, 0x3F800000,
                      0x7F800000, 0x7FC00000, 0x7FC00001], np.uint32).view(f32)
    k = em.keys(order).astype(np.int64)
    assert np.all(np.diff(k) > 0)


@pytest.mark.parametrize("h", [1, 3, 64])
@pytest.mark.parametrize("name", em.FAMILIES)
def test_direct_form_equals_threshold_form(name, h):
    x = em.family(name, h, seed=11)
    t = em.thresholds(x)
    assert np.all(np.diff(t.astype(np.int64), axis=1) >= 0)
    assert np.array_equal(em.equalize(x), em.equalize_threshold(x, t))


def test_anchor_to_the_histogram_model():
    import np_color_model as cm
    for h in (1, 3, 64):
        x = em.family("integers", h, seed=5)
        for lo in (0, em.HALF):
            half = x.reshape(h, 2080)[:, lo:lo + em.HALF]
            assert half.min() == 0.0 and half.max() == 255.0
        want, lo, hi = cm.process(x, "histogram")
        assert (lo, hi) == (0.0, 255.0)
        assert np.array_equal(em.equalize(x), want)


@pytest.mark.parametrize("h", [1, 2, 255, 1198, 16132])
def test_level_is_monotone_and_ends_at_255(h):
    n = em.HALF * h
    assert (n > 1 << 24) == (h == 16132) and em.HALF * 16131 <= 1 << 24
    lv = em.level(np.arange(1, n + 1, dtype=np.uint32), n)
    assert lv[-1] == 255
    assert np.all(np.diff(lv.astype(np.int16)) >= 0)
    if h <= 255:
        c = em.ranks(n)
        assert np.all(lv[c - 1] >= np.arange(1, 256)) and np.all((c == 1) | (lv[c - 2] < np.arange(1, 256)))


def test_public_surface():
    import noaa_apt_amd as apt
    assert apt.Contrast.HISTOGRAM_FLOAT != apt.Contrast.HISTOGRAM
    assert apt.Contrast._c(apt.Contrast.HISTOGRAM_FLOAT) == (4, 0.0)
    assert apt.Contrast._c(apt.Contrast.HISTOGRAM) == (3, 0.0)
    with open(os.path.join(ROOT, "include", "aptgpu.h")) as f:
        header = f.read()
    assert re.search(r"^#define APTGPU_CONTRAST_HISTOGRAM_FLOAT 4\b", header, re.M)
    assert re.search(r"^#define APTGPU_ABI_VERSION 2\b", header, re.M)
