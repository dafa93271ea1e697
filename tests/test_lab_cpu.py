"""aptgpu_lab_from_rgb / aptgpu_lab_to_rgb (CPU) bit for bit against np_lab_model.py, the restatement of the lab
crate 0.11.0 that the GPU's Lab equalisation is pinned to.  The host tables behind the GPU path are these two
functions' arithmetic, so this is the CPU seam of that path."""
import os

import numpy as np
import pytest

import noaa_apt_amd as apt
import np_lab_model as lm

f32 = np.float32
PALETTES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "palettes")


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _palette(name):
    from PIL import Image
    with Image.open(os.path.join(PALETTES, name)) as im:
        return np.asarray(im.convert("RGB"), np.uint8).reshape(-1, 3)


def test_from_rgb_grays_bit_exact():
    v = np.arange(256, dtype=np.uint8)
    rgb = np.stack([v, v, v], -1)
    assert np.array_equal(_bits(apt.lab_from_rgb(rgb)), _bits(lm.from_rgb(rgb)))


@pytest.mark.parametrize("name", ["noaa-apt-daylight.png", "WXtoImg-NO.png"])
def test_from_rgb_palette_colours_bit_exact(name):
    rgb = np.unique(_palette(name), axis=0)
    got = apt.lab_from_rgb(rgb)
    assert np.array_equal(_bits(got), _bits(lm.from_rgb(rgb)))
    assert np.all(got[:, 0] >= 0) and np.all(got[:, 0] <= 100)


def test_from_rgb_random_bit_exact():
    rgb = np.random.default_rng(31).integers(0, 256, (100_000, 3), dtype=np.uint8)
    got = apt.lab_from_rgb(rgb)
    assert got.shape == rgb.shape and got.dtype == f32
    assert np.array_equal(_bits(got), _bits(lm.from_rgb(rgb)))


def test_to_rgb_seeded_lab_bit_exact():
    rng = np.random.default_rng(32)
    n = 30_000
    lab = np.stack([rng.uniform(-5, 105, n), rng.uniform(-130, 130, n), rng.uniform(-130, 130, n)], -1).astype(f32)
    # and the palettes' own colours with their L replaced, as the equalisation does
    pal = lm.from_rgb(np.unique(_palette("noaa-apt-daylight.png"), axis=0)[::7])
    pal[:, 0] = rng.uniform(0, 100, pal.shape[0]).astype(f32)
    lab = np.concatenate([lab, pal, np.array([[100, 0, 0], [0, 0, 0], [np.nan, 0, 0], [50, np.inf, -np.inf]], f32)])
    assert np.array_equal(apt.lab_to_rgb(lab), lm.to_rgb(lab))


def _thresholds():
    """t[k] = the smallest non-negative f32 c with q(c) >= k, by bisection over bit patterns (model's q)."""
    lo = np.zeros(255, np.uint32)
    hi = np.full(255, 0x3F800000, np.uint32)
    k = np.arange(1, 256)
    while np.any(lo < hi):
        mid = lo + (hi - lo) // 2
        ok = lm.quantise(mid.view(f32)).astype(np.int64) >= k
        hi = np.where(ok & (lo < hi), mid, hi)
        lo = np.where(~ok & (lo < hi), mid + 1, lo)
    return lo.view(f32)


def test_quantiser_thresholds():
    t = _thresholds()
    assert np.all(np.diff(t) > 0)
    assert abs(float(t[0]) - 1.5176e-4) < 1e-7 and abs(float(t[254]) - 0.99554527) < 1e-7
    # q(t[k]) = k and q(prev(t[k])) = k - 1 through the library (gray L whose linear value is the threshold is
    # not reachable exactly, so check the model's own quantiser here and the library around it below)
    below = (t.view(np.uint32) - 1).view(f32)
    assert np.array_equal(lm.quantise(t), np.arange(1, 256)) and np.array_equal(lm.quantise(below), np.arange(255))


def test_to_rgb_near_every_threshold():
    """Lab inputs whose linear r, g or b lies within +-256 ulps of a quantiser threshold, on both sides."""
    t = _thresholds()
    rng = np.random.default_rng(33)
    # the L of a gray whose linear value crosses t[k]: bisection over L's bits (to_linear grows with L)
    lo = np.zeros(255, np.uint32)
    hi = np.full(255, np.float32(100.0).view(np.uint32), np.uint32)
    while np.any(lo < hi):
        mid = lo + (hi - lo) // 2
        lin = lm.to_linear(np.stack([mid.view(f32), np.zeros(255, f32), np.zeros(255, f32)], -1))[:, 0]
        ok = lin >= t
        hi = np.where(ok & (lo < hi), mid, hi)
        lo = np.where(~ok & (lo < hi), mid + 1, lo)
    steps = np.arange(-96, 97, dtype=np.int64)
    lbits = (lo.astype(np.int64)[:, None] + steps[None, :]).ravel()
    lbits = lbits[(lbits >= 0) & (lbits <= np.float32(100.0).view(np.uint32))].astype(np.uint32)
    l = lbits.view(f32)
    ab = np.zeros((l.size, 2), f32)
    jitter = rng.integers(0, 2, l.size).astype(bool)  # half of them with a tint, which moves g and b apart
    ab[jitter] = rng.uniform(-0.02, 0.02, (int(jitter.sum()), 2)).astype(f32)
    lab = np.concatenate([l[:, None], ab], -1)
    lin = lm.to_linear(lab)
    tb = t.view(np.uint32).astype(np.int64)
    near = np.zeros(lab.shape[0], bool)
    below = above = 0
    for ch in range(3):
        cb = lin[:, ch].view(np.uint32).astype(np.int64)
        pos = np.clip(np.searchsorted(tb, cb), 1, 254)
        j = np.where(np.abs(cb - tb[pos]) < np.abs(cb - tb[pos - 1]), pos, pos - 1)  # the nearest threshold
        hit = (lin[:, ch] > 0) & (np.abs(cb - tb[j]) <= 256)
        near |= hit
        below += int(np.sum(hit & (cb < tb[j])))
        above += int(np.sum(hit & (cb >= tb[j])))
    lab = lab[near]
    assert lab.shape[0] > 20_000 and below > 1000 and above > 1000
    assert np.array_equal(apt.lab_to_rgb(lab), lm.to_rgb(lab))


def test_anchors():
    rgb = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0], [128, 128, 128]], np.uint8)
    lab = apt.lab_from_rgb(rgb)
    want = [[53.24, 80.10, 67.20], [87.73, -86.18, 83.18], [32.30, 79.19, -107.86], [100.0, 0, 0], [0, 0, 0],
            [53.585, 0, 0]]
    assert np.allclose(lab, np.array(want, f32), atol=1e-2), lab
    assert lab[3, 0] == f32(100.0)
    assert np.array_equal(apt.lab_to_rgb(lab), rgb)


def test_gray_round_trip():
    v = np.arange(256, dtype=np.uint8)
    rgb = np.stack([v, v, v], -1)
    assert np.array_equal(apt.lab_to_rgb(apt.lab_from_rgb(rgb)), rgb)


def test_shapes_and_errors():
    assert apt.lab_from_rgb(np.zeros((0, 3), np.uint8)).shape == (0, 3)
    assert apt.lab_to_rgb(np.zeros((2, 4, 3), f32)).shape == (2, 4, 3)
    with pytest.raises(apt.InvalidError):
        apt.lab_from_rgb(np.zeros((4, 2), np.uint8))
    with pytest.raises(apt.InvalidError):
        apt.lab_to_rgb(np.zeros(5, f32))
