"""The numpy colour model (np_color_model.py) pinned to answers derived by hand from the reference's
arithmetic, and ColorSettings' palette loading.  CPU only."""
import os

import numpy as np
import pytest

import noaa_apt_amd as apt
import np_color_model as cm

f32 = np.float32
PALETTES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "palettes")


def test_equalize_half_and_half():
    """520 zeros and 520 x 255 in a half: cum = 520 / 1040, 255 * 0.5 = 127.5 truncates to 127."""
    row = np.zeros((1, 2080), np.uint8)
    row[0, 520:1040] = 255
    row[0, 1040:] = np.arange(1040) % 2 * 200  # half B: 520 zeros, 520 x 200
    out = cm.equalize(row)
    assert set(out[0, :520]) == {127} and set(out[0, 520:1040]) == {255}
    assert np.array_equal(out[0, 1040:], np.where(row[0, 1040:] == 0, 127, 255).astype(np.uint8))


def test_equalize_ramp_and_count_rounding():
    # one of each value in a half: cum[v] = v + 1, total = 1040 pixels of 256 values
    lut = cm.equalize_lut(np.arange(256, dtype=np.uint8))
    want = [int(f32(255.0) * (f32(v + 1) / f32(256))) for v in range(256)]
    assert lut.tolist() == want and lut[255] == 255
    # past 2^24 pixels the counts round: 2^24 + 3 zeros and one 255 -> cum[0] as f32 rounds (tie to even) up to
    # 2^24 + 4 == total, so 0 maps to 255 where exact counts give 255 * (2^24 + 3) / (2^24 + 4) -> 254
    hist_half = np.zeros(2 ** 24 + 4, np.uint8)
    hist_half[-1] = 255
    assert cm.equalize_lut(hist_half)[0] == 255
    hist_half = np.zeros(2 ** 24 + 2, np.uint8)  # 2^24 + 1 rounds down to 2^24, 2^24 + 2 is exact: 254
    hist_half[-1] = 255
    assert cm.equalize_lut(hist_half)[0] == 254


def test_constant_signal_equalises_to_white(oracle):
    """MinMax limits of a constant signal are equal: (x - low) / 0 is NaN, max(0) maps it to 0, and the
    histogram of an all-zero half puts every pixel at cum[0] == total -> 255."""
    sig = np.full(3 * 2080 + 5, 42.0, f32)
    img, lo, hi = cm.process(sig, "histogram")
    assert lo == hi == f32(42.0)
    assert img.shape == (3, 2080) and np.all(img == 255)
    gray, _, _ = cm.process(sig, "minmax")
    assert np.all(gray == 0)


def test_tune_values():
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(cm.tune(v, 0.0, 0.0), v.astype(np.uint32))  # k = 1, o = 0: identity
    # end = 1: k = 1 + 0.3f = 1.3f, 100 * 1.3f = 130.00000476... -> 130, saturating at 255
    t = cm.tune(v, 0.0, 1.0)
    assert t[100] == 130 and t[196] == 254 and t[197] == 255 and t[255] == 255
    # start = 1: k = 1 - 0.3f, o = 0.3f * 255 = 76.5: low values clamp to 0, 255 * 0.7 - 76.5 = 102
    t = cm.tune(v, 1.0, 0.0)
    assert t[0] == 0 and t[109] == 0 and t[110] == 0 and t[255] == 102
    # start = -1: k = 1.3f, o = -76.5: 0 -> 76, 138 -> 255
    t = cm.tune(v, -1.0, 0.0)
    assert t[0] == 76 and t[138] == 255
    # end = -1: k = 0.7f
    assert cm.tune(v, 0.0, -1.0)[255] == 178
    # NaN anywhere -> every value NaN -> 0
    assert not cm.tune(v, np.nan, 0.0).any() and not cm.tune(v, 0.0, np.nan).any()
    # end = +inf: 0 * inf is NaN -> 0, anything else +inf -> 255
    t = cm.tune(v, 0.0, np.inf)
    assert t[0] == 0 and np.all(t[1:] == 255)
    # end = -inf: 0 -> NaN -> 0, the rest -inf -> 0
    assert not cm.tune(v, 0.0, -np.inf).any()
    # start = +inf: k = -inf, o = +inf -> 0 everywhere; start = -inf: k = +inf, o = -inf -> 0 * inf - (-inf) is NaN
    assert not cm.tune(v, np.inf, 0.0).any()
    t = cm.tune(v, -np.inf, 0.0)
    assert t[0] == 0 and np.all(t[1:] == 255)


def test_tune_matches_scalar_f32():
    """The vectorised tune against the reference's expression evaluated one f32 operation at a time."""
    rng = np.random.default_rng(5)
    for _ in range(50):
        s, e = (f32(x) for x in rng.uniform(-3, 3, 2))
        got = cm.tune(np.arange(256), s, e)
        sp, ep = s * f32(0.3), e * f32(0.3)
        for v in range(0, 256, 17):
            out = f32(v) * ((f32(1) + ep) - sp) - sp * f32(255)
            want = 0 if np.isnan(out) else int(min(max(out, f32(0)), f32(255)))
            assert got[v] == want


def test_palette_axes():
    """palette.get_pixel(val_a, val_b): the channel-A value picks the column, channel B the row."""
    a, b = np.meshgrid(np.arange(256), np.arange(256))
    palette = np.stack([a, b, np.full_like(a, 7)], axis=2).astype(np.uint8)  # palette[b, a] = (a, b, 7)
    gray = np.zeros((2, 2080), np.uint8)
    gray[:, :1040] = 10
    gray[:, 1040:] = 200
    img = cm.false_color(gray, palette)
    assert img.shape == (2, 2080, 4)
    assert np.all(img[:, 86:995] == [10, 200, 7, 255])
    assert np.all(img[:, 85] == [10, 10, 10, 255]) and np.all(img[:, 995] == [10, 10, 10, 255])
    assert np.all(img[:, 1040:] == [200, 200, 200, 255])


def test_rotate_commutes_with_colour_and_equalisation():
    rng = np.random.default_rng(9)
    gray = rng.integers(0, 256, (7, 2080), dtype=np.uint8)
    palette = rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)
    assert np.array_equal(cm.rotate(cm.false_color(gray, palette, 0.2, -0.4, 0.5, 1.0)),
                          cm.false_color(cm.rotate(gray), palette, 0.2, -0.4, 0.5, 1.0))
    assert np.array_equal(cm.rotate(cm.equalize(gray)), cm.equalize(cm.rotate(gray)))


def test_rgba_fixture_drops_alpha():
    from PIL import Image
    path = os.path.join(PALETTES, "noaa-apt-daylight.png")
    with Image.open(path) as im:
        assert im.mode == "RGBA" and im.size == (256, 256)
        raw = np.asarray(im)
    c = apt.ColorSettings(path)
    assert c.palette.shape == (256, 256, 3) and c.palette.dtype == np.uint8
    assert np.array_equal(c.palette, raw[:, :, :3])
    assert np.array_equal(apt.ColorSettings(raw).palette, raw[:, :, :3])
    rgb = apt.ColorSettings(os.path.join(PALETTES, "WXtoImg-NO.png"), 0.1, 0.2, 0.3, 0.4)
    assert rgb.palette.shape == (256, 256, 3)
    assert (rgb.ch_a_tune_start, rgb.ch_a_tune_end, rgb.ch_b_tune_start, rgb.ch_b_tune_end) == (0.1, 0.2, 0.3, 0.4)


def test_color_settings_errors(tmp_path):
    for bad in (np.zeros((255, 256, 3), np.uint8), np.zeros((256, 256, 2), np.uint8),
                np.zeros((256, 256), np.uint8), np.zeros((256, 256, 3), np.float32)):
        with pytest.raises(apt.InvalidInputError, match="^Invalid palette image dimensions$"):
            apt.ColorSettings(bad)
    small = tmp_path / "small.png"
    from PIL import Image
    Image.new("RGB", (128, 256)).save(small)
    with pytest.raises(apt.InvalidInputError, match="^Invalid palette image dimensions$"):
        apt.ColorSettings(str(small))
    missing = tmp_path / "none.png"
    with pytest.raises(apt.InvalidInputError) as e:
        apt.ColorSettings(str(missing))
    assert str(e.value) == f'Could not load "{missing}"'
    notpng = tmp_path / "x.png"
    notpng.write_bytes(b"not an image")
    with pytest.raises(apt.InvalidInputError, match="^Could not load "):
        apt.ColorSettings(notpng)
