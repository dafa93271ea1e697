"""process() with histogram equalisation and false colour on the GPU (aptgpu_process_image,
aptgpu_plan_process_device_image), bit for bit against the numpy model of np_color_model.py on the
CPU oracle's gray image.  No tolerance anywhere."""
import ctypes as C
import os

import numpy as np
import pytest

import noaa_apt_amd as apt
import np_color_model as cm
from noaa_apt_amd.testing.synth import synth_apt

pytestmark = pytest.mark.gpu

f32 = np.float32
PALETTES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "palettes")
CONTRASTS = {"telemetry": apt.Contrast.TELEMETRY, "percent": apt.Contrast.Percent(0.98),
             "minmax": apt.Contrast.MINMAX, "histogram": apt.Contrast.HISTOGRAM}
FIRST_TEXT = {"telemetry": "Adjusting contrast from telemetry", "percent": "Adjusting contrast using 98 percent",
              "minmax": "Mapping values", "histogram": "Mapping values"}


@pytest.fixture(scope="module")
def decoded(oracle):
    """decode() output of a 3-minute synthetic pass (360 rows)."""
    return oracle.decode(synth_apt(48000, 180, seed=77), 48000, True)


@pytest.fixture(scope="module")
def palettes():
    rng = np.random.default_rng(2024)
    return {"daylight": apt.ColorSettings(os.path.join(PALETTES, "noaa-apt-daylight.png")).palette,
            "wxtoimg_no": apt.ColorSettings(os.path.join(PALETTES, "WXtoImg-NO.png")).palette,
            "random": rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)}


TUNES = {"zero": (0.0, 0.0, 0.0, 0.0), "random": (0.35, -0.6, -0.8, 0.45),
         "special": (np.nan, np.inf, -np.inf, 0.5)}


def _raw(signal, contrast, rotate=False, color=None, channels=1, percent=0.98, ctx=None):
    """aptgpu_process_image through ctypes: channels given explicitly (apt.process picks 1 or 4 itself)."""
    x = np.ascontiguousarray(signal, f32)
    kind, p = apt.Contrast._c(CONTRASTS[contrast] if contrast != "percent" else apt.Contrast.Percent(percent))
    ccol = color._c() if color is not None else None
    img, n, info = C.POINTER(C.c_uint8)(), C.c_size_t(), apt.ImageResult()
    err = C.create_string_buffer(1024)
    cctx = (ctx or apt.Context())._c()
    rc = apt.lib().aptgpu_process_image(C.byref(cctx), x.ctypes.data_as(C.POINTER(C.c_float)), x.size, kind, p,
                                        int(rotate), C.byref(ccol) if ccol is not None else None, channels,
                                        C.byref(img), C.byref(n), C.byref(info), err, 1024)
    apt.api._check(rc, err)
    out = apt.api._take(img, n.value, np.uint8)
    return (out.reshape(-1, 2080, 4) if channels == 4 else out.reshape(-1, 2080)), info


def _check(signal, contrast, rotate=False, color=None, tune=None, channels=None):
    """apt.process (or the raw entry for channels 4 without colour) == the model, limits included."""
    channels = channels or (4 if color is not None else 1)
    want, lo, hi = cm.process(signal, contrast, 0.98, rotate,
                              None if color is None else (color.palette,) + tuple(tune or (0, 0, 0, 0)), channels)
    if channels == 4 and color is None:
        got, info = _raw(signal, contrast, rotate, None, 4)
    else:
        got, info = apt.process(apt.Context(), signal, CONTRASTS[contrast], apt.Rotate.YES if rotate else apt.Rotate.NO,
                                color=color, return_info=True)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want)
    assert info.status == 0 and info.height == want.shape[0] and info.n_px == want.shape[0] * 2080
    assert f32(info.low).tobytes() == f32(lo).tobytes() and f32(info.high).tobytes() == f32(hi).tobytes()
    return got


# ------------------------------------------------------------------ histogram equalisation, gray
@pytest.mark.parametrize("channels", [1, 4])
@pytest.mark.parametrize("rotate", [False, True])
def test_histogram_decoded(oracle, decoded, channels, rotate):
    from oracle import image_binding as oi
    got = _check(decoded, "histogram", rotate, channels=channels)
    gray, _, _ = oi.process_gray(decoded, oi.CONTRAST_MINMAX)
    gray = cm.rotate(gray.reshape(-1, 2080)) if rotate else gray.reshape(-1, 2080)
    assert not np.array_equal(got if channels == 1 else got[..., 0], gray), "nothing equalised"
    seen = []
    apt.process(apt.Context(ui_callback=lambda p, t: seen.append((round(p, 2), t))), decoded,
                apt.Contrast.HISTOGRAM, apt.Rotate.YES if rotate else apt.Rotate.NO)
    assert seen == [(0.1, "Mapping values"), (0.3, "Generating image")] + ([(0.9, "Rotating output image")] if rotate else [])


def test_histogram_limits_are_minmax(decoded):
    _, info = apt.process(apt.Context(), decoded, apt.Contrast.HISTOGRAM, return_info=True)
    assert f32(info.low) == apt.get_min(decoded) and f32(info.high) == apt.get_max(decoded)


def test_histogram_edge_signals(oracle):
    rng = np.random.default_rng(11)
    specials = rng.standard_normal(40 * 2080).astype(f32) * 100
    idx = rng.choice(specials.size, 3000, replace=False)
    specials[idx[:1000]] = np.nan
    specials[idx[1000:2000]] = np.inf
    specials[idx[2000:]] = -np.inf
    nan_first = specials.copy()
    nan_first[0] = np.nan
    finite_inf = rng.standard_normal(20 * 2080).astype(f32)
    finite_inf[5] = np.inf  # range inf: every finite pixel maps to 0
    cases = {
        "constant": np.full(50 * 2080, 3.5, f32),
        "specials": specials,
        "nan_first": nan_first,
        "finite_inf": finite_inf,
        "one_row": rng.standard_normal(2080).astype(f32),
        "partial_row": rng.standard_normal(7 * 2080 + 1234).astype(f32),
        "less_than_a_row": rng.standard_normal(1500).astype(f32),
    }
    for name, sig in cases.items():
        for rotate in (False, True):
            for channels in (1, 4):
                got = _check(sig, "histogram", rotate, channels=channels)
                assert got.shape[0] == sig.size // 2080, name
    assert np.all(_check(cases["constant"], "histogram") == 255)


def test_histogram_zero_length():
    for contrast in ("histogram", "minmax"):
        with pytest.raises(apt.InternalError, match="^Can't get minimum of a zero length vector$"):
            _raw(np.zeros(0, f32), contrast)
    with pytest.raises(apt.InternalError, match="^Can't get minimum of a zero length vector$"):
        apt.process(apt.Context(), np.zeros(0, f32), apt.Contrast.HISTOGRAM)


def test_histogram_past_2_24_pixels_per_half(oracle):
    """16 200 rows: a half holds 16.8 M pixels > 2^24, so `cum[v] as f32` and `total` round."""
    rng = np.random.default_rng(16200)
    sig = (rng.standard_normal(16200 * 2080) * 40).astype(f32)
    got = _check(sig, "histogram")
    # the f32 rounding of the counts shows: exact (f64) counts give another image
    g, _, _ = cm.process(sig, "minmax")
    exact = g.copy()
    for lo in (0, 1040):
        h = np.bincount(g[:, lo:lo + 1040].ravel(), minlength=256).cumsum()
        exact[:, lo:lo + 1040] = np.floor(255.0 * h / h[255]).astype(np.uint8)[g[:, lo:lo + 1040]]
    assert not np.array_equal(got, exact)


# ------------------------------------------------------------------ false colour
@pytest.mark.parametrize("contrast", ["telemetry", "percent", "minmax"])
@pytest.mark.parametrize("rotate", [False, True])
def test_false_color(decoded, palettes, contrast, rotate):
    for pkey, pal in palettes.items():
        for tkey, tune in TUNES.items():
            color = apt.ColorSettings(pal, *tune)
            got = _check(decoded, contrast, rotate, color=color, tune=tune)
            assert got.shape == (decoded.size // 2080, 2080, 4) and np.all(got[..., 3] == 255), (pkey, tkey)


def test_false_color_fixture_paths_and_statuses(decoded):
    color = apt.ColorSettings(os.path.join(PALETTES, "noaa-apt-daylight.png"), 0.1, 0.9, -0.2, 0.3)
    seen = []
    img = apt.process(apt.Context(ui_callback=lambda p, t: seen.append((round(p, 2), t))), decoded,
                      apt.Contrast.TELEMETRY, apt.Rotate.YES, color=color)
    assert seen == [(0.1, FIRST_TEXT["telemetry"]), (0.3, "Generating image"), (0.9, "Rotating output image")]
    want, _, _ = cm.process(decoded, "telemetry", rotated=True, color=(color.palette, 0.1, 0.9, -0.2, 0.3))
    assert np.array_equal(img, want)


def test_false_color_edge_signals(palettes):
    rng = np.random.default_rng(12)
    sig = rng.standard_normal(30 * 2080 + 77).astype(f32)
    sig[rng.choice(sig.size, 500, replace=False)] = np.nan
    sig[rng.choice(sig.size, 500, replace=False)] = np.inf
    for rotate in (False, True):
        for tune in TUNES.values():
            color = apt.ColorSettings(palettes["random"], *tune)
            _check(sig, "percent", rotate, color=color, tune=tune)
            _check(sig[:2080], "minmax", rotate, color=color, tune=tune)


# ------------------------------------------------------------------ refusals
def test_refusals(decoded, palettes):
    color = apt.ColorSettings(palettes["daylight"])
    seen = []
    ctx = apt.Context(ui_callback=lambda p, t: seen.append(t))
    with pytest.raises(apt.UnsupportedError):
        apt.process(ctx, decoded, apt.Contrast.HISTOGRAM, color=color)
    with pytest.raises(apt.UnsupportedError):
        _raw(decoded, "histogram", color=color, channels=4, ctx=ctx)
    with pytest.raises(apt.UnsupportedError):
        apt.process(ctx, decoded, apt.Contrast.HISTOGRAM, rotate=apt.Rotate.ORBIT)
    with pytest.raises(apt.UnsupportedError):
        apt.process(ctx, decoded, apt.Contrast.MINMAX, rotate=apt.Rotate.ORBIT, color=color)
    with pytest.raises(apt.UnsupportedError):
        apt.process(ctx, decoded, apt.Contrast.HISTOGRAM, color=object())
    assert seen == []
    with pytest.raises(apt.InvalidError):
        _raw(decoded, "minmax", color=color, channels=1)
    with pytest.raises(apt.InvalidError):
        _raw(decoded, "minmax", channels=3)
    assert seen == []
    with pytest.raises(apt.InvalidInputError, match="^Could not load "):
        apt.process(ctx, decoded, apt.Contrast.MINMAX, color=apt.ColorSettings(os.path.join(PALETTES, "none.png")))
    # the existing gray entry keeps refusing Histogram's code
    with pytest.raises(apt.InvalidError, match="unknown contrast"):
        x = np.ascontiguousarray(decoded, f32)
        img, n = C.POINTER(C.c_uint8)(), C.c_size_t()
        err = C.create_string_buffer(256)
        apt.api._check(apt.lib().aptgpu_process_gray(C.byref(apt.Context()._c()), x.ctypes.data_as(C.POINTER(C.c_float)),
                                                     x.size, 3, 0.0, 0, C.byref(img), C.byref(n), None, err, 256), err)


# ------------------------------------------------------------------ device-resident chain
def test_plan_decode_then_process_image_on_device(oracle, palettes):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    recs = [synth_apt(48000, 125 + 10 * i, 400 + i, ppm=10.0 * i) for i in range(3)]
    recs.append(synth_apt(48000, 30, 410))  # 60 rows: too short for telemetry
    nmax = max(r.size for r in recs)
    k = len(recs)
    tune = (0.2, -0.3, 0.4, 0.1)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        plan = apt.Plan(apt.Settings(), apt.Rate.hz(48000), True, max_samples=nmax, max_batch=k,
                        stream=stream.cuda_stream)
        plan.enable_timing(2)
        cap = int(plan.info.max_rows)
        d_in = [torch.from_numpy(r).to(dev) for r in recs]
        d_rows = [torch.empty(cap * 2080, dtype=torch.float32, device=dev) for _ in recs]
        d_gray = [torch.zeros(cap * 2080, dtype=torch.uint8, device=dev) for _ in recs]
        d_rgba = [torch.zeros(cap * 2080 * 4, dtype=torch.uint8, device=dev) for _ in recs]
        ptr = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
        for it, pkey in enumerate(("random", "daylight")):  # the second call changes the palette
            plan.decode_device(ptr(d_in), [r.size for r in recs], ptr(d_rows), [cap] * k)
            plan.process_device_image(ptr(d_rows), [cap] * k, apt.Contrast.HISTOGRAM, ptr(d_gray),
                                      rotate=apt.Rotate.YES if it else apt.Rotate.NO)
            gres = plan.image_results(k)
            plan.process_device_image(ptr(d_rows), [cap] * k, apt.Contrast.Percent(0.98), ptr(d_rgba),
                                      rotate=apt.Rotate.YES, color=apt.ColorSettings(palettes[pkey], *tune))
        res = plan.results(k)
        cres = plan.image_results(k)
        timing = plan.collect_timing()
    assert "image_equalize" in timing and "image_color" in timing and "image_minmax" in timing
    for i, r in enumerate(recs):
        rows = oracle.decode(r, 48000, True)
        h = rows.size // 2080
        assert res[i].status == 0 and res[i].n_out == rows.size
        want_g, lo, hi = cm.process(rows, "histogram", rotated=True)
        got_g = d_gray[i][:h * 2080].cpu().numpy().reshape(h, 2080)
        assert np.array_equal(got_g, want_g), i
        assert np.array_equal(got_g, apt.process(apt.Context(), rows, apt.Contrast.HISTOGRAM, apt.Rotate.YES))
        assert gres[i].status == 0 and gres[i].height == h and gres[i].n_px == h * 2080
        assert f32(gres[i].low) == lo and f32(gres[i].high) == hi
        color = apt.ColorSettings(palettes["daylight"], *tune)
        want_c, lo, hi = cm.process(rows, "percent", 0.98, True, (color.palette,) + tune)
        got_c = d_rgba[i][:h * 2080 * 4].cpu().numpy().reshape(h, 2080, 4)
        assert np.array_equal(got_c, want_c), i
        assert np.array_equal(got_c, apt.process(apt.Context(), rows, apt.Contrast.Percent(0.98), apt.Rotate.YES,
                                                 color=color))
        assert cres[i].status == 0 and cres[i].height == h and cres[i].n_px == h * 2080
        assert f32(cres[i].low) == lo and f32(cres[i].high) == hi
    # telemetry on the short recording: the record says so, nothing is written
    with torch.cuda.stream(stream):
        d_tele = [torch.zeros(cap * 2080 * 4, dtype=torch.uint8, device=dev) for _ in recs]
        plan.process_device_image(ptr(d_rows), [cap] * k, apt.Contrast.TELEMETRY, ptr(d_tele),
                                  color=apt.ColorSettings(palettes["wxtoimg_no"]))
        tres = plan.image_results(k)
    assert tres[3].status == 1 and tres[3].reason == 2 and tres[3].n_px == 0
    assert not d_tele[3].any().item()
    rows0 = oracle.decode(recs[0], 48000, True)
    want_t, _, _ = cm.process(rows0, "telemetry", color=(palettes["wxtoimg_no"], 0, 0, 0, 0))
    assert np.array_equal(d_tele[0][:want_t.size].cpu().numpy().reshape(want_t.shape), want_t)
    with pytest.raises(apt.UnsupportedError):
        plan.process_device_image(ptr(d_rows), [cap] * k, apt.Contrast.HISTOGRAM, ptr(d_rgba),
                                  color=apt.ColorSettings(palettes["daylight"]))
    with pytest.raises(apt.InvalidError):
        plan.process_device_image(ptr(d_rows), [cap] * k, apt.Contrast.MINMAX, ptr(d_gray),
                                  color=apt.ColorSettings(palettes["daylight"]), channels=1)
    plan.close()


# ------------------------------------------------------------------ mini-soak
def test_soak_random_row_images(oracle, palettes):
    cases = int(os.environ.get("APT_SOAK_CASES", "300"))
    rng = np.random.default_rng(707)
    keys = list(palettes)
    for case in range(cases):
        contrast = str(rng.choice(["telemetry", "percent", "minmax", "histogram"]))
        rotate = bool(rng.random() < 0.5)
        color = tune = None
        if contrast != "histogram" and rng.random() < 0.6:
            tune = tuple(float(v) for v in rng.uniform(-2, 2, 4))
            if rng.random() < 0.15:
                tune = (tune[0], float(rng.choice([np.nan, np.inf, -np.inf])), tune[2], tune[3])
            color = apt.ColorSettings(palettes[keys[int(rng.integers(0, len(keys)))]], *tune)
        rows = int(rng.choice([1, 2, 5, 30, 205, 260]))
        # a partial last row only where the new entry serves the call (the gray path returns all n pixels)
        extra = int(rng.integers(0, 2080)) if (color is not None or contrast == "histogram") and rng.random() < 0.2 else 0
        sig = (rng.standard_normal(rows * 2080 + extra) * rng.uniform(1, 1e4)).astype(f32)
        if rng.random() < 0.5:
            k = int(rng.integers(1, 50))
            sig[rng.integers(0, sig.size, k)] = rng.choice([np.nan, np.inf, -np.inf], k)
        try:
            want = cm.process(sig, contrast, 0.98, rotate, None if color is None else (color.palette,) + tune)
        except Exception:  # the oracle's error (telemetry on a short recording, percent without a low bucket)
            with pytest.raises(apt.AptError):
                apt.process(apt.Context(), sig, CONTRASTS[contrast], apt.Rotate.YES if rotate else apt.Rotate.NO,
                            color=color)
            continue
        got = apt.process(apt.Context(), sig, CONTRASTS[contrast], apt.Rotate.YES if rotate else apt.Rotate.NO,
                          color=color)
        assert np.array_equal(got, want[0]), (case, contrast, rotate, tune)
