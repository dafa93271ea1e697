"""Histogram + false colour equalised in CIE Lab on the GPU (APTGPU_COLOR_EQUALIZE_LAB / ColorSettings(equalize_lab=True)),
bit for bit against np_lab_model.py (a restatement of the lab crate 0.11.0) on the CPU oracle's gray image.
No tolerance anywhere."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import noaa_apt_amd as apt
import np_lab_model as lm
from noaa_apt_amd.testing.synth import synth_apt

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PALETTES = os.path.join(ROOT, "tests", "golden", "palettes")
TUNES = {"zero": (0.0, 0.0, 0.0, 0.0), "random": (0.35, -0.6, -0.8, 0.45),
         "special": (np.nan, np.inf, -np.inf, 0.5)}


@pytest.fixture(scope="module")
def decoded(oracle):
    """decode() output of a 3-minute synthetic pass (360 rows)."""
    return oracle.decode(synth_apt(48000, 180, seed=77), 48000, True)


@pytest.fixture(scope="module")
def palettes():
    rng = np.random.default_rng(2025)
    return {"daylight": apt.ColorSettings(os.path.join(PALETTES, "noaa-apt-daylight.png")).palette,
            "wxtoimg_no": apt.ColorSettings(os.path.join(PALETTES, "WXtoImg-NO.png")).palette,
            "random": rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)}


def _raw(signal, color, rotate=False, channels=4, flags=None, ctx=None):
    """aptgpu_process_image with APTGPU_CONTRAST_HISTOGRAM through ctypes; flags overrides the ColorSettings'."""
    x = np.ascontiguousarray(signal, f32)
    ccol = color._c()
    if flags is not None:
        ccol.flags = flags
    img, n, info = C.POINTER(C.c_uint8)(), C.c_size_t(), apt.ImageResult()
    err = C.create_string_buffer(1024)
    cctx = (ctx or apt.Context())._c()
    rc = apt.lib().aptgpu_process_image(C.byref(cctx), x.ctypes.data_as(C.POINTER(C.c_float)), x.size, 3, 0.0,
                                        int(rotate), C.byref(ccol), channels, C.byref(img), C.byref(n),
                                        C.byref(info), err, 1024)
    apt.api._check(rc, err)
    return apt.api._take(img, n.value, np.uint8).reshape(-1, 2080, 4), info


def _check(signal, palette, tune=(0.0, 0.0, 0.0, 0.0), rotate=False, raw=True):
    """apt.process and the raw entry == the model, limits included."""
    want, lo, hi = lm.process(signal, rotate, palette, tune)
    color = apt.ColorSettings(palette, *tune, equalize_lab=True)
    got, info = apt.process(apt.Context(), signal, apt.Contrast.HISTOGRAM, apt.Rotate.YES if rotate else apt.Rotate.NO,
                            color=color, return_info=True)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want)
    assert info.status == 0 and info.height == want.shape[0] and info.n_px == want.shape[0] * 2080
    assert f32(info.low).tobytes() == f32(lo).tobytes() and f32(info.high).tobytes() == f32(hi).tobytes()
    if raw:
        got_raw, _ = _raw(signal, color, rotate)
        assert np.array_equal(got_raw, want)
    return got


# ------------------------------------------------------------------ host-buffer entry
@pytest.mark.parametrize("rotate", [False, True])
@pytest.mark.parametrize("pkey", ["daylight", "wxtoimg_no", "random"])
def test_lab_decoded(decoded, palettes, pkey, rotate):
    for tkey, tune in TUNES.items():
        got = _check(decoded, palettes[pkey], tune, rotate)
        assert np.all(got[..., 3] == 255), tkey
    # the Lab path differs from both the plain false colour and the gray equalisation of channel A
    plain = apt.process(apt.Context(), decoded, apt.Contrast.Percent(0.98), color=apt.ColorSettings(palettes[pkey]))
    lab = _check(decoded, palettes[pkey])
    assert not np.array_equal(lab[:, :1040], plain[:, :1040])


def test_lab_statuses_and_zero_length(decoded, palettes):
    color = apt.ColorSettings(palettes["daylight"], equalize_lab=True)
    for rotate in (False, True):
        seen = []
        apt.process(apt.Context(ui_callback=lambda p, t: seen.append((round(p, 2), t))), decoded,
                    apt.Contrast.HISTOGRAM, apt.Rotate.YES if rotate else apt.Rotate.NO, color=color)
        assert seen == [(0.1, "Mapping values"), (0.3, "Generating image")] + (
            [(0.9, "Rotating output image")] if rotate else [])
    with pytest.raises(apt.InternalError, match="^Can't get minimum of a zero length vector$"):
        apt.process(apt.Context(), np.zeros(0, f32), apt.Contrast.HISTOGRAM, color=color)
    with pytest.raises(apt.InternalError, match="^Can't get minimum of a zero length vector$"):
        _raw(np.zeros(0, f32), color)


def test_lab_edge_signals(palettes):
    rng = np.random.default_rng(21)
    specials = (rng.standard_normal(40 * 2080) * 100).astype(f32)
    idx = rng.choice(specials.size, 3000, replace=False)
    specials[idx[:1000]] = np.nan
    specials[idx[1000:2000]] = np.inf
    specials[idx[2000:]] = -np.inf
    cases = {
        "specials": specials,
        "one_row": rng.standard_normal(2080).astype(f32),
        "partial_row": rng.standard_normal(7 * 2080 + 1234).astype(f32),
        "less_than_a_row": rng.standard_normal(1500).astype(f32),
    }
    for name, sig in cases.items():
        for rotate in (False, True):
            for pkey in ("daylight", "random"):
                got = _check(sig, palettes[pkey], TUNES["special" if rotate else "random"], rotate)
                assert got.shape[0] == sig.size // 2080, name


def test_lab_single_colour_channel_a():
    """Channel A all white (every pixel in L bin 100, so every l' = 100): it stays white."""
    rng = np.random.default_rng(22)
    rows = 30
    sig = np.empty((rows, 2080), f32)
    sig[:, :1040] = 1000.0  # above the 98 % limit: maps to 255
    sig[:, 1040:] = rng.standard_normal((rows, 1040)).astype(f32)
    pal = np.full((256, 256, 3), 255, np.uint8)
    for rotate in (False, True):
        got = _check(sig.ravel(), pal, rotate=rotate)
        assert np.all(got[:, :1040, :3] == 255)


def test_lab_past_2_24_pixels_per_half(palettes):
    """16 200 rows: a half holds 16.8 M pixels > 2^24, so `cum[bin] as f32` and the total round."""
    rng = np.random.default_rng(16201)
    sig = (rng.standard_normal(16200 * 2080) * 40).astype(f32)
    _check(sig, palettes["wxtoimg_no"], TUNES["random"], raw=False)


# ------------------------------------------------------------------ refusals
def test_lab_refusals(decoded, palettes):
    seen = []
    ctx = apt.Context(ui_callback=lambda p, t: seen.append(t))
    off = apt.ColorSettings(palettes["daylight"])
    on = apt.ColorSettings(palettes["daylight"], equalize_lab=True)
    with pytest.raises(apt.UnsupportedError, match="APTGPU_COLOR_EQUALIZE_LAB"):
        apt.process(ctx, decoded, apt.Contrast.HISTOGRAM, color=off)
    with pytest.raises(apt.UnsupportedError):
        _raw(decoded, off, ctx=ctx)
    for bits in (2, 3, 1 << 31):
        with pytest.raises(apt.InvalidError):
            _raw(decoded, on, flags=bits, ctx=ctx)
    with pytest.raises(apt.InvalidError):
        _raw(decoded, on, channels=1, ctx=ctx)
    with pytest.raises(apt.UnsupportedError):
        apt.process(ctx, decoded, apt.Contrast.HISTOGRAM, rotate=apt.Rotate.ORBIT, color=on)
    assert seen == []
    # no effect with the other contrasts
    for ca in (apt.Contrast.Percent(0.98), apt.Contrast.MINMAX, apt.Contrast.TELEMETRY):
        assert np.array_equal(apt.process(apt.Context(), decoded, ca, color=on),
                              apt.process(apt.Context(), decoded, ca, color=off))


# ------------------------------------------------------------------ device-resident chain
def test_plan_lab_on_device(oracle, palettes):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    k = 16
    recs = [synth_apt(48000, 32 + 3 * (i % 5), 500 + i, ppm=5.0 * (i % 3)) for i in range(k)]
    nmax = max(r.size for r in recs)
    tune = (0.2, -0.3, 0.4, 0.1)
    rows = [oracle.decode(r, 48000, True) for r in recs]
    stream = torch.cuda.Stream(device=dev)
    # (palette, equalize_lab, rotate): a change, the same palette twice, the flag off (plain colour) and on again
    calls = [("daylight", True, False), ("random", True, True), ("random", True, False),
             ("random", False, False), ("wxtoimg_no", True, True)]
    with torch.cuda.stream(stream):
        plan = apt.Plan(apt.Settings(), apt.Rate.hz(48000), True, max_samples=nmax, max_batch=k,
                        stream=stream.cuda_stream)
        plan.enable_timing(2)
        cap = int(plan.info.max_rows)
        d_in = [torch.from_numpy(r).to(dev) for r in recs]
        d_rows = [torch.empty(cap * 2080, dtype=torch.float32, device=dev) for _ in recs]
        d_rgba = [torch.zeros(cap * 2080 * 4, dtype=torch.uint8, device=dev) for _ in recs]
        ptr = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
        plan.decode_device(ptr(d_in), [r.size for r in recs], ptr(d_rows), [cap] * k)
        res = plan.results(k)
        for pkey, lab, rotate in calls:
            color = apt.ColorSettings(palettes[pkey], *tune, equalize_lab=lab)
            contrast = apt.Contrast.HISTOGRAM if lab else apt.Contrast.Percent(0.98)
            plan.process_device_image(ptr(d_rows), [cap] * k, contrast, ptr(d_rgba),
                                      rotate=apt.Rotate.YES if rotate else apt.Rotate.NO, color=color)
            ires = plan.image_results(k)
            for i in range(k):
                assert res[i].status == 0 and res[i].n_out == rows[i].size
                h = rows[i].size // 2080
                if lab:
                    want, lo, hi = lm.process(rows[i], rotate, palettes[pkey], tune)
                else:
                    import np_color_model as cm
                    want, lo, hi = cm.process(rows[i], "percent", 0.98, rotate, (palettes[pkey],) + tune)
                got = d_rgba[i][:h * 2080 * 4].cpu().numpy().reshape(h, 2080, 4)
                assert np.array_equal(got, want), (pkey, lab, rotate, i)
                assert ires[i].status == 0 and ires[i].height == h and ires[i].n_px == h * 2080
                assert f32(ires[i].low) == lo and f32(ires[i].high) == hi
        timing = plan.collect_timing()
        assert "image_equalize_lab" in timing and "image_color" in timing
        with pytest.raises(apt.UnsupportedError):
            plan.process_device_image(ptr(d_rows), [cap] * k, apt.Contrast.HISTOGRAM, ptr(d_rgba),
                                      color=apt.ColorSettings(palettes["daylight"]))
    plan.close()


# ------------------------------------------------------------------ the C example
def test_c_example_lab(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    from noaa_apt_amd.testing.wavfile import make_wav
    exe = tmp_path / "aptgpu_decode"
    libdir = os.path.dirname(apt.lib_path())
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                           os.path.join(ROOT, "examples", "aptgpu_decode.c"), "-L", libdir, "-laptgpu",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    x = synth_apt(11025, 130, seed=14)
    wav = tmp_path / "pass.wav"
    wav.write_bytes(make_wav(x.astype(np.int16), 11025))
    signal, _ = apt.load(str(wav))
    rows = apt.decode(apt.Context(), apt.Settings(), signal, apt.Rate.hz(11025), True)
    h = rows.size // 2080
    color = apt.ColorSettings(os.path.join(PALETTES, "noaa-apt-daylight.png"), equalize_lab=True)
    raw = tmp_path / "daylight.rgb"
    raw.write_bytes(color.palette.tobytes())
    ppm = tmp_path / "lab.ppm"
    r = subprocess.run([str(exe), str(wav), str(ppm), "--histogram", "--palette", str(raw), "--lab"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    header = f"P6\n2080 {h}\n255\n".encode()
    data = ppm.read_bytes()
    assert data.startswith(header)
    want = apt.process(apt.Context(), rows, apt.Contrast.HISTOGRAM, color=color)
    assert data[len(header):] == np.ascontiguousarray(want[..., :3]).tobytes()
    r = subprocess.run([str(exe), str(wav), str(tmp_path / "x.ppm"), "--histogram", "--palette", str(raw)],
                       capture_output=True, text=True)
    assert r.returncode == 1


# ------------------------------------------------------------------ mini-soak
def test_soak_lab_random_row_images(palettes):
    cases = int(os.environ.get("APT_SOAK_CASES", "200"))
    rng = np.random.default_rng(808)
    keys = list(palettes)
    for case in range(cases):
        rotate = bool(rng.random() < 0.5)
        tune = tuple(float(v) for v in rng.uniform(-2, 2, 4))
        if rng.random() < 0.15:
            tune = (tune[0], float(rng.choice([np.nan, np.inf, -np.inf])), tune[2], tune[3])
        pal = palettes[keys[int(rng.integers(0, len(keys)))]]
        rows = int(rng.choice([1, 2, 5, 30, 205, 260]))
        extra = int(rng.integers(0, 2080)) if rng.random() < 0.2 else 0
        sig = (rng.standard_normal(rows * 2080 + extra) * rng.uniform(1, 1e4)).astype(f32)
        if rng.random() < 0.5:
            k = int(rng.integers(1, 50))
            sig[rng.integers(0, sig.size, k)] = rng.choice([np.nan, np.inf, -np.inf], k)
        color = apt.ColorSettings(pal, *tune, equalize_lab=True)
        ro = apt.Rotate.YES if rotate else apt.Rotate.NO
        try:
            want = lm.process(sig, rotate, pal, tune)
        except Exception:  # the oracle's error (percent without a low bucket)
            with pytest.raises(apt.AptError):
                apt.process(apt.Context(), sig, apt.Contrast.HISTOGRAM, ro, color=color)
            continue
        got = apt.process(apt.Context(), sig, apt.Contrast.HISTOGRAM, ro, color=color)
        assert np.array_equal(got, want[0]), (case, rotate, tune)
