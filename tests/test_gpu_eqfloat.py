"""Contrast.HISTOGRAM_FLOAT on the GPU (apt_kernels_eqfloat.hip) against its numpy model (np_eqfloat_model.py): every
case exact, no tolerance.  The shapes are the smallest that still reach each way the kernels can go wrong: one to
64 rows (one workgroup to several, partial waves), inputs that make one radix level decide at a time, contention on one
counter, and one realistic 1198-row recording."""
import ctypes as C
import os

import numpy as np
import pytest

import noaa_apt_amd as apt
import np_color_model as cm
import np_eqfloat_model as em
from noaa_apt_amd.testing.synth import synth_apt

pytestmark = pytest.mark.gpu

f32 = np.float32
FLOAT = apt.Contrast.HISTOGRAM_FLOAT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHP = os.path.join(ROOT, "tests", "golden", "shapefiles")
PALETTES = os.path.join(ROOT, "tests", "golden", "palettes")


def _raw(signal, kind=4, rotate=False, color=None, channels=1, ctx=None):
    """aptgpu_process_image through ctypes: contrast code and channels given explicitly."""
    x = np.ascontiguousarray(signal, f32)
    ccol = color._c() if color is not None else None
    img, n, info = C.POINTER(C.c_uint8)(), C.c_size_t(), apt.ImageResult()
    err = C.create_string_buffer(1024)
    cctx = (ctx or apt.Context())._c()
    rc = apt.lib().aptgpu_process_image(C.byref(cctx), x.ctypes.data_as(C.POINTER(C.c_float)), x.size, kind, 0.0,
                                        int(rotate), C.byref(ccol) if ccol is not None else None, channels,
                                        C.byref(img), C.byref(n), C.byref(info), err, 1024)
    apt.api._check(rc, err)
    out = apt.api._take(img, n.value, np.uint8)
    return (out.reshape(-1, 2080, 4) if channels == 4 else out.reshape(-1, 2080)), info


def _check(signal, rotations=(False,), channel_counts=(1,)):
    """The library == the model for the given rotations and channel counts; returns the unrotated gray model."""
    want = em.equalize(signal)
    for rotate in rotations:
        for channels in channel_counts:
            got, info = _raw(signal, 4, rotate, None, channels)
            exp = cm.rgba(want) if channels == 4 else want
            exp = cm.rotate(exp) if rotate else exp
            assert got.shape == exp.shape, (got.shape, exp.shape)
            assert np.array_equal(got, exp), (rotate, channels, int((got != exp).sum()))
            assert info.status == 0 and info.height == want.shape[0] and info.n_px == want.size
    return want


# ------------------------------------------------------------------ basic inputs
@pytest.mark.parametrize("h", [1, 2, 3, 64])
@pytest.mark.parametrize("name", em.FAMILIES)
def test_families(name, h):
    x = em.family(name, h, seed=21)
    _check(x, (False, True), (1, 4))
    if h == 3:  # through the public entry too, limits as HISTOGRAM reports them
        got, info = apt.process(None, x, FLOAT, return_info=True)
        _, ref = apt.process(None, x, apt.Contrast.HISTOGRAM, return_info=True)
        assert np.array_equal(got, em.equalize(x))
        assert f32(info.low).tobytes() == f32(ref.low).tobytes() and f32(info.high).tobytes() == f32(ref.high).tobytes()


def test_partial_row():
    x = em.family("normal", 3, seed=2, extra=517)
    x[3 * 2080:] = 1e9  # would be the top of both halves if counted
    want = _check(x, (False, True), (1, 4))
    assert want.shape == (3, 2080)
    assert np.array_equal(want, em.equalize(x[:3 * 2080]))


@pytest.mark.parametrize("n", [0, 1, 2079])
def test_short_signal_is_what_histogram_does(n):
    x = em.family("normal", 1, seed=4)[:n]
    outcomes = []
    for contrast in (apt.Contrast.HISTOGRAM, FLOAT):
        try:
            img, info = apt.process(None, x, contrast, return_info=True)
            outcomes.append(("image", img.shape, img.tobytes(), info.status, info.height, info.n_px))
        except apt.AptError as e:
            outcomes.append((type(e), str(e)))
    assert outcomes[0] == outcomes[1]


@pytest.mark.parametrize("swap", [False, True])
def test_halves_are_equalised_apart(swap):
    rng = np.random.default_rng(8)
    h = 5
    a, b = rng.standard_normal((h, 1040)).astype(f32), rng.exponential(3.0, (h, 1040)).astype(f32)
    x = np.concatenate([b, a] if swap else [a, b], axis=1).reshape(-1)
    _check(x, (False,), (1,))


# ------------------------------------------------------------------ one level deciding at a time
def _from_bits(bits, h, seed):
    rng = np.random.default_rng(seed)
    return np.asarray(bits, np.uint32)[rng.integers(0, len(bits), h * 2080)].view(f32).copy()


def test_all_samples_equal():
    want = _check(np.full(3 * 2080, 0.25, f32), (False, True), (1, 4))
    assert np.all(want == 255)


def test_two_values():
    x = _from_bits([0x3E800000, 0xC1200000], 3, 1)
    want = _check(x)
    assert len(np.unique(want)) <= 2 * 2


def test_only_bits_21_to_31_differ():
    # signed powers of two over every finite exponent: 508 values in 508 level-1 bins, so the 255 thresholds of a
    # half fall in 255 distinct ones
    e = np.arange(1, 255, dtype=np.uint32) << 23
    bits = np.concatenate([e, e | np.uint32(0x80000000)])
    assert np.all(bits & np.uint32(0x001FFFFF) == 0) and len(np.unique(bits >> 21)) == 508
    x = _from_bits(bits, 8, 2)
    _check(x)
    t = em.thresholds(x)
    assert all(len(np.unique(t[i] >> 21)) == 255 for i in (0, 1))


def test_only_bits_10_to_20_differ():
    bits = np.uint32(0x3F800000) | (np.arange(2048, dtype=np.uint32) << 10)
    _check(_from_bits(bits, 8, 3))


def test_only_bits_0_to_9_differ():
    bits = np.uint32(0xC0490000) | np.arange(1024, dtype=np.uint32)
    _check(_from_bits(bits, 8, 4))


def test_contention_on_one_counter():
    rng = np.random.default_rng(6)
    h = 64
    x = np.tile(np.repeat(rng.standard_normal(2080 // 52).astype(f32), 52), h)  # one row value across 64 rows
    x[:] = x[7]
    at = rng.choice(x.size, 300, replace=False)
    x[at] = rng.standard_normal(300).astype(f32)
    _check(x, (False, True), (1,))


def test_anchor_integer_signal_equals_histogram():
    for h in (1, 3, 64):
        x = em.family("integers", h, seed=5)
        for rotate in (apt.Rotate.NO, apt.Rotate.YES):
            assert np.array_equal(apt.process(None, x, FLOAT, rotate), apt.process(None, x, apt.Contrast.HISTOGRAM, rotate))


# ------------------------------------------------------------------ the plan path, thresholds
@pytest.fixture(scope="module")
def chain():
    """A plan behind a decode of 16 synthetic recordings of different lengths; the rows of 15 of them are then
    overwritten on the device with the input families (the decode record keeps each one's height).  decode() refuses
    a recording of fewer than 10 rows, so the heights below 10 come from a rows_cap below the decoded height: the image
    stage takes min(decoded pixels, rows_cap * 2080)."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    secs = [6, 6, 6, 6, 6, 6, 6, 8, 10, 12, 15, 18, 21, 24, 27, 33]
    small = [1, 2, 3, 5, 7, 9]
    recs = [synth_apt(48000, s, 500 + i) for i, s in enumerate(secs)]
    k = len(recs)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        plan = apt.Plan(apt.Settings(), apt.Rate.hz(48000), True, max_samples=max(r.size for r in recs), max_batch=k,
                        stream=stream.cuda_stream)
        plan.enable_timing(2)
        cap = int(plan.info.max_rows)
        d_in = [torch.from_numpy(r).to(dev) for r in recs]
        d_rows = [torch.zeros(cap * 2080, dtype=torch.float32, device=dev) for _ in recs]
        plan.decode_device([t.data_ptr() for t in d_in], [r.size for r in recs], [t.data_ptr() for t in d_rows], [cap] * k)
        res = plan.results(k)
    caps = small + [cap] * (k - len(small))
    heights = [min(int(r.n_out) // 2080, c) for r, c in zip(res, caps)]
    assert all(r.status == 0 for r in res) and min(heights) >= 1 and max(heights) <= 64 and len(set(heights)) == k
    yield {"torch": torch, "dev": dev, "stream": stream, "plan": plan, "cap": cap, "k": k, "d_rows": d_rows, "caps": caps,
           "heights": heights}
    plan.close()


def _plan_run(ch, contrast, rows, channels=1, rotate=apt.Rotate.NO, plan=None):
    """Put rows[i] (None: keep what is there) into the device buffers, run one call, return the images."""
    torch = ch["torch"]
    k, cap, caps = ch["k"], ch["cap"], ch["caps"]
    with torch.cuda.stream(ch["stream"]):
        for i, r in enumerate(rows):
            if r is not None:
                ch["d_rows"][i][:r.size].copy_(torch.from_numpy(r))
        d_img = [torch.zeros(cap * 2080 * channels, dtype=torch.uint8, device=ch["dev"]) for _ in range(k)]
        (plan or ch["plan"]).process_device_image([t.data_ptr() for t in ch["d_rows"]], caps, contrast,
                                                  [t.data_ptr() for t in d_img], rotate=rotate, channels=channels)
        info = (plan or ch["plan"]).image_results(k)
    out = []
    for i, h in enumerate(ch["heights"]):
        assert info[i].status == 0 and info[i].height == h and info[i].n_px == h * 2080
        img = d_img[i].cpu().numpy()
        assert not img[h * 2080 * channels:].any()
        out.append(img[:h * 2080 * channels].reshape((h, 2080, 4) if channels == 4 else (h, 2080)))
    return out


def _current(ch):
    return [ch["d_rows"][i][:h * 2080].cpu().numpy() for i, h in enumerate(ch["heights"])]


def test_plan_path(chain):
    ch = chain
    hs = ch["heights"]
    decoded = hs.index(max(hs))  # this one stays the decoded synth_apt
    rows = [None if i == decoded else em.family(em.FAMILIES[i % 5], h, seed=30 + i) for i, h in enumerate(hs)]
    got = _plan_run(ch, FLOAT, rows)
    sig = _current(ch)
    for i in range(ch["k"]):
        assert np.array_equal(got[i], em.equalize(sig[i])), (i, hs[i])
        assert np.array_equal(got[i], apt.process(None, sig[i], FLOAT)), (i, hs[i])
    timing = ch["plan"].collect_timing()
    assert "image_equalize_float" in timing and "image_color_float" in timing and "image_minmax" in timing
    # the thresholds of a slot, read back
    t = ch["plan"].read_internal("eqfloat_thresholds", np.uint32, 2 * 255, i=decoded).reshape(2, 255)
    assert np.array_equal(t, em.thresholds(sig[decoded]))
    # other data on the same plan (the workspace is clean again), RGBA and rotated
    rows2 = [em.family(em.FAMILIES[(i + 2) % 5], h, seed=60 + i) for i, h in enumerate(hs)]
    got2 = _plan_run(ch, FLOAT, rows2, channels=4, rotate=apt.Rotate.YES)
    for i in range(ch["k"]):
        assert np.array_equal(got2[i], em.process(rows2[i], True, 4)), (i, hs[i])
    # HISTOGRAM behind HISTOGRAM_FLOAT on the same plan == the library's HISTOGRAM
    got3 = _plan_run(ch, apt.Contrast.HISTOGRAM, [None] * ch["k"])
    for i in range(ch["k"]):
        assert np.array_equal(got3[i], apt.process(None, rows2[i], apt.Contrast.HISTOGRAM)), (i, hs[i])
    with pytest.raises(apt.InvalidError, match="unknown contrast"):
        ch["plan"].process_device([t.data_ptr() for t in ch["d_rows"]], [ch["cap"]] * ch["k"], FLOAT,
                                  [t.data_ptr() for t in ch["d_rows"]])
    with pytest.raises(apt.UnsupportedError):
        ch["plan"].process_device_image([t.data_ptr() for t in ch["d_rows"]], [ch["cap"]] * ch["k"], FLOAT,
                                        [t.data_ptr() for t in ch["d_rows"]],
                                        color=apt.ColorSettings(os.path.join(PALETTES, "noaa-apt-daylight.png")))


def test_thresholds_at_64_rows(chain):
    ch = chain
    i = ch["heights"].index(max(ch["heights"]))
    rows = [None] * ch["k"]
    if ch["heights"][i] == 64:
        rows[i] = em.family("normal", 64, seed=90)
    _plan_run(ch, FLOAT, rows)
    t = ch["plan"].read_internal("eqfloat_thresholds", np.uint32, 2 * 255, i=i).reshape(2, 255)
    assert np.array_equal(t, em.thresholds(_current(ch)[i]))


def test_realistic_1198_rows(oracle):
    rows = oracle.decode(synth_apt(48000, 600, seed=7), 48000, True)
    assert rows.size // 2080 >= 1190
    got = apt.process(None, rows, FLOAT)
    want = em.equalize(rows)
    assert np.array_equal(got, want)
    for lo in (0, 1040):  # what the mode is for: every level in use
        assert len(np.unique(got[:, lo:lo + 1040])) == 256


# ------------------------------------------------------------------ downstream
def test_chaining():
    import np_map_model as mm
    from test_gpu_project import _compare, _grid
    from test_gpu_sat_track import PASSES, _decode_png
    from test_sat_cpu import orbit
    rows = 120
    sig = em.family("runs", rows, seed=12)
    gray = em.equalize(sig)
    pre = cm.rgba(gray)
    # PNG
    assert np.array_equal(_decode_png(apt.process(None, sig, FLOAT, png=True)).reshape(gray.shape), gray)
    # map overlay
    parts = {"countries": apt.read_shapefile(os.path.join(SHP, "countries.shp"), 5),
             "lakes": apt.read_shapefile(os.path.join(SHP, "lakes.shp"), 5)}
    layers = apt.MapLayers(countries=parts["countries"], lakes=parts["lakes"])
    pos = mm.great_circle_track(-52.0, -68.0, 8.0, rows)
    got = apt.process(None, sig, FLOAT, orbit=apt.MapOverlay(pos, apt.MapSettings(), layers))
    want, excused, _ = mm.overlay(pre, pos, parts, {}, {}, False)
    assert mm.compare(got, want, excused) == (0, 0)
    assert np.any(got != pre)
    # orbit: the track from the TLE, the map drawn over it
    tle, name, ms, _ = PASSES["noaa19_north"]
    o = orbit(tle, name, "end", ms + 500 * rows, apt.MapSettings())
    track = apt.sat_track(o, rows)
    got = apt.process(None, sig, FLOAT, orbit=o, layers=layers)
    want, excused, _ = mm.overlay(pre, track, parts, {}, {}, False)
    assert mm.compare(got, want, excused) == (0, 0)
    # projection
    ps = _grid(pos, apt.Projection.EQUIRECTANGULAR, 131, 77, 0.043, sampling=apt.Projection.BILINEAR)
    _compare(apt.process(None, sig, FLOAT, orbit=pos, projection=ps), gray, pos, ps, "HISTOGRAM_FLOAT")


# ------------------------------------------------------------------ refusals
def test_refusals():
    x = em.family("normal", 2, seed=1)
    seen = []
    ctx = apt.Context(ui_callback=lambda p, t: seen.append(t))
    for lab in (False, True):
        color = apt.ColorSettings(os.path.join(PALETTES, "noaa-apt-daylight.png"), equalize_lab=lab)
        with pytest.raises(apt.UnsupportedError, match="HISTOGRAM_FLOAT"):
            apt.process(ctx, x, FLOAT, color=color)
        with pytest.raises(apt.UnsupportedError, match="HISTOGRAM_FLOAT"):
            _raw(x, 4, color=color, channels=4, ctx=ctx)
    assert seen == []
    with pytest.raises(apt.InvalidError, match="unknown contrast"):
        _raw(x, 5)
    with pytest.raises(apt.InvalidError, match="unknown contrast"):
        img, n = C.POINTER(C.c_uint8)(), C.c_size_t()
        err = C.create_string_buffer(256)
        apt.api._check(apt.lib().aptgpu_process_gray(C.byref(apt.Context()._c()), x.ctypes.data_as(C.POINTER(C.c_float)),
                                                     x.size, 4, 0.0, 0, C.byref(img), C.byref(n), None, err, 256), err)
    _raw(x, 4, ctx=ctx)
    assert seen == ["Mapping values", "Generating image"]
