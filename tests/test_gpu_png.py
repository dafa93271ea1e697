"""The PNG encoder on the GPU (encode_png, process(png=True), the plan chain, the C example): every file is read back
by two independent readers, np_png_model.py (zlib + numpy) and Pillow, and must give the input bytes exactly.  No
tolerance anywhere.  The sizes of the two argentina_rows.npy files are pinned (the encoder is deterministic): a change
that makes them bigger fails, one that makes them smaller updates the record."""
import io
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest
from PIL import Image

import noaa_apt_amd as apt
import np_map_model as mm
import np_png_model as pm
from noaa_apt_amd.testing.synth import synth_apt
from noaa_apt_amd.testing.wavfile import make_wav

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PALETTES = os.path.join(ROOT, "tests", "golden", "palettes")
SHP = os.path.join(ROOT, "tests", "golden", "shapefiles")
CHUNK = 16384  # apt::png::kChunk: filtered bytes per independent deflate chunk

# Recorded file sizes for tests/golden/reference_image/argentina_rows.npy (96 x 2080): at most these, no margin.
ARGENTINA_GRAY_BYTES = 129745
ARGENTINA_RGBA_BYTES = 264645


@pytest.fixture(scope="module")
def argentina():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_image", "argentina_rows.npy"))


@pytest.fixture(scope="module")
def decoded(oracle):
    return oracle.decode(synth_apt(48000, 120, seed=91), 48000, True)


def as_rgba(gray):
    return np.ascontiguousarray(np.stack([gray, gray, gray, np.full_like(gray, 255)], axis=-1))


def check_file(data, px):
    """Both readers give px; the structure is signature, IHDR, IDAT, IEND; the file is within the bound."""
    px = np.asarray(px)
    h, w = px.shape[:2]
    channels = px.shape[2] if px.ndim == 3 else 1
    kinds = [k for k, _ in pm.chunks(data)]  # (also checks every CRC)
    assert kinds == [b"IHDR", b"IDAT", b"IEND"], kinds
    assert pm.header(data) == (w, h, 8, 6 if channels == 4 else 0, 0, 0, 0)
    z = pm.idat(data)
    assert z[0] & 15 == 8 and (z[0] * 256 + z[1]) % 31 == 0 and not z[1] & 32, "zlib header"
    got = pm.read(data)
    assert got.shape == px.reshape(got.shape).shape and np.array_equal(got, px.reshape(got.shape))
    with Image.open(io.BytesIO(data)) as im:
        assert im.mode == ("RGBA" if channels == 4 else "L") and im.size == (w, h)
        assert np.array_equal(np.asarray(im).reshape(got.shape), got)
    assert len(data) <= apt.png_bound(w, h, channels), (len(data), apt.png_bound(w, h, channels))
    return z


def check_blocks(data):
    """Walks the deflate blocks with the model's own inflater: only the last has BFINAL, no match reaches before its
    chunk.  Returns the blocks."""
    blocks, raw = pm.deflate_blocks(pm.idat(data))
    assert [b[0] for b in blocks] == [0] * (len(blocks) - 1) + [1], "BFINAL on the last block only"
    assert raw == pm.filtered(data)[0].tobytes()
    assert all(far <= CHUNK for _, _, _, far in blocks)
    return blocks


# ------------------------------------------------------------------ process(png=True)
def test_process_variants_round_trip(decoded):
    daylight = os.path.join(PALETTES, "noaa-apt-daylight.png")
    parts = {"countries": apt.read_shapefile(os.path.join(SHP, "countries.shp"), 5),
             "lakes": apt.read_shapefile(os.path.join(SHP, "lakes.shp"), 5)}
    layers = apt.MapLayers(countries=parts["countries"], lakes=parts["lakes"])
    rows = decoded.size // 2080
    overlay = apt.MapOverlay(mm.great_circle_track(-45.0, -66.0, 10.0, rows), apt.MapSettings(), layers)
    variants = {
        "gray": dict(contrast_adjustment=apt.Contrast.Percent(0.98)),
        "gray_telemetry_rotate": dict(contrast_adjustment=apt.Contrast.TELEMETRY, rotate=apt.Rotate.YES),
        "histogram": dict(contrast_adjustment=apt.Contrast.HISTOGRAM),
        "histogram_rotate": dict(contrast_adjustment=apt.Contrast.HISTOGRAM, rotate=apt.Rotate.YES),
        "colour": dict(contrast_adjustment=apt.Contrast.MINMAX, color=apt.ColorSettings(daylight)),
        "colour_rotate": dict(contrast_adjustment=apt.Contrast.Percent(0.98), rotate=apt.Rotate.YES,
                              color=apt.ColorSettings(daylight, 0.2, -0.3, 0.4, 0.1)),
        "lab": dict(contrast_adjustment=apt.Contrast.HISTOGRAM, color=apt.ColorSettings(daylight, equalize_lab=True)),
        "map_gray": dict(contrast_adjustment=apt.Contrast.MINMAX, orbit=overlay),
        "map_colour_rotate": dict(contrast_adjustment=apt.Contrast.MINMAX, orbit=overlay, rotate=apt.Rotate.YES,
                                  color=apt.ColorSettings(daylight)),
    }
    for name, kw in variants.items():
        px = apt.process(apt.Context(), decoded, **kw)
        data, info = apt.process(apt.Context(), decoded, png=True, return_info=True, **kw)
        assert isinstance(data, bytes) and info.status == 0 and info.png_bytes == len(data), name
        assert info.height == rows and info.n_px == rows * 2080
        check_file(data, px)
        assert data == apt.process(apt.Context(), decoded, png=True, **kw), name  # deterministic
    # the gray image as RGBA (channels = 4 without colour): the reference's RgbaImage of a gray decode
    gray = apt.process(apt.Context(), decoded, apt.Contrast.MINMAX)
    data = apt.api._process_image(apt.Context(), decoded, apt.Contrast.MINMAX, apt.Rotate.NO, None, False, channels=4,
                                  png=True)
    check_file(data, as_rgba(gray))
    check_blocks(data)
    # callbacks: the PNG call reports what the pixel call reports
    seen, seen_png = [], []
    apt.process(apt.Context(ui_callback=lambda p, t: seen.append((round(p, 2), t))), decoded, apt.Contrast.MINMAX)
    apt.process(apt.Context(ui_callback=lambda p, t: seen_png.append((round(p, 2), t))), decoded, apt.Contrast.MINMAX,
                png=True)
    assert seen == seen_png and seen
    # errors of the image stage come through unchanged; an image without a row cannot be a PNG
    with pytest.raises(apt.InternalError, match="^Can't get minimum of a zero length vector$"):
        apt.process(apt.Context(), np.zeros(0, np.float32), apt.Contrast.MINMAX, png=True)
    with pytest.raises(apt.InvalidError):
        apt.process(apt.Context(), np.zeros(1000, np.float32), apt.Contrast.MINMAX, png=True)


def test_argentina_round_trip_sizes_and_matcher(argentina):
    gray = apt.encode_png(argentina)
    rgba = apt.encode_png(as_rgba(argentina))
    check_file(gray, argentina)
    z = check_file(rgba, as_rgba(argentina))
    check_blocks(gray)
    # the matcher works: smaller than Huffman coding alone of the encoder's own filtered bytes
    raw = pm.filtered(rgba)[0].tobytes()
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
    huff = co.compress(raw) + co.flush()
    print(f"argentina RGBA: IDAT {len(z)} bytes, Z_HUFFMAN_ONLY {len(huff)}, level 6 {len(zlib.compress(raw, 6))}, "
          f"level 1 {len(zlib.compress(raw, 1))}; files: gray {len(gray)}, RGBA {len(rgba)}")
    assert len(z) < len(huff), (len(z), len(huff))
    # real rows are noisy: more than one filter type is in use, and each is the row's minimum-sum choice
    ftypes = pm.filter_types(gray)
    cur = argentina.astype(np.int64)
    up = np.vstack([np.zeros((1, 2080), np.int64), cur[:-1]])
    left = np.hstack([np.zeros((96, 1), np.int64), cur[:, :-1]])
    upleft = np.hstack([np.zeros((96, 1), np.int64), up[:, :-1]])
    preds = [np.zeros_like(cur), left, up, (left + up) >> 1, pm._paeth(left, up, upleft)]
    sums = np.stack([np.abs(((cur - p) & 255).astype(np.uint8).view(np.int8).astype(np.int64)).sum(axis=1)
                     for p in preds])
    assert np.array_equal(ftypes, np.argmin(sums, axis=0))  # (argmin: ties to the lower filter number)
    assert len(gray) <= ARGENTINA_GRAY_BYTES, len(gray)
    assert len(rgba) <= ARGENTINA_RGBA_BYTES, len(rgba)


# ------------------------------------------------------------------ encode_png: shapes and patterns
def _patterns(rng, h, w, channels):
    shape = (h, w) if channels == 1 else (h, w, 4)
    n = int(np.prod(shape))
    run = rng.integers(0, 256, n, dtype=np.uint8)
    run[n // 3: n // 3 + min(n, 700)] = 77
    yield "zeros", np.zeros(shape, np.uint8)
    yield "all255", np.full(shape, 255, np.uint8)
    yield "random", rng.integers(0, 256, shape, dtype=np.uint8)
    yield "long_run", run.reshape(shape)
    yield "two_pixel_period", np.resize(rng.integers(0, 256, 2 * channels, dtype=np.uint8), n).reshape(shape)
    yield "smooth", (np.cumsum(rng.integers(-2, 3, shape), axis=1) & 255).astype(np.uint8)
    yield "few_values", rng.choice(np.array([0, 1, 128, 255], np.uint8), shape)


def test_encode_shapes_and_patterns():
    rng = np.random.default_rng(11)
    # 16383 and 4095 px wide rows: with the filter byte exactly one chunk (gray) and one chunk per row (RGBA)
    shapes = [(1, 1), (1, 300), (300, 1), (7, 3), (2080, 1), (1, 2080), (37, 1001), (4, 16383), (8, 4095), (3, 20000)]
    for h, w in shapes:
        for channels in (1, 4):
            for name, px in _patterns(rng, h, w, channels):
                data = apt.encode_png(px)
                check_file(data, px)
                if h * w * channels < 40000:
                    check_blocks(data)
                assert data == apt.encode_png(px), (name, h, w, channels)
    # exact multiples of the chunk and one byte either side
    for total in (CHUNK, 2 * CHUNK, 3 * CHUNK):
        for w in (total - 1 - 1, total - 1, total):  # 1 row: filtered bytes = w + 1
            px = rng.integers(0, 4, (1, w), dtype=np.uint8)
            data = apt.encode_png(px)
            check_file(data, px)
            blocks = check_blocks(data)
            assert len(blocks) >= -(-(w + 1) // CHUNK)


def test_run_across_a_chunk_border():
    """One run longer than 258 that crosses the border between two chunks: matches stay inside their chunk."""
    rng = np.random.default_rng(12)
    px = rng.integers(0, 4, (1, 3 * CHUNK), dtype=np.uint8)  # (compressible, so the chunks are Huffman-coded)
    px[0, CHUNK - 400: CHUNK + 600] = 9  # None-filtered or Sub-filtered, the run straddles byte CHUNK
    data = apt.encode_png(px)
    check_file(data, px)
    blocks = check_blocks(data)
    assert any(far > 0 for _, _, _, far in blocks)  # the run was matched
    px4 = np.zeros((2, CHUNK // 4 + 50, 4), np.uint8)
    px4[..., 3] = 255
    data = apt.encode_png(px4)
    check_file(data, px4)
    check_blocks(data)
    assert len(data) < 1000


def test_random_image_is_stored_and_bounded():
    rng = np.random.default_rng(13)
    for shape in ((100, 2080), (40, 333, 4)):
        px = rng.integers(0, 256, shape, dtype=np.uint8)
        data = apt.encode_png(px)
        check_file(data, px)
        raw = px.size + shape[0]
        assert len(data) <= apt.png_bound(shape[1], shape[0], 1 if len(shape) == 2 else 4)
        assert len(data) >= raw  # cannot compress
        blocks = check_blocks(data) if raw < 300000 else []
        assert all(b[1] == 0 for b in blocks) and blocks  # every chunk fell back to a stored block
        assert len(data) == raw + 5 * len(blocks) + 63


# ------------------------------------------------------------------ the plan chain
def _plan_run(recs, contrast, color, channels, caps_delta=None, guard=64):
    """One decode_device + process_device_image(png=...) call; returns per recording (pixels, png bytes or None,
    record, guard bytes)."""
    import torch
    dev = torch.device("cuda", 0)
    k = len(recs)
    nmax = max(r.size for r in recs)
    plan = apt.Plan(apt.Settings(), apt.Rate.hz(48000), True, max_samples=nmax, max_batch=k)
    cap = int(plan.info.max_rows)
    d_in = [torch.from_numpy(r).to(dev) for r in recs]
    d_rows = [torch.empty(cap * 2080, dtype=torch.float32, device=dev) for _ in recs]
    d_img = [torch.zeros(cap * 2080 * channels, dtype=torch.uint8, device=dev) for _ in recs]
    bound = apt.png_bound(2080, cap, channels)
    ptr = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
    out = []
    for caps in ([bound] * k,) if caps_delta is None else caps_delta:
        d_png = [torch.full((int(c) + guard,), 0xA5, dtype=torch.uint8, device=dev) for c in caps]
        plan.decode_device(ptr(d_in), [r.size for r in recs], ptr(d_rows), [cap] * k)
        plan.process_device_image(ptr(d_rows), [cap] * k, contrast, ptr(d_img), color=color, channels=channels,
                                  png=(ptr(d_png), caps))
        res = plan.image_results(k)
        call = []
        for i in range(k):
            buf = d_png[i].cpu().numpy()
            h = res[i].height
            px = d_img[i].cpu().numpy()[:h * 2080 * channels]
            px = px.reshape(h, 2080, 4) if channels == 4 else px.reshape(h, 2080)
            data = buf[:res[i].png_bytes].tobytes() if res[i].status == 0 else None
            call.append((px.copy(), data, res[i], buf[int(caps[i]):].copy(), buf[:int(caps[i])].copy()))
        out.append(call)
    sizes_ok = None
    try:
        sizes_ok = plan.png_sizes(k)
    except apt.InternalError:
        pass
    plan.close()
    return out, sizes_ok


def test_plan_deterministic_across_slots_and_against_one_shot(oracle):
    a = synth_apt(48000, 60, seed=301)
    others = [synth_apt(48000, 40 + 5 * (i % 4), seed=310 + i) for i in range(14)]
    color = apt.ColorSettings(os.path.join(PALETTES, "noaa-apt-daylight.png"))
    for channels, col in ((1, None), (4, color)):
        (alone,), _ = _plan_run([a], apt.Contrast.MINMAX, col, channels)
        (batch,), sizes = _plan_run([a] + others + [a], apt.Contrast.MINMAX, col, channels)
        assert sizes == [len(c[1]) for c in batch]
        rows = oracle.decode(a, 48000, True)
        one_shot = apt.process(apt.Context(), rows, apt.Contrast.MINMAX, color=col, png=True)
        assert alone[0][1] == batch[0][1] == batch[15][1] == one_shot
        for px, data, rec, guard, _ in batch:
            assert rec.status == 0 and rec.png_bytes == len(data)
            check_file(data, px)
            assert np.all(guard == 0xA5)
        # the pixels are what the call without png leaves
        assert np.array_equal(batch[0][0], apt.process(apt.Context(), rows, apt.Contrast.MINMAX, color=col))


def test_plan_capacity_is_reported_not_truncated():
    recs = [synth_apt(48000, 45, seed=320), synth_apt(48000, 50, seed=321)]
    (full,), _ = _plan_run(recs, apt.Contrast.MINMAX, None, 1)
    need = [len(c[1]) for c in full]
    calls, sizes = _plan_run(recs, apt.Contrast.MINMAX, None, 1,
                             caps_delta=[[need[0] - 1, need[1]], [need[0], need[1]]])
    short, again = calls
    px, data, rec, guard, buf = short[0]
    assert rec.status == 1 and rec.reason == apt.PNG_REASON_CAPACITY and rec.png_bytes == need[0] and data is None
    assert np.all(guard == 0xA5) and np.all(buf == 0xA5)  # nothing written, inside or behind the buffer
    assert short[1][2].status == 0 and short[1][1] == full[1][1]  # the other recording is not affected
    assert np.all(short[1][3] == 0xA5)
    for i in range(2):  # the next call with enough room succeeds
        assert again[i][2].status == 0 and again[i][1] == full[i][1]
        assert np.all(again[i][3] == 0xA5)
    assert sizes == need
    # one-shot errors carry the reference-style text for the new reason
    assert apt.PNG_REASON_CAPACITY == 9


# ------------------------------------------------------------------ the C example
def test_c_example_png(tmp_path):
    assert shutil.which("gcc") is not None, "the example needs gcc"
    exe = tmp_path / "aptgpu_decode"
    libdir = os.path.dirname(apt.lib_path())
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                           os.path.join(ROOT, "examples", "aptgpu_decode.c"), "-L", libdir, "-laptgpu",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    x = synth_apt(11025, 130, seed=13)
    wav = tmp_path / "pass.wav"
    wav.write_bytes(make_wav(x.astype(np.int16), 11025))
    color = apt.ColorSettings(os.path.join(PALETTES, "noaa-apt-daylight.png"))
    raw = tmp_path / "daylight.rgb"
    raw.write_bytes(color.palette.tobytes())

    def run(out, *args):
        r = subprocess.run([str(exe), str(wav), str(out), *args], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return out.read_bytes()

    ppm = run(tmp_path / "c.ppm", "percent", "--palette", str(raw))
    png = run(tmp_path / "c.png", "percent", "--palette", str(raw), "--png")
    h = pm.header(png)[1]
    header = f"P6\n2080 {h}\n255\n".encode()
    assert ppm.startswith(header)
    want = np.frombuffer(ppm[len(header):], np.uint8).reshape(h, 2080, 3)
    px = pm.read(png)
    assert np.array_equal(px[..., :3], want) and np.all(px[..., 3] == 255)
    check_file(png, px)
    # gray, Histogram and Lab compose with --png
    pgm = run(tmp_path / "g.pgm", "--histogram")
    png = run(tmp_path / "g.png", "--histogram", "--png")
    header = f"P5\n2080 {h}\n255\n".encode()
    assert pgm.startswith(header)
    check_file(png, np.frombuffer(pgm[len(header):], np.uint8).reshape(h, 2080))
    ppm = run(tmp_path / "l.ppm", "--histogram", "--lab", "--palette", str(raw))
    png = run(tmp_path / "l.png", "--histogram", "--lab", "--palette", str(raw), "--png")
    header = f"P6\n2080 {h}\n255\n".encode()
    assert np.array_equal(pm.read(png)[..., :3], np.frombuffer(ppm[len(header):], np.uint8).reshape(h, 2080, 3))
    # the map overlay
    track = tmp_path / "track.f64"
    track.write_bytes(mm.great_circle_track(-45.0, -66.0, 10.0, h).astype(np.float64).tobytes())
    shp = tmp_path / "shp"
    shp.mkdir()
    for name in ("countries.shp", "lakes.shp"):
        shutil.copy(os.path.join(SHP, name), shp / name)
    (shp / "states.shp").write_bytes(_polyline_shp([(-70.0, -40.0), (-60.0, -35.0), (-55.0, -30.0)]))
    ppm = run(tmp_path / "m.ppm", "minmax", "--map", str(shp), "--track", str(track))
    png = run(tmp_path / "m.png", "minmax", "--map", str(shp), "--track", str(track), "--png")
    assert np.array_equal(pm.read(png)[..., :3], np.frombuffer(ppm[len(header):], np.uint8).reshape(h, 2080, 3))


def _polyline_shp(points):
    """A shapefile with one Polyline record of one part (ESRI shapefile technical description, 1998)."""
    import struct
    xs, ys = [p[0] for p in points], [p[1] for p in points]
    box = struct.pack("<4d", min(xs), min(ys), max(xs), max(ys))
    content = struct.pack("<i", 3) + box + struct.pack("<3i", 1, len(points), 0) + b"".join(
        struct.pack("<2d", *p) for p in points)
    record = struct.pack(">2i", 1, len(content) // 2) + content
    head = struct.pack(">7i", 9994, 0, 0, 0, 0, 0, (100 + len(record)) // 2) + struct.pack("<2i", 1000, 3) + box + bytes(32)
    return head + record


# ------------------------------------------------------------------ soak
def test_soak_100_images():
    rng = np.random.default_rng(2026)
    for case in range(100):
        channels = int(rng.choice([1, 4]))
        kind = case % 5
        if kind == 0:
            h, w = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        elif kind == 1:
            h, w = 1, int(rng.integers(1, 70000 // channels))
        elif kind == 2:
            h, w = int(rng.integers(1, 3000)), int(rng.integers(1, 8))
        else:
            h, w = int(rng.integers(1, 200)), int(rng.integers(1, 1200))
        pats = list(_patterns(rng, h, w, channels))
        name, px = pats[int(rng.integers(0, len(pats)))]
        if rng.random() < 0.5:  # mix two patterns by rows
            other = pats[int(rng.integers(0, len(pats)))][1]
            cut = int(rng.integers(0, h + 1))
            px = np.concatenate([px[:cut], other[cut:]], axis=0)
        data = apt.encode_png(np.ascontiguousarray(px))
        check_file(data, px)
        if px.size < 30000:
            check_blocks(data)
