"""The CPU side of the PNG encoder: the numpy reader the GPU tests rely on, against Pillow-written files of every
filter type and both colour types; the ABI's symbols, struct size and refusals (all checked before the device is
touched); aptgpu_png_bound against a file of stored blocks computed here."""
import ctypes as C
import io
import os
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

import noaa_apt_amd as apt
import np_png_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _filtered_png(px, ftype):
    """A PNG of px whose every row uses filter `ftype`, built here (Pillow's writer picks its own filters, so the
    files of a given type are made by hand and Pillow is the second reader of them)."""
    px = np.ascontiguousarray(px)
    h, w = px.shape[:2]
    bpp = px.shape[2] if px.ndim == 3 else 1
    cur = px.reshape(h, w * bpp).astype(np.int64)
    up = np.vstack([np.zeros((1, w * bpp), np.int64), cur[:-1]])
    left = np.hstack([np.zeros((h, bpp), np.int64), cur[:, :-bpp]])
    upleft = np.hstack([np.zeros((h, bpp), np.int64), up[:, :-bpp]])
    pred = [np.zeros_like(cur), left, up, (left + up) >> 1, pm._paeth(left, up, upleft)][ftype]
    rows = np.hstack([np.full((h, 1), ftype, np.int64), (cur - pred) & 255]).astype(np.uint8)

    def chunk(kind, payload):
        return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload))
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 6 if bpp == 4 else 0, 0, 0, 0)
    return pm.SIGNATURE + chunk(b"IHDR", ihdr) + chunk(b"IDAT", zlib.compress(rows.tobytes())) + chunk(b"IEND", b"")


@pytest.mark.parametrize("channels", [1, 4])
def test_model_reads_every_filter_type(channels):
    rng = np.random.default_rng(7 + channels)
    shape = (23, 37) if channels == 1 else (23, 37, 4)
    smooth = (np.cumsum(rng.integers(-3, 4, shape), axis=1) & 255).astype(np.uint8)
    for px in (smooth, rng.integers(0, 256, shape, dtype=np.uint8)):
        for ftype in range(5):
            data = _filtered_png(px, ftype)
            assert np.all(pm.filter_types(data) == ftype)
            assert np.array_equal(pm.read(data), px)
            with Image.open(io.BytesIO(data)) as im:  # the file built here is a PNG Pillow agrees on
                assert np.array_equal(np.asarray(im), px)


@pytest.mark.parametrize("channels", [1, 4])
def test_model_reads_pillow_files(channels):
    rng = np.random.default_rng(70 + channels)
    rows = np.load(os.path.join(ROOT, "tests", "golden", "reference_image", "argentina_rows.npy"))[:24]
    gray = [rows, rng.integers(0, 256, (9, 300), dtype=np.uint8), np.zeros((5, 1), np.uint8),
            np.full((1, 7), 255, np.uint8)]
    for g in gray:
        px = g if channels == 1 else np.stack([g, g // 2, 255 - g, np.full_like(g, 255)], axis=-1)
        buf = io.BytesIO()
        Image.fromarray(px, "L" if channels == 1 else "RGBA").save(buf, format="PNG")
        data = buf.getvalue()
        assert np.array_equal(pm.read(data), px)
        assert pm.header(data)[:4] == (px.shape[1], px.shape[0], 8, 0 if channels == 1 else 6)


def test_model_block_walk_matches_zlib():
    rng = np.random.default_rng(5)
    raw = (np.cumsum(rng.integers(-2, 3, 40000)) & 255).astype(np.uint8).tobytes()
    for level in (0, 1, 6):
        blocks, out = pm.deflate_blocks(zlib.compress(raw, level))
        assert out == raw
        assert [b[0] for b in blocks] == [0] * (len(blocks) - 1) + [1]
        assert sum(b[2] for b in blocks) == len(raw)
    assert all(b[1] == 0 for b in pm.deflate_blocks(zlib.compress(raw, 0))[0])


def test_png_symbols_and_struct():
    lib = apt.lib()
    for name in ("aptgpu_png_bound", "aptgpu_encode_png", "aptgpu_process_image_png",
                 "aptgpu_plan_process_device_image_png"):
        assert hasattr(lib, name), name
    assert C.sizeof(apt.api._CPngSettings) == 8
    assert apt.abi_version() == 2
    # the record keeps its layout: the length lives in the former reserved field
    assert apt.ImageResult.png_bytes.offset == 36 and apt.ImageResult.png_bytes.size == 4
    assert apt.ImageResult.n_px.offset == 40 and C.sizeof(apt.ImageResult) == 176
    assert apt.PNG_REASON_CAPACITY == 9
    for name in ("encode_png", "png_bound", "process"):
        assert callable(getattr(apt, name))
    assert hasattr(apt.Plan, "png_sizes")


def _encode_raw(px, width, height, channels, settings):
    out, n = C.POINTER(C.c_uint8)(), C.c_size_t(123)
    err = C.create_string_buffer(1024)
    cctx = apt.Context()._c()
    rc = apt.lib().aptgpu_encode_png(C.byref(cctx), px.ctypes.data_as(C.POINTER(C.c_uint8)), width, height, channels,
                                     C.byref(settings) if settings is not None else None, C.byref(out), C.byref(n),
                                     err, 1024)
    return rc, bool(out), n.value, err.value.decode()


def test_png_refusals_need_no_gpu():
    px = np.zeros(64, np.uint8)
    ok = apt.api._CPngSettings(8, 0)
    for args in ((0, 4, 1, ok), (4, 0, 1, ok), (4, 4, 3, ok), (4, 4, 2, ok), (4, 4, 0, ok),
                 (4, 4, 1, apt.api._CPngSettings(8, 1)), (4, 4, 1, apt.api._CPngSettings(8, 1 << 31)),
                 (4, 4, 1, apt.api._CPngSettings(4, 0)), (4, 4, 1, apt.api._CPngSettings(0, 0)),
                 (1 << 20, 1 << 12, 4, ok)):
        rc, out, n, msg = _encode_raw(px, *args)
        assert rc == 4 and not out and n == 0 and msg, (args[:3], rc, msg)
    with pytest.raises(apt.InvalidError):
        apt.encode_png(np.zeros((4, 4, 3), np.uint8))
    with pytest.raises(apt.InvalidError):
        apt.encode_png(np.zeros((0, 4), np.uint8))
    with pytest.raises(apt.InvalidError):
        apt.encode_png(np.zeros((4, 4), np.float32))
    with pytest.raises(apt.InvalidError):
        apt.png_bound(0, 1, 1)
    with pytest.raises(apt.InvalidError):
        apt.png_bound(1, 1, 3)
    # the process entry point refuses bad PNG settings before anything else runs
    sig = np.zeros(2080, np.float32)
    img, n, info = C.POINTER(C.c_uint8)(), C.c_size_t(), apt.ImageResult()
    err = C.create_string_buffer(1024)
    cctx = apt.Context()._c()
    bad = apt.api._CPngSettings(8, 2)
    rc = apt.lib().aptgpu_process_image_png(C.byref(cctx), sig.ctypes.data_as(C.POINTER(C.c_float)), sig.size, 2, 0.0,
                                            0, None, 1, None, None, None, C.byref(bad), C.byref(img), C.byref(n),
                                            C.byref(info), err, 1024)
    assert rc == 4 and not img and n.value == 0


def test_png_bound_covers_stored_blocks():
    for width in (1, 2, 7, 300, 2080, 65535):
        for height in (1, 2, 3, 300, 1198, 3000):
            for channels in (1, 4):
                if height * (1 + width * channels) >= 1 << 31:
                    continue
                b = apt.png_bound(width, height, channels)
                assert b >= pm.stored_file_size(width, height, channels), (width, height, channels, b)
                # and not absurdly above the pixels: 5 bytes per 16 KiB chunk plus the fixed 63
                raw = height * (1 + width * channels)
                assert b <= raw + 63 + 5 * (raw // 16384 + 1)
    assert apt.png_bound(1, 1, 1) >= pm.stored_file_size(1, 1, 1) == 8 + 25 + 12 + 2 + 2 + 5 + 4 + 12
    assert apt.png_bound(2080, 3000, 4) >= pm.stored_file_size(2080, 3000, 4)
