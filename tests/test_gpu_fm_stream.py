"""The streaming FM demodulator on the GPU (k_fm_stream) and the live decode from IQ.  Everything is asserted as bits
against the one-shot on the same side: fm_demodulate() of the whole recording (k_fm) for FmStream, decode() of that
audio and a LiveDecoder fed its slices for LiveIqDecoder.  The twin is compared under fm.bound, push for push.

The device-resident walks put every push's outputs into a region of their own with one canary float between
neighbours, so a write behind audio_cap of ANY push shows."""
import numpy as np
import pytest

import fm_cases as fc
import fm_stream_cases as fsc
import np_fm_model as fm

import noaa_apt_amd as apt

pytestmark = pytest.mark.gpu

f32 = np.float32
CANARY = f32(-7.25)


def tile_nv(d, t):
    """tile_of()'s nv (apt_kernels_fm.hpp), restated: the v[m] of one workgroup"""
    halo = (t + d - 1) // d
    r_max = (8192 - (d >> 3) - 1) // d
    nv = max(r_max - halo + 1, 2) if r_max > halo else 2
    vpt = 4 if nv >= 1024 else 2 if nv >= 512 else 1
    return min(nv, vpt * 256)


@pytest.fixture(scope="module")
def wanted():
    return {case: apt.fm_demodulate(fsc.cut(case).iq, fsc.cut(case).settings)[0] for case in fsc.CASES}


def device_walk(stream, iq, sizes, t, d, offset_components=0):
    """fsc.walk through push_device: the recording sits `offset_components` components behind a 256-byte aligned base,
    so chunk k begins at component offset + 2 * (frames before it)"""
    import torch
    dev = torch.device("cuda:0")
    raw = np.frombuffer(np.ascontiguousarray(iq).tobytes(), np.uint8)
    cb = iq.dtype.itemsize
    buf = torch.zeros(raw.size + 64, dtype=torch.uint8, device=dev)
    off = offset_components * cb
    if raw.size:
        buf[off:off + raw.size] = torch.from_numpy(raw.copy()).to(dev)
    total = fm.out_len(iq.size // 2, t, d)
    out = torch.full((total + len(sizes) + 32,), float(CANARY), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    bytes_before = stream.get_info().device_bytes
    spans, p, at = [], 0, 0
    for k in sizes:
        expect = fm.out_len(p + k, t, d) - fm.out_len(p, t, d)
        assert stream.out_len(k) == expect
        n = stream.push_device(buf.data_ptr() + off + 2 * p * cb, k, out.data_ptr() + 4 * at, expect)
        p += k
        assert n == expect
        fsc.check_info(stream.get_info(), p, t, d)
        spans.append((at, expect))
        at += expect + 1  # one canary between the pushes' regions
    torch.cuda.synchronize()
    a = out.cpu().numpy()
    keep = np.zeros(a.size, bool)
    for s, n in spans:
        keep[s:s + n] = True
    assert np.all(a[~keep] == CANARY), "a write behind audio_cap"
    info = stream.get_info()
    assert info.device_bytes == bytes_before and info.max_push_frames == stream.info.max_push_frames
    return a[keep].copy()


# ---------------------------------------------------------------- chunkings, as bits
@pytest.mark.parametrize("form", ("host_fed", "device_narrow", "device_aligned"))
@pytest.mark.parametrize("chunking", fsc.CHUNKINGS)
@pytest.mark.parametrize("case", fsc.CASES, ids=fsc.IDS)
def test_every_chunking_gives_the_one_shot_bits(case, chunking, form, wanted):
    r = fsc.cut(case)
    sizes = fsc.sizes_of(chunking, r.n, r.t, r.d)
    with apt.FmStream(r.settings, max_push_frames=fsc.max_push_of(chunking)) as s:
        before = s.get_info()
        if form == "host_fed":
            got = fsc.walk(s, r.iq, sizes, r.t, r.d)
        else:  # 1 component off a 16-byte boundary: component loads; on it: 16-byte loads wherever a run is aligned
            got = device_walk(s, r.iq, sizes, r.t, r.d, offset_components=1 if form == "device_narrow" else 0)
        after = s.get_info()
        assert (after.device_bytes, after.max_push_frames) == (before.device_bytes, before.max_push_frames)
    assert got.size == wanted[case].size and got.tobytes() == wanted[case].tobytes()


def test_wide_loads_on_every_run_and_on_none():
    """chunks of multiples of 8 frames from an aligned base (every whole run of the chunk is one wide load) and the same
    chunks from a base 8 bytes off (none is)"""
    case = fsc.CASES[0]
    r = fsc.cut(case)
    want, _ = apt.fm_demodulate(r.iq, r.settings)
    sizes = [8 * 500, 8 * 3, 8 * 1000, 8, r.n - 8 * 1504]
    for off in (0, 4):  # s16: 4 components = 8 bytes
        with apt.FmStream(r.settings) as s:
            assert device_walk(s, r.iq, sizes, r.t, r.d, offset_components=off).tobytes() == want.tobytes()


def test_gpu_against_twin_push_for_push():
    case = fsc.CASES[1]
    r = fsc.cut(case)
    sizes = fsc.sizes_of("random", r.n, r.t, r.d)
    with apt.FmStream(r.settings) as g, apt.FmStream(r.settings, host=True) as h:
        got, twin, p = [], [], 0
        for k in sizes:
            a, b = g.push(r.iq[2 * p:2 * (p + k)]), h.push(r.iq[2 * p:2 * (p + k)])
            p += k
            gi, hi = g.get_info(), h.get_info()
            assert a.size == b.size
            assert (gi.frames, gi.outputs, gi.carry_frames) == (hi.frames, hi.outputs, hi.carry_frames)
            got.append(a)
            twin.append(b)
    got, twin = np.concatenate(got), np.concatenate(twin)
    c = r.case
    n_out = got.size
    b, skip = fm.bound(c.info.taps, c.x_max, c.v[:n_out + 1], c.audio[:n_out], fm.gain(48000, c.settings.deviation_hz))
    err = np.abs(got.astype(np.float64) - twin.astype(np.float64))
    print(f"fm stream gpu - twin: max {err[~skip].max():.3e}, max/bound {(err[~skip] / b[~skip]).max():.4f}")
    assert skip.sum() <= 1e-3 * skip.size and np.all(err[~skip] <= b[~skip])


@pytest.mark.parametrize("delta", (-1, 0, 1))
def test_tile_seams_against_chunk_seams(delta, wanted):
    case = fsc.CASES[0]
    r = fsc.cut(case)
    k = (tile_nv(r.d, r.t) - 1) * r.d + delta
    assert 2 * k < r.n
    sizes = [k] * (r.n // k) + ([r.n % k] if r.n % k else [])
    with apt.FmStream(r.settings) as s:
        assert fsc.walk(s, r.iq, sizes, r.t, r.d).tobytes() == wanted[case].tobytes()
    with apt.FmStream(r.settings) as s:
        assert device_walk(s, r.iq, sizes, r.t, r.d).tobytes() == wanted[case].tobytes()


def test_tile_above_64_kib():
    """test_gpu_fm.test_tile_above_64_kib's settings in three pushes: k_fm_stream's dynamic-LDS limit is raised too"""
    d, fs_out = 2800, 1000
    st = apt.FmSettings(apt.IqFormat.S8, fs_out * d, d, 12345.0, channel_cutout_hz=50.0, channel_atten=21.0,
                        channel_delta_hz=800.0, deviation_hz=100.0)
    info = apt.fm_design(st)
    t = info.n_taps
    assert d < t <= 2 * d
    n = t + 4 * d + 17
    tone = fm.modulate(np.full(n, 0.4), fs_out * d, 100.0, fm.shift_used(info.pw, fs_out * d))
    iq = fm.quantize(tone, fm.S8)
    want, _ = apt.fm_demodulate(iq, st)
    assert want.size == 4
    sizes = [t + d + 3, 2 * d - 1, n - t - 3 * d - 2]
    with apt.FmStream(st) as s:
        assert fsc.walk(s, iq, sizes, t, d).tobytes() == want.tobytes()
    with apt.FmStream(st) as s:
        assert device_walk(s, iq, sizes, t, d, offset_components=3).tobytes() == want.tobytes()


@pytest.mark.parametrize("case", [fsc.CASES[0], fsc.CASES[2], fsc.CASES[3]], ids=["D5-s16", "D1-f32", "D50-u8"])
def test_short_streams(case):
    r = fsc.cut(case)
    t, d = r.t, r.d
    for n in (0, t - 1, t, t + d - 1, t + d, t + d + 1):
        iq = r.iq[:2 * n]
        with apt.FmStream(r.settings) as s:
            got = device_walk(s, iq, [n // 2, n - n // 2], t, d)
        assert got.size == fm.out_len(n, t, d)
        assert got.tobytes() == apt.fm_demodulate(iq, r.settings)[0].tobytes()


def test_non_finite_frames_at_a_seam():
    st, clean, dirty, sizes, want_nan, t, d = fsc.non_finite_recording()
    ref, _ = apt.fm_demodulate(clean, st)
    for walk in (fsc.walk, device_walk):
        with apt.FmStream(st) as s:
            got = walk(s, dirty, sizes, t, d)
        assert np.array_equal(np.isnan(got), want_nan)
        assert got[~want_nan].tobytes() == ref[~want_nan].tobytes()


def test_first_frame(wanted):
    import types
    case = fsc.CASES[1]
    r = fsc.cut(case)
    sizes = fsc.sizes_of("random", r.n, r.t, r.d)
    for ff in (1 << 32, 1 << 35):
        with apt.FmStream(r.settings, first_frame=ff) as s:
            assert device_walk(s, r.iq, sizes, r.t, r.d).tobytes() == wanted[case].tobytes()
    ff = (1 << 32) - 8 * 61 - 3  # the crossing mid-run, inside the first chunk
    c, n_out = r.case, fm.out_len(r.n, r.t, r.d)
    model = types.SimpleNamespace(settings=c.settings, info=c.info, audio=c.audio[:n_out], v=c.v[:n_out + 1], x_max=c.x_max)
    for walk in (fsc.walk, device_walk):
        with apt.FmStream(r.settings, first_frame=ff) as s:
            got = walk(s, r.iq, [4096, r.n - 4096], r.t, r.d)
        fc.check(model, got, s.rate, f"gpu first_frame=2^32-{8 * 61 + 3}")
    with apt.FmStream(r.settings, first_frame=ff) as s:  # (first_frame shifts the run grid: chunking invariance again)
        assert fsc.walk(s, r.iq, sizes, r.t, r.d).tobytes() == got.tobytes()


def test_reset_and_refusals():
    r = fsc.cut(fsc.CASES[0])
    with apt.FmStream(r.settings) as s:
        first = fsc.walk(s, r.iq, fsc.sizes_of("4096", r.n, r.t, r.d), r.t, r.d)
        s.reset()
        fsc.check_info(s.get_info(), 0, r.t, r.d)
        again = device_walk(s, r.iq, fsc.sizes_of("random", r.n, r.t, r.d), r.t, r.d)
        assert first.tobytes() == again.tobytes()
        before = s.get_info().frames
        for args, text in (((0, 4 * r.d, 256, 16), "d_iq is null"), ((256, 4 * r.d, 0, 16), "d_audio is null"),
                           ((257, 4 * r.d, 256, 16), "d_iq is not aligned"), ((256, 4 * r.d, 258, 16), "d_audio is not aligned"),
                           ((256, 4 * r.d, 256, 3), "audio_cap")):
            with pytest.raises(apt.InvalidError, match=text):
                s.push_device(*args)
            assert s.get_info().frames == before
        assert s.push_device(0, 0, 0, 0) == 0  # nothing to read or write
    with pytest.raises(apt.InvalidError, match="max_push_frames"):
        apt.FmStream(r.settings, max_push_frames=0)


# ---------------------------------------------------------------- live decode from IQ
@pytest.fixture(scope="module")
def live():
    import types
    rec = fsc.live_recording()
    audio, rate = apt.fm_demodulate(rec.iq, rec.settings)
    assert rate.get_hz() == 48000
    rows = {sync: apt.decode(apt.Context(device=0), apt.Settings(), audio, rate, sync) for sync in (True, False)}
    return types.SimpleNamespace(rec=rec, audio=audio, rows=rows)


@pytest.mark.parametrize("sync", (True, False), ids=("sync", "nosync"))
@pytest.mark.parametrize("chunking", ("quarter_second", "random", "one"))
def test_live_iq_decoder_host_fed(chunking, sync, live):
    rec = live.rec
    with apt.LiveIqDecoder(apt.Settings(), rec.settings, sync) as dec_iq, \
            apt.LiveDecoder(apt.Settings(), apt.Rate.hz(48000), sync) as dec:
        rows = fsc.live_against_decoder(dec_iq, dec, live.audio, rec, fsc.live_sizes(chunking, rec.n))
    assert rows.reshape(-1).tobytes() == live.rows[sync].tobytes()
    if sync:
        assert rows.shape == (14, 2080)


def test_live_iq_decoder_over_max_push_frames(live):
    rec = live.rec
    with apt.LiveIqDecoder(apt.Settings(), rec.settings, True, max_push_frames=100000, max_push=4096) as dec_iq, \
            apt.LiveDecoder(apt.Settings(), apt.Rate.hz(48000), True) as dec:
        rows = fsc.live_against_decoder(dec_iq, dec, live.audio, rec, [rec.n // 3, rec.n - rec.n // 3])
    assert rows.reshape(-1).tobytes() == live.rows[True].tobytes()


def test_live_iq_decoder_device_resident(live):
    """push_device / finish_device with rows_cap exactly rows_bound and a sentinel row behind it, no synchronisation
    between the pushes, results() at the end: the rows and positions of a LiveDecoder fed the one-shot's audio"""
    import torch
    rec = live.rec
    dev = torch.device("cuda:0")
    sizes = fsc.live_sizes("quarter_second", rec.n)
    stream = torch.cuda.Stream(device=dev)
    with apt.LiveDecoder(apt.Settings(), apt.Rate.hz(48000), True) as dec:
        want_rows, want_pos = [], []
        p = 0
        for k in sizes:
            a0, a1 = fm.out_len(p, rec.t, rec.d), fm.out_len(p + k, rec.t, rec.d)
            rws, pos = dec.push(live.audio[a0:a1])
            p += k
            want_rows.append(rws)
            want_pos.append(pos)
        rws, pos = dec.finish()
        want_rows.append(rws)
        want_pos.append(pos)
        want_record = fsc.record_of(dec.result)
    with torch.cuda.stream(stream):
        d_iq = torch.from_numpy(rec.iq.view(np.uint8).copy()).to(dev)
        with apt.LiveIqDecoder(apt.Settings(), rec.settings, True, context=apt.Context(device=0, stream=stream.cuda_stream)) as dec_iq:
            with pytest.raises(apt.InvalidError, match="rows_cap"):  # refused before anything is consumed
                dec_iq.push_device(d_iq.data_ptr(), 240000, d_iq.data_ptr(), d_iq.data_ptr(), dec_iq.rows_bound(240000) - 1)
            assert dec_iq.get_info()[0].frames == 0
            outs, p = [], 0
            for k in sizes + [None]:
                cap = dec_iq.rows_bound(k or 0)  # (host arithmetic on the frames pushed so far)
                d_rows = torch.full(((cap + 1) * 2080,), -7.0, dtype=torch.float32, device=dev)  # on `stream`, like the push
                d_pos = torch.full((cap + 1,), -1, dtype=torch.int64, device=dev)
                outs.append((d_rows, d_pos, cap))
                if k is None:
                    dec_iq.finish_device(d_rows.data_ptr(), d_pos.data_ptr(), cap)
                else:
                    dec_iq.push_device(d_iq.data_ptr() + 4 * p, k, d_rows.data_ptr(), d_pos.data_ptr(), cap)
                    p += k
            res = dec_iq.results()
            assert fsc.record_of(res) == want_record
    for (d_rows, d_pos, cap), rws, pos in zip(outs, want_rows, want_pos):
        got_pos = d_pos.cpu().numpy()
        got_rows = d_rows.cpu().numpy().reshape(cap + 1, 2080)
        n = len(pos)
        assert n <= cap and got_pos[:n].astype(np.uint64).tolist() == pos.tolist()
        assert np.all(got_pos[n:] == -1) and np.all(got_rows[n:] == f32(-7.0)), "a write behind the released rows"
        assert got_rows[:n].tobytes() == rws.tobytes()
    assert sum(len(q) for q in want_pos) == 14


def test_decode_live_iq(live):
    rec = live.rec
    sizes = fsc.live_sizes("random", rec.n)
    edges = np.concatenate([[0], np.cumsum(sizes)])
    chunks = (rec.iq[2 * a:2 * b] for a, b in zip(edges[:-1], edges[1:]))
    rows = apt.decode_live_iq(apt.Context(device=0), apt.Settings(), rec.settings, chunks, True)
    assert rows.tobytes() == live.rows[True].tobytes()


# ---------------------------------------------------------------- the C example
def test_c_example_iq_with_and_without_live(tmp_path):
    """examples/aptgpu_decode.c --iq s16:240000:5:25000: the PGM through aptgpu_iq_live_* (--live 0.25) is the PGM through
    aptgpu_fm_demodulate + aptgpu_decode, byte for byte.  The recording is 6 s long, not 3: the decode behind either path
    refuses fewer than 10 rows (two a second), so 3 s would compare two error messages."""
    import os
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "aptgpu_decode"
    libdir = os.path.dirname(apt.lib_path())
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-I", os.path.join(root, "include"), "-o", str(exe),
                           os.path.join(root, "examples", "aptgpu_decode.c"), "-L", libdir, "-laptgpu",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    rec = fsc.live_recording(6.0)
    raw = tmp_path / "pass.iq"
    raw.write_bytes(rec.iq.tobytes())
    outs = []
    for extra in ([], ["--live", "0.25"]):
        pgm = tmp_path / f"out{len(extra)}.pgm"
        r = subprocess.run([str(exe), str(raw), str(pgm), "--iq", "s16:240000:5:25000"] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert "48000 Hz audio from 240000 Hz IQ" in r.stderr
        outs.append(pgm.read_bytes())
    assert ("pushes of 0.25 s" in r.stderr) and outs[0].startswith(b"P5\n2080 ")
    assert outs[0] == outs[1]
    audio, rate = apt.fm_demodulate(rec.iq, rec.settings)
    rows = apt.decode(apt.Context(), apt.Settings(), audio, rate, True)
    header = f"P5\n2080 {rows.size // 2080}\n255\n".encode()
    assert outs[0].startswith(header)
    assert outs[0][len(header):] == apt.process(apt.Context(), rows, apt.Contrast.Percent(0.98)).tobytes()
