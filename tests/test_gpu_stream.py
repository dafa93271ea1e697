"""Live decode on the GPU (include/aptgpu.h §4d): k_stream_front / k_stream_sync / k_stream_rows against
the oracle bit for bit, against the release schedule of np_stream_model.py after every push, and against the C++ twin
push for push; the device-resident entry points with rows_cap exactly at the bound; rings that wrap; reset."""
import numpy as np
import pytest

import stream_cases as sc

import noaa_apt_amd as apt

pytestmark = pytest.mark.gpu
f32 = np.float32


def decoder(rate, profile, sync=True, dtype=f32, max_push=None, host=False, context=None):
    return apt.LiveDecoder(sc.settings_of(profile), apt.Rate.hz(rate), sync, context=context, dtype=dtype, max_push=max_push,
                           host=host)


def run_both(kind, rate, profile, rows_x100, sync, chunking, max_push=None, dtype=f32):
    """the GPU and the twin through the same chunking: the oracle's rows, the model's schedule, the same bits per push"""
    ref = sc.reference(kind, rate, profile, rows_x100, sync)
    x = ref.x.astype(dtype)
    what = (kind, rate, profile, rows_x100, sync, chunking)
    with decoder(rate, profile, sync, dtype, max_push) as dec, decoder(rate, profile, sync, dtype, max_push, host=True) as tw:
        sizes = sc.chunk_sizes(chunking, x.size, rate, ref.g, dec.info.max_push)
        before = dec.get_info()
        calls, err = sc.run_stream(dec, x, sizes)
        assert bytes(before) == bytes(dec.get_info()), what
        twin_calls, twin_err = sc.run_stream(tw, x, sizes)
        for field in ("cap_in", "cap_f", "cap_corr", "max_push", "l", "m", "pw"):
            assert getattr(before, field) == getattr(tw.info, field), field
    sc.check_same(calls, twin_calls, what)
    assert (err is None) == (twin_err is None) and str(err) == str(twin_err), (what, err, twin_err)
    sc.check_against_reference(calls, err, ref, sizes, what)
    return calls, before, ref


@pytest.mark.parametrize("sync", (True, False))
@pytest.mark.parametrize("rate,profile", sc.RATES)
def test_every_rate_and_profile(rate, profile, sync, oracle):
    run_both("apt", rate, profile, 1237, sync, "random")


@pytest.mark.parametrize("chunking", sc.CHUNKINGS)
@pytest.mark.parametrize("rate,profile", ((11025, "standard"), (24960, "standard")))
def test_every_chunking(rate, profile, chunking, oracle):
    run_both("apt", rate, profile, 1237, True, chunking, max_push=3000 if chunking == "over_max_push" else None)


@pytest.mark.parametrize("rate,profile,sync", ((11025, "standard", True), (48000, "standard", True), (24960, "standard", False),
                                               (44100, "fast", True)))
def test_thirty_rows_through_rings_that_wrap(rate, profile, sync, oracle):
    g = sc.geometry(rate, profile)
    quarter_row = g.spr * g.m // g.l // 4
    _, info, ref = run_both("apt", rate, profile, 3050, sync, "half_second", max_push=quarter_row)
    assert info.max_push == quarter_row
    assert ref.x.size >= 3 * info.cap_in and ref.work_len >= 3 * info.cap_f


@pytest.mark.parametrize("rate,max_push", ((11025, 1 << 18), (48000, 1 << 20)))
def test_a_launch_sequence_of_thirty_rows(rate, max_push, oracle):
    calls, info, ref = run_both("apt", rate, "standard", 3050, True, "one", max_push=max_push)
    assert info.max_push == max_push > ref.x.size and calls[0][0].shape[0] >= 27


@pytest.mark.parametrize("chunking", ("one", "half_second"))
@pytest.mark.parametrize("rate,profile", sc.LOW_RATES)
def test_low_input_rates_with_the_default_max_push(rate, profile, chunking, oracle):
    run_both("apt", rate, profile, 3050, True, chunking)


@pytest.mark.parametrize("chunking", ("half_second", "one", "single_samples"))
def test_a_fading_carrier_pushes_many_peaks_at_one_event(chunking, oracle):
    ref = sc.reference("fading", 12480, "standard", 4900, True)
    assert ref.error is None and sc.most_copies(ref) >= 16
    calls, _, _ = run_both("fading", 12480, "standard", 4900, True, chunking)
    assert max(c[0].shape[0] for c in calls) >= 16


@pytest.mark.parametrize("kind", ("apt_ppm", "noise", "zeros", "constant", "nonfinite"))
@pytest.mark.parametrize("rate", (11025, 48000, 24960))
def test_signals(rate, kind, oracle):
    run_both(kind, rate, "standard", 1237, True, "4096")


@pytest.mark.parametrize("rate,profile", ((11025, "standard"), (48000, "standard"), (12480, "standard")))
def test_ten_rows_exactly_and_one_sample_less(rate, profile, oracle):
    run_both("apt", rate, profile, 1000, True, "half_second")
    calls, _, ref = run_both("apt", rate, profile, 999, True, "half_second")
    assert "less than 10 rows" in ref.error and sum(c[0].shape[0] for c in calls) >= 5  # rows handed out stay handed out


@pytest.mark.parametrize("rate", (11025, 24960))
def test_s16_samples_decode_like_their_f32_values(rate, oracle):
    a, _, _ = run_both("apt", rate, "standard", 1237, True, "4096", dtype=np.int16)
    b, _, _ = run_both("apt", rate, "standard", 1237, True, "4096")
    sc.check_same([c[:2] + (0,) for c in a], [c[:2] + (0,) for c in b], "s16")


def test_reset_reproduces_the_output(oracle):
    ref = sc.reference("apt", 48000, "standard", 1237, True)
    sizes = sc.chunk_sizes("4096", ref.x.size, 48000, ref.g)
    with decoder(48000, "standard") as dec:
        first, err = sc.run_stream(dec, ref.x, sizes)
        with pytest.raises(apt.InvalidError, match="finished"):
            dec.push(ref.x[:10])
        dec.reset()
        again, err2 = sc.run_stream(dec, ref.x, sizes)
    assert err is None and err2 is None
    sc.check_same(first, again, "reset")
    sc.check_against_reference(again, err2, ref, sizes, "after reset")


@pytest.mark.parametrize("dtype", (f32, np.int16))
@pytest.mark.parametrize("rate,sync,max_push", ((11025, True, None), (48000, True, 9000), (24960, False, 5000)))
def test_device_resident_against_host_fed(rate, sync, max_push, dtype, oracle):
    """push_device / finish_device with rows_cap exactly at rows_bound (one sentinel row behind it), one of the pushes
    longer than max_push (several launch sequences, nothing read back between them): the host-fed form's bits"""
    import torch
    ref = sc.reference("apt", rate, "standard", 1237, sync)
    x = ref.x.astype(dtype)
    sizes = sc.chunk_sizes("half_second", x.size, rate, ref.g)
    sizes = [sizes[0] + sizes[1] + sizes[2]] + sizes[3:]  # 1.5 s first: longer than the small max_push values
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    with decoder(rate, "standard", sync, dtype, max_push) as fed:
        want, want_err = sc.run_stream(fed, x, sizes)
    assert want_err is None
    calls = []
    with torch.cuda.stream(stream):
        d_x = torch.from_numpy(x.copy()).to(dev)
        with decoder(rate, "standard", sync, dtype, max_push, context=apt.Context(device=0, stream=stream.cuda_stream)) as dec:
            if max_push:
                assert sizes[0] > dec.info.max_push
            with pytest.raises(apt.InvalidError, match="rows_cap"):  # refused before anything is consumed
                dec.push_device(d_x.data_ptr(), 16, d_x.data_ptr(), d_x.data_ptr(), dec.rows_bound(16) - 1)
            at = 0
            for c in sizes + [None]:
                cap = dec.rows_bound(c or 0)
                d_rows = torch.full(((cap + 1) * 2080,), -7.0, dtype=torch.float32, device=dev)
                d_pos = torch.full((cap + 1,), -1, dtype=torch.int64, device=dev)
                stream.synchronize()
                if c is None:
                    dec.finish_device(d_rows.data_ptr(), d_pos.data_ptr(), cap)
                else:
                    dec.push_device(d_x.data_ptr() + at * x.itemsize, c, d_rows.data_ptr(), d_pos.data_ptr(), cap)
                    at += c
                r = dec.results()
                k = int(r.n_rows)
                rows, pos = d_rows.cpu().numpy().reshape(-1, 2080), d_pos.cpu().numpy()
                assert (rows[k:] == -7.0).all() and (pos[k:] == -1).all()  # nothing beyond what the record counts
                calls.append((rows[:k].copy(), pos[:k].astype(np.uint64),
                              (int(r.work_len), int(r.scan_pos), k, int(r.n_sync), int(r.n_in), int(r.rows_total))))
    sc.check_same(calls, want, (rate, sync, max_push))
    sc.check_against_reference(calls, None, ref, sizes, (rate, sync, max_push, "device"))


def test_decode_live_is_decode(oracle):
    ref = sc.reference("apt", 11025, "standard", 1237, True)
    rows = apt.decode_live(apt.Context(device=0), sc.settings_of("standard"), np.array_split(ref.x, 9), apt.Rate.hz(11025), True)
    assert np.array_equal(sc.bits(rows), sc.bits(ref.rows.reshape(-1)))
    rows_gpu = apt.decode(apt.Context(device=0), sc.settings_of("standard"), ref.x, apt.Rate.hz(11025), True)
    assert np.array_equal(sc.bits(rows), sc.bits(rows_gpu))


def test_c_example_live_writes_the_same_image(tmp_path, oracle):
    """examples/aptgpu_decode.c --live 0.25: the same PGM as without the flag"""
    import os
    import shutil
    import subprocess
    from noaa_apt_amd.testing.wavfile import make_wav
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "aptgpu_decode"
    libdir = os.path.dirname(apt.lib_path())
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-I", os.path.join(root, "include"), "-o", str(exe),
                           os.path.join(root, "examples", "aptgpu_decode.c"), "-L", libdir, "-laptgpu",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    ref = sc.reference("apt", 11025, "standard", 1237, True)
    wav = tmp_path / "pass.wav"
    wav.write_bytes(make_wav(ref.x.astype(np.int16), 11025))
    plain, live = tmp_path / "plain.pgm", tmp_path / "live.pgm"
    for out, extra in ((plain, []), (live, ["--live", "0.25"])):
        r = subprocess.run([str(exe), str(wav), str(out)] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    assert "pushes of 0.25 s" in r.stderr
    data = live.read_bytes()
    assert data.startswith(f"P5\n2080 {ref.rows.shape[0]}\n255\n".encode()) and data == plain.read_bytes()
