"""The streaming FM demodulator's twin (FmStream(host=True)) and the live decode from IQ on the CPU
(LiveIqDecoder(host=True)): no GPU.  The concatenated pushes of every chunking are fm_demodulate_host() of the whole
recording bit for bit, the release schedule and the info follow the host formulas after every push (fm_stream_cases.walk),
and a LiveIqDecoder equals a LiveDecoder fed the one-shot's audio, push for push."""
import types

import numpy as np
import pytest

import fm_cases as fc
import fm_stream_cases as fsc
import np_fm_model as fm

import noaa_apt_amd as apt

f32 = np.float32


def twin(st, **kw):
    return apt.FmStream(st, host=True, **kw)


# ---------------------------------------------------------------- chunking invariance, as bits
@pytest.fixture(scope="module")
def wanted():
    return {case: apt.fm_demodulate_host(fsc.cut(case).iq, fsc.cut(case).settings)[0] for case in fsc.CASES}


@pytest.mark.parametrize("chunking", fsc.CHUNKINGS)
@pytest.mark.parametrize("case", fsc.CASES, ids=fsc.IDS)
def test_every_chunking_gives_the_one_shot_bits(case, chunking, wanted):
    r = fsc.cut(case)
    with twin(r.settings, max_push_frames=fsc.max_push_of(chunking)) as s:
        if chunking == "over_max_push":
            assert s.info.max_push_frames == fsc.MAX_PUSH_SMALL < r.n
        got = fsc.walk(s, r.iq, fsc.sizes_of(chunking, r.n, r.t, r.d), r.t, r.d)
    assert got.size == wanted[case].size and got.tobytes() == wanted[case].tobytes()


@pytest.mark.parametrize("case", [fsc.CASES[0], fsc.CASES[2], fsc.CASES[3]], ids=["D5-s16", "D1-f32", "D50-u8"])
def test_short_streams(case):
    r = fsc.cut(case)
    t, d = r.t, r.d
    # (T + D + 1 frames hold a third window where D == 1: M = (D + 1) / D + 1)
    for n, want in zip([0, t - 1, t, t + d - 1, t + d, t + d + 1], [0, 0, 0, 0, 1, 2 if d == 1 else 1]):
        iq = r.iq[:2 * n]
        with twin(r.settings) as s:
            got = fsc.walk(s, iq, [n // 2, n - n // 2], t, d)
        assert got.size == want == fm.out_len(n, t, d)
        assert got.tobytes() == apt.fm_demodulate_host(iq, r.settings)[0].tobytes()


def test_non_finite_frames_at_a_seam():
    st, clean, dirty, sizes, want_nan, t, d = fsc.non_finite_recording()
    with twin(st) as s:
        ref = fsc.walk(s, clean, sizes, t, d)
    with twin(st) as s:
        got = fsc.walk(s, dirty, sizes, t, d)
    assert want_nan.sum() >= 2 * (t // d)
    assert np.array_equal(np.isnan(got), want_nan)
    assert got[~want_nan].tobytes() == ref[~want_nan].tobytes()
    assert ref.tobytes() == apt.fm_demodulate_host(clean, st)[0].tobytes()


# ---------------------------------------------------------------- first_frame
def _model_of_cut(r):
    """fm_cases.check's case record for the cut recording: the model's valid part is a prefix of the whole case's"""
    n_out = fm.out_len(r.n, r.t, r.d)
    c = r.case
    return types.SimpleNamespace(settings=c.settings, info=c.info, audio=c.audio[:n_out], v=c.v[:n_out + 1], x_max=c.x_max)


def test_first_frame(wanted):
    case = fsc.CASES[1]  # a pw that is not a round number
    r = fsc.cut(case)
    assert r.case.info.pw % (1 << 16) != 0
    sizes = fsc.sizes_of("random", r.n, r.t, r.d)
    for ff in (1 << 32, 1 << 35):  # the low 32 bits (the phase) and the low 3 (the run grid) are those of 0
        with twin(r.settings, first_frame=ff) as s:
            assert s.info.first_frame == ff
            assert fsc.walk(s, r.iq, sizes, r.t, r.d).tobytes() == wanted[case].tobytes()
    ff = (1 << 32) - 8 * 61 - 3  # the crossing mid-run, inside the first chunk
    with twin(r.settings, first_frame=ff) as s:
        got = fsc.walk(s, r.iq, [4096, r.n - 4096], r.t, r.d)
    # a constant phase offset does not move the discriminator: the model of first_frame 0 is the model
    fc.check(_model_of_cut(r), got, s.rate, f"twin first_frame=2^32-{8 * 61 + 3}")
    assert got.tobytes() != wanted[case].tobytes()  # (the phasors did change)


def test_reset_reproduces_the_bits(wanted):
    case = fsc.CASES[0]
    r = fsc.cut(case)
    with twin(r.settings, first_frame=12345) as s:
        first = fsc.walk(s, r.iq, fsc.sizes_of("random", r.n, r.t, r.d), r.t, r.d)
        s.reset()
        fsc.check_info(s.get_info(), 0, r.t, r.d)
        assert s.get_info().first_frame == 12345
        again = fsc.walk(s, r.iq, fsc.sizes_of("4096", r.n, r.t, r.d), r.t, r.d)
    assert first.tobytes() == again.tobytes()


# ---------------------------------------------------------------- refusals
def _refused(call, match):
    with pytest.raises(apt.InvalidError, match=match):
        call()


def _snapshot(info):
    return (info.frames, info.outputs, info.carry_frames, info.max_push_frames, info.first_frame)


def test_refusals():
    r = fsc.cut(fsc.CASES[0])  # s16
    st = r.settings
    _refused(lambda: twin(st, max_push_frames=0), "max_push_frames")
    _refused(lambda: twin(st, max_push_frames=(1 << 28) + 1), "max_push_frames")
    _refused(lambda: twin(st, struct_size=8), "struct_size")
    for bad, name in ((dict(decimation=0), "decimation"), (dict(sample_rate=0), "sample_rate_hz"),
                      (dict(format=7), "format"), (dict(flags=2), "flags"), (dict(shift_hz=float("nan")), "shift_hz"),
                      (dict(channel_delta_hz=1.0), "4096 taps"), (dict(deviation_hz=-1.0), "deviation_hz")):
        kw = dict(format=st.format, sample_rate=st.sample_rate, decimation=st.decimation, shift_hz=st.shift_hz)
        kw.update(bad)
        fmt, rate, dec = kw.pop("format"), kw.pop("sample_rate"), kw.pop("decimation")
        _refused(lambda: twin(apt.FmSettings(fmt, rate, dec, **kw)), name)  # what design_of refuses
    lib, C = apt.lib(), __import__("ctypes")
    with twin(st) as s:
        s.push(r.iq[:2 * (r.t + 3 * r.d + 2)])
        before = _snapshot(s.get_info())
        chunk = np.ascontiguousarray(r.iq[:2 * 4 * r.d])
        out = np.zeros(16, f32)
        n, err = C.c_size_t(), C.create_string_buffer(512)

        def push(iq_ptr, frames, audio_ptr, cap):
            rc = lib.aptgpu_fm_stream_push(s._p, iq_ptr, frames, audio_ptr, cap, C.byref(n), err, 512)
            return rc, err.value.decode()

        assert s.out_len(4 * r.d) == 4
        for args, text in (((None, 4 * r.d, out.ctypes.data, 16), "iq is null"),
                           ((chunk.ctypes.data, 4 * r.d, None, 16), "audio is null"),
                           ((chunk.ctypes.data + 1, 4 * r.d, out.ctypes.data, 16), "iq is not aligned"),
                           ((chunk.ctypes.data, 4 * r.d, out.ctypes.data + 2, 16), "audio is not aligned"),
                           ((chunk.ctypes.data, 4 * r.d, out.ctypes.data, 3), "audio_cap")):
            rc, msg = push(*args)
            assert rc == 4 and text in msg, (rc, msg)
            assert _snapshot(s.get_info()) == before
        with pytest.raises(apt.InvalidError, match="no device entry points"):
            s.push_device(256, 8, 256, 8)
        assert _snapshot(s.get_info()) == before
        assert push(None, 0, None, 0)[0] == 0  # nothing to read or write
        assert push(chunk.ctypes.data, 4 * r.d, out.ctypes.data, 4)[0] == 0 and n.value == 4
    with pytest.raises(apt.InvalidError, match="dtype"):
        with twin(st) as s:
            s.push(np.zeros(8, np.float32))


# ---------------------------------------------------------------- live decode from IQ
@pytest.fixture(scope="module")
def live_audio():
    rec = fsc.live_recording()
    audio, rate = apt.fm_demodulate_host(rec.iq, rec.settings)
    assert rate.get_hz() == 48000
    return audio


@pytest.mark.parametrize("sync", (True, False), ids=("sync", "nosync"))
@pytest.mark.parametrize("chunking", ("quarter_second", "random", "one"))
def test_live_iq_decoder_equals_a_live_decoder_fed_the_one_shot_audio(chunking, sync, live_audio):
    rec = fsc.live_recording()
    with apt.LiveIqDecoder(apt.Settings(), rec.settings, sync, host=True) as live, \
            apt.LiveDecoder(apt.Settings(), apt.Rate.hz(48000), sync, host=True) as dec:
        fi, si = live.get_info()
        assert fi.fs_out == 48000 and si.work_rate == dec.info.work_rate
        rows = fsc.live_against_decoder(live, dec, live_audio, rec, fsc.live_sizes(chunking, rec.n))
        fsc.check_info(live.get_info()[0], rec.n, rec.t, rec.d)
    if sync:
        assert rows.shape == (14, 2080)


def test_live_iq_over_max_push_frames(live_audio):
    """pieces of 100 000 frames inside one push of 8 s: the same rows, positions and record"""
    rec = fsc.live_recording()
    with apt.LiveIqDecoder(apt.Settings(), rec.settings, True, max_push_frames=100000, max_push=4096, host=True) as live, \
            apt.LiveDecoder(apt.Settings(), apt.Rate.hz(48000), True, host=True) as dec:
        assert live.fm_info.max_push_frames == 100000 and live.info.max_push == 4096
        fsc.live_against_decoder(live, dec, live_audio, rec, [rec.n // 3, rec.n - rec.n // 3])


def test_decode_live_iq_is_decode_of_the_demodulated_recording(live_audio):
    rec = fsc.live_recording()
    sizes = fsc.live_sizes("quarter_second", rec.n)
    edges = np.concatenate([[0], np.cumsum(sizes)])
    chunks = (rec.iq[2 * a:2 * b] for a, b in zip(edges[:-1], edges[1:]))
    rows = apt.decode_live_iq(None, apt.Settings(), rec.settings, chunks, True, host=True)
    want = apt.decode_live(None, apt.Settings(), [live_audio], apt.Rate.hz(48000), True, host=True)
    assert rows.size == 14 * 2080 and rows.tobytes() == want.tobytes()


def test_a_short_recording_raises_the_decode_text():
    rec = fsc.live_recording(1.0)
    with apt.LiveIqDecoder(apt.Settings(), rec.settings, True, host=True) as live:
        live.push(rec.iq)
        with pytest.raises(apt.InternalError, match="less than 10 rows"):
            live.finish()
        with pytest.raises(apt.InvalidError, match="finished"):
            live.push(rec.iq[:16])
        live.reset()
        assert live.get_info()[0].frames == 0
        live.push(rec.iq[:2000])


def test_live_refusals():
    rec = fsc.live_recording(1.0)
    bad = apt.FmSettings(rec.settings.format, rec.settings.sample_rate, 0)
    with pytest.raises(apt.InvalidError, match="decimation"):
        apt.LiveIqDecoder(apt.Settings(), bad, True, host=True)
    with pytest.raises(apt.InvalidError, match="max_push_frames"):
        apt.LiveIqDecoder(apt.Settings(), rec.settings, True, max_push_frames=(1 << 28) + 1, host=True)
    with apt.LiveIqDecoder(apt.Settings(), rec.settings, True, host=True) as live:
        live.push(rec.iq[:2 * 100000])
        before = fsc.record_of(live.result), live.get_info()[0].frames
        with pytest.raises(apt.InvalidError, match="rows_cap"):
            live.push(rec.iq[2 * 100000:], rows_cap=0)
        with pytest.raises(apt.InvalidError, match="no device entry points"):
            live.push_device(256, 8, 256, 256, 8)
        assert (fsc.record_of(live.result), live.get_info()[0].frames) == before


def test_struct_sizes():
    import ctypes as C
    from noaa_apt_amd import api
    assert C.sizeof(api._CFmStreamSettings) == 24 and C.sizeof(api.FmStreamInfo) == 80 and C.sizeof(api._CIqLiveSettings) == 24
    assert apt.abi_version() == 2
