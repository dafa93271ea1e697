"""The FM demodulator without a GPU: anchors of the f64 model (np_fm_model.py) that need no library, the C++ twin
(fm_demodulate_host) against the model under the bound of fm_cases.check, the design, the output lengths, every refusal
of the definition with its field in the message, and load_iq."""
import numpy as np
import pytest

import fm_cases as fc
import np_fm_model as fm

import noaa_apt_amd as apt
from noaa_apt_amd.testing.wavfile import make_wav

f32 = np.float32


# ---------------------------------------------------------------- the model alone
def test_model_carrier_is_a_constant():
    fs, d, shift, f0, dev = 240000, 5, 25000.0, 3000.0, 17000.0
    taps = apt.fm_design(fc.settings(d, shift, fm.F32)).taps
    # the model's own frequency is the one the integer phase stands for: put the carrier f0 above it
    used = fm.shift_used(fm.pw_of(shift, fs), fs)
    z = np.exp(2j * np.pi * (used + f0) * np.arange(6000) / fs)
    iq = np.empty(2 * z.size)
    iq[0::2], iq[1::2] = z.real, z.imag
    v = fm.filtered(iq.astype("<f4"), fm.F32, taps, d, fm.pw_of(shift, fs))
    # (the components were rounded to f32: redo in f64 for the 1e-9 anchor)
    x = z * np.exp(-1j * fm.theta(np.arange(z.size), fm.pw_of(shift, fs)))
    h = taps.astype(np.float64)
    m = (z.size - h.size) // d + 1
    v64 = sum(h[k] * x[h.size - 1 - k:h.size - 1 - k + (m - 1) * d + 1:d] for k in range(h.size))
    a = fm.discriminate(v64, fm.gain(fs // d, dev))
    assert a.size == m - 1 == fm.out_len(z.size, h.size, d)
    assert np.abs(a - f0 / dev).max() <= 1e-9
    assert np.abs(fm.discriminate(v, fm.gain(fs // d, dev)) - f0 / dev).max() <= 1e-5


def test_model_negating_q_negates_the_audio():
    c = fc.case(1, 0.0, fm.F32, 0.5)
    iq = c.iq.copy()
    iq[1::2] = -iq[1::2]
    a, _ = fc.model_of(iq, c.settings, c.info.taps)
    assert np.array_equal(a, -c.audio)


def test_model_phase_wraps():
    for pw in (fm.pw_of(-31250.5, 384000), fm.pw_of(100000.0, 2400000), 0xFFFFFFFF, 1):
        assert fm.phase(2 ** 32 + 5, pw) == fm.phase(5, pw) == (5 * pw) % 2 ** 32
        i = np.array([5, 2 ** 32 + 5, 2 ** 33 + 5, 2 ** 31], dtype=np.uint64)
        assert fm.phase(i, pw).tolist() == [(int(k) % 2 ** 32) * pw % 2 ** 32 for k in i]
    assert fm.pw_of(-31250.5, 384000) == (2 ** 32 - round(31250.5 / 384000 * 2 ** 32))
    assert fm.pw_of(120000, 240000) == fm.pw_of(-120000, 240000) == 2 ** 31


# ---------------------------------------------------------------- the twin
@pytest.mark.parametrize("case", fc.BOUND_CASES, ids=fc.IDS)
def test_twin_against_model(case):
    c = fc.case(*case)
    got, rate = apt.fm_demodulate_host(c.iq, c.settings)
    fc.check(c, got, rate, f"twin {case}")


def test_twin_accepts_bytes_and_complex64():
    c = fc.case(1, 0.0, fm.F32, 0.5)
    a, _ = apt.fm_demodulate_host(c.iq, c.settings)
    b, _ = apt.fm_demodulate_host(c.iq.tobytes(), c.settings)
    z, _ = apt.fm_demodulate_host(c.iq.view(np.complex64), c.settings)
    assert a.tobytes() == b.tobytes() == z.tobytes()
    with pytest.raises(apt.InvalidError, match="dtype"):
        apt.fm_demodulate_host(c.iq.astype(np.float64), c.settings)


def test_twin_non_finite_frames():
    c = fc.case(1, 0.0, fm.F32, 0.5)
    t = c.info.n_taps
    iq = c.iq[:2 * 400].copy()
    clean, _ = apt.fm_demodulate_host(iq, c.settings)
    iq[2 * 100], iq[2 * 250 + 1] = np.nan, np.inf
    got, _ = apt.fm_demodulate_host(iq, c.settings)
    want = np.zeros(got.size, bool)
    for i in (100, 250):  # v[m] reads frames [m, m + T); a[m] needs v[m] and v[m + 1]
        want[max(i - t, 0):i + 1] = True
    assert np.array_equal(np.isnan(got), want)
    assert got[~want].tobytes() == clean[~want].tobytes()
    assert np.array_equal(np.isnan(fc.model_of(iq, c.settings, c.info.taps)[0]), want)


def test_zero_input_is_zero():
    st = fc.settings(3, -8000.0, fm.S8)
    got, _ = apt.fm_demodulate_host(np.zeros(2 * 1000, np.int8), st)
    assert got.size and not got.any() and not np.signbit(got).any()


# ---------------------------------------------------------------- design, lengths
def test_design_is_the_stated_lowpass():
    for d, shift in ((5, 25000.0), (8, -31250.5), (1, 0.0), (50, 100000.0)):
        st = fc.settings(d, shift, fm.U8)
        info = apt.fm_design(st)
        rate = apt.Rate.hz(st.sample_rate)
        want = apt.Lowpass(apt.Freq.hz(st.channel_cutout_hz, rate), st.channel_atten,
                           apt.Freq.hz(st.channel_delta_hz, rate)).design()
        assert info.taps.tobytes() == want.tobytes()
        assert info.rate.get_hz() == 48000 and info.decimation == d
        assert info.pw == fm.pw_of(shift, st.sample_rate)
        assert info.shift_hz_used == fm.shift_used(info.pw, st.sample_rate)
    assert apt.fm_design(fc.settings(1, 0.0, fm.U8)).n_taps == 15
    assert apt.fm_design(fc.settings(50, 0.0, fm.U8)).n_taps == 671


@pytest.mark.parametrize("d,fmt", [(1, fm.F32), (5, fm.S16), (8, fm.U8), (3, fm.S8)])
def test_out_len_at_the_edges(d, fmt):
    st = fc.settings(d, 0.0, fmt)
    t = apt.fm_design(st).n_taps
    for n, want in ((0, 0), (t - 1, 0), (t, 0), (t + d - 1, 0), (t + d, 1), (t + d + 1, 2 if d == 1 else 1),
                    (t + 2 * d, 2)):
        iq = np.zeros(2 * n, fm.DTYPES[fmt])
        got, rate = apt.fm_demodulate_host(iq, st)
        assert got.size == want == fm.out_len(n, t, d), (n, got.size)
        assert rate.get_hz() == 48000


# ---------------------------------------------------------------- refusals (no device is touched: there may be none)
def _settings_only(**kw):
    st = fc.settings(5, 0.0, fm.U8)
    for k, v in kw.items():
        setattr(st, k, v)
    return st


@pytest.mark.parametrize("change,match", [
    (dict(sample_rate=240001), "sample_rate_hz is not a multiple of decimation"),
    (dict(sample_rate=0), "sample_rate_hz"),
    (dict(decimation=0), "decimation"),
    (dict(decimation=4097, sample_rate=4097 * 48000), "decimation"),
    (dict(channel_cutout_hz=0.0), "channel_cutout_hz"),
    (dict(channel_cutout_hz=float("nan")), "channel_cutout_hz"),
    (dict(channel_delta_hz=-1.0), "channel_delta_hz"),
    (dict(channel_delta_hz=float("inf")), "channel_delta_hz"),
    (dict(deviation_hz=0.0), "deviation_hz"),
    (dict(deviation_hz=float("nan")), "deviation_hz"),
    (dict(channel_atten=float("nan")), "channel_atten"),
    (dict(channel_atten=8.0), "channel_atten"),
    (dict(shift_hz=float("nan")), "shift_hz"),
    (dict(shift_hz=120000.5), "shift_hz"),
    (dict(shift_hz=-120000.5), "shift_hz"),
    (dict(channel_cutout_hz=20000.0, channel_delta_hz=10000.0), "channel_cutout_hz \\+ channel_delta_hz / 2"),
    (dict(channel_delta_hz=100.0), "4096 taps"),
    (dict(channel_delta_hz=1e-30), "4096 taps"),
    (dict(flags=2), "flags"),
    (dict(format=4), "format"),
    (dict(format=-1), "format"),
])
def test_refusals_name_the_field(change, match):
    st = _settings_only(**change)
    iq = np.zeros(64, fm.DTYPES.get(change.get("format", fm.U8), np.uint8))
    with pytest.raises(apt.InvalidError, match=match):
        apt.fm_design(st)
    if "format" in change:
        return  # (the Python side refuses the array's dtype itself)
    for call in (lambda: apt.fm_demodulate_host(iq, st), lambda: apt.fm_demodulate(iq, st),
                 lambda: apt.FmDemodulator(st)):
        with pytest.raises(apt.InvalidError, match=match):  # before a device is asked for: there may be none here
            call()


def test_short_struct_size_is_refused():
    st = fc.settings(5, 0.0, fm.U8)
    with pytest.raises(apt.InvalidError, match="struct_size"):
        apt.fm_design(st, struct_size=40)
    assert apt.fm_design(st, struct_size=48).n_taps > 0


def test_accepted_at_the_limits():
    assert apt.fm_design(_settings_only(shift_hz=120000.0)).pw == 2 ** 31
    assert apt.fm_design(_settings_only(channel_cutout_hz=20000.0, channel_delta_hz=8000.0)).n_taps > 0  # == 24 000


# ---------------------------------------------------------------- load_iq
def test_load_iq(tmp_path):
    rng = np.random.default_rng(3)
    s16 = rng.integers(-32768, 32767, 2 * 500)
    p = tmp_path / "iq16.wav"
    p.write_bytes(make_wav(s16, 240000, channels=2, bits=16))
    iq, fmt, rate = apt.load_iq(p)
    assert (fmt, rate.get_hz(), iq.dtype) == (apt.IqFormat.S16, 240000, np.dtype("<i2"))
    assert np.array_equal(iq, s16)
    flt = rng.standard_normal(2 * 300).astype(f32)
    p = tmp_path / "iqf.wav"
    p.write_bytes(make_wav(flt, 1024000, channels=2, is_float=True))
    iq, fmt, rate = apt.load_iq(p)
    assert (fmt, rate.get_hz()) == (apt.IqFormat.F32, 1024000) and iq.tobytes() == flt.tobytes()
    # raw frames: both arguments, a trailing partial frame dropped
    p = tmp_path / "raw.u8"
    p.write_bytes(bytes(range(7)))
    iq, fmt, rate = apt.load_iq(p, apt.IqFormat.U8, 2400000)
    assert iq.tolist() == [0, 1, 2, 3, 4, 5] and fmt == apt.IqFormat.U8 and rate.get_hz() == 2400000
    with pytest.raises(apt.InvalidError):
        apt.load_iq(p, apt.IqFormat.U8)
    # what the recording says goes into the settings: the twin on the loaded WAV equals the twin on the array
    c = fc.case(5, 25000.0, fm.S16, 0.5)
    wav = make_wav(c.iq[:2 * 3000], 240000, channels=2, bits=16)
    iq, fmt, rate = apt.load_iq(wav)
    st = fc.settings(5, 25000.0, fmt)
    assert rate.get_hz() == st.sample_rate
    assert apt.fm_demodulate_host(iq, st)[0].tobytes() == apt.fm_demodulate_host(c.iq[:2 * 3000], c.settings)[0].tobytes()


def test_load_iq_unsupported(tmp_path):
    mono = make_wav(np.arange(100), 48000, channels=1, bits=16)
    with pytest.raises(apt.UnsupportedError):
        apt.load_iq(mono)
    wide = make_wav(np.arange(200), 240000, channels=2, bits=24)
    with pytest.raises(apt.UnsupportedError):
        apt.load_iq(wide)
    st = fc.settings(5, 0.0, fm.S16)
    for data in (mono, wide):
        with pytest.raises(apt.UnsupportedError):  # the parse comes before the device here too
            apt.fm_demodulate_wav(data, st)
