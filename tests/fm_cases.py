"""Cases for the FM demodulator's tests (test_fm_cpu.py, test_gpu_fm.py): synth_apt() audio at 48 kHz, repeated D-fold,
FM-modulated at 17 kHz deviation around shift_hz, quantised to the format; the f64 model's answer, computed once per
case and shared (the arrays are read-only).

Settings: the library's usual ones, 18 000 Hz / 40 dB / 8 000 Hz.  (The pair 20 000 / 10 000 is refused at an output
rate of 48 kHz by the definition's own rule: 20 000 + 10 000 / 2 is above 24 000.)  T is then 15 at D = 1 and 671 at
D = 50.

check() is the assertion of the bound: with e = sqrt(2) * 2 (T + 8) * 2^-24 * sum|h| * max|x| every output lies within
g (e / |v[m]| + e / |v[m + 1]|) + 4 * 2^-24 * max(|a_model|, 1e-3 g) of the model; outputs with
e / |v[m]| + e / |v[m + 1]| > 0.01 are left out, and at most 0.1 % of a case may be."""
import functools
import types

import numpy as np

import np_fm_model as fm

import noaa_apt_amd as apt
from noaa_apt_amd.testing.synth import synth_apt

CHANNEL = dict(channel_cutout_hz=18000.0, channel_atten=40.0, channel_delta_hz=8000.0, deviation_hz=17000.0)
AUDIO_RATE = 48000

# (D, shift_hz, format, seconds, noise sigma, swap)
BOUND_CASES = [
    (5, 25000.0, fm.S16, 0.5, 0.0, False),
    (8, -31250.5, fm.U8, 0.5, 0.0, False),   # even D; a pw that is not a round number
    (1, 0.0, fm.F32, 0.5, 0.0, False),       # no decimation, no mix
    (50, 100000.0, fm.U8, 0.1, 0.0, False),  # T = 671: several columns of halo in a tile of 150
    (5, 12000.0, fm.F32, 0.5, 0.05, False),  # complex noise
    (3, -8000.0, fm.S8, 0.5, 0.0, False),
    (3, -8000.0, fm.S8, 0.5, 0.0, True),     # the same recording stored Q first
]
IDS = ["D5-s16", "D8-u8", "D1-f32", "D50-u8", "D5-f32-noise", "D3-s8", "D3-s8-swap"]


def settings(d, shift, fmt, swap=False, **over):
    kw = dict(CHANNEL)
    kw.update(over)
    return apt.FmSettings(fmt, AUDIO_RATE * d, d, shift, swap_iq=swap, **kw)


def recording(d, shift, fmt, seconds, sigma=0.0, swap=False, seed=11):
    """the interleaved components of one case"""
    audio = synth_apt(AUDIO_RATE, seconds, seed).astype(np.float64) / 32768.0
    z = fm.modulate(np.repeat(audio, d), AUDIO_RATE * d, 17000.0, shift, phase0=0.3)
    if sigma:
        rng = np.random.default_rng(seed + 1)
        z = z + sigma * (rng.standard_normal(z.size) + 1j * rng.standard_normal(z.size))
    if swap:
        z = z.imag + 1j * z.real
    return fm.quantize(z, fmt)


def model_of(iq, st, taps):
    a, v, _ = fm.demodulate(iq, st.format, st.sample_rate, st.decimation, taps, st.shift_hz, st.deviation_hz, st.swap_iq)
    return a, v


@functools.lru_cache(maxsize=None)
def case(d, shift, fmt, seconds, sigma=0.0, swap=False):
    st = settings(d, shift, fmt, swap)
    iq = recording(d, shift, fmt, seconds, sigma, swap)
    info = apt.fm_design(st)
    a, v = model_of(iq, st, info.taps)
    for arr in (iq, a, v):
        arr.flags.writeable = False
    return types.SimpleNamespace(settings=st, iq=iq, info=info, audio=a, v=v, x_max=float(np.abs(fm.convert(iq, fmt)).max()))


def check(c, got, rate, note=""):
    """asserts the bound for one case; prints the figures first"""
    g = fm.gain(AUDIO_RATE, c.settings.deviation_hz)
    assert rate.get_hz() == AUDIO_RATE and got.dtype == np.float32 and got.shape == c.audio.shape, (rate, got.shape)
    b, skip = fm.bound(c.info.taps, c.x_max, c.v, c.audio, g)
    err = np.abs(got.astype(np.float64) - c.audio)
    keep = ~skip
    print(f"fm {note}: T={c.info.n_taps} n_out={got.size} skipped={int(skip.sum())} max_err={err[keep].max():.3e} "
          f"max_err/bound={(err[keep] / b[keep]).max():.4f} min|v|/max|x|={np.abs(c.v).min() / c.x_max:.3f}")
    assert skip.sum() <= 1e-3 * skip.size, (note, int(skip.sum()))
    assert np.all(np.isfinite(got[keep]))
    assert np.all(err[keep] <= b[keep]), (note, float((err[keep] / b[keep]).max()))
    return float(err[keep].max())


def check_recording(iq, st, got, rate, note=""):
    """check() for a recording that is not one of the cached cases (the model runs here)"""
    info = apt.fm_design(st)
    a, v = model_of(iq, st, info.taps)
    c = types.SimpleNamespace(settings=st, iq=iq, info=info, audio=a, v=v,
                              x_max=float(np.abs(fm.convert(iq, st.format)).max()) if len(iq) else 0.0)
    if a.size == 0:
        assert got.size == 0 and rate.get_hz() == AUDIO_RATE
        return 0.0
    return check(c, got, rate, note)
