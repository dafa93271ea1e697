"""Cases and assertions for the AFC's tests (test_afc_cpu.py: the twin; test_gpu_afc.py: the kernels), include/aptgpu.h
§4b'.  Signals are fm_cases.recording's recipe with an offset curve passed to np_fm_model.modulate.  Every check takes a
backend (the GPU entry points or their _host forms) and makes the same assertions on it.

Bounds:
 - sums: bit for bit for u8 / s8 / s16; F32 within 1e-12 * en[b] (f64 sums of at most 4096 products: 4096 * 2^-53 * en
   is 4.5e-13 * en).
 - table, with the model fed the library's own sums: coherence, good and the hold bit for bit; pw within 1 LSB on at most
   1 % of blocks (atan2 is the only inexact step); phase0 and step follow from the returned pw, step within one f32 ulp on
   at most 1 % of blocks.  The cases keep clear of the two thresholds (asserted on the model).
 - tracked demodulation: np_fm_model.bound around an f64 model of stage C, skip cap 0.1 %."""
import functools
import types

import numpy as np

import fm_cases as fc
import np_afc_model as am
import np_fm_model as fm

import noaa_apt_amd as apt
from noaa_apt_amd.testing.synth import synth_apt

GPU = types.SimpleNamespace(name="gpu", sums=apt.fm_afc_sums, estimate=apt.fm_afc_estimate,
                            tracked=apt.fm_demodulate_tracked, afc=apt.fm_demodulate_afc, plain=apt.fm_demodulate)
HOST = types.SimpleNamespace(name="host", sums=apt.fm_afc_sums_host, estimate=apt.fm_afc_estimate_host,
                             tracked=apt.fm_demodulate_tracked_host, afc=apt.fm_demodulate_afc_host,
                             plain=apt.fm_demodulate_host)


def read_only(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays[0] if len(arrays) == 1 else arrays


# ---------------------------------------------------------------- signals
def tanh_sweep(n, fs, f0=12000.0, f1=6000.0):
    """the carrier's offset per frame: f0 -> f1 on a tanh curve centred on the recording"""
    t = (np.arange(n) / n - 0.5) * 6.0
    return 0.5 * (f0 + f1) + 0.5 * (f1 - f0) * np.tanh(t)


@functools.lru_cache(maxsize=None)
def swept(d, fmt, seconds, sigma=0.0, base=0.0, gate=0.0, seed=11):
    """(iq, true offset per frame): APT audio FM-modulated around base + the sweep; `gate` seconds at both ends carry no
    signal; complex noise of sigma (of the signal's amplitude 1) everywhere"""
    fs = fc.AUDIO_RATE * d
    audio = synth_apt(fc.AUDIO_RATE, seconds, seed).astype(np.float64) / 32768.0
    n = audio.size * d
    off = base + tanh_sweep(n, fs)
    z = fm.modulate(np.repeat(audio, d), fs, 17000.0, off, phase0=0.3)
    if gate:
        g = int(gate * fs)
        z[:g] = 0.0
        z[n - g:] = 0.0
    if sigma:
        rng = np.random.default_rng(seed + 1)
        z = z + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return read_only(fm.quantize(z, fmt), off)


@functools.lru_cache(maxsize=None)
def noise_only(d, fmt, seconds, seed=5):
    rng = np.random.default_rng(seed)
    n = int(fc.AUDIO_RATE * d * seconds)
    return read_only(fm.quantize(0.3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)), fmt))


def settings(d, fmt, shift=0.0, swap=False):
    return fc.settings(d, shift, fmt, swap)


# ---------------------------------------------------------------- 1. sums
def _const(fmt, n, value):
    return np.full(2 * n, value, fm.DTYPES[fmt])


@functools.lru_cache(maxsize=None)
def _base(fmt):
    return read_only(fc.recording(5, 9000.0, fmt, 0.1, sigma=0.02))  # 24000 frames


# (id, format, B, L, frames or a constant recording, swap)
SUMS_CASES = [
    ("u8-B64-L1-odd", fm.U8, 64, 1, 1003, False),
    ("s16-B64-L7-edges", fm.S16, 64, 7, 1003, False),        # terms reach across block edges
    ("s8-B4096-L7-swap", fm.S8, 4096, 7, 2 * 4096 + 5, True),
    ("u8-B4096-L1", fm.U8, 4096, 1, 10000, False),            # several chunks of 2048 frames per block
    ("s16-B4096-L64", fm.S16, 4096, 64, 24000, False),        # the longest lag: the whole look-ahead
    ("s16-n-below-L", fm.S16, 64, 7, 5, False),
    ("s16-n-equals-L", fm.S16, 64, 7, 7, False),
    ("u8-empty", fm.U8, 64, 1, 0, False),
    ("s8-last-block-no-term", fm.S8, 64, 7, 3 * 64 + 3, False),
    ("s16-most-negative", fm.S16, 4096, 1, ("const", 4096, -32768), False),
    ("u8-all-0", fm.U8, 4096, 1, ("const", 4096, 0), False),
    ("u8-all-255", fm.U8, 4096, 1, ("const", 4096, 255), False),
]


def sums_recording(case):
    _, fmt, _, _, what, _ = case
    if isinstance(what, tuple):
        return _const(fmt, what[1], what[2])
    return _base(fmt)[:2 * what]


def check_sums_exact(got, iq, fmt, b, lag, swap, note=""):
    want = am.sums(iq, fmt, b, lag, swap)
    assert got.dtype == np.float64 and got.shape == want.shape, (note, got.shape, want.shape)
    assert np.all(np.abs(want) < 2 ** 53)  # the conversion of the exact sums to f64 is exact
    assert np.array_equal(got, want.astype(np.float64)), (note, np.flatnonzero((got != want).any(axis=1))[:8])
    return want


def check_sums_case(backend, case):
    name, fmt, b, lag, _, swap = case
    iq = sums_recording(case)
    got = backend.sums(iq, settings(5, fmt, swap=swap), apt.AfcSettings(block_frames=b, lag=lag))
    want = check_sums_exact(got, iq, fmt, b, lag, swap, name)
    if name == "s16-most-negative":
        assert want[0, 2] == 2 ** 43 and want[0, 0] == 4095 * 2 ** 31  # (2 * 32768^2 per frame: past int32)
    if name == "s8-last-block-no-term":
        assert want.shape[0] == 4 and want[3, 0] == 0 and want[3, 1] == 0 and want[3, 2] > 0


def check_sums_f32(backend):
    iq = _base(fm.F32)[:2 * 9001]
    for b, lag in ((64, 7), (4096, 1)):
        got = backend.sums(iq, settings(5, fm.F32), apt.AfcSettings(block_frames=b, lag=lag))
        want = am.sums(iq, fm.F32, b, lag)
        err = np.abs(got - want)
        print(f"afc sums f32 {backend.name} B={b} L={lag}: max err / en = {(err.max(axis=1) / want[:, 2]).max():.3e}")
        assert got.shape == want.shape and np.all(err <= 1e-12 * want[:, 2:3])


# ---------------------------------------------------------------- 2. table
def check_table(got, sums_in, info, b, note="", expect_good=None):
    """got: the library's AfcTable for `sums_in` (the library's own sums).  Returns the model's table."""
    w, lag = info.smooth_blocks, info.lag
    coh, est, good, rel, finite = am.estimate(sums_in, lag, w, info.pw_base, info.sample_rate, info.max_offset_hz,
                                              info.min_coherence)
    nb = coh.size
    # the two conditions on the case, on the model alone
    fin = np.isfinite(coh)
    assert not np.any(np.abs(coh[fin] - info.min_coherence) <= 1e-9 * info.min_coherence), note
    limit = info.max_offset_hz * 2.0 ** 32 / info.sample_rate
    assert not np.any(finite & (np.abs(np.abs(rel) - limit) <= 2.0)), note
    if expect_good is not None:
        assert expect_good(good), (note, good.astype(int).tolist())
    assert got.records.shape == (nb,) and got.coherence.shape == (nb,) and got.good.shape == (nb,)
    # coherence and good: bit for bit
    assert got.coherence.view(np.uint32).tolist() == am.coherence_f32(coh).view(np.uint32).tolist(), note
    assert got.good.tolist() == good.tolist(), note
    # pw: within 1 LSB of the model's estimate on good blocks, different on at most 1 % of blocks
    pw = got.records["pw"].astype(np.int64)
    model_pw = am.hold(est, good, info.pw_base)
    diff = (pw - model_pw + (1 << 31)) % am.TWO32 - (1 << 31)
    print(f"afc table {note}: nb={nb} good={int(good.sum())} pw differs on {int((diff != 0).sum())} blocks, "
          f"max |diff| = {int(np.abs(diff).max()) if nb else 0} LSB")
    assert np.all(np.abs(diff) <= 1), note
    assert (diff != 0).sum() <= 0.01 * nb, note
    # the hold, bit for bit: every block carries the returned pw of the block the model's hold points to
    if good.any():
        g = np.flatnonzero(good)
        last = np.maximum.accumulate(np.where(good, np.arange(nb), -1))
        j = np.where(last >= 0, last, g[0])
        assert np.array_equal(pw, pw[j]), note
    else:
        assert np.all(pw == info.pw_base), note
    # phase0 and step from the returned pw
    want = am.records_of(pw, b)
    assert np.array_equal(got.records["phase0"], want["phase0"]), note
    for f in ("step_re", "step_im"):
        a, m = got.records[f], want[f]
        ulp = np.spacing(np.abs(m).astype(np.float32)).astype(np.float64)
        d = np.abs(a.astype(np.float64) - m.astype(np.float64))
        assert np.all(d <= ulp) and (d != 0).sum() <= 0.01 * nb, (note, f)
    return types.SimpleNamespace(coherence=coh, good=good, est=est, pw=model_pw)


def run_table_case(backend, iq, st, afc, note, expect_good=None):
    s = backend.sums(iq, st, afc)
    info = apt.fm_afc_design(st, afc)
    got = backend.estimate(s, st, afc)
    assert got.info == info
    return got, check_table(got, s, info, afc.block_frames, f"{backend.name} {note}", expect_good), s


def check_table_gated(backend):
    """signal off for 0.4 s at both ends: the noise blocks hold the nearest good block's estimate"""
    iq, _ = swept(5, fm.U8, 2.0, sigma=0.05, gate=0.4)
    afc = apt.AfcSettings()
    got, model, _ = run_table_case(backend, iq, settings(5, fm.U8), afc, "gated",
                                   lambda g: g.any() and not g[:15].any() and not g[-15:].any())
    on = model.good
    print(f"afc gated: noise coherence <= {model.coherence[~on].max():.4f}, signal coherence >= {model.coherence[on].min():.4f}")
    first, last = np.flatnonzero(on)[[0, -1]]
    assert np.all(got.records["pw"][:first] == got.records["pw"][first])
    assert np.all(got.records["pw"][last:] == got.records["pw"][last])


def check_table_no_good_block(backend):
    st = settings(5, fm.S8, shift=-8000.0)
    got, _, _ = run_table_case(backend, noise_only(5, fm.S8, 0.5), st, apt.AfcSettings(), "no good block",
                               lambda g: not g.any())
    assert np.all(got.records["pw"] == apt.fm_design(st).pw)


def check_table_windows(backend):
    iq, _ = swept(5, fm.S16, 0.5, sigma=0.1)
    for w in (1, 1023):  # (0.5 s is 30 blocks: 1023 is wider than nb)
        run_table_case(backend, iq, settings(5, fm.S16), apt.AfcSettings(smooth_blocks=w), f"W={w}", lambda g: g.all())


def check_table_nan_frame(backend):
    iq = swept(5, fm.F32, 0.5)[0].copy()
    iq[2 * 50000] = np.nan  # block 12
    afc = apt.AfcSettings(smooth_blocks=3)
    got, model, s = run_table_case(backend, iq, settings(5, fm.F32), afc, "NaN frame",
                                   lambda g: not g[11:14].any() and g[:11].all() and g[14:].all())
    assert np.isnan(s[12]).any() and np.isnan(got.coherence[11:14]).all()
    assert np.all(got.records["pw"][11:14] == got.records["pw"][10])


def check_table_base_shift(backend):
    """a 100 kHz base shift with L = 3: L * pw_base wraps, the estimate is relative to it"""
    iq, _ = swept(5, fm.U8, 0.5, base=100000.0)
    st = settings(5, fm.U8, shift=100000.0)
    got, _, _ = run_table_case(backend, iq, st, apt.AfcSettings(lag=3), "100 kHz base, L=3", lambda g: g.all())
    off = got.offset_hz
    assert np.all((off > 100000.0 + 5000.0) & (off < 100000.0 + 13000.0)), (off.min(), off.max())


# ---------------------------------------------------------------- 3. tracked demodulation
def stepping_table(pw_base, nb, b):
    """a table whose pw steps at every block, by up to +-40 LSB around pw_base + 1000"""
    k = np.arange(nb, dtype=np.int64)
    return am.records_of(pw_base + 1000 + 20 * ((k * 7) % 5 - 2), b)


def check_tracked_bound(backend, case, b):
    c = fc.case(*case)
    st = c.settings
    n = c.iq.size // 2
    afc = apt.AfcSettings(block_frames=b)
    rec = stepping_table(c.info.pw, am.n_blocks(n, b), b)
    got, rate = backend.tracked(c.iq, rec, st, afc)
    a, v = am.demodulate_tracked(c.iq, st.format, st.sample_rate, st.decimation, c.info.taps, rec, b, st.deviation_hz,
                                 st.swap_iq)
    m = types.SimpleNamespace(settings=st, iq=c.iq, info=c.info, audio=a, v=v, x_max=c.x_max)
    fc.check(m, got, rate, f"tracked {backend.name} B={b} {case}")


def constant_table(pw_base, nb, b):
    return am.records_of(np.full(nb, pw_base, np.int64), b)


def check_constant_table_is_plain(backend):
    for case in (fc.BOUND_CASES[0], fc.BOUND_CASES[1], fc.BOUND_CASES[4]):
        c = fc.case(*case)
        assert c.info.pw != 0
        n = c.iq.size // 2
        for b in (64, 4096):
            rec = constant_table(c.info.pw, am.n_blocks(n, b), b)
            # (the step of design_of: the same f64 expression, so the same f32)
            got, _ = backend.tracked(c.iq, rec, c.settings, apt.AfcSettings(block_frames=b))
            plain, _ = backend.plain(c.iq, c.settings)
            assert got.tobytes() == plain.tobytes(), (backend.name, case, b)


# ---------------------------------------------------------------- 4. end to end
# (D, format, seconds, sigma, lag, the model's largest offset error in Hz as measured for this case).
# The error peaks in the middle of the sweep, where the carrier moves by 9 kHz / s (far more than Doppler does) and a
# window of 15 blocks averages over 0.26 s of it; the test allows twice the measured value.
E2E_CASES = [
    (5, fm.U8, 2.0, 0.0, 0, 65.0),
    (5, fm.U8, 2.0, 0.5, 0, 146.0),
    (10, fm.S16, 1.0, 0.05, 3, 65.0),
]
E2E_IDS = ["D5-u8-clean", "D5-u8-noise0.5", "D10-s16-L3"]


def block_truth(off, b):
    """the true offset of a block: the mean over its frames"""
    nb = am.n_blocks(off.size, b)
    return np.array([off[k * b:(k + 1) * b].mean() for k in range(nb)])


def check_end_to_end_table(backend, case):
    d, fmt, seconds, sigma, lag, measured = case
    iq, off = swept(d, fmt, seconds, sigma)
    st, afc = settings(d, fmt), apt.AfcSettings(lag=lag)
    audio, rate, table = backend.afc(iq, st, afc)
    s = backend.sums(iq, st, afc)
    info = apt.fm_afc_design(st, afc)
    model = check_table(table, s, info, afc.block_frames, f"e2e {backend.name} {case}", lambda g: g.all())
    # the model's own error against the truth: a factor 2 over the value measured for this case
    err = np.abs(am.offset_hz(model.pw, info.sample_rate) - block_truth(off, afc.block_frames))
    print(f"afc e2e {case}: the model's offset error: max {err.max():.1f} Hz (measured {measured} Hz)")
    assert err.max() <= 2.0 * measured
    # the audio is stage C of the returned table, bit for bit
    again, _ = backend.tracked(iq, table, st, afc)
    assert rate.get_hz() == fc.AUDIO_RATE and audio.tobytes() == again.tobytes()
    return iq, st, afc, audio, table


def check_uncorrected_is_wrong():
    """model only: the same recording demodulated with shift_hz = 0 is far from the audio demodulated with the true
    offset (discriminator wrap-around)"""
    d, fmt = 5, fm.U8
    iq, off = swept(d, fmt, 2.0)
    st = settings(d, fmt)
    taps = apt.fm_design(st).taps
    b = 64
    nb = am.n_blocks(off.size, b)
    truth = am.records_of(np.array([fm.pw_of(f, st.sample_rate) for f in block_truth(off, b)], np.int64), b)
    a_true, _ = am.demodulate_tracked(iq, fmt, st.sample_rate, d, taps, truth, b)
    a_zero, _, _ = fm.demodulate(iq, fmt, st.sample_rate, d, taps, 0.0)
    worst = float(np.abs(a_zero - a_true).max())
    print(f"afc: shift_hz = 0 against the true offset: max |difference| = {worst:.3f} of full scale")
    assert nb == truth.size and worst > 0.5
    return a_true


# ---------------------------------------------------------------- 5. refusals
FM_OK = dict(format=fm.U8, sample_rate=240000, decimation=5)
REFUSALS = [
    (dict(block_frames=32), "block_frames"),
    (dict(block_frames=1 << 21), "block_frames"),
    (dict(block_frames=4097), "block_frames"),
    (dict(block_frames=96), "block_frames"),
    (dict(lag=65), "lag"),
    (dict(smooth_blocks=0), "smooth_blocks"),
    (dict(smooth_blocks=14), "smooth_blocks"),
    (dict(smooth_blocks=1025), "smooth_blocks"),
    (dict(max_offset_hz=0.0), "max_offset_hz"),
    (dict(max_offset_hz=-5.0), "max_offset_hz"),
    (dict(max_offset_hz=float("inf")), "max_offset_hz"),
    (dict(max_offset_hz=float("nan")), "max_offset_hz"),
    (dict(min_coherence=-0.01), "min_coherence"),
    (dict(min_coherence=1.0), "min_coherence"),
    (dict(min_coherence=float("nan")), "min_coherence"),
]
