"""The approximate front ends — APTGPU_MODE_FAST on the VALU (kModeFast), the same mode on the matrix cores (kModeMfma)
and APTGPU_MODE_FP16_TAPS (kModeF16Taps): 13 rows of csrc/apt_kernels_fused_variants.hpp, 26 kernels with their PCM16
instantiations — judged on EVERY work-rate sample of F (the low-pass output, `read_internal("filtered")`) against a
float64 model of the arithmetic each mode documents (tests/np_f64_model.py), first and last tile included.

The rule (np_f64_model.accept):   max |F_gpu - F_pred| <= MARGIN[mode] * max |F_oracle - F64|,  the same for the rms,

with F64 the all-f64 chain on the oracle's f32 taps, F_oracle the strict oracle's `filtered` step on the same input — so
the yardstick is the reference's own f32 rounding, never the code under test — and F_pred what the mode's documented
arithmetic gives in f64: F64 itself for the VALU fast kernels; for the matrix cores the chain on the sum of the five
products of bf16 pieces (taps h = h0 + h1 + h2 exactly, samples x0 + x1 by truncation, the remainder of a sample
dropped); for fp16 taps the chain on the resampler with prescaled fp16 taps and fp16 samples.  A kernel that loses one of
the five products, a plane, or a tap at a tile's edge leaves the prediction by far more than the oracle's rounding; the
mutants below show on the CPU that the rule, at the margins in use, rejects each of them.

Every case names the kernel it means to test and checks `read_internal("fused_variant")` for it; the case list itself is
checked against the table of variants without a GPU, so a new approximate row without a case fails here.

Inputs (6 s each, sync=False): `synth_apt` as it is (int16-valued: at most 16 significant bits), the same as a float WAV
(/ 32768 with a seeded multiplicative jitter of +-2^-9: full 24-bit mantissas) and the int16 one times 2^-4.  fp16 mode
leaves the float WAV out: its samples reach fp16's subnormals, where the conversion is a mode setting.

MARGIN: one per mode, 1.5 x the worst ratio measured on an MI355X (the kernels are deterministic: a ratio moves only with
the input), and below what the mutants need: on the CPU (`test_the_rule_rejects_the_mutant`, 48 kHz, both inputs of the
mode) the matrix-core arithmetic without its h2 x0 product stands at 15.8 (max) / 41.8 (rms) x the oracle's rounding,
without h1 x1 at 27 / 48, without the x1 plane at 8 500 / 19 000; a zeroed last resampler tap at 1 960 / 3 430, a zeroed
low-pass tap at 46 000 / 133 000 in every mode; fp16 taps rounded WITHOUT the prescale at 1.30 / 2.39 — the tight one,
0.855 x 1.5 = 1.28 is below both.  (The taps are split as the host splits them, by truncation: h2 is up to 2^-16 |h|.)

Measured on an MI355X — error of F against the mode's prediction over the error of the strict oracle against F64, worst
over the row's cases (stock and tuned tap count, f32 and PCM16 input) and inputs:

    row                  mode   max     rms        row                  mode   max     rms
    48k_fast             fast   1.000   1.044      phase_std_fast       fast   1.145   1.042
    96k_fast             fast   1.090   1.029      phase2_std_fast      fast   1.031   1.055
    48k_slow_fast        fast   1.000   1.004      phase4_std_fast      fast   1.160   1.060
    48k_mfma             mfma   0.841   0.878      phase512_std_fast    fast   1.031   1.055
    96k_mfma             mfma   1.014   0.855      phase1024_std_fast   fast   1.160   1.060
    tab_std_fast         fast   1.160   1.060      phase_fastp_fast     fast   1.123   1.031
    48k_f16taps          f16    0.804   0.855

(The int16 input and its 2^-4 scaling give the same ratios to the last digit: nothing in these kernels depends on the
scale.)  In absolute terms, of max |F|, kernel against the f64 chain: VALU fast 3.7e-7 .. 6.4e-7 max, 5.3e-8 .. 9.2e-8 rms
(the oracle: 3.4e-7 .. 6.4e-7, 5.0e-8 .. 9.3e-8); matrix cores on samples of at most 16 significant bits 4.3e-7 .. 5.8e-7
max, 6.5e-8 .. 7.9e-8 rms; matrix cores on full-mantissa samples 1.30e-5 max, 3.70e-6 rms at 48 kHz (96 kHz: 1.24e-5,
3.65e-6; tuned tap count: 1.36e-5, 3.64e-6) — the dropped remainder of the samples, which the prediction contains:
against the prediction these cases stand at 3.8e-7 .. 5.2e-7 like the others; fp16 taps 2.2e-4 max, 3.9e-5 rms, against
its prediction 3.9e-7 / 6.0e-8.
"""
import functools
import math
import os
import re
from collections import namedtuple

import numpy as np
import pytest

import noaa_apt_amd as apt
from noaa_apt_amd.testing.synth import synth_apt
import np_f64_model as m64

gpu = pytest.mark.gpu

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS_HPP = os.path.join(ROOT, "noaa_apt_amd", "csrc", "apt_kernels_fused_variants.hpp")

SECONDS = 6  # decode() needs ten rows of work samples: 3 s is refused, 6 s is not
MARGIN = {"fast": 1.5 * 1.160, "mfma": 1.5 * 1.014, "f16": 1.5 * 0.855}  # 1.5 x the worst ratio of the table above
SWITCHES = ("APTGPU_FAST_MFMA", "APTGPU_PHASE_WIDE", "APTGPU_PHASE_FIRST")

# ---- the cases: which plan runs which row
Case = namedtuple("Case", "row rate profile kind env tuned")


def _c(row, rate, profile="standard", kind="fast", env=(), tuned=()):
    return Case(row, rate, profile, kind, tuple(env), tuple(tuned))


CASES = [
    # SPLIT stage 1 on the VALU: 48 / 96 kHz, and 48 kHz at the slow profile
    _c("48k_fast", 48000), _c("96k_fast", 96000), _c("48k_slow_fast", 48000, "slow"),
    # ... on the matrix cores: the A/B switch at the stock tap counts, and a tuned tap count, which takes it by default
    _c("48k_mfma", 48000, kind="mfma", env=[("APTGPU_FAST_MFMA", "1")]),
    _c("96k_mfma", 96000, kind="mfma", env=[("APTGPU_FAST_MFMA", "1")]),
    _c("48k_mfma", 48000, kind="mfma", tuned=[("resample_atten", 31.0)]),
    _c("96k_mfma", 96000, kind="mfma", tuned=[("resample_atten", 31.0)]),
    # TABLE stage 1 (11 025 Hz with the phase-resident form switched off)
    _c("tab_std_fast", 11025, env=[("APTGPU_PHASE_FIRST", "0")]),
    # PHASE stage 1: one, two, four branches per thread; the 512- / 1024-thread workgroups
    _c("phase_std_fast", 44100), _c("phase2_std_fast", 22050), _c("phase4_std_fast", 11025),
    _c("phase512_std_fast", 22050, env=[("APTGPU_PHASE_WIDE", "1")]),
    _c("phase1024_std_fast", 11025, env=[("APTGPU_PHASE_WIDE", "1")]),
    # ... with the fast profile's work-rate stages
    _c("phase_fastp_fast", 48000, "fast"),
    # fp16 taps
    _c("48k_f16taps", 48000, kind="f16"),
]
INPUTS = {"fast": ("int16", "floatwav", "scaled"), "mfma": ("int16", "floatwav", "scaled"), "f16": ("int16", "scaled")}


def _case_id(c):
    return c.row + ("-tuned" if c.tuned else "")


F32_PARAMS = [pytest.param(c, inp, id=f"{_case_id(c)}_f32-{inp}") for c in CASES for inp in INPUTS[c.kind]]
I16_PARAMS = [pytest.param(c, id=f"{_case_id(c)}_i16") for c in CASES]


# ---- the case list against the table of variants (no GPU)
def _approximate_rows():
    """(name, instantiated for PCM16 too) of every row of APT_FUSED_VARIANTS whose mode is not a strict one."""
    rows = []
    for kind, name, mode in re.findall(r"^\s*(BOTH|F32)\((\w+),[^()]*?,\s*(kMode\w+)\)", open(VARIANTS_HPP).read(), re.M):
        if name != "name" and mode not in ("kModeStrict", "kModeStrictPad", "kModeStrictPad2"):
            rows.append((name, kind == "BOTH"))
    return rows


def test_every_approximate_row_has_a_case():
    text = open(VARIANTS_HPP).read()
    parsed = re.findall(r"^\s*(BOTH|F32)\((\w+),[^()]*?,\s*(kMode\w+)\)", text, re.M)
    # (the parse sees every row of the list: as many as there are lines that open one)
    assert len(parsed) == len(re.findall(r"^\s*(?:BOTH|F32)\(", text, re.M)) > 0
    rows = _approximate_rows()
    want = {n + "_f32" for n, _ in rows} | {n + "_i16" for n, both in rows if both}
    have = {c.row + "_f32" for c in CASES} | {c.row + "_i16" for c in CASES}
    assert have == want, (sorted(want - have), sorted(have - want))
    mode_of = {name: mode for _, name, mode in parsed}
    kinds = {"kModeFast": "fast", "kModeMfma": "mfma", "kModeF16Taps": "f16"}
    assert all(c.kind == kinds[mode_of[c.row]] for c in CASES)


# ---- inputs, the oracle's steps and the f64 chain: computed once per (rate, settings, input), never modified
def _settings(profile, tuned):
    s = apt.Settings.profile(profile)
    for k, v in tuned:
        setattr(s, k, v)
    return s


def _oracle_settings(s):
    return {k: getattr(s, k) for k in ("work_rate", "resample_atten", "resample_delta_freq", "resample_cutout",
                                       "demodulation_atten")}


@functools.lru_cache(maxsize=None)
def make_input(rate, which):
    x = synth_apt(rate, SECONDS, seed=rate % 1000 + 11)
    if which == "floatwav":  # a float WAV of the same recording: +-1 full scale, full mantissas
        jitter = np.random.default_rng(rate + 5).uniform(-2.0 ** -9, 2.0 ** -9, x.size)
        x = (x.astype(f64) / 32768.0 * (1.0 + jitter)).astype(f32)
        assert np.count_nonzero(x.view(np.uint32) & np.uint32(0xFF)) > 0.9 * x.size
    elif which == "scaled":
        x = (x * f32(2.0 ** -4)).astype(f32)
    else:
        assert which == "int16" and np.array_equal(x, x.astype(np.int16).astype(f32))
    x.setflags(write=False)
    return x


Ref = namedtuple("Ref", "x l m work_rate h h2 F_oracle F64")


@functools.lru_cache(maxsize=None)
def reference(rate, profile, tuned, which):
    from oracle import binding as oracle
    s = _settings(profile, tuned)
    x = make_input(rate, which)
    _, st = oracle.decode(x, rate, False, settings=_oracle_settings(s), want_steps=True)
    work = int(s.work_rate)
    g = math.gcd(rate, work)
    l, m = work // g, rate // g
    h, h2 = st["resample_filter"], st["filter_filter"]
    F64 = m64.chain64(x, l, m, h, work, h2)
    assert F64.size == st["filtered"].size == st["resampled"].size
    for a in (h, h2, st["filtered"], F64):
        a.setflags(write=False)
    return Ref(x, l, m, work, h, h2, st["filtered"], F64)


@functools.lru_cache(maxsize=None)
def prediction(kind, rate, profile, tuned, which):
    """F as the mode's documented arithmetic gives it, in f64."""
    r = reference(rate, profile, tuned, which)
    if kind == "fast":
        return r.F64
    R = m64.resample_mfma64(r.x, r.l, r.m, r.h) if kind == "mfma" else m64.resample_f16taps64(r.x, r.l, r.m, r.h)
    F = m64.work_stages64(R, r.work_rate, r.h2)
    F.setflags(write=False)
    return F


# ---- the GPU side
def _run(case, x, monkeypatch, pcm16=False, mode=None):
    """F (every work-rate sample) and the name of the kernel that produced it."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env:
        monkeypatch.setenv(k, v)
    if mode is None:
        mode = apt.MODE_FP16_TAPS if case.kind == "f16" else apt.MODE_FAST
    plan = apt.Plan(_settings(case.profile, case.tuned), apt.Rate.hz(case.rate), False, max_samples=x.size, mode=mode)
    try:
        cap = int(plan.info.max_rows)
        d_out = torch.empty((cap + 2) * 2080, dtype=torch.float32, device=dev)
        if pcm16:
            d_in = torch.from_numpy(x.astype(np.int16)).to(dev)
            torch.cuda.synchronize()
            spec = apt.WavSpec(1, 16, 2, 0, case.rate, 1, 0, 2 * x.size, x.size, x.size)
            plan.decode_device_wav([d_in.data_ptr()], [spec], [d_out.data_ptr()], [cap])
        else:
            d_in = torch.from_numpy(np.array(x, f32)).to(dev)
            torch.cuda.synchronize()
            plan.decode_device([d_in.data_ptr()], [x.size], [d_out.data_ptr()], [cap])
        res = plan.results(1)[0]
        assert res.status == 0, res.status
        F = plan.read_internal("filtered", f32, int(res.work_len))
        name = bytes(plan.read_internal("fused_variant", np.uint8, 64)).rstrip(b"\0").decode()
    finally:
        plan.close()
    return F, name


@gpu
@pytest.mark.parametrize("rate,want_name", [(48000, "48k_f32"), (44100, "phase_std_f32")])
def test_strict_filtered_is_the_oracles_bit_for_bit(rate, want_name, monkeypatch):
    """The buffer everything below reads: in strict mode "filtered" IS the oracle's `filtered` step, sample for sample."""
    case = _c("", rate)
    r = reference(rate, "standard", (), "int16")
    F, name = _run(case, r.x, monkeypatch, mode=apt.MODE_STRICT)
    assert name == want_name
    assert F.size == r.F_oracle.size and np.array_equal(F.view(np.uint32), r.F_oracle.view(np.uint32))


def _judge(case, which, F, what):
    r = reference(case.rate, case.profile, case.tuned, which)
    F_pred = prediction(case.kind, case.rate, case.profile, case.tuned, which)
    ok, rmax, rrms = m64.accept(F, F_pred, r.F_oracle, r.F64, MARGIN[case.kind])
    emax, erms = m64.error_figures(F, F_pred)
    omax, orms = m64.error_figures(r.F_oracle, r.F64)
    dmax, drms = m64.error_figures(F, r.F64)
    full = float(np.max(np.abs(r.F64)))
    print(f"RATIO {what:34s} {case.kind:4s} max {rmax:8.3f} rms {rrms:8.3f} | of max|F|: kernel - prediction "
          f"{emax / full:.2e} / {erms / full:.2e}, oracle - f64 {omax / full:.2e} / {orms / full:.2e}, "
          f"kernel - f64 {dmax / full:.2e} / {drms / full:.2e}")
    assert ok, (what, rmax, rrms, MARGIN[case.kind])


@gpu
@pytest.mark.parametrize("case,which", F32_PARAMS)
def test_f32_input_every_work_sample(case, which, monkeypatch):
    r = reference(case.rate, case.profile, case.tuned, which)
    F, name = _run(case, r.x, monkeypatch)
    assert name == case.row + "_f32"
    _judge(case, which, F, f"{_case_id(case)}_f32-{which}")


@gpu
@pytest.mark.parametrize("case", I16_PARAMS)
def test_pcm16_input_every_work_sample(case, monkeypatch):
    r = reference(case.rate, case.profile, case.tuned, "int16")
    F, name = _run(case, r.x, monkeypatch, pcm16=True)
    assert name == case.row + "_i16"
    _judge(case, "int16", F, f"{_case_id(case)}_i16")


# ---- the mutants (no GPU): what the rule must reject at the margins in use, built from the model at 48 kHz
MUTANT_INPUTS = {"fast": ("int16", "floatwav"), "mfma": ("int16", "floatwav"), "f16": ("int16", "scaled")}


def _mutant(kind, name, which):
    r = reference(48000, "standard", (), which)

    def stage1(h, **kw):
        if kind == "fast":
            return m64.resample64(r.x, r.l, r.m, h)
        if kind == "mfma":
            return m64.resample_mfma64(r.x, r.l, r.m, h, **kw)
        return m64.resample_f16taps64(r.x, r.l, r.m, h, **kw)

    h, h2 = r.h, r.h2
    if name == "no_h2x0":
        R = stage1(h, terms=[t for t in m64.MFMA_TERMS if t != (2, 0)])
    elif name == "no_h1x1":
        R = stage1(h, terms=[t for t in m64.MFMA_TERMS if t != (1, 1)])
    elif name == "no_x1_plane":
        R = stage1(h, terms=[t for t in m64.MFMA_TERMS if t[1] == 0])
    elif name == "last_resampler_tap_zero":
        h = h.copy()
        assert h[-1] != 0
        h[-1] = 0
        R = stage1(h)
    elif name == "one_lowpass_tap_zero":
        h2 = h2.copy()
        assert h2[5] != 0
        h2[5] = 0
        R = stage1(h)
    elif name == "no_prescale":
        R = stage1(h, prescale=False)
    else:
        raise AssertionError(name)
    return m64.work_stages64(R, r.work_rate, h2)


MUTANTS = ([("mfma", n) for n in ("no_h2x0", "no_h1x1", "no_x1_plane")] +
           [(k, n) for k in ("fast", "mfma", "f16") for n in ("last_resampler_tap_zero", "one_lowpass_tap_zero")] +
           [("f16", "no_prescale")])


@pytest.mark.parametrize("kind,name", MUTANTS, ids=[f"{k}-{n}" for k, n in MUTANTS])
def test_the_rule_rejects_the_mutant(kind, name):
    for which in MUTANT_INPUTS[kind]:
        r = reference(48000, "standard", (), which)
        ok, rmax, rrms = m64.accept(_mutant(kind, name, which), prediction(kind, 48000, "standard", (), which),
                                    r.F_oracle, r.F64, MARGIN[kind])
        print(f"MUTANT {kind:4s} {name:24s} {which:8s} max {rmax:10.3f} rms {rrms:10.3f}")
        assert not ok, (kind, name, which, rmax, rrms, MARGIN[kind])


def test_the_model_itself():
    """The tap split is exact, the planes are truncations that leave a remainder below 2^-15 |x| of x's sign (none for
    16-bit samples), the prediction of an exact mode accepts itself, and the oracle against the f64 chain is f32-sized."""
    for which in ("int16", "floatwav"):
        r = reference(48000, "standard", (), which)
        p0, p1, p2 = m64.tap_pieces(r.h)
        assert np.array_equal(p0.astype(f64) + p1.astype(f64) + p2.astype(f64), r.h.astype(f64))
        assert all(not np.any(p.view(np.uint32) & np.uint32(0xFFFF)) for p in (p0, p1, p2))
        x0, x1 = m64.sample_planes(r.x)
        rem = r.x.astype(f64) - x0.astype(f64) - x1.astype(f64)
        assert np.all(np.abs(rem) <= 2.0 ** -15 * np.abs(r.x)) and np.all(rem * r.x >= 0)
        assert (which == "floatwav") == bool(np.any(rem != 0))
        ok, rmax, rrms = m64.accept(r.F64, r.F64, r.F_oracle, r.F64, 0.0)
        assert ok and rmax == 0 and rrms == 0
        omax, orms = m64.error_figures(r.F_oracle, r.F64)
        full = float(np.max(np.abs(r.F64)))
        print(f"MODEL {which:8s} oracle - f64: max {omax / full:.2e} rms {orms / full:.2e} of max|F|")
        assert 1e-8 < orms / full < 3e-7 and omax / full < 2e-6
        # the documented matrix-core arithmetic against the f64 chain: what the mode costs on this input
        dmax, drms = m64.error_figures(prediction("mfma", 48000, "standard", (), which), r.F64)
        print(f"MODEL {which:8s} mfma prediction - f64: max {dmax / full:.2e} rms {drms / full:.2e} of max|F|")
        assert (dmax / full < 1e-7) if which == "int16" else (1e-6 < dmax / full < 1e-4)
