"""The AFC in front of the FM demodulator, on the CPU (include/aptgpu.h §4b'): the twin of apt_afc.cpp
through the assertions of afc_cases.py that test_gpu_afc.py makes on the kernels, the refusals by name, the struct
layouts and the example.  No GPU is touched."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import afc_cases as ac
import fm_cases as fc
import np_afc_model as am
import np_fm_model as fm

import noaa_apt_amd as apt
from noaa_apt_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = ac.HOST


# ---------------------------------------------------------------- 1. sums
@pytest.mark.parametrize("case", ac.SUMS_CASES, ids=[c[0] for c in ac.SUMS_CASES])
def test_sums_bit_for_bit(case):
    ac.check_sums_case(B, case)


def test_sums_f32():
    ac.check_sums_f32(B)


# ---------------------------------------------------------------- 2. table
def test_table_gated_signal():
    ac.check_table_gated(B)


def test_table_no_good_block():
    ac.check_table_no_good_block(B)


def test_table_window_of_one_and_wider_than_the_recording():
    ac.check_table_windows(B)


def test_table_nan_frame():
    ac.check_table_nan_frame(B)


def test_table_base_shift_of_100_khz_with_lag_3():
    ac.check_table_base_shift(B)


def test_auto_lag():
    for d, dev, off in ((5, 17000.0, 15000.0), (10, 17000.0, 15000.0), (50, 17000.0, 500.0), (1, 17000.0, 15000.0)):
        st = fc.settings(d, 0.0, fm.U8, deviation_hz=dev)
        info = apt.fm_afc_design(st, apt.AfcSettings(max_offset_hz=off))
        assert info.lag == am.auto_lag(st.sample_rate, off, dev), (d, info)
    assert apt.fm_afc_design(fc.settings(50, 0.0, fm.U8), apt.AfcSettings(max_offset_hz=10.0)).lag == 35
    assert apt.fm_afc_design(fc.settings(1, 0.0, fm.U8), apt.AfcSettings()).lag == 1  # clamped from 0
    assert apt.fm_afc_design(fc.settings(5, 0.0, fm.U8), apt.AfcSettings(lag=9)).lag == 9


# ---------------------------------------------------------------- 3. tracked demodulation
@pytest.mark.parametrize("b", [64, 1 << 16], ids=["B64", "B65536"])
@pytest.mark.parametrize("case", fc.BOUND_CASES, ids=fc.IDS)
def test_tracked_bound(case, b):
    ac.check_tracked_bound(B, case, b)


def test_constant_table_equals_fm_demodulate():
    ac.check_constant_table_is_plain(B)


def test_tracked_edges_and_table_length():
    c = fc.case(*fc.BOUND_CASES[0])
    st, t, d = c.settings, c.info.n_taps, c.settings.decimation
    afc = apt.AfcSettings(block_frames=64)
    for n in (0, t - 1, t, t + d, t + d + 1):
        rec = ac.stepping_table(c.info.pw, am.n_blocks(n, 64), 64)
        got, rate = apt.fm_demodulate_tracked_host(c.iq[:2 * n], rec, st, afc)
        assert got.size == fm.out_len(n, t, d) and rate.get_hz() == 48000
    with pytest.raises(apt.InvalidError, match="n_blocks"):
        apt.fm_demodulate_tracked_host(c.iq[:2 * 1000], ac.stepping_table(c.info.pw, 15, 64), st, afc)
    with pytest.raises(apt.InvalidError, match="AFC_RECORD_DTYPE"):
        apt.fm_demodulate_tracked_host(c.iq[:2 * 1000], np.zeros(16, np.uint32), st, afc)


# ---------------------------------------------------------------- 4. end to end
@pytest.mark.parametrize("case", ac.E2E_CASES, ids=ac.E2E_IDS)
def test_end_to_end_table_and_audio(case):
    ac.check_end_to_end_table(B, case)


def test_uncorrected_demodulation_is_wrong_and_afc_is_not():
    a_true = ac.check_uncorrected_is_wrong()
    iq, _ = ac.swept(5, fm.U8, 2.0)
    audio, _, _ = apt.fm_demodulate_afc_host(iq, ac.settings(5, fm.U8))
    worst = float(np.abs(audio - a_true).max())
    print(f"afc: the twin's audio against the true offset's: max |difference| = {worst:.4f}")
    assert worst < 0.01


# ---------------------------------------------------------------- 5. refusals and the ABI
@pytest.mark.parametrize("over,name", ac.REFUSALS, ids=[f"{n}-{i}" for i, (_, n) in enumerate(ac.REFUSALS)])
def test_refusals_name_the_field(over, name):
    st = apt.FmSettings(**ac.FM_OK)
    afc = apt.AfcSettings(**over)
    iq = np.zeros(2 * 256, np.uint8)
    calls = [lambda: apt.fm_afc_design(st, afc), lambda: apt.fm_afc_sums_host(iq, st, afc),
             lambda: apt.fm_afc_estimate_host(np.zeros((4, 3)), st, afc),
             lambda: apt.fm_demodulate_tracked_host(iq, np.zeros(4, apt.AFC_RECORD_DTYPE), st, afc),
             lambda: apt.fm_demodulate_afc_host(iq, st, afc),
             # the device forms refuse before a device is touched (this test runs without one)
             lambda: apt.fm_afc_sums(iq, st, afc), lambda: apt.fm_afc_estimate(np.zeros((4, 3)), st, afc),
             lambda: apt.fm_demodulate_tracked(iq, np.zeros(4, apt.AFC_RECORD_DTYPE), st, afc),
             lambda: apt.fm_demodulate_afc(iq, st, afc)]
    for call in calls:
        with pytest.raises(apt.InvalidError, match=name) as e:
            call()
        assert "aptgpu_afc_settings" in str(e.value)


def test_other_refusals():
    st = apt.FmSettings(**ac.FM_OK)
    with pytest.raises(apt.InvalidError, match="struct_size"):
        apt.fm_afc_design(st, apt.AfcSettings(), struct_size=8)
    with pytest.raises(apt.InvalidError, match="deviation_hz"):  # §4b's refusals come first
        apt.fm_afc_design(apt.FmSettings(deviation_hz=0.0, **ac.FM_OK), apt.AfcSettings())
    with pytest.raises(apt.InvalidError, match="AfcSettings"):
        apt.fm_afc_design(st, object())
    with pytest.raises(apt.InvalidError, match="2\\^20 blocks"):  # nb <= 2^20, before the recording is read
        err = C.create_string_buffer(256)
        cs, ca = st._c(), apt.AfcSettings(block_frames=64)._c()
        out, n = C.POINTER(C.c_double)(), C.c_size_t()
        rc = apt.lib().aptgpu_fm_afc_sums_host(C.byref(cs), C.byref(ca), None, (64 << 20) + 1, C.byref(out), C.byref(n),
                                               err, 256)
        api._check(rc, err)
    with pytest.raises(apt.InvalidError, match="shape"):
        apt.fm_afc_estimate_host(np.zeros(12), st)
    with pytest.raises(apt.InvalidError, match="FmDemodulator"):
        apt.FmAfc(None)


def test_null_table_is_refused_through_the_c_abi():
    """a NULL table with the right n_blocks must not be read: refused by name, on both forms, before a device is touched"""
    st, afc = apt.FmSettings(**ac.FM_OK), apt.AfcSettings(block_frames=64)
    cs, ca, cctx = st._c(), afc._c(), apt.Context()._c()
    iq = np.zeros(2 * 1000, np.uint8)
    for head, fn in (((), apt.lib().aptgpu_fm_demodulate_tracked_host),
                     ((C.byref(cctx),), apt.lib().aptgpu_fm_demodulate_tracked)):
        out, n, rate, err = C.POINTER(C.c_float)(), C.c_size_t(), C.c_uint32(), C.create_string_buffer(256)
        rc = fn(*head, C.byref(cs), C.byref(ca), iq.ctypes.data, 1000, None, 16, C.byref(out), C.byref(n), C.byref(rate),
                err, 256)
        assert rc == apt.InvalidError.code and b"table is null" in err.value and not out
        rc = fn(*head, C.byref(cs), C.byref(ca), iq.ctypes.data, 1000, None, 0, C.byref(out), C.byref(n), C.byref(rate),
                err, 256)
        assert rc == apt.InvalidError.code and b"n_blocks" in err.value


def test_struct_layouts():
    assert C.sizeof(api._CAfcSettings) == 24 and api._CAfcSettings.min_coherence.offset == 20
    assert C.sizeof(api._CAfcInfo) == 40 and api._CAfcInfo.max_offset_hz.offset == 24
    assert apt.AFC_RECORD_DTYPE.itemsize == 16 and am.RECORD == apt.AFC_RECORD_DTYPE
    hdr = open(os.path.join(ROOT, "include", "aptgpu.h")).read()
    for name in ("aptgpu_afc_settings", "aptgpu_afc_info", "aptgpu_afc_record"):
        assert f"}} {name};" in hdr
    d = api._CAfcSettings()
    apt.lib().aptgpu_fm_afc_default_settings(C.byref(d))
    py = apt.AfcSettings()
    assert (d.struct_size, d.block_frames, d.lag, d.smooth_blocks, d.max_offset_hz, d.min_coherence) == \
        (24, py.block_frames, py.lag, py.smooth_blocks, py.max_offset_hz, np.float32(py.min_coherence))


def test_example_compiles_with_afc(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = open(os.path.join(ROOT, "examples", "aptgpu_decode.c")).read()
    assert "--afc" in src and "aptgpu_fm_demodulate_afc" in src
    exe = tmp_path / "aptgpu_decode"
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-pedantic", "-Werror",
                           "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                           os.path.join(ROOT, "examples", "aptgpu_decode.c"),
                           "-L", os.path.dirname(apt.lib_path()), "-laptgpu",
                           "-Wl,-rpath," + os.path.dirname(apt.lib_path()), "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 2 and "--afc" in r.stderr
