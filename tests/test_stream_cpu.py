"""Live decode without a GPU (include/aptgpu.h §4d): the C++ twin (aptgpu_stream_create_host) against the
oracle bit for bit and against the release schedule of np_stream_model.py after every push, chunking invariance,
bounded state, reset, and every refusal — on the GPU form too, which refuses before it touches a device."""
import ctypes as C

import numpy as np
import pytest

import stream_cases as sc

import noaa_apt_amd as apt
from noaa_apt_amd import api

f32 = np.float32


def twin(rate, profile, sync=True, dtype=f32, max_push=None):
    return apt.LiveDecoder(sc.settings_of(profile), apt.Rate.hz(rate), sync, dtype=dtype, max_push=max_push, host=True)


def run_case(kind, rate, profile, rows_x100, sync, chunking, max_push=None, dtype=f32):
    ref = sc.reference(kind, rate, profile, rows_x100, sync)
    x = ref.x
    with twin(rate, profile, sync, dtype, max_push) as dec:
        sizes = sc.chunk_sizes(chunking, x.size, rate, ref.g, dec.info.max_push)
        before = dec.get_info()
        calls, err = sc.run_stream(dec, x.astype(dtype), sizes)
        after = dec.get_info()
    what = (kind, rate, profile, rows_x100, sync, chunking)
    out = sc.check_against_reference(calls, err, ref, sizes, what)
    # bounded state: nothing depends on how much was pushed
    assert bytes(before) == bytes(after), what
    return out, calls, before


# ---------------------------------------------------------------- parity and schedule
@pytest.mark.parametrize("sync", (True, False))
@pytest.mark.parametrize("rate,profile", sc.RATES)
def test_every_rate_and_profile(rate, profile, sync, oracle):
    """12.37 rows of a synthetic pass in random chunks (zeros and ones forced in)"""
    run_case("apt", rate, profile, 1237, sync, "random")


@pytest.mark.parametrize("chunking", sc.CHUNKINGS)
@pytest.mark.parametrize("rate,profile", ((11025, "standard"), (48000, "standard"), (24960, "standard")))
def test_every_chunking_gives_the_same_rows(rate, profile, chunking, oracle):
    """... and all of them the oracle's rows: chunking invariance through parity with one reference"""
    max_push = 3000 if chunking == "over_max_push" else None
    run_case("apt", rate, profile, 1237, True, chunking, max_push=max_push)


@pytest.mark.parametrize("rate,profile", ((11025, "standard"), (48000, "standard"), (20800, "slow")))
def test_two_chunkings_agree_push_for_push_where_they_coincide(rate, profile, oracle):
    (rows_a, pos_a), _, _ = run_case("apt", rate, profile, 1237, True, "4096")
    (rows_b, pos_b), _, _ = run_case("apt", rate, profile, 1237, True, "half_second")
    assert np.array_equal(pos_a, pos_b) and np.array_equal(sc.bits(rows_a), sc.bits(rows_b))


@pytest.mark.parametrize("sync", (True, False))
@pytest.mark.parametrize("rate,profile", ((11025, "standard"), (48000, "standard"), (12480, "standard"), (44100, "fast")))
def test_ten_rows_exactly_decode_and_one_sample_less_does_not(rate, profile, sync, oracle):
    ref = sc.reference("apt", rate, profile, 1000, sync)
    assert 10 * ref.g.spr <= ref.work_len <= 10 * ref.g.spr + 1 and ref.error is None
    run_case("apt", rate, profile, 1000, sync, "half_second")
    short = sc.reference("apt", rate, profile, 999, sync)
    assert short.work_len < 10 * short.g.spr and "less than 10 rows" in short.error
    run_case("apt", rate, profile, 999, sync, "half_second")


@pytest.mark.parametrize("kind", sc.SIGNALS)
def test_signals(kind, oracle):
    """slant, noise (the oracle's peaks or its "less than 5 sync frames"), silence, a constant, a NaN and an Inf"""
    run_case(kind, 11025, "standard", 1237, True, "4096")
    if kind in ("nonfinite", "noise"):
        run_case(kind, 48000, "standard", 1237, True, "random")
        run_case(kind, 24960, "standard", 1237, False, "4096")


@pytest.mark.parametrize("rate,profile", ((11025, "standard"), (24960, "standard")))
def test_s16_samples_decode_like_their_f32_values(rate, profile, oracle):
    (rows, pos), _, _ = run_case("apt", rate, profile, 1237, True, "4096", dtype=np.int16)
    (rows_f, pos_f), _, _ = run_case("apt", rate, profile, 1237, True, "4096")
    assert np.array_equal(pos, pos_f) and np.array_equal(sc.bits(rows), sc.bits(rows_f))


# ---------------------------------------------------------------- launch sequences of many rows, events of many copies
@pytest.mark.parametrize("rate,max_push", ((11025, 1 << 18), (48000, 1 << 20)))
@pytest.mark.parametrize("chunking", ("one", "half_second"))
def test_a_launch_sequence_of_thirty_rows(rate, max_push, chunking, oracle):
    """max_push above the whole recording: one push (and one launch sequence) covers 30.5 rows"""
    ref = sc.reference("apt", rate, "standard", 3050, True)
    assert ref.x.size < max_push
    _, calls, info = run_case("apt", rate, "standard", 3050, True, chunking, max_push=max_push)
    assert info.max_push == max_push
    if chunking == "one":
        assert calls[0][0].shape[0] >= 27


@pytest.mark.parametrize("sync", (True, False))
@pytest.mark.parametrize("chunking", ("one", "half_second", "random"))
@pytest.mark.parametrize("rate,profile", sc.LOW_RATES)
def test_low_input_rates_with_the_default_max_push(rate, profile, chunking, sync, oracle):
    """65 536 samples at 8 000 / 6 000 Hz are 16 / 22 rows of work signal per launch sequence"""
    run_case("apt", rate, profile, 3050, sync, chunking)


@pytest.mark.parametrize("chunking", ("half_second", "one", "random", "single_samples"))
def test_a_fading_carrier_pushes_many_peaks_at_one_event(chunking, oracle):
    """the reference pushes two dozen copies at once; the rows of all of them come out of one push, within the bound"""
    ref = sc.reference("fading", 12480, "standard", 4900, True)
    assert ref.error is None and sc.most_copies(ref) >= 16, np.unique(ref.peaks, return_counts=True)
    _, calls, _ = run_case("fading", 12480, "standard", 4900, True, chunking)
    assert max(c[0].shape[0] for c in calls) >= 16


# ---------------------------------------------------------------- bounded state
@pytest.mark.parametrize("rate,profile,sync", ((11025, "standard", True), (48000, "standard", True), (24960, "standard", False),
                                               (44100, "fast", True)))
def test_thirty_rows_through_rings_that_wrap(rate, profile, sync, oracle):
    g = sc.geometry(rate, profile)
    quarter_row = g.spr * g.m // g.l // 4
    ref = sc.reference("apt", rate, profile, 3050, sync)
    _, calls, info = run_case("apt", rate, profile, 3050, sync, "half_second", max_push=quarter_row)
    assert info.max_push == quarter_row
    # every ring wraps several times
    assert ref.x.size >= 3 * info.cap_in and ref.work_len >= 3 * info.cap_f
    assert (info.cap_corr == info.cap_f) if sync else (info.cap_corr == 0)
    for cap in (info.cap_in, info.cap_f):
        assert cap & (cap - 1) == 0


def test_capacities_do_not_depend_on_the_recording():
    a = twin(11025, "standard", max_push=4096)
    b = twin(11025, "standard", max_push=4096)
    b.push(np.zeros(4096, f32))
    assert bytes(a.get_info()) == bytes(b.get_info())
    assert a.info.device_bytes < 4 * (a.info.cap_in + a.info.cap_f + a.info.cap_corr) + (1 << 18)


def test_reset_reproduces_the_output(oracle):
    ref = sc.reference("apt", 11025, "standard", 1237, True)
    sizes = sc.chunk_sizes("4096", ref.x.size, 11025, ref.g)
    with twin(11025, "standard") as dec:
        first, err = sc.run_stream(dec, ref.x, sizes)
        with pytest.raises(apt.InvalidError, match="finished"):
            dec.push(ref.x[:10])
        with pytest.raises(apt.InvalidError, match="finished"):
            dec.finish()
        dec.reset()
        again, err2 = sc.run_stream(dec, ref.x, sizes)
    assert err is None and err2 is None
    sc.check_same(first, again, "reset")
    sc.check_against_reference(again, err2, ref, sizes, "after reset")


def test_rows_released_before_a_failing_finish_stay_released(oracle):
    """the one difference from decode(): 9.99 rows hand out rows, then finish() raises decode()'s error"""
    ref = sc.reference("apt", 11025, "standard", 999, True)
    long = sc.reference("apt", 11025, "standard", 1237, True)
    sizes = sc.chunk_sizes("4096", ref.x.size, 11025, ref.g)
    with twin(11025, "standard") as dec:
        calls, err = sc.run_stream(dec, ref.x, sizes)
    assert isinstance(err, apt.InternalError) and "less than 10 rows" in str(err)
    rows = np.concatenate([c[0] for c in calls])
    assert 5 <= rows.shape[0] < 10
    assert np.array_equal(sc.bits(rows), sc.bits(long.rows[:rows.shape[0]]))  # final means final


def test_decode_live_is_decode(oracle):
    ref = sc.reference("apt", 48000, "standard", 1237, True)
    chunks = np.array_split(ref.x, 7)
    rows = apt.decode_live(None, sc.settings_of("standard"), chunks, apt.Rate.hz(48000), True, host=True)
    assert np.array_equal(sc.bits(rows), sc.bits(ref.rows.reshape(-1)))
    short = sc.reference("apt", 48000, "standard", 999, True)
    with pytest.raises(apt.InternalError, match="less than 10 rows"):
        apt.decode_live(None, sc.settings_of("standard"), [short.x], apt.Rate.hz(48000), True, host=True)


# ---------------------------------------------------------------- refusals
def _refused(exc, call, text):
    with pytest.raises(exc) as e:
        call()
    assert text in str(e.value), str(e.value)


def _create_raw(host, struct_size=None, fmt=0):
    """aptgpu_stream_create[_host] through ctypes with a settings struct the wrapper would not build"""
    L = api.lib()
    css = api._CStreamSettings(C.sizeof(api._CStreamSettings) if struct_size is None else struct_size, 11025, 1, fmt, 0, 0)
    cctx, cs = apt.Context()._c(), sc.settings_of("standard")._c()
    handle, err = C.c_void_p(), C.create_string_buffer(1024)
    fn = L.aptgpu_stream_create_host if host else L.aptgpu_stream_create
    rc = fn(C.byref(cctx), C.byref(cs), C.byref(css), C.byref(handle), err, 1024)
    assert not handle.value
    api._check(rc, err)


@pytest.mark.parametrize("host", (True, False))
def test_refusals(host):
    """every one before a device is touched: the GPU form refuses on a machine without one"""
    std, r = sc.settings_of("standard"), apt.Rate.hz(11025)

    def make(settings=std, rate=r, **kw):
        return apt.LiveDecoder(settings, rate, host=host, **kw)

    _refused(apt.InvalidError, lambda: _create_raw(host, struct_size=0), "struct_size")
    _refused(apt.InvalidError, lambda: _create_raw(host, fmt=7), "format")
    _refused(apt.InvalidError, lambda: make(dtype=np.float64), "dtype")
    _refused(apt.InvalidError, lambda: make(rate=apt.Rate.hz(0)), "rate")
    _refused(apt.InvalidError, lambda: make(max_push=(1 << 24) + 1), "max_push")
    odd = sc.settings_of("standard")
    odd.work_rate = 12481
    _refused(apt.InternalError, lambda: make(settings=odd), "work_rate is not multiple of FINAL_RATE")
    _refused(apt.InternalError, lambda: make(settings=odd, sync=False), "work_rate is not multiple of FINAL_RATE")
    _refused(apt.RateOverflowError, lambda: make(rate=apt.Rate.hz(4294967291)), "Can't resample, looks like the sample rates do not have a big")
    for mode in (apt.MODE_FAST, apt.MODE_FP16_TAPS):
        _refused(apt.UnsupportedError, lambda: make(context=apt.Context(mode=mode)), "strict mode only")
    for flag in ("export_wav", "export_resample_filtered"):
        s = sc.settings_of("standard")
        setattr(s, flag, True)
        _refused(apt.UnsupportedError, lambda: make(settings=s), "export")


def test_the_matrix_core_switch_is_refused(monkeypatch):
    monkeypatch.setenv("APTGPU_FAST_MFMA", "1")
    with pytest.raises(apt.UnsupportedError, match="matrix-core"):
        apt.LiveDecoder(sc.settings_of("standard"), apt.Rate.hz(48000), host=True)


def test_rows_cap_below_the_bound_is_refused_before_anything_is_consumed():
    with twin(11025, "standard") as dec:
        x = np.zeros(5000, f32)
        bound = dec.rows_bound(x.size)
        assert bound >= 1 and dec.rows_bound(0) >= 1
        with pytest.raises(apt.InvalidError, match="rows_cap"):
            dec.push(x, rows_cap=bound - 1)
        with pytest.raises(apt.InvalidError, match="rows_cap"):
            dec.finish(rows_cap=dec.rows_bound(0) - 1)
        assert dec.result.n_in == 0
        dec.push(x, rows_cap=bound)
        assert dec.result.n_in == 5000
        with pytest.raises(apt.InvalidError, match="host handle"):
            dec.push_device(0x1000, 16, 0x1000, 0x1000, 64)


def test_abi_version_and_struct_sizes():
    assert apt.abi_version() == 2
    assert C.sizeof(api._CStreamSettings) == 24 and C.sizeof(apt.StreamInfo) == 56 and C.sizeof(apt.StreamResult) == 56
