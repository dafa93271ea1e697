"""F in pixel-phase planes: the k_fused instantiations store F[i] at plane i % pw, index i / pw of the
slot's filtered buffer; the row gather, the no-sync tail, k_sync_words' window loads and read_internal("filtered") read
it through the same index map, and a slot whose F came from k_fused_any or the unfused kernels stays contiguous.

Every case decodes short recordings (11-14 image rows: about 20 front-end tiles of 3172 owned samples at 48 kHz, so
the phase of a tile's first sample — tile % 3 — takes each value many times) and compares rows, sync positions and the
result record with the oracle's, bit for bit:

* work lengths w with w % 3 = 0, 1, 2 whose last tile holds 1, 2, 3 owned samples (w % 3172);
* four recordings of different lengths in one call;
* pixel widths 4 and 5 (fast / slow profile at 48 kHz, and the fast profile at 96 kHz, whose front end is a SPLIT
  instantiation where 48 kHz runs a PHASE one), a PHASE rate (44 100 Hz), a rate served by k_fused_any (60 kHz:
  contiguous F in every consumer), PCM16 input, sync=False, a run of NaN, rows_cap below the row count;
* rows pointers off a 16-byte boundary: the eight-rows gather, storing quads and single floats in one call;
* read_internal("filtered"): the oracle's filtered signal in natural order, and what an unfused plan returns;
* widened bounds (APTGPU_GM_SLACK_SCALE), so that k_sync_words' exact settlement loads windows too;
* both forms of k_sync_words (APTGPU_WORDS_FORM=0 and the default), each in a fresh child process.

Tolerance: none (a NaN compares as a NaN: its sign and payload are not part of IEEE arithmetic).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))

import noaa_apt_amd as apt  # noqa: E402
from noaa_apt_amd.testing.synth import synth_apt  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
RATE = 48000
OWN_K = 3172  # owned work samples of a front-end tile at 48 / 96 kHz, standard profile (244 threads of 13)
OFF_48K = (959 - 1) // 2  # fast_resampling's offset with the 959 taps of 48 kHz -> 12 480 Hz


def _samples_for_work_len(w):
    """the shortest 48 kHz input whose work-rate signal has w samples: w = ceil((13 n - off) / 50)"""
    return (50 * (w - 1) + OFF_48K) // 13 + 1


# work lengths: (w % 3, w % OWN_K) = (2, 1), (1, 2), (0, 3) — 11.2, 11.7 and 12.2 rows
WORK_LENS = [22 * OWN_K + 1, 23 * OWN_K + 2, 24 * OWN_K + 3]


def _standard(w, seed):
    x = synth_apt(RATE, 7.0, seed)[:_samples_for_work_len(w)].copy()
    assert x.size == _samples_for_work_len(w), "the synthetic recording is too short for this work length"
    return x


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (recordings, rate, profile)"""
    if name.startswith("w"):
        return [_standard(WORK_LENS[int(name[1:])], 60 + int(name[1:]))], RATE, "standard"
    if name == "four":
        lens = WORK_LENS + [13 * 6240 + 777]
        return [_standard(w, 70 + k) for k, w in enumerate(lens)], RATE, "standard"
    if name == "fast-profile":
        return [synth_apt(RATE, 6.0, 81)], RATE, "fast"
    if name == "slow-profile":
        return [synth_apt(RATE, 6.0, 82)], RATE, "slow"
    if name == "fastp-96000":  # (pixel width 4 behind a SPLIT stage 1)
        return [synth_apt(96000, 6.0, 86)], 96000, "fast"
    if name == "phase-44100":
        return [synth_apt(44100, 6.0, 83)], 44100, "standard"
    if name == "any-60000":
        return [synth_apt(60000, 6.0, 84)], 60000, "standard"
    if name == "nan-run":
        x = _standard(WORK_LENS[1], 85)
        x[x.size // 2 - 150:x.size // 2 + 150] = np.nan  # the filters spread it over some 330 work samples
        return [x], RATE, "standard"
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _oracle(name, sync=True):
    from oracle import binding
    xs, rate, profile = _case(name)
    settings = {"standard": binding.STANDARD, "fast": binding.FAST, "slow": binding.SLOW}[profile]
    out = [binding.decode(x, rate, sync, settings=settings, want_steps=True) for x in xs]
    for rows, st in out:
        rows.setflags(write=False)
    return out


def _same(got, want, what, nan_ok=False):
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if nan_ok:
        gn, wn = np.isnan(got), np.isnan(want)
        assert np.array_equal(gn, wn), (what, "NaN positions differ", int(np.flatnonzero(gn != wn)[0]))
        got, want = got[~wn], want[~wn]
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (what, f"{bad.size} of {got.size} differ, first at {int(bad[0])}", got[bad[0]], want[bad[0]])


def _decode(name, sync=True, pcm16=False, mode=apt.MODE_STRICT, cap=None, want_f=False, want_flags=False, offsets=None):
    """the recordings of a case through ONE decode_device call of a fresh plan.  offsets: floats per recording by which
    its rows pointer lies behind the start of its (that much larger) tensor"""
    import torch  # (a missing module is an error here, not a skip)
    xs, rate, profile = _case(name)
    offs = [0] * len(xs) if offsets is None else list(offsets)
    assert len(offs) == len(xs)
    dev = torch.device("cuda:0")
    plan = apt.Plan(apt.Settings.profile(profile), apt.Rate.hz(rate), sync, max_samples=max(x.size for x in xs),
                    max_batch=len(xs), mode=mode)
    try:
        room = int(plan.info.max_rows) + 2
        caps = [room if cap is None else cap] * len(xs)
        d_full = [torch.full((room * 2080 + off,), -7.0, dtype=torch.float32, device=dev) for off in offs]
        d_out = [t[off:] for t, off in zip(d_full, offs)]  # (data_ptr() of a view: the tensor's + 4 off bytes)
        assert all(t.data_ptr() % 16 == 0 for t in d_full), "the allocator is meant to return 16-byte aligned tensors"
        if pcm16:
            for x in xs:
                assert np.array_equal(x, x.astype(np.int16).astype(f32)), "the case is no 16-bit recording"
            d_in = [torch.from_numpy(x.astype(np.int16)).to(dev) for x in xs]
            specs = [apt.WavSpec(1, 16, 2, 0, rate, 1, 0, 2 * x.size, x.size, x.size) for x in xs]
            torch.cuda.synchronize()
            plan.decode_device_wav([t.data_ptr() for t in d_in], specs, [t.data_ptr() for t in d_out], caps)
        else:
            d_in = [torch.from_numpy(x).to(dev) for x in xs]
            torch.cuda.synchronize()
            plan.decode_device([t.data_ptr() for t in d_in], [x.size for x in xs], [t.data_ptr() for t in d_out], caps)
        res = plan.results(len(xs))
        out = []
        for i in range(len(xs)):
            r = res[i]
            out.append(dict(
                rows=d_out[i][:r.n_out].cpu().numpy(), behind=d_out[i][r.n_out:].cpu().numpy(),
                front=d_full[i][:offs[i]].cpu().numpy(),
                record=(int(r.status), int(r.reason), int(r.n_rows), int(r.n_sync), int(r.work_len), int(r.n_out)),
                pos=plan.sync_positions(i) if sync else None,
                variant=bytes(plan.read_internal("fused_variant", np.uint8, 64, i=i)).rstrip(b"\0").decode(),
                F=plan.read_internal("filtered", f32, int(r.work_len), i=i) if want_f else None,
                flags=plan.read_internal("picker_flags", np.uint32, 32, i=i) if want_flags else None))
    finally:
        plan.close()
    return out


def _check(name, got, nan_ok=False):
    for i, g in enumerate(got):
        want, st = _oracle(name)[i]
        what = f"{name}[{i}]"
        assert g["record"] == (0, 0, want.size // 2080, st["sync_pos"].size, st["filtered"].size, want.size), (what, g["record"])
        assert g["pos"].tolist() == st["sync_pos"].tolist(), what
        _same(g["rows"], want, what, nan_ok)
        assert np.all(g["behind"] == f32(-7.0)), (what, "written behind the rows")
        assert np.all(g["front"] == f32(-7.0)), (what, "written in front of the rows")


@pytest.mark.parametrize("k", [0, 1, 2])
def test_short_recordings_every_phase_and_last_tile(oracle, k):
    name = f"w{k}"
    w = _oracle(name)[0][1]["filtered"].size
    assert w == WORK_LENS[k] and (w % 3, w % OWN_K) == ((2, 1), (1, 2), (0, 3))[k], "the case misses the length it is about"
    assert 11 <= w // 6240 <= 14
    got = _decode(name)
    assert got[0]["variant"] == "48k_f32"
    _check(name, got)


def test_four_recordings_of_different_lengths_in_one_call(oracle):
    """The plane length is ONE value per plan (from max_samples), carried per slot: recordings of different lengths
    share it, and a short recording's planes end well inside it.  The stride itself is not visible from here; F read
    back through it in natural order is — for every slot of the call."""
    got = _decode("four", want_f=True)
    for i, g in enumerate(got):
        _same(g["F"], _oracle("four")[i][1]["filtered"], f"four[{i}] filtered")
    assert [g["variant"] for g in got] == ["48k_f32"] * 4
    assert len({g["record"][4] for g in got}) == 4, "the work lengths are meant to differ"
    _check("four", got)


# (48 kHz at the fast profile is 26 / 75: a PHASE instantiation; 96 kHz has a SPLIT one)
VARIANT_OF = {"fast-profile": "phase", "fastp-96000": "96k_fastp_f32", "slow-profile": "48k_slow_f32", "phase-44100": "phase"}


@pytest.mark.parametrize("name", sorted(VARIANT_OF))
def test_other_pixel_widths_and_a_phase_rate(oracle, name):
    got = _decode(name)
    v = got[0]["variant"]
    assert v.startswith("phase") if VARIANT_OF[name] == "phase" else v == VARIANT_OF[name], (name, v)
    _check(name, got)


def test_k_fused_any_keeps_the_contiguous_layout(oracle):
    got = _decode("any-60000", want_f=True)
    assert got[0]["variant"] == "", "60 kHz is meant to run k_fused_any"
    _check("any-60000", got)
    _same(got[0]["F"], _oracle("any-60000")[0][1]["filtered"], "any-60000 filtered")


@pytest.mark.parametrize("name,offsets", [("four", [0, 1, 0, 2]), ("any-60000", [1])])
def test_rows_pointers_that_are_not_16_byte_aligned(oracle, name, offsets):
    """One rows pointer of a call off a 16-byte boundary sends the whole call through the eight-rows gather
    (k_gather_rows_call): recordings whose own pointer is aligned store quads there, the others single floats.  `four`:
    F in planes, both kinds in one call; `any-60000`: contiguous F.  Same rows, nothing written outside them."""
    got = _decode(name, offsets=offsets)
    assert [g["variant"] for g in got] == (["48k_f32"] * 4 if name == "four" else [""])
    _check(name, got)


def test_pcm16_input(oracle):
    got = _decode("w1", pcm16=True)
    assert got[0]["variant"] == "48k_i16"
    _check("w1", got)


@pytest.mark.parametrize("name", ["w0", "w2", "slow-profile"])
def test_no_sync_tail(oracle, name):
    got = _decode(name, sync=False)
    assert got[0]["variant"] != ""
    want, st = _oracle(name, False)[0]
    assert got[0]["record"] == (0, 0, want.size // 2080, 0, st["filtered"].size, want.size), got[0]["record"]
    _same(got[0]["rows"], want, name + " no sync")
    assert np.all(got[0]["behind"] == f32(-7.0))


def test_run_of_nan(oracle):
    st = _oracle("nan-run")[0][1]
    assert np.isnan(st["correlation"]).sum() > 100 and np.isnan(_oracle("nan-run")[0][0]).any(), "the NaN run is gone"
    _check("nan-run", _decode("nan-run"), nan_ok=True)


@pytest.mark.parametrize("name", ["w1", "slow-profile"])
def test_exact_settlement_loads_its_windows_from_the_planes(oracle, monkeypatch, name):
    """Bounds widened a thousand times (APTGPU_GM_SLACK_SCALE, read when the plan is created) leave comparisons open, so
    k_sync_words' second pass — the window loads of its exact settlement, rare on recordings — runs: picker_flags[11]
    counts them (as tests/test_gpu_bounds.py reads it).  Same results."""
    monkeypatch.setenv("APTGPU_GM_SLACK_SCALE", "1e3")
    got = _decode(name, want_flags=True)
    assert got[0]["variant"] != ""
    assert int(got[0]["flags"][11]) > 0, "no comparison was left open: the case misses the path it is about"
    _check(name, got)


def test_rows_cap_below_the_row_count(oracle):
    cap = 5
    g = _decode("w1", cap=cap)[0]
    want, st = _oracle("w1")[0]
    assert want.size // 2080 > cap
    assert g["record"] == (0, 4, cap, st["sync_pos"].size, st["filtered"].size, cap * 2080), g["record"]
    _same(g["rows"], want[:cap * 2080], "w1 clamped")
    assert np.all(g["behind"] == f32(-7.0)), "written behind the caller's rows"


@pytest.mark.parametrize("name", ["w0", "w1", "w2", "fastp-96000"])
def test_read_internal_filtered_is_in_natural_order(oracle, name):
    fused = _decode(name, want_f=True)[0]
    unfused = _decode(name, mode=apt.MODE_GENERIC, want_f=True)[0]
    assert fused["variant"] != "" and unfused["variant"] == ""
    want = _oracle(name)[0][1]["filtered"]
    _same(fused["F"], want, name + " filtered (planes)")
    _same(unfused["F"], want, name + " filtered (unfused)")


# ---- both forms of k_sync_words, each in a process of its own (the switch is read when a plan is created)
CHILD_CASES = ["w0", "w1", "w2", "nan-run", "fast-profile", "slow-profile"]


def _child(out_path):
    ctx = apt.Context(device=0)
    rows = {}
    for name in CHILD_CASES:
        xs, rate, profile = _case(name)
        rows[name] = apt.decode(ctx, apt.Settings.profile(profile), xs[0], apt.Rate.hz(rate), True)
    np.savez(out_path, **rows)


@pytest.mark.parametrize("form", ["default", "0"])
def test_both_forms_of_k_sync_words(oracle, tmp_path, form):
    env = {k: v for k, v in os.environ.items() if k != "APTGPU_WORDS_FORM"}
    if form != "default":
        env["APTGPU_WORDS_FORM"] = form
    out = tmp_path / "rows.npz"
    done = subprocess.run([sys.executable, "-s", os.path.abspath(__file__), str(out)], env=env, cwd=ROOT,
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, (done.returncode, done.stdout[-2000:], done.stderr[-2000:])
    with np.load(out) as got:
        for name in CHILD_CASES:
            _same(got[name], _oracle(name)[0][0], f"{name} form {form}", nan_ok=name == "nan-run")


if __name__ == "__main__":
    _child(sys.argv[1])
