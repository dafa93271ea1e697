"""k_sync_words / k_sync_slots in their lean form (the default) against the oracle, against the definition of the
terminal words, and against their earlier form (APTGPU_WORDS_FORM=0).

Every case is a short 48 kHz recording (11-14 image rows, 10-13 chunks of 128 groups), decoded once per form:

* sync positions and rows: bit for bit the oracle's;
* the plan's terminal words: bit i of word g  <=>  T[52 g + i], T[i] <=> no j in (i, i + md] has corr[j] > corr[i],
  evaluated in numpy from the oracle's correlation (NaN read as -inf, position 0 clamped to >= 0), for every group
  the kernel evaluates — those whose upper bound no lower bound of the next R-1 groups exceeds (the plan's
  "group_max") — and zero for every other group;
* both forms: equal terminal words, peaks and picker flags [0] (list overflow), [1] (sequential walk), [7] and [11]
  (comparisons the bounds left open: the counter, and its copy in the result record's kernel).

The lean form's workgroup still serves ONE chunk of 128 groups (a block of k = 1 chunks), so the block-end cases of
a k-chunk block coincide with the group-count cases: chunk counts 11 and 12 are both in.

Tolerance: none.
"""
import functools

import numpy as np
import pytest

import noaa_apt_amd as apt
from noaa_apt_amd.testing.synth import synth_apt
from test_gpu_parity import assert_bitexact, assert_same_values

pytestmark = pytest.mark.gpu

f32 = np.float32
GS = 52
CHUNK = 128
RATE = 48000


def _samples_for_groups(ng, pw=3):
    """Input samples at 48 kHz whose correlation has `ng` groups (ten positions short of the group's end, so that a
    work-rate length a few samples off the plain ratio still lands in the group)."""
    w = ng * GS - 10 + 38 * pw
    return -(-w * RATE // (4160 * pw))


def _standard(n, seed):
    return synth_apt(RATE, 7.0, seed)[:n].copy()


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (list of recordings, profile, expected group counts or None)"""
    if name.startswith("groups-"):  # 11 chunks exactly, one group more (12 chunks), one group less
        ng = {"groups-0": 11 * CHUNK, "groups-1": 11 * CHUNK + 1, "groups-127": 11 * CHUNK - 1}[name]
        return [_standard(_samples_for_groups(ng), 21)], "standard", [ng]
    if name == "ragged":
        ngs = [10 * CHUNK + 40, 12 * CHUNK + 127, 11 * CHUNK + 1]
        return [_standard(_samples_for_groups(g), 30 + k) for k, g in enumerate(ngs)], "standard", ngs
    if name in ("nan-run", "flat"):
        x = _standard(_samples_for_groups(11 * CHUNK + 60), 41)
        mid = 5 * CHUNK * GS * RATE // 12480  # the input sample under the first position of chunk 5
        if name == "nan-run":
            x[mid - 150:mid + 150] = np.nan  # the filters spread it: NaN correlations on both sides of the boundary
        else:
            x[mid - 16000:mid + 16000] = 0.0  # F == 0 exactly over 8320 work samples > md = 4992: ties
        return [x], "standard", [11 * CHUNK + 60]
    if name == "fast-profile":
        return [synth_apt(RATE, 6.0, 51)], "fast", None
    if name == "slow-profile":
        return [synth_apt(RATE, 6.0, 52)], "slow", None
    raise KeyError(name)


NAMES = ["groups-0", "groups-1", "groups-127", "ragged", "nan-run", "flat", "fast-profile", "slow-profile"]
PW = {"standard": 3, "fast": 4, "slow": 5}


@functools.lru_cache(maxsize=None)
def _oracle(name):
    from oracle import binding
    xs, profile, _ = _case(name)
    settings = {"standard": binding.STANDARD, "fast": binding.FAST, "slow": binding.SLOW}[profile]
    return [binding.decode(x, RATE, True, settings=settings, want_steps=True) for x in xs]


def _window_max_ahead(v, n):
    """out[i] = max(v[i+1 .. i+n]) (clipped at the end; -inf where empty), by doubling"""
    size = v.size
    pad = np.concatenate([v, np.full(n + 1, -np.inf, v.dtype)])
    span, m = 1, pad.copy()  # m[i] = max(pad[i .. i+span-1])
    while 2 * span <= n:
        m = np.maximum(m, np.concatenate([m[span:], np.full(span, -np.inf, v.dtype)]))
        span *= 2
    a = np.arange(size)
    return np.maximum(m[a + 1], m[a + 1 + n - span])


def _terminal_bits(corr, md):
    c = corr.astype(f32).copy()
    if not c[0] > 0:
        c[0] = 0.0
    c = np.where(np.isnan(c), -np.inf, c).astype(f32)
    return ~(_window_max_ahead(c, md) > c)


def _expected_words(corr, gm, pw):
    """terminal words by the definition, for the groups the coarse pass keeps; zero elsewhere"""
    md = 1664 * pw
    r = md // GS
    n_corr = corr.size
    ng = (n_corr + GS - 1) // GS
    t = np.zeros(ng * GS, bool)
    t[:n_corr] = _terminal_bits(corr, md)
    words = (t.reshape(ng, GS).astype(np.uint64) << np.arange(GS, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    hi, lo = gm[:, 0], gm[:, 1]
    keep = ~(_window_max_ahead(lo, r - 1) > hi)
    return np.where(keep, words, np.uint64(0)), keep


def _run(name, form, torch):
    xs, profile, _ = _case(name)
    dev = torch.device("cuda:0")
    plan = apt.Plan(apt.Settings.profile(profile), apt.Rate.hz(RATE), True, max_samples=max(x.size for x in xs),
                    max_batch=len(xs))
    cap = int(plan.info.max_rows)
    d_in = [torch.from_numpy(x).to(dev) for x in xs]
    d_out = [torch.empty(cap * 2080, dtype=torch.float32, device=dev) for _ in xs]
    torch.cuda.synchronize()
    plan.decode_device([t.data_ptr() for t in d_in], [x.size for x in xs], [t.data_ptr() for t in d_out], [cap] * len(xs))
    res = plan.results(len(xs))
    out = []
    for i, x in enumerate(xs):
        n_corr = _oracle(name)[i][1]["correlation"].size
        ng = (n_corr + GS - 1) // GS
        out.append(dict(
            rows=d_out[i][:res[i].n_out].cpu().numpy(), n_sync=int(res[i].n_sync), status=int(res[i].status),
            pos=plan.sync_positions(i),
            words=plan.read_internal("terminal_words", np.uint64, ng, i=i),
            peaks=plan.read_internal("peaks", np.uint32, int(res[i].n_sync), i=i),
            flags=plan.read_internal("picker_flags", np.uint32, 32, i=i),
            gm=plan.read_internal("group_max", f32, 2 * ng, i=i).reshape(ng, 2)))
    plan.close()
    return out


@pytest.fixture(scope="module")
def runs():
    """(case, form) -> what the plan computed; each decoded once and shared by the tests below"""
    torch = pytest.importorskip("torch")
    cache = {}

    def get(name, form, monkeypatch):
        if (name, form) not in cache:
            monkeypatch.setenv("APTGPU_WORDS_FORM", form)  # read when the plan is created
            cache[(name, form)] = _run(name, form, torch)
        return cache[(name, form)]
    return get


@pytest.mark.parametrize("form", ["1", "0"])
@pytest.mark.parametrize("name", NAMES)
def test_words_rows_and_positions_match_the_oracle(oracle, runs, monkeypatch, name, form):
    xs, profile, ngs = _case(name)
    got = runs(name, form, monkeypatch)
    for i, g in enumerate(got):
        want, st = _oracle(name)[i]
        what = f"{name}[{i}] form {form}"
        corr = st["correlation"]
        ng = (corr.size + GS - 1) // GS
        if ngs is not None:
            assert ng == ngs[i], (what, "the case misses the group count it is about", ng, ngs[i])
        assert g["status"] == 0 and g["n_sync"] == st["sync_pos"].size, what
        assert g["pos"].tolist() == st["sync_pos"].tolist(), what
        (assert_same_values if name == "nan-run" else assert_bitexact)(g["rows"], want, what)
        words, keep = _expected_words(corr, g["gm"], PW[profile])
        bad = np.flatnonzero(g["words"] != words)
        assert bad.size == 0, (what, "terminal word of group", int(bad[0]), hex(int(g["words"][bad[0]])),
                               hex(int(words[bad[0]])), "evaluated" if keep[bad[0]] else "pruned")
        # teeth: the coarse pass prunes most groups and keeps some in every chunk-sized stretch of rows
        assert 0 < int(keep.sum()) < ng // 4, (what, int(keep.sum()), ng)
        if name == "nan-run":
            assert np.isnan(corr[5 * CHUNK * GS - 1]) and np.isnan(corr[5 * CHUNK * GS]), "the NaN run misses the chunk boundary"
        if name == "flat":
            b = 5 * CHUNK * GS
            assert np.all(corr[b - 2600:b + 2600] == corr[b]), "the flat stretch misses the chunk boundary"


@pytest.mark.parametrize("name", NAMES)
def test_both_forms_agree(runs, monkeypatch, name):
    new, old = runs(name, "1", monkeypatch), runs(name, "0", monkeypatch)
    for i, (a, b) in enumerate(zip(new, old)):
        what = f"{name}[{i}]"
        assert np.array_equal(a["words"], b["words"]), what
        assert np.array_equal(a["peaks"], b["peaks"]), what
        for k in (0, 1, 7, 11):
            assert int(a["flags"][k]) == int(b["flags"][k]), (what, "picker_flags", k, int(a["flags"][k]), int(b["flags"][k]))
        assert np.array_equal(a["rows"].view(np.uint32), b["rows"].view(np.uint32)), what
