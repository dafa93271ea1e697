"""Which front end a plan gets (noaa_apt_amd/csrc/apt_front_end.hpp: select_front_end), checked without a GPU: a small
host-only program goes from (input rate, settings, mode, export_resample_filtered, APTGPU_* switches) through the
project's own filter design (design_plan) and switch reader (read_plan_switches) to select_front_end and prints, per case,
the record the plan would store — kind, kernel mode, both variants, the padding bounds, the flags, the LDS floats, every
TableGeom field — and a 64-bit FNV-1a hash of the stage-1 table the PHASE / TABLE / run-time kernels would be given.

The expectations (tests/golden/front_end_choice.txt: the distinct records, which of them each case of _cases() gets, in
its order, and a hash of the case list) were NOT made by this code: they were recorded from commit f671802, the last
one in which plan_create decided the front end inline and run_call decided the kernel again at every launch.  That commit's decision block of plan_create (apt_plan.hip), its table-upload block, the
launch-time dispatch of run_call and the host functions of its apt_kernels_fused.hip / apt_kernels_fused_any.hip were
compiled unchanged into a scratch harness with the HIP calls stubbed, and each case's switches were given to it through
setenv.  A wrong choice is invisible to the GPU tests where two kernels compute the same bits (the stock 48 kHz plan on the
padded kernel is only slower): this table is what pins it."""
import hashlib
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "noaa_apt_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "front_end_choice.txt")

PROGRAM = r"""
#include "apt_front_end.hpp"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
using namespace apt;
using namespace apt::gpu;
static uint64_t fnv1a(const void *p, size_t n)
{
    const unsigned char *b = static_cast<const unsigned char *>(p);
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}
int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream is(line);
        aptgpu_settings st{};
        uint32_t rate = 0;
        int mode = 0, exportf = 0;
        is >> rate >> st.work_rate >> st.resample_atten >> st.resample_delta_freq >> st.resample_cutout >> st.demodulation_atten >>
            mode >> exportf;
        st.export_resample_filtered = exportf;
        std::vector<std::string> names;
        std::string kv;
        while (is >> kv) {
            const size_t eq = kv.find('=');
            names.push_back(kv.substr(0, eq));
            setenv(names.back().c_str(), kv.substr(eq + 1).c_str(), 1);
        }
        try {
            const PlanDesign d = design_plan(st, rate, true);
            const PlanSwitches sw = read_plan_switches();
            const uint32_t t1 = static_cast<uint32_t>(d.taps_resample.size()), t2 = static_cast<uint32_t>(d.taps_lowpass.size());
            const FrontEnd fe = select_front_end(d.l, d.m, t1, t2, d.pw, mode, d.work_is_multiple, exportf != 0, sw);
            uint64_t hash = 0;
            if (fe.kind == FrontEndKind::Any || fe.kind == FrontEndKind::Table || fe.kind == FrontEndKind::Phase) {
                const bool phase = fe.kind == FrontEndKind::Phase;
                std::vector<float> tab(static_cast<size_t>(phase ? fused_phase_table_floats(fe.geom) : fused_any_table_floats(d.l, t1)) + 16, 0.f);
                if (phase)
                    fused_phase_table(fe.geom, static_cast<uint32_t>(kFusedVariants[fe.variant[0]].t2), d.pw, d.taps_resample.data(),
                                      tab.data(), sw);
                else fused_any_table(d.l, d.taps_resample.data(), t1, tab.data());
                hash = fnv1a(tab.data(), tab.size() * sizeof(float));
            }
            const TableGeom &g = fe.geom;
            std::printf("l=%u m=%u t1=%u t2=%u pw=%u kind=%d kmode=%d f32=%s i16=%s pad_t1=%u pad_t2=%u fast=%d f16=%d mfma=%d lds=%zu geom=",
                        d.l, d.m, t1, t2, d.pw, static_cast<int>(fe.kind), fe.kmode,
                        fe.variant[0] == kFusedNone ? "none" : kFusedVariants[fe.variant[0]].name,
                        fe.variant[1] == kFusedNone ? "none" : kFusedVariants[fe.variant[1]].name, fe.pad_t1, fe.pad_t2, fe.fast ? 1 : 0,
                        fe.f16 ? 1 : 0, fe.mfma ? 1 : 0, fe.lds_floats);
            const uint32_t f[] = {g.l, g.m, g.jlim, g.tpp, g.xt, g.off_x, g.step_q, g.step_r, g.jl_a, g.jl_b, g.nthr, g.perm_off, g.nperm,
                                  g.nq, g.sq, g.stream, g.exact, g.perm_shift, g.cp_off, g.xd, g.tt_off};
            for (uint32_t x : f) std::printf("%u,", x);
            for (int i = 0; i < 8; ++i) std::printf("%d,", g.x0r[i]);
            for (int i = 0; i < 8; ++i) std::printf("%u%s", g.rbr[i], i < 7 ? "," : "");
            std::printf(" table=%016llx\n", static_cast<unsigned long long>(hash));
        } catch (const Error &e) {
            std::printf("error kind=%d\n", static_cast<int>(e.kind));
        }
        for (const std::string &n : names) unsetenv(n.c_str());
    }
    return 0;
}
"""

RATES = (8000, 11025, 12000, 16000, 22050, 32000, 44100, 48000, 96000, 192000, 206000, 250000,
         44101)  # (44101: coprime to every profile's work rate)
# work_rate, resample_atten, resample_delta_freq, resample_cutout, demodulation_atten
PROFILES = {"standard": (12480, 30.0, 1000.0, 4800.0, 25.0), "fast": (16640, 30.0, 3000.0, 4800.0, 23.0),
            "slow": (20800, 40.0, 500.0, 4800.0, 25.0)}
STRICT, GENERIC, FP16_TAPS, FAST = range(4)  # APTGPU_MODE_*
SWITCHES = ("APTGPU_FUSED_ANY=1", "APTGPU_PHASE_FIRST=0", "APTGPU_FAST_MFMA=0", "APTGPU_FAST_MFMA=1", "APTGPU_FUSED_PAD=0",
            "APTGPU_FUSED_PAD=1", "APTGPU_PHASE_WIDE=1", "APTGPU_PHASE_BALANCED=0", "APTGPU_PHASE_BALANCED=1",
            "APTGPU_PHASE_TT=0", "APTGPU_PHASE_IDENTITY=1", "APTGPU_TABLE_LDS_KB=16", "APTGPU_TABLE_LDS_KB=160")


def _line(rate, settings, mode, export, *switches):
    return " ".join([str(rate), "%d %g %g %g %g" % settings, str(mode), str(export), *switches])


def _tuned(profile, **kw):
    names = ("work_rate", "resample_atten", "resample_delta_freq", "resample_cutout", "demodulation_atten")
    return tuple(kw.get(n, v) for n, v in zip(names, PROFILES[profile]))


def _cases():
    """The input lines of the program: rate, the five settings, mode, export_resample_filtered, switches."""
    out = []
    for rate in RATES:
        for settings in PROFILES.values():
            for mode in (STRICT, GENERIC, FP16_TAPS, FAST):
                for export in (0, 1):
                    out.append(_line(rate, settings, mode, export))
    # tuned filters: another resampler tap count, another low-pass length (49 dB: 87 low-pass taps, beyond the bound of 45)
    tuned = [dict(resample_atten=29.0), dict(resample_atten=31.0), dict(resample_delta_freq=900.0),
             dict(resample_delta_freq=1100.0), dict(demodulation_atten=24.0), dict(demodulation_atten=26.0),
             dict(demodulation_atten=49.0), dict(resample_atten=31.0, demodulation_atten=26.0)]
    for rate in (11025, 22050, 44100, 48000, 96000):
        for kw in tuned:
            for mode in (STRICT, FAST, FP16_TAPS):
                out.append(_line(rate, _tuned("standard", **kw), mode, 0))
    for profile in ("fast", "slow"):
        for rate in (44100, 48000, 96000):
            for kw in (dict(resample_atten=PROFILES[profile][1] + 1.0), dict(demodulation_atten=PROFILES[profile][4] + 1.0)):
                for mode in (STRICT, FAST):
                    out.append(_line(rate, _tuned(profile, **kw), mode, 0))
    # every switch alone
    for sw in SWITCHES:
        for rate in (8000, 11025, 22050, 44100, 48000, 96000):
            for settings in PROFILES.values():
                for mode in (STRICT, FAST):
                    out.append(_line(rate, settings, mode, 0, sw))
    # ... and with a tuned filter, where the padded and matrix-core kernels are in play (APTGPU_FUSED_PAD=0 with a tuned
    # low-pass at 44 100 Hz: the plan's fast flag used to come from a second read of the environment)
    for sw in ("APTGPU_FUSED_ANY=1", "APTGPU_FAST_MFMA=0", "APTGPU_FAST_MFMA=1", "APTGPU_FUSED_PAD=0", "APTGPU_FUSED_PAD=1",
               "APTGPU_PHASE_FIRST=0"):
        for rate in (44100, 48000, 96000):
            for kw in (dict(resample_atten=31.0), dict(demodulation_atten=26.0)):
                for mode in (STRICT, FAST):
                    out.append(_line(rate, _tuned("standard", **kw), mode, 0, sw))
    return out


def _golden():
    """(number of cases, sha256 of the case list, the expected line per case)"""
    geoms, recs, idx, count, sha, keys = {}, {}, [], None, None, []
    with open(GOLDEN) as f:
        for ln in f:
            kind, _, rest = ln.rstrip("\n").partition(" ")
            if kind == "cases":
                count, _, sha = rest.split()
            elif kind == "geom":
                n, _, text = rest.partition(" ")
                geoms[int(n)] = text
            elif kind == "keys":
                keys = rest.split()
            elif kind == "rec":
                n, *values, g = rest.split()
                assert len(values) == len(keys)
                recs[int(n)] = " ".join(k + "=" + v for k, v in zip(keys, values)) + " geom=" + geoms[int(g)]
            elif kind == "idx":
                idx += [int(x) for x in rest.split()]
    return int(count), sha, [recs[i] for i in idx]


@pytest.fixture(scope="module")
def chosen(tmp_path_factory):
    """The program's record per case."""
    d = tmp_path_factory.mktemp("front_end_choice")
    (d / "main.cpp").write_text(PROGRAM)
    cxx = shutil.which("c++") or shutil.which("g++")
    cmd = [cxx] if cxx else ["/opt/rocm/bin/hipcc", "-x", "c++"]
    # (-ffp-contract=off: the filter design rounds every product and sum separately, as in the library's build)
    subprocess.run([*cmd, "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-I", CSRC, "-o", str(d / "choice"), str(d / "main.cpp"),
                    os.path.join(CSRC, "apt_front_end.cpp"), os.path.join(CSRC, "apt_host.cpp")], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("APTGPU_")}
    env["APTGPU_QUIET"] = "1"
    out = subprocess.run([str(d / "choice")], input="".join(c + "\n" for c in _cases()), capture_output=True, text=True,
                         check=True, env=env).stdout
    return out.splitlines()


def test_the_recorded_table_covers_exactly_these_cases():
    cases, (count, sha, want) = _cases(), _golden()
    assert len(set(cases)) == len(cases) == count == len(want)
    assert hashlib.sha256("\n".join(cases).encode()).hexdigest() == sha


def test_every_case_gets_the_front_end_the_inline_decision_gave_it(chosen):
    want = _golden()[2]
    assert len(chosen) == len(want)
    wrong = [(case, w, got) for case, w, got in zip(_cases(), want, chosen) if w != got]
    assert not wrong, (len(wrong), wrong[:5])


def test_the_cases_reach_every_kind_and_every_instantiation(chosen):
    """(a table that never left one family would pin little)"""
    fields = [dict(kv.split("=", 1) for kv in ln.split()) for ln in chosen]
    assert {f["kind"] for f in fields} == {"0", "1", "2", "3", "4"}
    rows = subprocess.run(["sed", "-n", r"s/^ *\(BOTH\|F32\)(\([0-9a-z_]*\),.*/\2/p",
                           os.path.join(CSRC, "apt_kernels_fused_variants.hpp")], capture_output=True, text=True, check=True).stdout.split()
    assert len(rows) == 41 and set(rows) == {f["f32"] for f in fields} - {"none"}
    assert all(f["i16"] in (f["f32"], "none") for f in fields)
    assert any(int(f["t2"]) > 45 for f in fields) and any(f["pad_t2"] != "0" and f["kind"] == "4" for f in fields)
