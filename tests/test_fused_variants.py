"""Which k_fused instantiation serves which plan (noaa_apt_amd/csrc/apt_kernels_fused_variants.hpp), checked without a
GPU: a small host-only program includes the header and prints the variant its selection functions choose for a list of
cases; the expectations below were written from the three if-chains those functions replaced (fused_front_end,
fused_table_front_end and fused_phase_front_end dispatched and launched in one statement until then), with the numbers
those chains spelled out — not from the functions under test.  A wrong choice is invisible to the GPU tests where two
kernels compute the same thing (stock 48 kHz on the padded kernel is bit-identical, only slower)."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "noaa_apt_amd", "csrc")

STRICT, F16TAPS, FAST, MFMA, PAD, PAD2 = range(6)  # k_fused's MODE argument (kModeStrict ... kModeStrictPad2)

PROGRAM = r"""
#include "apt_kernels_fused_variants.hpp"
#include <cstdio>
#include <cstring>
using namespace apt::gpu;
int main()
{
    char kind[16];
    while (std::scanf("%15s", kind) == 1) {
        unsigned a[6] = {0, 0, 0, 0, 0, 0};
        int mode = 0;
        FusedVariant v = kFusedNone;
        if (!std::strcmp(kind, "rows")) {
            for (const FusedVariantRow &r : kFusedVariants)
                std::printf("%s %d %d %d %d %d %d %d %d\n", r.name, r.l, r.m, r.t1, r.t2, r.pw, r.nthr, r.mode, r.i16 ? 1 : 0);
            continue;
        } else if (!std::strcmp(kind, "split")) {  // l m t1 t2 pw mode pcm16
            if (std::scanf("%u %u %u %u %u %d %u", &a[0], &a[1], &a[2], &a[3], &a[4], &mode, &a[5]) != 7) return 2;
            v = fused_split_variant(a[0], a[1], a[2], a[3], a[4], mode, a[5] != 0);
        } else if (!std::strcmp(kind, "table")) {  // mode
            if (std::scanf("%d", &mode) != 1) return 2;
            v = fused_table_variant(mode);
        } else if (!std::strcmp(kind, "phase")) {  // nq nthr stream t2 pw mode
            if (std::scanf("%u %u %u %u %u %d", &a[0], &a[1], &a[2], &a[3], &a[4], &mode) != 6) return 2;
            v = fused_phase_variant(a[0], a[1], a[2] != 0, a[3], a[4], mode);
        } else {
            return 2;
        }
        std::puts(v == kFusedNone ? "none" : kFusedVariants[v].name);
    }
    return 0;
}
"""

# ---- SPLIT (fused_front_end): (l, m, t1, t2, pw) of the five stock geometries
G48, G96 = (13, 50, 959, 37, 3), (13, 100, 1915, 37, 3)
G48S, G96S, G96F = (13, 30, 2783, 61, 5), (13, 60, 5565, 61, 5), (13, 75, 639, 43, 4)
# geometry -> mode -> (kernel for f32 input, kernel for 16-bit PCM input)
STOCK = {
    G48: {STRICT: ("48k", "48k"), FAST: ("48k_fast", "48k_fast"), F16TAPS: ("48k_f16taps", "48k_f16taps"),
          MFMA: ("48k_mfma", "48k_mfma"), PAD: ("48k_pad", "48k_pad")},
    G96: {STRICT: ("96k", "96k"), FAST: ("96k_fast", "96k_fast"), F16TAPS: ("none", "none"),
          MFMA: ("96k_mfma", "96k_mfma"), PAD: ("96k_pad", "96k_pad")},
    G48S: {STRICT: ("48k_slow", "48k_slow"), FAST: ("48k_slow_fast", "48k_slow_fast"), F16TAPS: ("none", "none"),
           MFMA: ("none", "none"), PAD: ("48k_slow_pad", "48k_slow_pad")},
    # (fast mode at 96 kHz / slow and fast profiles: no fast instantiation — the front end refuses, and the plan, which asks
    # fused_fast_supported first, runs the strict kernel)
    G96S: {STRICT: ("96k_slow", "96k_slow"), FAST: ("none", "none"), F16TAPS: ("none", "none"),
           MFMA: ("none", "none"), PAD: ("96k_slow_pad", "96k_slow_pad")},
    # (odd m: f32 input only)
    G96F: {STRICT: ("96k_fastp", "none"), FAST: ("none", "none"), F16TAPS: ("none", "none"),
           MFMA: ("none", "none"), PAD: ("96k_fastp_pad", "none")},
}
# tuned filters: ((l, m, t1, t2, pw), mode, pcm16) -> kernel
TUNED = [
    # a tuned resampler: t1 at each padded kernel's bound, and the next odd count above it
    ((13, 50, 1079, 37, 3), PAD, 0, "48k_pad"), ((13, 50, 1081, 37, 3), PAD, 0, "none"),
    ((13, 100, 2145, 37, 3), PAD, 1, "96k_pad"), ((13, 100, 2147, 37, 3), PAD, 1, "none"),
    ((13, 30, 3133, 61, 5), PAD, 0, "48k_slow_pad"), ((13, 30, 3135, 61, 5), PAD, 0, "none"),
    ((13, 60, 6253, 61, 5), PAD, 1, "96k_slow_pad"), ((13, 60, 6255, 61, 5), PAD, 1, "none"),
    ((13, 75, 727, 43, 4), PAD, 0, "96k_fastp_pad"), ((13, 75, 729, 43, 4), PAD, 0, "none"),
    ((13, 75, 727, 43, 4), PAD, 1, "none"),
    ((13, 50, 961, 37, 3), PAD, 0, "48k_pad"), ((13, 50, 960, 37, 3), PAD, 0, "none"),  # (Kaiser lengths are odd)
    ((13, 50, 961, 61, 5), PAD, 0, "none"), ((13, 30, 2785, 37, 3), PAD, 0, "none"),    # (a profile's stages at another's rate)
    ((12, 50, 959, 37, 3), PAD, 0, "none"),
    # ... on the matrix cores
    ((13, 50, 1053, 37, 3), MFMA, 0, "48k_mfma"), ((13, 50, 1055, 37, 3), MFMA, 1, "none"),
    ((13, 100, 2119, 37, 3), MFMA, 1, "96k_mfma"), ((13, 100, 2121, 37, 3), MFMA, 0, "none"),
    ((13, 50, 958, 37, 3), MFMA, 0, "none"), ((13, 50, 959, 35, 3), MFMA, 0, "none"),
    # ... with no padded mode asked for: only the exact counts have kernels
    ((13, 50, 961, 37, 3), STRICT, 0, "none"), ((13, 50, 961, 37, 3), FAST, 0, "none"),
    # a tuned low-pass: odd t2 <= 45 other than the profile's 37 takes the kernel whose low-pass length is a bound too
    ((13, 50, 959, 35, 3), PAD, 0, "48k_pad2"), ((13, 50, 1079, 45, 3), PAD, 1, "48k_pad2"),
    ((13, 100, 1915, 39, 3), PAD, 0, "96k_pad2"), ((13, 100, 2145, 45, 3), PAD, 1, "96k_pad2"),
    ((13, 50, 1081, 35, 3), PAD, 0, "none"),
    ((13, 50, 959, 37, 3), PAD, 1, "48k_pad"), ((13, 50, 959, 36, 3), PAD, 0, "none"), ((13, 50, 959, 47, 3), PAD, 0, "none"),
    ((13, 100, 1915, 36, 3), PAD, 1, "none"), ((13, 100, 1915, 47, 3), PAD, 1, "none"),
    ((13, 50, 959, 35, 3), STRICT, 0, "none"), ((13, 50, 959, 35, 3), FAST, 0, "none"),
    # any other mode value falls where strict does at the geometries whose chain only asked "not fp16 taps"
    (G48, PAD2, 0, "48k"), (G96, PAD2, 1, "96k"), (G48S, PAD2, 0, "48k_slow"), (G96S, PAD2, 0, "none"), (G96F, PAD2, 0, "none"),
]

# ---- TABLE (fused_table_front_end)
TABLE = {STRICT: "tab_std", FAST: "tab_std_fast", F16TAPS: "none", MFMA: "none", PAD: "none"}

# ---- PHASE (fused_phase_front_end)
PHASE_NQ, PHASE_NTHR = (0, 1, 2, 4, 8, 16), (256, 512, 1024)
PHASE_PROFILES = ((37, 3), (61, 5), (43, 4),               # standard, slow, fast
                  (35, 3), (45, 3), (36, 3), (47, 3))      # a tuned low-pass at the standard profile's pixel width


def _phase_expected(nq, nthr, stream, t2, pw, mode):
    """fused_phase_front_end's chain as it stood, branch by branch in its order."""
    wide, huge = nthr == 512, nthr == 1024
    if (t2, pw) == (61, 5):      # slow profile: streamed taps, strict instantiations only (they serve fast mode too)
        if wide or huge or not stream:
            return "none"
        return {1: "phase_slowp", 2: "phase2_slowp", 4: "phase4_slowp"}.get(nq, "none")
    if (t2, pw) == (43, 4) and nq > 1:   # fast profile, several branches per thread: strict instantiations only
        if wide or huge:
            return "none"
        return {4: "phase4_fastp", 8: "phase8_fastp", 16: "phase16_fastp"}.get(nq, "none")
    if (t2, pw) == (43, 4):
        if wide or huge:
            return "none"
        return {FAST: "phase_fastp_fast", STRICT: "phase_fastp"}.get(mode, "none")
    if pw == 3 and t2 != 37:     # a tuned low-pass: the pad2 kernel whatever the mode
        if wide or huge or t2 % 2 == 0 or t2 > 45:
            return "none"
        return {0: "phase_std_pad2", 1: "phase_std_pad2", 2: "phase2_std_pad2", 4: "phase4_std_pad2"}.get(nq, "none")
    suffix = {FAST: "_fast", STRICT: ""}.get(mode)
    if nq in (2, 4):
        if wide or huge or suffix is None:
            return "none"
        return f"phase{nq}_std{suffix}"
    if suffix is None:
        return "none"
    return ("phase1024_std" if huge else "phase512_std" if wide else "phase_std") + suffix


def _cases():
    """(input line of the program, expected variant name)"""
    cases = []
    for geom, by_mode in STOCK.items():
        for mode, names in by_mode.items():
            for pcm16 in (0, 1):
                cases.append(("split %d %d %d %d %d %d %d" % (*geom, mode, pcm16), names[pcm16]))
    for geom, mode, pcm16, name in TUNED:
        cases.append(("split %d %d %d %d %d %d %d" % (*geom, mode, pcm16), name))
    for mode, name in TABLE.items():
        cases.append(("table %d" % mode, name))
    for nq, nthr, stream, (t2, pw), mode in itertools.product(PHASE_NQ, PHASE_NTHR, (0, 1), PHASE_PROFILES,
                                                              (STRICT, FAST, F16TAPS, MFMA, PAD)):
        cases.append(("phase %d %d %d %d %d %d" % (nq, nthr, stream, t2, pw, mode),
                      _phase_expected(nq, nthr, stream, t2, pw, mode)))
    return cases


@pytest.fixture(scope="module")
def chosen(tmp_path_factory):
    """The program's answers: (rows of the table, variant name per case)."""
    d = tmp_path_factory.mktemp("fused_variants")
    (d / "main.cpp").write_text(PROGRAM)
    cxx = shutil.which("c++") or shutil.which("g++")
    cmd = [cxx] if cxx else ["/opt/rocm/bin/hipcc", "-x", "c++"]
    subprocess.run([*cmd, "-std=c++17", "-Wall", "-I", CSRC, "-o", str(d / "variants"), str(d / "main.cpp")], check=True)
    stdin = "rows\n" + "".join(line + "\n" for line, _ in _cases())
    out = subprocess.run([str(d / "variants")], input=stdin, capture_output=True, text=True, check=True).stdout.split("\n")
    rows = [ln.split() for ln in out if " " in ln]
    return rows, [ln for ln in out if ln and " " not in ln]


def test_every_case_gets_the_kernel_the_dispatch_chains_gave_it(chosen):
    _, names = chosen
    cases = _cases()
    assert len(names) == len(cases)
    wrong = [(line, want, got) for (line, want), got in zip(cases, names) if want != got]
    assert not wrong, wrong[:20]


def test_a_few_phase_rows_spelled_out(chosen):
    """(the PHASE expectations come from a transcription of the chain: these pin the transcription itself)"""
    got = dict(zip((line for line, _ in _cases()), chosen[1]))
    for line, want in (("phase 1 256 0 37 3 0", "phase_std"), ("phase 1 256 0 37 3 2", "phase_std_fast"),
                       ("phase 1 512 0 37 3 0", "phase512_std"), ("phase 1 1024 0 37 3 2", "phase1024_std_fast"),
                       ("phase 2 256 0 37 3 2", "phase2_std_fast"), ("phase 4 256 0 37 3 0", "phase4_std"),
                       ("phase 2 512 0 37 3 0", "none"), ("phase 1 256 0 37 3 4", "none"),
                       ("phase 1 256 1 61 5 2", "phase_slowp"), ("phase 4 256 1 61 5 0", "phase4_slowp"),
                       ("phase 1 256 0 61 5 0", "none"), ("phase 0 256 1 61 5 0", "none"), ("phase 8 256 1 61 5 0", "none"),
                       ("phase 1 256 0 43 4 2", "phase_fastp_fast"), ("phase 0 256 0 43 4 0", "phase_fastp"),
                       ("phase 8 256 0 43 4 2", "phase8_fastp"), ("phase 16 256 0 43 4 0", "phase16_fastp"),
                       ("phase 2 256 0 43 4 0", "none"), ("phase 4 512 0 43 4 0", "none"),
                       ("phase 0 256 0 35 3 2", "phase_std_pad2"), ("phase 4 256 0 45 3 0", "phase4_std_pad2"),
                       ("phase 2 256 0 35 3 1", "phase2_std_pad2"), ("phase 1 256 0 47 3 0", "none"),
                       ("phase 1 256 0 36 3 0", "none"), ("phase 1 1024 0 35 3 0", "none"), ("phase 8 256 0 35 3 0", "none")):
        assert got[line] == want, (line, got[line], want)


def test_no_dead_instantiation_and_unique_names(chosen):
    rows, names = chosen
    row_names = [r[0] for r in rows]
    assert len(row_names) == 41 and len(set(row_names)) == len(row_names)
    assert sum(2 if r[8] == "1" else 1 for r in rows) == 80   # the objects the library is linked from
    assert sorted(r[0] for r in rows if r[8] == "0") == ["96k_fastp", "96k_fastp_pad"]
    assert len({tuple(r[1:8]) for r in rows}) == len(rows)   # no two rows instantiate the same kernel
    assert set(row_names) - set(names) == set()              # every row serves at least one case
    assert set(names) - set(row_names) == {"none"}
