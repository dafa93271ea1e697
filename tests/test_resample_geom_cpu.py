"""apt::ResampleGeom (noaa_apt_amd/csrc/apt_host.hpp): the lengths and the decimation phase of one resample_with_filter
stage, which every caller of the stage — the plan's work length and no-sync output length, the launches, the step
export — reads from this one value.  Checked without a GPU: a small host-only program prints out_len, d0 and
expanded_len for both values of the flag, and the oracle's fast_resampling / fast_resampling_export (l > 1) and
decimate (l == 1: filter + decimate, dsp.rs:106-122) say how many samples the reference's loops produce."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_oracle_export_filtered import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "noaa_apt_amd", "csrc")

PROGRAM = r"""
#include "apt_host.hpp"
#include <cstdio>
int main()
{
    unsigned l, m;
    unsigned long long ntaps, n;
    while (std::scanf("%u %u %llu %llu", &l, &m, &ntaps, &n) == 4)
        for (int flagged = 0; flagged < 2; ++flagged) {
            const apt::ResampleGeom g{l, m, ntaps, flagged != 0};
            std::printf("%llu %llu %llu %u\n", (unsigned long long)g.out_len(n), (unsigned long long)g.d0(n),
                        (unsigned long long)g.expanded_len(n), g.filtered_rate(1000));
        }
    return 0;
}
"""

# (l, m, ntaps, n): the oracle tests' cases, then n == 0, n*l <= off (also among CASES: (3, 2, 41, 5) and
# (13, 50, 959, 20)), n*l == off + 1, m == 1, and l == 1 with and without a remainder of n / m
EDGES = [(13, 50, 959, 0), (3, 2, 1, 0), (3, 2, 41, 6), (3, 2, 41, 7), (13, 50, 959, 37), (3, 1, 5, 40), (4, 1, 1, 9),
         (2, 1, 9, 2), (1, 2, 41, 101), (1, 3, 7, 99), (1, 1, 1, 17), (1, 4, 959, 0), (1, 5, 3, 4)]
ALL = CASES + EDGES


@pytest.fixture(scope="module")
def geom(tmp_path_factory):
    """{(l, m, ntaps, n, flagged): (out_len, d0, expanded_len, filtered_rate(1000))}"""
    d = tmp_path_factory.mktemp("resample_geom")
    (d / "main.cpp").write_text(PROGRAM)
    cxx = shutil.which("c++") or shutil.which("g++")
    cmd = [cxx] if cxx else ["/opt/rocm/bin/hipcc", "-x", "c++"]
    subprocess.run([*cmd, "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-I", CSRC, "-o", str(d / "geom"), str(d / "main.cpp"),
                    os.path.join(CSRC, "apt_host.cpp")], check=True)
    out = subprocess.run([str(d / "geom")], input="".join("%d %d %d %d\n" % c for c in ALL), capture_output=True, text=True,
                         check=True).stdout.split("\n")
    vals = [tuple(int(v) for v in ln.split()) for ln in out if ln]
    assert len(vals) == 2 * len(ALL)
    return {(*c, f): vals[2 * k + f] for k, c in enumerate(ALL) for f in (0, 1)}


@pytest.mark.parametrize("l,m,ntaps,n", ALL)
def test_lengths_and_phase_are_the_reference_loops(oracle, geom, l, m, ntaps, n):
    rng = np.random.default_rng(l + 31 * m + n)
    x = rng.standard_normal(n).astype(np.float32)
    c = rng.standard_normal(ntaps).astype(np.float32)
    plain, flagged = geom[(l, m, ntaps, n, 0)], geom[(l, m, ntaps, n, 1)]
    assert plain[3] == flagged[3] == 1000 * l
    if l == 1:
        # filter() keeps the length, decimate() takes every m-th sample (dsp.rs:299-303); the flag is never looked at
        assert plain == flagged == (oracle.decimate(x, m).size if n else 0, 0, n, 1000)
        return
    nrm = oracle.fast_resampling(x, l, m, c) if n else np.zeros(0, np.float32)
    out, ex = oracle.fast_resampling_export(x, l, m, c) if n else (np.zeros(0, np.float32),) * 2
    assert plain[0] == nrm.size and plain[1] == 0
    assert flagged[0] == out.size
    assert plain[2] == flagged[2] == ex.size
    # the phase: the flagged output is the expanded signal from d0 on, every m-th sum; the normal one from 0 on
    d0 = flagged[1]
    assert np.array_equal(out.view(np.uint32), ex[d0 + np.arange(out.size) * m].view(np.uint32))
    assert np.array_equal(nrm.view(np.uint32), ex[np.arange(nrm.size) * m].view(np.uint32))
    if ex.size == 0:
        assert d0 == 0
