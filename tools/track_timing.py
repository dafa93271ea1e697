#!/usr/bin/env python3
"""tools/track_timing.py [--calls N] [--seconds S] [--recordings R] [--configs a,b] — device time of the flywheel sync
stage: Plan.track_device behind one decode_device call of R recordings (16 ten-minute ones by default),
with the plan's HIP-event timer around every kernel, at

    std_11025    11 025 Hz, standard profile (pw = 3, F in pixel-phase planes)
    fast_48000   48 000 Hz, fast profile     (pw = 4)

Per configuration and kernel (track_score, track_dp, track_rows): ms per launch, median and minimum of N calls after
two warm-up calls; for the score kernel also the lane operations it issues (4 G + 1 per work sample: three chain
steps and a share of the square) against the measured time, and its 8 bytes of traffic per work sample at 8 TB/s; for
the dynamic programme the barriers of its chain (M / (L - w)).  The recordings are one synthetic pass copied R times
(the kernels' time does not depend on the values).
GPU box."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import noaa_apt_amd as apt  # noqa: E402
from noaa_apt_amd.testing.synth import synth_apt  # noqa: E402

CONFIGS = {"std_11025": (11025, "standard"), "fast_48000": (48000, "fast")}
HBM_BYTES_PER_S = 8e12
KERNELS = ("track_score", "track_dp", "track_rows")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--recordings", type=int, default=16)
    ap.add_argument("--jitter", type=int, default=8)
    ap.add_argument("--penalty", type=float, default=0.1)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    k = args.recordings
    print(f"# {torch.cuda.get_device_name(0)}; {k} recordings of {args.seconds:g} s per launch, {args.calls} calls, "
          f"w = {args.jitter}, lambda = {args.penalty:g}")
    print("config,kernel,work_samples_per_recording,ms_median,ms_min,note")
    for name in args.configs.split(","):
        rate, profile = CONFIGS[name]
        settings = apt.Settings.profile(profile)
        pw = settings.work_rate // 4160
        x = synth_apt(rate, args.seconds, 5, noise_sigma=8000.0)
        plan = apt.Plan(settings, apt.Rate.hz(rate), True, max_samples=x.size, max_batch=k)
        cap = int(plan.info.max_rows)
        d_in = [torch.from_numpy(x).to(dev) for _ in range(k)]
        d_rows = [torch.empty(cap * 2080, dtype=torch.float32, device=dev) for _ in range(k)]
        d_trk = [torch.empty(cap * 2080, dtype=torch.float32, device=dev) for _ in range(k)]
        plan.decode_device([t.data_ptr() for t in d_in], [x.size] * k, [t.data_ptr() for t in d_rows], [cap] * k)
        w_len = int(plan.results(1)[0].work_len)
        st = apt.TrackSettings(args.jitter, args.penalty)
        trk_p = [t.data_ptr() for t in d_trk]
        for _ in range(2):
            plan.track_device(trk_p, [cap] * k, st)
        plan.synchronize()
        plan.enable_timing(2)
        ms = {kn: [] for kn in KERNELS}
        for _ in range(args.calls):
            plan.track_device(trk_p, [cap] * k, st)
            t = plan.collect_timing()  # (one launch of each kernel since the last collect)
            for kn in KERNELS:
                ms[kn].append(t[kn][0])
        res = plan.track_results(k)
        assert all(r.status == 0 for r in res), [(r.status, r.reason) for r in res]
        g, L = 38 * pw, 2080 * pw
        for kn in KERNELS:
            med, lo = float(np.median(ms[kn])), float(min(ms[kn]))
            if kn == "track_score":
                ops = (4 * g + 1) * w_len * k
                hbm_ms = 8.0 * w_len * k / HBM_BYTES_PER_S * 1e3
                note = f"{ops / (med * 1e-3) / 1e12:.2f} T lane-ops/s; 8 B/sample at 8 TB/s = {hbm_ms:.3f} ms"
            elif kn == "track_dp":
                chunks = (w_len - g + L - args.jitter - 1) // (L - args.jitter)
                note = f"{chunks} chunks of {L - args.jitter} positions; {res[0].n_positions} positions back-tracked; " \
                       f"{med * 1e3 / chunks:.2f} us per chunk"
            else:
                note = f"{res[0].n_rows} rows per recording"
            print(f"{name},{kn},{w_len},{med:.3f},{lo:.3f},{note}")
        plan.close()
        del d_in, d_rows, d_trk
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
