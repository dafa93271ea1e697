#!/usr/bin/env python3
"""tools/geoloc_timing.py [--calls N] [--seconds S] [--recordings R] — device time of the geolocation stage (DESIGN.md
§25): Plan.geolocate_device behind one decode_device call of R recordings (16 ten-minute ones at 48 000 Hz by default:
1198 rows, 1.09 M video pixels each), with the plan's HIP-event timer around every launch, for every output mask:

    latlon   cos   rows   (and their unions; `rows` out of place, so the copy in front is in the figure;
                           `rows_inplace` without it; `none`: the record's counters alone)

Per mask and timer name (image_geoloc_track, image_geoloc_rows, image_geoloc): ms per recording, the median over N
calls after two warm-up calls; for image_geoloc the bytes the mask moves per recording and their share of 8 TB/s;
the wall time per recording of one call of R with the timer off; and image_thermal_map of the same rows in the same
run, the figure to put beside it.  The recordings are one synthetic pass copied R times.
GPU box."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import noaa_apt_amd as apt  # noqa: E402
from noaa_apt_amd.testing.synth import synth_apt  # noqa: E402
import np_map_model as mm  # noqa: E402
import np_thermal_model as tm  # noqa: E402

HBM_BYTES_PER_S = 8e12
NAMES = ("image_geoloc_track", "image_geoloc_rows", "image_geoloc")
# mask name -> (latlon, cos, rows: 0 none, 1 out of place, 2 in place)
MASKS = {"none": (0, 0, 0), "latlon": (1, 0, 0), "cos": (0, 1, 0), "rows": (0, 0, 1), "rows_inplace": (0, 0, 2),
         "latlon_cos": (1, 1, 0), "cos_rows": (0, 1, 1), "all": (1, 1, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--recordings", type=int, default=16)
    ap.add_argument("--rate", type=int, default=48000)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    k = args.recordings
    x = synth_apt(args.rate, args.seconds, 5)
    plan = apt.Plan(apt.Settings(), apt.Rate.hz(args.rate), True, max_samples=x.size, max_batch=k)
    cap = int(plan.info.max_rows)
    d_in = [torch.from_numpy(x).to(dev) for _ in range(k)]
    d_rows = [torch.empty(cap * 2080, dtype=torch.float32, device=dev) for _ in range(k)]
    d_ll = [torch.empty(cap * 909 * 2, dtype=torch.float64, device=dev) for _ in range(k)]
    d_cos = [torch.empty(cap * 909, dtype=torch.float32, device=dev) for _ in range(k)]
    d_out = [torch.empty(cap * 2080, dtype=torch.float32, device=dev) for _ in range(k)]
    ptr = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
    plan.decode_device(ptr(d_in), [x.size] * k, ptr(d_rows), [cap] * k)
    h = int(plan.results(1)[0].n_out) // 2080
    px = h * 909
    print(f"# {torch.cuda.get_device_name(0)}; {k} recordings of {args.seconds:g} s at {args.rate} Hz per call, {h} rows = "
          f"{px} video pixels each, {args.calls} calls per mask; ms per recording")
    track = mm.great_circle_track(52.0, 8.0, 192.0, h)
    st = apt.GeolocSettings(channel="A", ref_time=apt.RefTime.Start(1730635200000), black=0.0)
    print("mask,timer,ms_per_recording_median,ms_min,note")
    for name, (want_ll, want_cos, want_rows) in MASKS.items():
        a_ll = ptr(d_ll) if want_ll else None
        a_cos = ptr(d_cos) if want_cos else None
        a_out = None if want_rows == 0 else ptr(d_out) if want_rows == 1 else ptr(d_rows)

        def call():
            plan.geolocate_device(ptr(d_rows), [cap] * k, [track] * k, st, None, a_ll, a_cos, a_out)
        plan.enable_timing(0)
        for _ in range(2):
            call()
        plan.synchronize()
        t0 = time.perf_counter()
        call()
        plan.synchronize()
        wall = (time.perf_counter() - t0) / k * 1e3
        plan.enable_timing(2)
        ms = {n: [] for n in NAMES}
        for _ in range(args.calls):
            call()
            t = plan.collect_timing()
            for n in NAMES:
                ms[n].append(t[n][0])
        rec = plan.geoloc_results(k)
        assert all(r.status == 0 and r.height == h for r in rec), [(r.status, r.reason) for r in rec]
        # stores of the planes, load and store of the video (and, out of place, the copy of the whole rows both ways)
        nbytes = px * (16 * want_ll + 4 * want_cos + (8 if want_rows else 0)) + (2 * cap * 2080 * 4 if want_rows == 1 else 0)
        for n in NAMES:
            med, lo = float(np.median(ms[n])), float(min(ms[n]))
            note = ""
            if n == "image_geoloc":
                note = (f"{nbytes / 1e6:.2f} MB per recording -> {nbytes / (med * 1e-3) / 1e12:.3f} TB/s = "
                        f"{nbytes / (med * 1e-3) / HBM_BYTES_PER_S * 100:.1f} % of 8 TB/s; "
                        f"{px / (med * 1e-3) / 1e9:.2f} G pixels/s")
            print(f"{name},{n},{med:.4f},{lo:.4f},{note}")
        print(f"{name},sum (events),{sum(float(np.median(ms[n])) for n in NAMES):.4f},,")
        print(f"{name},wall / rec,{wall:.4f},,one call of {k}, timing off; record: {rec[0].n_outside} outside, "
              f"{rec[0].n_capped} capped, cos {rec[0].cos_min:.3f} .. {rec[0].cos_max:.3f}")
    # image_thermal_map of the same rows in the same run
    co = apt.ThermalCoefficients(tm.PRT, tm.CH3B, tm.CH4, tm.CH5)
    ts = apt.ThermalSettings("B", "4", t_low=180, t_high=320, image_channels=0)
    d_kelvin = [torch.empty(cap * 909, dtype=torch.float32, device=dev) for _ in range(k)]
    plan.decode_device(ptr(d_in), [x.size] * k, ptr(d_rows), [cap] * k)
    vals = []
    for _ in range(args.calls + 2):
        plan.calibrate_thermal_device(ptr(d_rows), [cap] * k, ptr(d_kelvin), co, ts)
        vals.append(plan.collect_timing()["image_thermal_map"][0])
    print(f"thermal_kelvin,image_thermal_map,{float(np.median(vals[2:])):.4f},{min(vals[2:]):.4f},the same rows, the same run")
    plan.close()


if __name__ == "__main__":
    main()
