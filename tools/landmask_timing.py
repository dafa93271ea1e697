#!/usr/bin/env python3
"""tools/landmask_timing.py [--calls N] [--seconds S] [--recordings R] [--bands B] [--oneshot] — device time of the land /
sea / lake mask: Plan.land_mask_device behind one decode_device call of R recordings (16 ten-minute ones
at 48 000 Hz by default: 1198 rows, 1.09 M video pixels each) over the fixture layers, with the plan's HIP-event timer
around every launch.

Per timer name (image_geoloc_track, image_geoloc_rows, image_land_mask): ms per recording, the median over N calls after
two warm-up calls, for the track form and the orbit form; image_geoloc of Plan.geolocate_device with the lat / lon plane
alone on the same rows in the same run, the figure to put beside it.  Only the swath source is timed with events: the
plane source and the colouriser have no plan form, so no timer brackets their launches.  Their one-shot calls (the
plane form on that plane) are timed as wall time per call, which holds their uploads and downloads; their kernels
alone (k_land_mask<Plane>, k_false_color_masked) come from `rocprofv3 --kernel-trace --stats -- python
tools/landmask_timing.py --oneshot`, which runs just those calls.
GPU box."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import noaa_apt_amd as apt  # noqa: E402
from noaa_apt_amd.testing.synth import synth_apt  # noqa: E402
import np_map_model as mm  # noqa: E402

SHP = os.path.join(ROOT, "tests", "golden", "shapefiles")
NAMES = ("image_geoloc_track", "image_geoloc_rows", "image_land_mask")
TLE = open(os.path.join(ROOT, "tests", "golden", "tle", "noaa_2020.txt")).read()


def layers_of():
    return apt.MapLayers(countries=apt.read_shapefile(os.path.join(SHP, "countries.shp"), 5),
                         lakes=apt.read_shapefile(os.path.join(SHP, "lakes.shp"), 5))


def oneshot(h, calls, layers, st):
    """the plane form on the swath's own plane, and the colouriser: wall time per call"""
    track = mm.great_circle_track(-20.0, -58.0, 190.0, h)
    ll, _, _ = apt.geolocate(h, track)
    mask, info = apt.land_mask(h, track, layers, None, st)
    rng = np.random.default_rng(1)
    gray = rng.integers(0, 256, (h, 2080), dtype=np.uint8)
    pals = [rng.integers(0, 256, (256, 256, 3), dtype=np.uint8) for _ in range(3)]
    out = {}
    for name, fn in (("land_mask_plane (one-shot call)", lambda: apt.land_mask_plane(ll, layers, st)),
                     ("land_mask (one-shot call)", lambda: apt.land_mask(h, track, layers, None, st)),
                     ("false_color_masked (one-shot call)", lambda: apt.false_color_masked(gray, mask, pals))):
        ts = []
        for _ in range(calls + 2):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        out[name] = (float(np.median(ts[2:])), min(ts[2:]))
    return out, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--recordings", type=int, default=16)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--bands", type=int, default=720)
    ap.add_argument("--oneshot", action="store_true", help="only the one-shot calls of 1198 rows (for a kernel trace)")
    args = ap.parse_args()
    layers = layers_of()
    st = apt.LandMaskSettings(n_bands=args.bands)
    if args.oneshot:
        res, info = oneshot(1198, args.calls, layers, st)
        for name, (med, lo) in res.items():
            print(f"{name},{med:.4f},{lo:.4f}")
        return
    import torch
    dev = torch.device("cuda:0")
    k = args.recordings
    x = synth_apt(args.rate, args.seconds, 5)
    plan = apt.Plan(apt.Settings(), apt.Rate.hz(args.rate), True, max_samples=x.size, max_batch=k)
    cap = int(plan.info.max_rows)
    d_in = [torch.from_numpy(x).to(dev) for _ in range(k)]
    d_rows = [torch.empty(cap * 2080, dtype=torch.float32, device=dev) for _ in range(k)]
    d_mask = [torch.empty(cap * 909, dtype=torch.uint8, device=dev) for _ in range(k)]
    d_ll = [torch.empty(cap * 909 * 2, dtype=torch.float64, device=dev) for _ in range(k)]
    ptr = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
    plan.decode_device(ptr(d_in), [x.size] * k, ptr(d_rows), [cap] * k)
    h = int(plan.results(1)[0].n_out) // 2080
    px = h * 909
    print(f"# {torch.cuda.get_device_name(0)}; {k} recordings of {args.seconds:g} s at {args.rate} Hz per call, {h} rows = "
          f"{px} video pixels each, {args.calls} calls per form, {args.bands} bands; ms per recording")
    track = mm.great_circle_track(-20.0, -58.0, 190.0, h)  # down South America: land, sea and lakes
    o = apt.OrbitSettings(apt.SatName.NOAA19, TLE, apt.RefTime.Start(1580246771392), None)
    print("form,timer,ms_per_recording_median,ms_min,note")
    for form, source in (("track", [track] * k), ("orbit", [o] * k)):
        def call():
            plan.land_mask_device(ptr(d_rows), [cap] * k, source, layers, ptr(d_mask), st)
        plan.enable_timing(0)
        for _ in range(2):
            call()
        plan.synchronize()
        t0 = time.perf_counter()
        call()
        plan.synchronize()
        wall = (time.perf_counter() - t0) / k * 1e3
        plan.enable_timing(2)
        plan.collect_timing()
        ms = {n: [] for n in NAMES}
        for _ in range(args.calls):
            call()
            t = plan.collect_timing()
            for n in NAMES:
                ms[n].append(t[n][0])
        rec = plan.land_mask_results(k)
        assert all(r.status == 0 and r.height == h for r in rec), [(r.status, r.reason) for r in rec]
        for n in NAMES:
            med, lo = float(np.median(ms[n])), float(min(ms[n]))
            note = f"{px / (med * 1e-3) / 1e9:.2f} G pixels/s" if n == "image_land_mask" else ""
            print(f"{form},{n},{med:.4f},{lo:.4f},{note}")
        r = rec[0]
        print(f"{form},wall / rec,{wall:.4f},,one call of {k}, timing off; record: {r.n_sea} sea, {r.n_land} land, "
              f"{r.n_lake} lake, {r.n_invalid} invalid; table {r.n_edges[0]} + {r.n_edges[1]} edges, {r.n_band_entries} entries")
    # image_geoloc with the lat / lon plane alone, the same rows, the same run
    gs = apt.GeolocSettings(channel="A", ref_time=apt.RefTime.Start(1730635200000), black=0.0)
    vals = []
    for _ in range(args.calls + 2):
        plan.geolocate_device(ptr(d_rows), [cap] * k, [track] * k, gs, None, ptr(d_ll), None, None)
        vals.append(plan.collect_timing()["image_geoloc"][0])
    print(f"geoloc_latlon,image_geoloc,{float(np.median(vals[2:])):.4f},{min(vals[2:]):.4f},the same rows, the same run")
    plan.close()
    res, _ = oneshot(h, min(args.calls, 10), layers, st)
    for name, (med, lo) in res.items():
        print(f"oneshot,{name},{med:.4f},{lo:.4f},wall per call of one recording: uploads, launches, download")


if __name__ == "__main__":
    main()
