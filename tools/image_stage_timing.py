#!/usr/bin/env python3
"""tools/image_stage_timing.py [--calls N] — device time of process()'s image stage per recording, at the config 2
shape (16 recordings x 600 s at 48 kHz, 1198 rows each, one decode_device call), in six variants:

    minmax_gray       aptgpu_plan_process_device, MinMax (the path before the colour stage: image_minmax + image_map_u8)
    minmax_gray_new   aptgpu_plan_process_device_image, MinMax, 1 byte per pixel (its output pass instead of image_map_u8)
    histogram_gray    ... Histogram, 1 byte per pixel (+ image_equalize)
    color_rgba        ... MinMax with false colour (the default palette), 4 bytes per pixel
    histogram_rotate  ... Histogram, 1 byte per pixel, Rotate::Yes
    histogram_color_lab ... Histogram with false colour (the default palette), channel A equalised in CIE Lab
                      (ColorSettings(equalize_lab=True)), 4 bytes per pixel

Per kernel: the plan's event timing (every launch bracketed, one call in flight), ms per recording.  Per variant also
the wall time of one call of 16 recordings with timing off (host clock around enqueue + synchronise).  Last, the host
cost of the Lab tables when the palette changes: one call with a new palette each time against one with the same.
GPU box."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import noaa_apt_amd as apt  # noqa: E402
from noaa_apt_amd.testing.synth import synth_apt  # noqa: E402

RECORDINGS, SECONDS, RATE = 16, 600, 48000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    if apt.device_count() < 1:
        sys.exit("image_stage_timing needs a GPU")
    dev = torch.device("cuda", 0)
    x = synth_apt(RATE, SECONDS, seed=2)  # one recording, fed 16 times (the image stage sees 16 row buffers)
    plan = apt.Plan(apt.Settings(), apt.Rate.hz(RATE), True, max_samples=x.size, max_batch=RECORDINGS)
    cap = int(plan.info.max_rows)
    d_in = torch.from_numpy(x).to(dev)
    d_rows = [torch.empty(cap * 2080, dtype=torch.float32, device=dev) for _ in range(RECORDINGS)]
    d_img = [torch.empty(cap * 2080 * 4, dtype=torch.uint8, device=dev) for _ in range(RECORDINGS)]
    ptr = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
    plan.decode_device([d_in.data_ptr()] * RECORDINGS, [x.size] * RECORDINGS, ptr(d_rows), [cap] * RECORDINGS)
    plan.synchronize()
    rows = plan.results(1)[0].n_rows
    color = apt.ColorSettings(os.path.join(ROOT, "tests", "golden", "palettes", "noaa-apt-daylight.png"))
    caps = [cap] * RECORDINGS
    lab = apt.ColorSettings(color.palette, equalize_lab=True)
    variants = {
        "minmax_gray": lambda: plan.process_device(ptr(d_rows), caps, apt.Contrast.MINMAX, ptr(d_img)),
        "minmax_gray_new": lambda: plan.process_device_image(ptr(d_rows), caps, apt.Contrast.MINMAX, ptr(d_img)),
        "histogram_gray": lambda: plan.process_device_image(ptr(d_rows), caps, apt.Contrast.HISTOGRAM, ptr(d_img)),
        "color_rgba": lambda: plan.process_device_image(ptr(d_rows), caps, apt.Contrast.MINMAX, ptr(d_img),
                                                        color=color),
        "histogram_rotate": lambda: plan.process_device_image(ptr(d_rows), caps, apt.Contrast.HISTOGRAM, ptr(d_img),
                                                              rotate=apt.Rotate.YES),
        "histogram_color_lab": lambda: plan.process_device_image(ptr(d_rows), caps, apt.Contrast.HISTOGRAM,
                                                                 ptr(d_img), color=lab),
    }
    print(f"image stage, {RECORDINGS} x {SECONDS} s at {RATE} Hz ({rows} rows = {rows * 2080 / 1e6:.2f} Mpx per "
          f"recording), {args.calls} calls per variant; ms per recording")
    print(f"{'variant':18s} {'kernel':16s} {'ms/rec':>8s}   (launches)")
    for name, call in variants.items():
        for _ in range(3):  # warm-up: code objects, first-use allocations, palette upload
            call()
        plan.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            call()
        plan.synchronize()
        wall = (time.perf_counter() - t0) / args.calls
        plan.enable_timing(2)
        for _ in range(args.calls):
            call()
            plan.synchronize()
        timing = plan.collect_timing()
        plan.enable_timing(0)
        total = 0.0
        for kname, (ms, launches) in sorted(timing.items()):
            if not kname.startswith("image_"):
                continue
            total += ms
            print(f"{name:18s} {kname:16s} {ms:8.4f}   ({launches})")
        print(f"{name:18s} {'sum (events)':16s} {total:8.4f}")
        print(f"{name:18s} {'wall / rec':16s} {wall * 1e3 / RECORDINGS:8.4f}   (one call of {RECORDINGS}, timing off)")
    # the Lab tables' host cost per palette change (Lab::from_rgb of 65 792 entries, then one pinned copy)
    rng = np.random.default_rng(5)
    fresh = [apt.ColorSettings(rng.integers(0, 256, (256, 256, 3), dtype=np.uint8), equalize_lab=True)
             for _ in range(args.calls)]
    same, new = [], []
    for c in fresh:
        for sink, cs in ((new, c), (same, c)):  # first call: a new palette; second: the same bytes again
            plan.synchronize()
            t0 = time.perf_counter()
            plan.process_device_image(ptr(d_rows), caps, apt.Contrast.HISTOGRAM, ptr(d_img), color=cs)
            plan.synchronize()
            sink.append(time.perf_counter() - t0)
    print(f"Lab palette change: one call of {RECORDINGS} with a new palette {np.median(new) * 1e3:.3f} ms, with the "
          f"same palette {np.median(same) * 1e3:.3f} ms (medians of {args.calls}); difference "
          f"{(np.median(new) - np.median(same)) * 1e3:.3f} ms per palette change")
    plan.close()


if __name__ == "__main__":
    main()
