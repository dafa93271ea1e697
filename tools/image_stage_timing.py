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
    map_fixture       color_rgba + the map overlay of the clipped South America shapefiles (tests/golden/shapefiles)
                      over a northbound track through them
    map_world         color_rgba + the map overlay of world-scale synthetic layers (~250 000 vertices)

Per kernel: the plan's event timing (every launch bracketed, one call in flight), ms per recording.  Per variant also
the wall time of one call of 16 recordings with timing off (host clock around enqueue + synchronise).  Last, the host
cost of the Lab tables when the palette changes: one call with a new palette each time against one with the same, and
the host cost of building a world-scale layer set and of its first upload.  --variants a,b runs only those.
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


def track(lat0, lon0, az, rows, altitude_km=850.0):
    """A great-circle ground track, one position every 0.5 s (lat, lon rad)."""
    omega = (398600.4418 / (6371.0 + altitude_km) ** 3) ** 0.5
    lat0, lon0, az = np.radians(lat0), np.radians(lon0), np.radians(az)
    d = omega * 0.5 * np.arange(rows)
    lat = np.arcsin(np.sin(lat0) * np.cos(d) + np.cos(lat0) * np.sin(d) * np.cos(az))
    lon = lon0 + np.arctan2(np.sin(az) * np.sin(d) * np.cos(lat0), np.cos(d) - np.sin(lat0) * np.sin(lat))
    return np.stack([lat, (lon + np.pi) % (2 * np.pi) - np.pi], axis=1)


def world_layers(seed=3, parts=2500, per_part=100):
    """Random-walk outlines spread over the globe: parts * per_part vertices, split over the three layers."""
    rng = np.random.default_rng(seed)
    lat = np.degrees(np.arcsin(rng.uniform(-1, 1, parts)))
    lon = rng.uniform(-180, 180, parts)
    out = [np.stack([lon[i] + np.cumsum(rng.normal(0, 0.08, per_part)),
                     np.clip(lat[i] + np.cumsum(rng.normal(0, 0.08, per_part)), -89, 89)], axis=1)
           for i in range(parts)]
    return {"states": out[:parts // 3], "countries": out[parts // 3:2 * parts // 3], "lakes": out[2 * parts // 3:]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--variants", default="")
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
    shp = os.path.join(ROOT, "tests", "golden", "shapefiles")
    fixture = apt.MapLayers(countries=apt.read_shapefile(os.path.join(shp, "countries.shp"), 5),
                            lakes=apt.read_shapefile(os.path.join(shp, "lakes.shp"), 5))
    t0 = time.perf_counter()
    world = apt.MapLayers(**world_layers())
    t_layers = time.perf_counter() - t0
    pos = track(-52.0, -68.0, 8.0, rows)
    map_fixture = apt.MapOverlay(pos, apt.MapSettings(), fixture)
    map_world = apt.MapOverlay(pos, apt.MapSettings(), world)
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
        "map_fixture": lambda: plan.process_device_image(ptr(d_rows), caps, apt.Contrast.MINMAX, ptr(d_img),
                                                         color=color, map=map_fixture),
        "map_world": lambda: plan.process_device_image(ptr(d_rows), caps, apt.Contrast.MINMAX, ptr(d_img),
                                                       color=color, map=map_world),
    }
    if args.variants:
        keep = args.variants.split(",")
        variants = {k: v for k, v in variants.items() if k in keep}
    if "map_world" in variants:
        # the first call uploads the layer set to every slot; a second, fresh set of the same size measures it
        variants["map_world"]()
        plan.synchronize()
        again = apt.MapOverlay(pos, apt.MapSettings(), apt.MapLayers(**world_layers()))
        t0 = time.perf_counter()
        plan.process_device_image(ptr(d_rows), caps, apt.Contrast.MINMAX, ptr(d_img), color=color, map=again)
        plan.synchronize()
        t_first = time.perf_counter() - t0
        t0 = time.perf_counter()
        plan.process_device_image(ptr(d_rows), caps, apt.Contrast.MINMAX, ptr(d_img), color=color, map=again)
        plan.synchronize()
        t_next = time.perf_counter() - t0
        nv = sum(len(p) for v in world_layers().values() for p in v)
        print(f"world layer set ({nv} vertices): build {t_layers * 1e3:.2f} ms on the host; first call of "
              f"{RECORDINGS} with a new set {t_first * 1e3:.3f} ms, next call {t_next * 1e3:.3f} ms")
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
    if "histogram_color_lab" not in variants:
        plan.close()
        return
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
