#!/usr/bin/env python3
"""tools/image_stage_timing.py [--calls N] — device time of process()'s image stage per recording, at the config 2
shape (16 recordings x 600 s at 48 kHz, 1198 rows each, one decode_device call), in these variants:

    minmax_gray       aptgpu_plan_process_device, MinMax (the path before the colour stage: image_minmax + image_map_u8)
    minmax_gray_new   aptgpu_plan_process_device_image, MinMax, 1 byte per pixel (its output pass instead of image_map_u8)
    histogram_gray    ... Histogram, 1 byte per pixel (+ image_equalize)
    histogram_float   ... HISTOGRAM_FLOAT, 1 byte per pixel (image_equalize_float: the three count / select levels;
                      image_color_float: its output pass)
    color_rgba        ... MinMax with false colour (the default palette), 4 bytes per pixel
    histogram_rotate  ... Histogram, 1 byte per pixel, Rotate::Yes
    histogram_color_lab ... Histogram with false colour (the default palette), channel A equalised in CIE Lab
                      (ColorSettings(equalize_lab=True)), 4 bytes per pixel
    map_fixture       color_rgba + the map overlay of the clipped South America shapefiles (tests/golden/shapefiles)
                      over a northbound track through them
    map_world         color_rgba + the map overlay of world-scale synthetic layers (~250 000 vertices)
    png_gray          minmax_gray_new + the PNG encoder (colour type 0), the file left in HBM
    png_rgba          the same image as RGBA (colour type 6: what the reference's RgbaImage saves as)
    png_color         color_rgba + the PNG encoder
    project_nearest   color_rgba + the reprojection onto the equirectangular grid that projection_fit
                      sizes for the track at 0.04 degrees per pixel, nearest sampling
    project_bilinear  the same, bilinear
    project_nearest_png, project_bilinear_png   the same + the PNG encoder on the projected grid
    composite_nadir   color_rgba + the composite of the 16 recordings, their tracks 1.5 degrees of
                      longitude apart, onto the one grid projection_fit sizes for all of them at 0.04 degrees per
                      pixel, nearest sampling, NADIR, with the coverage plane: image_composite is ONE launch per call
                      (its row is ms per call, not per recording) beside project_nearest's 16 image_project launches
    composite_feather the same, FEATHER
    despeckle_r1_t0, despeckle_r1_t01, despeckle_r2_t0, despeckle_r2_t01
                      the despeckle stage (radius 1 / 2, threshold 0 / 0.1: image_despeckle, and
                      image_percent when the threshold needs the 98 % limits) into a second rows buffer, then
                      minmax_gray on the filtered rows: image_minmax, one pass over the same samples, stands beside it
    thermal_kelvin, thermal_gray, thermal_rgba
                      the thermal calibration of channel B with the identity forced to "4": the
                      telemetry stage, image_thermal_space, image_thermal_setup and image_thermal_map, which writes
                      the Kelvin plane alone, with the gray scale image, or with the RGBA one; beside image_thermal_map
                      the bytes it moves per second (the 909 video columns read, the Kelvin plane and the whole scale
                      image written) against the 8 TB/s of HBM

Per kernel: the plan's event timing (every launch bracketed, one call in flight), ms per recording.  Per variant also
the wall time of one call of 16 recordings with timing off (host clock around enqueue + synchronise).  Last, the host
cost of the Lab tables when the palette changes: one call with a new palette each time against one with the same, and
the host cost of building a world-scale layer set and of its first upload.  --variants a,b runs only those.
For the png_* variants the wall time includes the copy of the encoded bytes to the host, and beside it stands the path
without the encoder, on the same host in the same run: copy the raw image to the host and save() it with Pillow at its
default level and at compress_level=1, single-threaded.  Then the file sizes against Pillow's for the committed rows
of the reference's example image and one full-size false-colour image.
GPU box."""
import argparse
import io
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


def cpu_name():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown CPU"


def pillow_save(px, **kw):
    """(seconds, bytes) of Pillow's PNG save() of a (h, w) or (h, w, 4) u8 image."""
    from PIL import Image
    buf = io.BytesIO()
    t0 = time.perf_counter()
    Image.fromarray(px, "RGBA" if px.ndim == 3 else "L").save(buf, format="PNG", **kw)
    return time.perf_counter() - t0, buf.tell()


def png_sizes_report(full_px):
    """File sizes of the encoder against Pillow's default save() (zlib level 6) and compress_level=1."""
    rows = np.load(os.path.join(ROOT, "tests", "golden", "reference_image", "argentina_rows.npy"))
    rgba = np.ascontiguousarray(np.stack([rows, rows, rows, np.full_like(rows, 255)], axis=-1))
    print("PNG file sizes: encoder / Pillow default (level 6) / Pillow compress_level=1, bytes and ratios")
    for name, px in (("argentina_rows gray", rows), ("argentina_rows RGBA", rgba),
                     (f"synthetic false colour {full_px.shape[0]} rows", full_px)):
        ours = len(apt.encode_png(px))
        _, p6 = pillow_save(px)
        _, p1 = pillow_save(px, compress_level=1)
        print(f"  {name:34s} {ours:9d} {p6:9d} {p1:9d}   x{ours / p6:.3f} of level 6, x{ours / p1:.3f} of level 1, "
              f"level 1 is x{p1 / p6:.3f} of level 6")


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
    png_cap = [apt.png_bound(2080, cap, 4)] * RECORDINGS
    d_png = [torch.empty(png_cap[0], dtype=torch.uint8, device=dev) for _ in range(RECORDINGS)]
    png = (ptr(d_png), png_cap)
    png_channels = {"png_gray": 1, "png_rgba": 4, "png_color": 4}
    fit = apt.projection_fit(pos, apt.Projection.EQUIRECTANGULAR, step=0.04)
    grids = {s: apt.ProjectionSettings(fit.kind, fit.width, fit.height, fit.lat_north, fit.lon_west, fit.step, sampling=s)
             for s in (apt.Projection.NEAREST, apt.Projection.BILINEAR)}
    grid_bytes = fit.width * fit.height * 4
    d_grid = [torch.empty(grid_bytes, dtype=torch.uint8, device=dev) for _ in range(RECORDINGS)]
    grid_png_cap = [apt.png_bound(fit.width, fit.height, 4)] * RECORDINGS
    d_grid_png = [torch.empty(grid_png_cap[0], dtype=torch.uint8, device=dev) for _ in range(RECORDINGS)]

    def project(sampling, with_png):
        return lambda: plan.process_device_image(
            ptr(d_rows), caps, apt.Contrast.MINMAX, ptr(d_img), color=color, map=[pos] * RECORDINGS,
            projection=(grids[sampling], ptr(d_grid), [grid_bytes] * RECORDINGS),
            png=(ptr(d_grid_png), grid_png_cap) if with_png else None)

    shifted = [pos + np.array([0.0, np.radians(1.5 * i)]) for i in range(RECORDINGS)]
    cfit = apt.projection_fit(shifted, apt.Projection.EQUIRECTANGULAR, step=0.04)
    d_comp = torch.empty(cfit.width * cfit.height * 4, dtype=torch.uint8, device=dev)
    d_cov = torch.empty(cfit.width * cfit.height, dtype=torch.uint8, device=dev)

    def composite(blend):
        def call():
            plan.process_device_image(ptr(d_rows), caps, apt.Contrast.MINMAX, ptr(d_img), color=color)
            plan.composite_device_images(ptr(d_img), caps, [4] * RECORDINGS, cfit, d_comp.data_ptr(), d_comp.numel(),
                                         tracks=shifted, blend=blend, d_coverage=d_cov.data_ptr())
        return call

    d_dsp = [torch.empty(cap * 2080, dtype=torch.float32, device=dev) for _ in range(RECORDINGS)]

    def despeckle(radius, threshold):
        def call():
            plan.despeckle_device(ptr(d_rows), caps, ptr(d_dsp), apt.DespeckleSettings(radius, threshold))
            plan.process_device(ptr(d_dsp), caps, apt.Contrast.MINMAX, ptr(d_img))
        return call

    # (coefficients with the magnitudes of an AVHRR/3, the values of no satellite)
    thermal_co = apt.ThermalCoefficients([(276.6, 0.0511, 1.4e-6)] * 4, (2670.0, 1.70, 0.9975, 0.0, 0.0, 0.0, 0.0),
                                         (928.0, 0.55, 0.9985, -5.5, 5.8, -0.11, 0.00052),
                                         (834.0, 0.40, 0.9990, -3.5, 2.7, -0.05, 0.00024))
    d_kelvin = [torch.empty(cap * 909, dtype=torch.float32, device=dev) for _ in range(RECORDINGS)]
    thermal_channels = {"thermal_kelvin": 0, "thermal_gray": 1, "thermal_rgba": 4}

    def thermal(channels):
        st = apt.ThermalSettings("B", "4", t_low=180.0, t_high=320.0, image_channels=channels)
        return lambda: plan.calibrate_thermal_device(ptr(d_rows), caps, ptr(d_kelvin), thermal_co, st,
                                                     ptr(d_img) if channels else None)

    variants = {
        "thermal_kelvin": thermal(0),
        "thermal_gray": thermal(1),
        "thermal_rgba": thermal(4),
        "despeckle_r1_t0": despeckle(1, 0.0),
        "despeckle_r1_t01": despeckle(1, 0.1),
        "despeckle_r2_t0": despeckle(2, 0.0),
        "despeckle_r2_t01": despeckle(2, 0.1),
        "composite_nadir": composite(apt.Composite.NADIR),
        "composite_feather": composite(apt.Composite.FEATHER),
        "project_nearest": project(apt.Projection.NEAREST, False),
        "project_bilinear": project(apt.Projection.BILINEAR, False),
        "project_nearest_png": project(apt.Projection.NEAREST, True),
        "project_bilinear_png": project(apt.Projection.BILINEAR, True),
        "png_gray": lambda: plan.process_device_image(ptr(d_rows), caps, apt.Contrast.MINMAX, ptr(d_img), png=png),
        "png_rgba": lambda: plan.process_device_image(ptr(d_rows), caps, apt.Contrast.MINMAX, ptr(d_img), channels=4,
                                                      png=png),
        "png_color": lambda: plan.process_device_image(ptr(d_rows), caps, apt.Contrast.MINMAX, ptr(d_img), color=color,
                                                       png=png),
        "minmax_gray": lambda: plan.process_device(ptr(d_rows), caps, apt.Contrast.MINMAX, ptr(d_img)),
        "minmax_gray_new": lambda: plan.process_device_image(ptr(d_rows), caps, apt.Contrast.MINMAX, ptr(d_img)),
        "histogram_gray": lambda: plan.process_device_image(ptr(d_rows), caps, apt.Contrast.HISTOGRAM, ptr(d_img)),
        "histogram_float": lambda: plan.process_device_image(ptr(d_rows), caps, apt.Contrast.HISTOGRAM_FLOAT,
                                                             ptr(d_img)),
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
    if any(k.startswith("project_") for k in variants):
        print(f"project_*: grid {fit.width} x {fit.height} = {fit.width * fit.height / 1e6:.2f} Mpx per recording")
    if any(k.startswith("composite_") for k in variants):
        print(f"composite_*: one grid {cfit.width} x {cfit.height} = {cfit.width * cfit.height / 1e6:.2f} Mpx for all "
              f"{RECORDINGS} recordings; image_composite's row is ms per call (one launch)")
    print(f"{'variant':18s} {'kernel':20s} {'ms/rec':>8s}   (launches)")
    for name, call in variants.items():
        for _ in range(3):  # warm-up: code objects, first-use allocations, palette upload
            call()
        plan.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            call()
        plan.synchronize()
        wall = (time.perf_counter() - t0) / args.calls
        if name in png_channels:
            # the whole product: the call, the lengths, and the encoded bytes on the host
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call()
                sizes = plan.png_sizes(RECORDINGS)
                files = [d_png[i][:sizes[i]].cpu() for i in range(RECORDINGS)]
            wall_png = (time.perf_counter() - t0) / args.calls
            # the path without the encoder: the raw image to the host, Pillow's save() there (one thread)
            ch = png_channels[name]
            shape = (rows, 2080, 4) if ch == 4 else (rows, 2080)
            host = {"default": [], "level1": []}
            copy = []
            for i in range(3):
                t0 = time.perf_counter()
                px = d_img[i][:rows * 2080 * ch].cpu().numpy().reshape(shape)
                copy.append(time.perf_counter() - t0)
                host["default"].append(pillow_save(px)[0])
                host["level1"].append(pillow_save(px, compress_level=1)[0])
            t_copy, t6, t1 = np.median(copy), np.median(host["default"]), np.median(host["level1"])
            per_rec = wall_png / RECORDINGS
            print(f"{name:18s} {'wall+copy / rec':16s} {per_rec * 1e3:8.4f}   (one call of {RECORDINGS}, png_sizes and "
                  f"{sum(len(f) for f in files) / RECORDINGS / 1e6:.2f} MB of file per recording copied to the host)")
            print(f"{name:18s} {'host path / rec':16s} {(t_copy + t6) * 1e3:8.2f}   (raw copy {t_copy * 1e3:.2f} ms + "
                  f"Pillow save() {t6 * 1e3:.1f} ms; compress_level=1: {t1 * 1e3:.1f} ms; medians of 3, one thread, "
                  f"{cpu_name()})")
            print(f"{name:18s} {'host / GPU':16s} {(t_copy + t6) / per_rec:8.1f}   (default level; level 1: "
                  f"{(t_copy + t1) / per_rec:.1f})")
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
            print(f"{name:18s} {kname:20s} {ms:8.4f}   ({launches})")
            if kname == "image_thermal_map":
                r = plan.thermal_results(1)[0]
                moved = rows * (909 * 8 + 2080 * thermal_channels[name])
                print(f"{name:18s} {'  bytes / s':20s} {moved / ms / 1e9:8.4f}   TB/s = {moved / ms / 1e9 / 8.0 * 100:.1f} % of "
                      f"8 TB/s ({moved / 1e6:.2f} MB per recording; record: status {r.status}, {r.n_nan} NaN of "
                      f"{rows * 909} px, {r.t_min:.1f} .. {r.t_max:.1f} K)")
        print(f"{name:18s} {'sum (events)':16s} {total:8.4f}")
        print(f"{name:18s} {'wall / rec':16s} {wall * 1e3 / RECORDINGS:8.4f}   (one call of {RECORDINGS}, timing off)")
    if any(k in png_channels for k in variants):
        plan.process_device_image(ptr(d_rows), caps, apt.Contrast.MINMAX, ptr(d_img), color=color)
        plan.synchronize()
        png_sizes_report(d_img[0][:rows * 2080 * 4].cpu().numpy().reshape(rows, 2080, 4))
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
