#!/usr/bin/env python3
"""tools/fit_timing.py [--calls N] [--rows H] — device time of one overlay fit: fit_overlay_device on
an image of H rows (1198 by default: a ten-minute pass) with the suggested default settings and a world-scale synthetic
layer set of about 250 000 vertices (tools/image_stage_timing.py's), all three layers sampled.  The image is the GPU's
own overlay of those layers, drawn in white over noise from a slice of the long track 37 rows late with yaw 0.02,
hscale 1.04 and vscale 0.97, so the fit has something to find; what it finds is printed, not judged.

Per kernel group (image_fit_edge; image_fit_angles = k_fit_frames + k_fit_angles; image_fit_score; k_fit_pick), from the
event pairs the library records with settings.timing: ms per call, the median over N calls after two warm-up calls,
summed over the rounds; for image_fit_score the sample points x candidates per second (all sample points, of which the
ones beyond 60 degrees of arc from a shift's start are compacted away before the kernel); and the wall time of one call
with the timing off, which includes the sampler on the host, the uploads and the workspace allocation.
GPU box."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import noaa_apt_amd as apt  # noqa: E402
from image_stage_timing import track as track_of, world_layers  # noqa: E402

TRUTH = (37, 0.02, 1.04, 0.97)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rows", type=int, default=1198)
    args = ap.parse_args()
    h = args.rows
    st = apt.FitSettings(layers=[apt.MAP_STATES, apt.MAP_COUNTRIES, apt.MAP_LAKES], timing=True)
    m = st.margin_rows
    parts = world_layers()
    layers = apt.MapLayers(**parts)
    track = track_of(52.0, 8.0, 192.0, h + 2 * m)
    white = (255, 255, 255, 255)
    s, yaw, hscale, vscale = TRUTH
    signal = (np.random.default_rng(1).random(h * 2080) * 60 + 90).astype(np.float32)
    signal[0], signal[1] = 0.0, 255.0
    drawn = apt.process(None, signal, apt.Contrast.MINMAX, rotate=apt.Rotate.NO,
                        orbit=apt.MapOverlay(track[m + s:m + s + h], apt.MapSettings(yaw, hscale, vscale, white, white, white),
                                             layers))
    d_image = torch.from_numpy(np.ascontiguousarray(drawn[:, :, 0])).to("cuda:0")
    torch.cuda.synchronize()

    def call(settings):
        return apt.fit_overlay_device(d_image.data_ptr(), h, track, layers, None, settings)

    for _ in range(2):
        fit = call(st)
    info = fit.info
    nv = sum(len(p) for v in parts.values() for p in v)
    per_round = info.n_points * info.n_candidates
    print(f"# {torch.cuda.get_device_name(0)}; h = {h}, {nv} vertices -> {info.n_points} sample points, "
          f"{info.n_candidates} candidates per round, {info.n_rounds} rounds; {args.calls} calls")
    print(f"# drawn with (shift, yaw, hscale, vscale) = {TRUTH}; found ({fit.shift_rows}, {fit.map_settings.yaw:g}, "
          f"{fit.map_settings.hscale:g}, {fit.map_settings.vscale:g}), q = {fit.q:.1f} over {fit.count} points, "
          f"reason {fit.reason}")
    ms = {k: [] for k in ("edge", "angles", "score", "pick")}
    for _ in range(args.calls):
        i = call(st).info
        for k in ms:
            ms[k].append(getattr(i, "ms_" + k))
    print("group,ms_per_call_median,ms_min,note")
    names = {"edge": "image_fit_edge", "angles": "image_fit_angles", "score": "image_fit_score", "pick": "k_fit_pick"}
    for k, name in names.items():
        med, lo = float(np.median(ms[k])), float(min(ms[k]))
        note = ""
        if k == "score":
            note = (f"{per_round * info.n_rounds / (med * 1e-3) / 1e9:.2f} G sample points x candidates / s "
                    f"({per_round * info.n_rounds / 1e9:.2f} G per call)")
        print(f"{name},{med:.4f},{lo:.4f},{note}")
    print(f"sum (events),{sum(float(np.median(v)) for v in ms.values()):.4f},,")
    quiet = apt.FitSettings(layers=st.layers)
    call(quiet)
    walls = []
    for _ in range(max(3, args.calls // 2)):
        t0 = time.perf_counter()
        call(quiet)
        walls.append((time.perf_counter() - t0) * 1e3)
    print(f"wall,{float(np.median(walls)):.4f},{min(walls):.4f},one call, timing off: sampler, uploads, allocation, "
          f"launches, record")


if __name__ == "__main__":
    main()
