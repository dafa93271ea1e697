"""A restatement of the composite for the tests: several passes, each reprojected as DESIGN.md §15
says (np_project_model.locate and its sampling, unchanged), combined per output pixel over the passes that cover it.

  FIRST    the sample of the first covering pass in list order
  NADIR    the sample of the covering pass with the smallest |x| (the corrected off-nadir distance); the lower index
           on an exact tie
  FEATHER  per channel, in f64 and in pass order, v = sum(w c) / sum(w) with w = 456 - |x|; floor(v + 0.5)
No covering pass gives (0, 0, 0, 0); the graticule is blended last, once.  Coverage is the number of covering passes.

Margins in px, the minimum of
  - the locate margin and the sample margin (np_project_model's) of every pass whose decision matters: all passes for
    NADIR and FEATHER, the passes up to and including the winner for FIRST (all of them where no pass covers);
  - NADIR: half the gap between the smallest and the second smallest |x| (each may move by tau);
  - FEATHER: per channel |v - (k + 0.5)| * sum(w) / sum(|c - v|): dv/dw_p = (c_p - v) / sum(w) and |dw_p| <= tau;
    infinite when all c are equal.
The GPU must equal this model bit for bit, image and coverage, on every pixel whose margin is >= np_map_model.TAU.
The coverage counts every pass, also those behind FIRST's winner, so it is judged by the smallest locate margin of all
passes (info["coverage_margin"]), which for NADIR and FEATHER is never below the pixel's margin.
"""
import math

import numpy as np

import np_project_model as pm
from np_map_model import TAU, Scalars, blend, rel_px

FIRST, NADIR, FEATHER = 0, 1, 2
MAX_PASSES = 16


def locate_passes(images, tracks, grid, geoms=None):
    """Steps 1-4 of §15 for every pass and every output pixel: a list of dicts with x (H, W), valid (H, W), located
    (H, W: the locate margin), margin (H, W: that and, where valid, the sample margin) and c (H, W, 4 uint8)."""
    kind, width, height = grid["kind"], grid["width"], grid["height"]
    sampling = grid.get("sampling", pm.NEAREST)
    base = 1579 if grid.get("channel", pm.CHANNEL_A) == pm.CHANNEL_B else 539
    lats = [pm.row_lat(kind, grid["lat_north"], grid["step"], float(i)) for i in range(height)]
    lons = [pm.col_lon(grid["lon_west"], grid["step"], float(j)) for j in range(width)]
    out = []
    for p, (img, positions) in enumerate(zip(images, tracks)):
        src = pm._rgba(img)
        h = src.shape[0]
        track = [(float(a), float(b)) for a, b in positions]
        assert len(track) == h
        geom = (geoms[p] if geoms else None) or {}
        sc = Scalars(track, geom.get("yaw", 0.0), geom.get("hscale", 1.0), geom.get("vscale", 1.0))
        xoff = [rel_px(sc, q)[0] for q in track]
        xs = np.full((height, width), np.nan)
        valid = np.zeros((height, width), bool)
        margin = np.full((height, width), math.inf)
        located = np.full((height, width), math.inf)
        c = np.zeros((height, width, 4), np.uint8)

        def px(xi, yi):
            return src[min(max(yi, 0), h - 1), min(max(xi, -455), 455) + base]

        for i in range(height):
            for j in range(width):
                x, y, ok, m, _ = pm.locate(sc, xoff, h, lats[i], lons[j])
                xs[i, j] = x
                located[i, j] = m
                if ok:
                    if sampling == pm.BILINEAR:
                        x0, y0 = math.floor(x), math.floor(y)
                        fx, fy = x - x0, y - y0
                        p00, p10 = px(int(x0), int(y0)), px(int(x0) + 1, int(y0))
                        p01, p11 = px(int(x0), int(y0) + 1), px(int(x0) + 1, int(y0) + 1)
                        for k in range(4):
                            v = (float(p00[k]) * (1.0 - fx) + float(p10[k]) * fx) * (1.0 - fy) + \
                                (float(p01[k]) * (1.0 - fx) + float(p11[k]) * fx) * fy
                            c[i, j, k] = int(math.floor(v + 0.5))
                            m = min(m, pm._near_half(v) / (2.0 * 255.0))
                    else:
                        m = min(m, pm._near_half(x), pm._near_half(y))
                        c[i, j] = px(int(math.floor(x + 0.5)), int(math.floor(y + 0.5)))
                valid[i, j] = ok
                margin[i, j] = m
        out.append({"x": xs, "valid": valid, "margin": margin, "located": located, "c": c})
    return out


def combine(located, grid, blend_mode):
    """The composite of located passes: (image, coverage, margin, info)."""
    kind, width, height = grid["kind"], grid["width"], grid["height"]
    n = len(located)
    assert 1 <= n <= MAX_PASSES
    valid = np.stack([q["valid"] for q in located])          # (n, H, W)
    ax = np.abs(np.stack([q["x"] for q in located]))
    pm_margin = np.stack([q["margin"] for q in located])
    c = np.stack([q["c"] for q in located])                  # (n, H, W, 4)
    coverage = valid.sum(axis=0).astype(np.uint8)
    covered = coverage > 0
    out = np.zeros((height, width, 4), np.uint8)
    winner = np.full((height, width), -1)
    if blend_mode == FIRST:
        first = np.argmax(valid, axis=0)                     # (first True; 0 where none)
        winner = np.where(covered, first, -1)
        last = np.where(covered, first, n - 1)               # the passes whose decision matters: 0..last
        matters = np.arange(n)[:, None, None] <= last[None]
        margin = np.where(matters, pm_margin, math.inf).min(axis=0)
    else:
        margin = pm_margin.min(axis=0)
        key = np.where(valid, ax, math.inf)
        winner = np.where(covered, np.argmin(key, axis=0), -1)  # (argmin: the lowest index on a tie)
        if blend_mode == NADIR and n > 1:
            two = np.sort(key, axis=0)[:2]
            with np.errstate(invalid="ignore"):
                gap = np.where(np.isfinite(two[1]), (two[1] - two[0]) / 2.0, math.inf)
            margin = np.minimum(margin, gap)
    if blend_mode == FEATHER:
        wsum = np.zeros((height, width))
        acc = np.zeros((height, width, 4))
        for p in range(n):                                    # in pass order, every product and sum rounded once
            w = 456.0 - ax[p]
            ok = valid[p]
            wsum = np.where(ok, wsum + w, wsum)
            acc = np.where(ok[..., None], acc + w[..., None] * c[p].astype(np.float64), acc)
        with np.errstate(invalid="ignore", divide="ignore"):
            v = acc / wsum[..., None]
            r = np.floor(v + 0.5)
            out = np.where(covered[..., None], np.clip(r, 0.0, 255.0), 0.0).astype(np.uint8)
            spread = np.where(valid[..., None], np.abs(c.astype(np.float64) - v[None]), 0.0).sum(axis=0)
            near = np.abs(v - (np.floor(v) + 0.5))
            fm = np.where(spread > 0.0, near * wsum[..., None] / spread, math.inf).min(axis=-1)
        margin = np.minimum(margin, np.where(covered, fm, math.inf))
    else:
        pick = np.take_along_axis(c, np.maximum(winner, 0)[None, ..., None], axis=0)[0]
        out = np.where(covered[..., None], pick, 0).astype(np.uint8)
    cols, rows = pm.graticule(kind, width, height, grid["lat_north"], grid["lon_west"], grid["step"],
                              grid.get("grid_deg", 0.0))
    if cols.any() or rows.any():
        fg = tuple(int(v) for v in grid.get("grid_color", (255, 255, 255, 255)))
        for i, j in zip(*np.nonzero(rows[:, None] | cols[None, :])):
            out[i, j] = blend(tuple(int(v) for v in out[i, j]), fg)
    excused = margin < TAU
    # the coverage counts every pass, also those behind FIRST's winner: its own margin is every pass's locate margin
    info = {"winner": winner, "valid": valid, "excused": int(np.count_nonzero(excused)),
            "coverage_margin": np.stack([q["located"] for q in located]).min(axis=0),
            "n_covered": int(np.count_nonzero(covered)), "x": np.stack([q["x"] for q in located])}
    return out, coverage, margin, info


def composite(images, tracks, grid, blend_mode, geoms=None):
    """(image, coverage, margin, info) of the passes on the grid (a dict: kind, width, height, lat_north, lon_west,
    step and optionally channel, sampling, grid_deg, grid_color); geoms: per pass None or a dict of yaw / hscale /
    vscale."""
    return combine(locate_passes(images, tracks, grid, geoms), grid, blend_mode)


def compare(gpu, gpu_coverage, model, model_coverage, margin, coverage_margin):
    """The parity contract: (pixels that differ with a margin >= TAU, those that differ below it).  The image is
    judged by `margin`, the coverage by `coverage_margin` (>= margin except behind FIRST's winner)."""
    d_img = np.any(np.asarray(gpu) != np.asarray(model), axis=-1)
    d_cov = np.asarray(gpu_coverage) != model_coverage
    bad = (d_img & (margin >= TAU)) | (d_cov & (coverage_margin >= TAU))
    return int(np.count_nonzero(bad)), int(np.count_nonzero((d_img | d_cov) & ~bad))
