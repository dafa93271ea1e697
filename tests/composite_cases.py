"""The inputs of the composite's tests, shared by the model-only CPU test and the GPU test: seeded,
block-constant swath images fed straight to composite_images (no process() in between, so both sides see the same
bytes), tracks along one great circle shifted in longitude so that neighbouring swaths overlap over several degrees,
and the grids.

Images are constant over blocks of 4 rows x 8 px (gray) or 16 rows x 52 px (RGBA, three distinct channels), as
tests/test_gpu_project.py argues: a bilinear sample can round within TAU of k + 0.5 only where its four neighbours
differ, which the blocks make rare enough for the 0.1 % allowance.

The track: from (-34, -62) heading 11 degrees, one row every 1.5 s, so 160 rows span about 14 degrees of latitude and
a grid of at most 160 x 80 pixels at 0.25 degrees holds whole swath edges: the first pass stops covering where the
later ones still do, so FIRST, NADIR and FEATHER all have every pass win somewhere.  A swath is about 31 degrees of
longitude wide there; neighbours are 14 degrees apart.

CASES are held to the conditions of tests/test_composite_cpu.py (few excused pixels, every pass wins, a real
overlap); SHAPES are the small grids where only the kernel's indexing can go wrong.
"""
import numpy as np

import np_map_model as mm

EQUIRECTANGULAR, MERCATOR = 0, 1
NEAREST, BILINEAR = 0, 1
SHIFT = 14.0  # degrees of longitude between neighbouring passes


def gray_image(rows, seed):
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, 256, ((rows + 3) // 4, 2080 // 8), dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(blocks, 4, axis=0), 8, axis=1)[:rows])


def rgba_image(rows, seed):
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, 256, ((rows + 15) // 16, 2080 // 52, 4), dtype=np.uint8)
    blocks[..., 3] = 255
    return np.ascontiguousarray(np.repeat(np.repeat(blocks, 16, axis=0), 52, axis=1)[:rows])


def track(rows, shift_deg):
    return mm.great_circle_track(-34.0, -62.0 + shift_deg, 11.0, rows, seconds_per_row=1.5)


def _pass(rows, seed, shift_deg, rgba=False, geom=None):
    return {"image": (rgba_image if rgba else gray_image)(rows, seed), "track": track(rows, shift_deg), "geom": geom}


def grid(kind, sampling, width=160, height=80, lat_north=-19.1, lon_west=-64.1, step=0.25, **kw):
    return dict(kind=kind, width=width, height=height, lat_north=lat_north, lon_west=lon_west, step=step,
                channel=0, sampling=sampling, **kw)


def case(name, kind=EQUIRECTANGULAR, sampling=NEAREST):
    """{"passes": [{"image", "track", "geom"}], "grid": {...}} of a named case on the given grid kind and sampling."""
    tilted = {"yaw": 0.02, "hscale": 1.1, "vscale": 0.95}
    if name == "two":      # heights 160 and 96, the second with its own geometry
        passes = [_pass(160, 7, 0.0), _pass(96, 8, SHIFT, geom=tilted)]
        return {"passes": passes, "grid": grid(kind, sampling, width=131, height=77)}
    if name == "three":
        passes = [_pass(160, 7, 0.0), _pass(96, 8, SHIFT, geom=tilted), _pass(160, 9, 2 * SHIFT)]
        return {"passes": passes, "grid": grid(kind, sampling)}
    if name == "mixed":    # a gray and an RGBA source
        passes = [_pass(160, 7, 0.0), _pass(160, 21, SHIFT, rgba=True)]
        return {"passes": passes, "grid": grid(kind, sampling, width=131, height=77)}
    raise KeyError(name)


CASES = ("two", "three", "mixed")


def shape(name):
    """The small grids: a single pixel, one tile, a tile edge plus one, the 16-pass maximum, and a pass far away."""
    three = [_pass(160, 7, 0.0), _pass(96, 8, 4.0), _pass(160, 9, 8.0)]
    if name == "1x1":
        return {"passes": three, "grid": grid(EQUIRECTANGULAR, BILINEAR, 1, 1, -27.03, -52.07)}
    if name == "64x4":
        return {"passes": three, "grid": grid(EQUIRECTANGULAR, NEAREST, 64, 4, -27.03, -60.07)}
    if name == "65x5":
        return {"passes": three, "grid": grid(MERCATOR, BILINEAR, 65, 5, -27.03, -60.07)}
    if name == "sixteen":  # 16 passes 1.5 degrees apart, heights alternating, on 70 x 9
        passes = [_pass(96 if p % 2 else 160, 30 + p, 1.5 * p) for p in range(16)]
        return {"passes": passes, "grid": grid(EQUIRECTANGULAR, NEAREST, 70, 9, -26.03, -58.07)}
    if name == "miss":     # the third pass is a third of the globe away: it covers no pixel
        passes = [_pass(160, 7, 0.0), _pass(96, 8, SHIFT), _pass(160, 9, 120.0)]
        return {"passes": passes, "grid": grid(EQUIRECTANGULAR, NEAREST, 70, 9, -26.03, -50.07)}
    raise KeyError(name)


SHAPES = ("1x1", "64x4", "65x5", "sixteen", "miss")
