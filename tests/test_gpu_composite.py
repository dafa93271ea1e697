"""The composite on the GPU (composite_images and Plan.composite_device_images).

Exact, every pixel: a composite of one pass is project_image of that pass; FIRST is the single-pass outputs painted
in reverse list order; the coverage of any blend is the number of single-pass outputs with alpha != 0.  These hold
only if the composite's kernel locates every pass with k_project's very bits.

Against tests/np_composite_model.py under its parity rule: NADIR and FEATHER equal the model bit for bit, image and
coverage, on every pixel whose margin is at least TAU; the model alone decides which pixels are left out, and
tests/test_composite_cpu.py holds every case to at most 16 of them and at most 0.1 % of its covered pixels.

The inputs are tests/composite_cases.py's, fed straight to composite_images."""
import functools

import numpy as np
import pytest

import composite_cases as cc
import noaa_apt_amd as apt
import np_composite_model as cm
from test_gpu_sat_track import PASSES, _decode_png
from test_sat_cpu import orbit

pytestmark = pytest.mark.gpu

B = apt.Composite
BLENDS = (B.FIRST, B.NADIR, B.FEATHER)


def _ps(grid):
    g = dict(grid)
    return apt.ProjectionSettings(g.pop("kind"), g.pop("width"), g.pop("height"), g.pop("lat_north"), g.pop("lon_west"),
                                  g.pop("step"), **g)


def _ms(geom):
    return apt.MapSettings(**geom) if geom else None


def _parts(c):
    return [p["image"] for p in c["passes"]], [p["track"] for p in c["passes"]], [_ms(p["geom"]) for p in c["passes"]]


def _composite(c, blend, **kw):
    images, tracks, settings = _parts(c)
    return apt.composite_images(images, tracks, _ps(c["grid"]), blend, settings=settings, **kw)


@functools.lru_cache(maxsize=None)
def _case(name, kind, sampling):
    """A case with its single-pass project_image outputs and its located model passes (computed once, read only)."""
    c = cc.case(name, kind, sampling) if name in cc.CASES else cc.shape(name)
    ps = _ps(c["grid"])
    singles = [apt.project_image(p["image"], p["track"], ps, settings=_ms(p["geom"])) for p in c["passes"]]
    located = cm.locate_passes([p["image"] for p in c["passes"]], [p["track"] for p in c["passes"]], c["grid"],
                               [p["geom"] for p in c["passes"]])
    return c, singles, located


def _painted(singles):
    want = np.zeros_like(singles[0])
    for one in reversed(singles):
        want[one[..., 3] != 0] = one[one[..., 3] != 0]
    return want


def _against_model(c, located, blend, label):
    got, cov = _composite(c, blend, return_coverage=True)
    want, wcov, margin, info = cm.combine(located, c["grid"], blend)
    assert got.shape == want.shape and got.dtype == np.uint8 and cov.shape == wcov.shape and cov.dtype == np.uint8
    bad, low = cm.compare(got, cov, want, wcov, margin, info["coverage_margin"])
    print(f"{label} blend {blend}: {info['n_covered']} covered of {cov.size} pixels, {info['excused']} left out "
          f"(margin < {cm.TAU}), {low} differ below the margin, {bad} differ outside")
    assert bad == 0, label
    assert info["excused"] <= min(16, int(0.001 * info["n_covered"])), (label, info["excused"])
    return got, cov, info


# ---------------------------------------------------------------- exact, every pixel
@pytest.mark.parametrize("sampling", [cc.NEAREST, cc.BILINEAR])
@pytest.mark.parametrize("blend", BLENDS)
def test_one_pass_is_project_image(blend, sampling):
    c = cc.case("two", cc.MERCATOR, sampling)
    c["grid"].update(grid_deg=5.0, grid_color=(255, 40, 0, 128))
    ps = _ps(c["grid"])
    for p in c["passes"]:  # (the second has its own yaw / hscale / vscale)
        want = apt.project_image(p["image"], p["track"], ps, settings=_ms(p["geom"]))
        got, cov = apt.composite_images([p["image"]], [p["track"]], ps, blend, settings=_ms(p["geom"]),
                                        return_coverage=True)
        assert np.array_equal(got, want)
        plain = apt.project_image(p["image"], p["track"], _ps(dict(c["grid"], grid_deg=0.0)), settings=_ms(p["geom"]))
        assert np.array_equal(cov, (plain[..., 3] != 0).astype(np.uint8)) and 1000 < cov.sum() < cov.size


@pytest.mark.parametrize("sampling", [cc.NEAREST, cc.BILINEAR])
@pytest.mark.parametrize("kind", [cc.EQUIRECTANGULAR, cc.MERCATOR])
def test_first_paints_in_reverse_order(kind, sampling):
    c, singles, _ = _case("three", kind, sampling)
    got = _composite(c, B.FIRST)
    assert np.array_equal(got, _painted(singles))
    assert all(one[..., 3].any() for one in singles)


@pytest.mark.parametrize("blend", BLENDS)
@pytest.mark.parametrize("name", ["three", "mixed"])
def test_coverage_counts_the_single_pass_outputs(name, blend):
    c, singles, _ = _case(name, cc.EQUIRECTANGULAR, cc.BILINEAR)
    _, cov = _composite(c, blend, return_coverage=True)
    assert np.array_equal(cov, sum((one[..., 3] != 0).astype(np.uint8) for one in singles))
    assert np.count_nonzero(cov >= 2) >= 500 and (cov == 0).any()


# ---------------------------------------------------------------- against the model, under the cap
@pytest.mark.parametrize("blend", [B.NADIR, B.FEATHER])
@pytest.mark.parametrize("sampling", [cc.NEAREST, cc.BILINEAR])
@pytest.mark.parametrize("kind", [cc.EQUIRECTANGULAR, cc.MERCATOR])
@pytest.mark.parametrize("name", cc.CASES)
def test_parity_with_the_model(name, kind, sampling, blend):
    c, singles, located = _case(name, kind, sampling)
    got, cov, info = _against_model(c, located, blend, f"{name} kind {kind} sampling {sampling}")
    assert info["n_covered"] > 5000
    if blend == B.FEATHER:  # a blend: somewhere in the overlap it is neither pass's sample
        both = cov >= 2
        assert np.any(both & np.all([np.any(got != one, axis=-1) for one in singles], axis=0))
    if name == "mixed":
        assert np.any(got[..., 0] != got[..., 1]) and np.any(got[..., 0] == got[..., 1])


# ---------------------------------------------------------------- shapes where the kernel can go wrong
@pytest.mark.parametrize("name", cc.SHAPES)
def test_shapes(name):
    c, singles, located = _case(name, None, None)
    got, cov = _composite(c, B.FIRST, return_coverage=True)
    assert got.shape == (c["grid"]["height"], c["grid"]["width"], 4)
    assert np.array_equal(got, _painted(singles))
    assert np.array_equal(cov, sum((one[..., 3] != 0).astype(np.uint8) for one in singles))
    assert np.array_equal(_composite(c, B.FIRST), got)  # (without the coverage FIRST may stop early: the same image)
    for blend in (B.NADIR, B.FEATHER):
        _against_model(c, located, blend, name)
    if name == "sixteen":
        assert len(singles) == apt.COMPOSITE_MAX_PASSES and cov.max() == 16
    if name == "miss":  # the far pass contributes nothing and fails nothing
        assert not singles[2].any()
        two = dict(c, passes=c["passes"][:2])
        for blend in BLENDS:
            a, ca = _composite(c, blend, return_coverage=True)
            b, cb = _composite(two, blend, return_coverage=True)
            assert np.array_equal(a, b) and np.array_equal(ca, cb) and ca.max() == 2


def test_graticule_is_blended_last_and_once():
    c, _, located = _case("two", cc.EQUIRECTANGULAR, cc.NEAREST)
    lined = dict(c, grid=dict(c["grid"], grid_deg=4.0, grid_color=(0, 255, 0, 128)))
    got, cov, _ = _against_model(lined, located, B.FEATHER, "graticule")
    plain = _composite(c, B.FEATHER)
    assert np.any(got != plain) and np.any(got[cov == 0][..., 3] == 128)


# ---------------------------------------------------------------- failures
def test_a_failing_pass_fails_the_call():
    c, _, _ = _case("two", cc.EQUIRECTANGULAR, cc.NEAREST)
    images, tracks, settings = _parts(c)
    with pytest.raises(apt.InternalError, match="APTGPU_COMPOSITE_REASON_PASS"):
        apt.composite_images(images, [tracks[0], tracks[1][:-1]], _ps(c["grid"]), B.NADIR, settings=settings)
    # and the next call is unaffected
    assert _composite(c, B.NADIR)[..., 3].any()


# ---------------------------------------------------------------- the plan chain, PNG
def test_png_decodes_to_the_pixels():
    c, _, _ = _case("mixed", cc.MERCATOR, cc.BILINEAR)
    want = _composite(c, B.FEATHER)
    data, cov = _composite(c, B.FEATHER, png=True, return_coverage=True)
    assert isinstance(data, bytes) and np.array_equal(_decode_png(data), want) and cov.max() == 2


def test_plan_chain():
    torch = pytest.importorskip("torch")
    from noaa_apt_amd.testing.synth import synth_apt
    dev = torch.device("cuda:0")
    k = 3
    recs = [synth_apt(48000, 14 + 3 * i, 900 + i) for i in range(k)]
    settings = [None, apt.MapSettings(yaw=0.02, hscale=1.1, vscale=0.95), None]
    orbits = [orbit(tle, name, "start", ms) for tle, name, ms, _ in PASSES.values()]
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        plan = apt.Plan(apt.Settings(), apt.Rate.hz(48000), True, max_samples=max(r.size for r in recs), max_batch=k,
                        stream=stream.cuda_stream)
        cap = int(plan.info.max_rows)
        d_in = [torch.from_numpy(r).to(dev) for r in recs]
        d_rows = [torch.empty(cap * 2080, dtype=torch.float32, device=dev) for _ in recs]
        d_img = [torch.zeros(cap * 2080, dtype=torch.uint8, device=dev) for _ in recs]
        ptr = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
        plan.decode_device(ptr(d_in), [r.size for r in recs], ptr(d_rows), [cap] * k)
        plan.process_device_image(ptr(d_rows), [cap] * k, apt.Contrast.MINMAX, ptr(d_img))
        first = plan.image_results(k)
        heights = [r.height for r in first]
        assert all(r.status == 0 for r in first) and min(heights) >= 20 and len(set(heights)) == k
        images = [d_img[i][:heights[i] * 2080].cpu().numpy().reshape(heights[i], 2080) for i in range(k)]
        # the passes' tracks 6 degrees apart (long rows, so that few rows still span a map), then three real orbits
        tracks = [cc.mm.great_circle_track(-34.0, -62.0 + 6.0 * i, 11.0, heights[i], seconds_per_row=8.0)
                  for i in range(k)]
        ps = apt.projection_fit(tracks, apt.Projection.EQUIRECTANGULAR, max_width=150)
        ps.sampling, ps.grid_deg = apt.Projection.BILINEAR, 10.0
        sat_tracks = [apt.sat_track(o, h) for o, h in zip(orbits, heights)]
        sat_ps = apt.projection_fit(sat_tracks, apt.Projection.MERCATOR, max_width=80)
        assert ps.width == 150 and ps.height <= 200 and sat_ps.width == 80 and sat_ps.height <= 200
        n_out = max(ps.width * ps.height, sat_ps.width * sat_ps.height) * 4
        d_out = torch.full((n_out,), 7, dtype=torch.uint8, device=dev)
        d_cov = torch.full((n_out // 4,), 9, dtype=torch.uint8, device=dev)
        d_png = torch.zeros(apt.png_bound(ps.width, ps.height, 4), dtype=torch.uint8, device=dev)

        def run(grid, blend, out_cap=None, **kw):
            d_out.fill_(7)
            d_cov.fill_(9)
            plan.composite_device_images(ptr(d_img), [cap] * k, [1] * k, grid, d_out.data_ptr(),
                                         grid.width * grid.height * 4 if out_cap is None else out_cap, blend=blend,
                                         d_coverage=d_cov.data_ptr(), **kw)
            res = plan.image_results(k + 1)
            n = grid.width * grid.height
            return res, d_out[:n * 4].cpu().numpy().reshape(grid.shape), d_cov[:n].cpu().numpy().reshape(grid.shape[:2])

        # tracks passed
        for blend in (B.NADIR, B.FEATHER):
            want, wcov = apt.composite_images(images, tracks, ps, blend, settings=settings, return_coverage=True)
            res, got, cov = run(ps, blend, tracks=tracks, settings=settings, png=(d_png.data_ptr(), d_png.numel()))
            assert all(r.status == 0 for r in res) and [r.height for r in res] == heights + [ps.height]
            assert np.array_equal(got, want) and np.array_equal(cov, wcov) and wcov.max() == 3
            assert np.array_equal(_decode_png(d_png[:res[k].png_bytes].cpu().numpy().tobytes()), want)
        # OrbitSettings: the tracks are computed on the device
        want, wcov = apt.composite_images(images, sat_tracks, sat_ps, B.NADIR, return_coverage=True)
        res, got, cov = run(sat_ps, B.NADIR, orbit=orbits)
        assert all(r.status == 0 for r in res)
        assert np.array_equal(got, want) and np.array_equal(cov, wcov) and wcov.any()
        # one byte short: reason 11 on the composite's record, the passes' records clean, nothing written
        res, got, cov = run(ps, B.NADIR, out_cap=ps.width * ps.height * 4 - 1, tracks=tracks, settings=settings)
        assert (res[k].status, res[k].reason) == (1, apt.PROJECT_REASON_CAPACITY)
        assert all(r.status == 0 for r in res[:k]) and (got == 7).all() and (cov == 9).all()
        # a pass whose position count differs from its height: its own reason on its record, PASS on the composite's
        short = [tracks[0], tracks[1][:-1], tracks[2]]
        res, got, cov = run(ps, B.FEATHER, tracks=short, settings=settings)
        assert (res[k].status, res[k].reason) == (1, apt.COMPOSITE_REASON_PASS)
        assert (res[1].status, res[1].reason) == (1, 7) and res[0].status == 0 and res[2].status == 0
        assert (got == 7).all() and (cov == 9).all()
    plan.close()
