"""The map overlay's host side without a GPU: the shapefile reader (aptgpu_map_read_shapefile) on hand-built files, the
layer-set handle, and np_map_model.py against geo.rs's own answers and hand-derived values."""
import math
import struct

import numpy as np
import pytest

import noaa_apt_amd as apt
import np_map_model as mm

PI = math.pi


def _record(num, shape_type, parts):
    """One Polyline / Polygon record: parts = list of [(x, y), ...]."""
    pts = [p for part in parts for p in part]
    xs, ys = [p[0] for p in pts] or [0.0], [p[1] for p in pts] or [0.0]
    offs, o = [], 0
    for part in parts:
        offs.append(o)
        o += len(part)
    body = struct.pack("<i4dii", shape_type, min(xs), min(ys), max(xs), max(ys), len(parts), len(pts))
    body += struct.pack(f"<{len(offs)}i", *offs) + b"".join(struct.pack("<2d", *p) for p in pts)
    return struct.pack(">ii", num, len(body) // 2) + body


def _shp(header_type, records):
    blob = b"".join(records)
    header = struct.pack(">i5ii", 9994, 0, 0, 0, 0, 0, (100 + len(blob)) // 2)
    header += struct.pack("<ii4d4d", 1000, header_type, 0, 0, 0, 0, 0, 0, 0, 0)
    assert len(header) == 100
    return header + blob


def _write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def test_reader_both_types_and_multipart(tmp_path):
    line = [[(1.0, 2.0), (3.0, 4.0)], [(5.0, 6.0), (7.0, 8.0), (9.0, 10.0)]]
    ring = [[(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 0.0)]]
    p = _write(tmp_path, "l.shp", _shp(3, [_record(1, 3, line), _record(2, 3, [[(-1.5, 2.5)]])]))
    parts = apt.read_shapefile(p, 3)
    assert len(parts) == 3
    assert parts[0].tolist() == [[1.0, 2.0], [3.0, 4.0]]
    assert parts[1].tolist() == [[5.0, 6.0], [7.0, 8.0], [9.0, 10.0]]
    assert parts[2].tolist() == [[-1.5, 2.5]]
    p = _write(tmp_path, "g.shp", _shp(5, [_record(1, 5, ring + line)]))
    parts = apt.read_shapefile(p, 5)
    assert [len(x) for x in parts] == [4, 2, 3] and parts[0][2].tolist() == [1.0, 1.0]


def test_reader_refusals(tmp_path):
    ring = [[(0.0, 0.0), (1.0, 0.0), (0.0, 0.0)]]
    p = _write(tmp_path, "wrong.shp", _shp(5, [_record(1, 5, ring)]))
    with pytest.raises(apt.InternalError, match="expected Polyline"):
        apt.read_shapefile(p, 3)  # iter_shapes_as::<Polyline> on a Polygon record
    p = _write(tmp_path, "point.shp", _shp(1, []))
    with pytest.raises(apt.UnsupportedError):
        apt.read_shapefile(p, 5)
    p = _write(tmp_path, "empty.shp", _shp(5, [_record(1, 5, [[(0.0, 0.0)], []])]))
    with pytest.raises(apt.InvalidError, match="empty part"):
        apt.read_shapefile(p, 5)
    p = _write(tmp_path, "short.shp", _shp(5, [_record(1, 5, ring)])[:-8])
    with pytest.raises(apt.InternalError):
        apt.read_shapefile(p, 5)
    missing = str(tmp_path / "nothing" / "states.shp")
    with pytest.raises(apt.InternalError) as e:
        apt.read_shapefile(missing, 3)
    assert str(e.value) == f'Could not load "{missing}"'


def test_layer_set_load_dir(tmp_path):
    ring = [[(0.0, 0.0), (1.0, 0.0), (0.0, 0.0)]]
    _write(tmp_path, "countries.shp", _shp(5, [_record(1, 5, ring)]))
    _write(tmp_path, "lakes.shp", _shp(5, [_record(1, 5, ring)]))
    with pytest.raises(apt.InternalError) as e:
        apt.MapLayers.load(str(tmp_path))  # the reference's copy has no states.shp either
    assert str(e.value) == f'Could not load "{tmp_path}/states.shp"'
    _write(tmp_path, "states.shp", _shp(3, [_record(1, 3, ring)]))
    apt.MapLayers.load(str(tmp_path)).close()
    with pytest.raises(apt.InvalidError):
        apt.MapLayers(countries=[np.zeros((2, 2)), np.zeros((0, 2))])
    with pytest.raises(apt.InvalidError):
        apt.MapSettings(lakes_color=(1, 2, 3))


def test_geo_known_answers():
    """geo.rs:112-145"""
    tol = PI / 1000.0
    d = mm.distance
    for a, b, want in [((0, 0), (0, PI / 6), PI / 6), ((0, 0), (PI / 6, 0), PI / 6), ((0, 0), (-PI / 6, 0), PI / 6),
                       ((PI / 6, 0), (0, 0), PI / 6), ((-PI / 6, 0), (0, 0), PI / 6), ((0, PI / 6), (0, 0), PI / 6),
                       ((0, 0), (PI, 0), PI), ((0, 0), (0, PI), PI), ((0, 0), (0, -PI), PI),
                       ((PI / 4, 0), (PI / 4, PI), PI / 2), ((0, PI / 4), (-PI / 6, PI / 4), PI / 6)]:
        assert abs(d(a, b) - want) <= tol
    for a, b, want in [((0, 0), (0, 0.001), 0.001), ((PI / 4, PI / 4), (PI / 4, PI / 4), 0.0), ((0, 0), (0, 2 * PI), 0.0)]:
        assert abs(d(a, b) - want) <= 0.000628
    az = mm.azimuth
    for a, b, want in [((0, 0), (0, PI / 6), PI / 2), ((0, 0), (PI / 6, 0), 0.0), ((0, 0), (-PI / 6, 0), PI),
                       ((PI / 6, 0), (0, 0), PI), ((-PI / 6, 0), (0, 0), 0.0), ((0, PI / 6), (0, 0), -PI / 2)]:
        assert abs(az(a, b) - want) <= tol


def test_xiaolin_wu_hand_derived():
    pts = mm.xiaolin_points
    # a zero-length segment still draws: one pixel on an integer y, two otherwise
    assert pts((2.0, 3.0), (2.0, 3.0)) == [((2, 3), 1.0)]
    assert pts((2.0, 3.25), (2.0, 3.25)) == [((2, 3), 0.75), ((2, 4), 0.25)]
    # shallow: gradient 1/2, y steps 0, 0.5, 1
    assert pts((0.0, 0.0), (2.0, 1.0)) == [((0, 0), 1.0), ((1, 0), 0.5), ((1, 1), 0.5), ((2, 1), 1.0)]
    # steep: the axes swap, points come back as (x, y)
    assert pts((0.0, 0.0), (1.0, 2.0)) == [((0, 0), 1.0), ((0, 1), 0.5), ((1, 1), 0.5), ((1, 2), 1.0)]
    # the end with the smaller major coordinate is the start
    assert pts((2.0, 1.0), (0.0, 0.0)) == pts((0.0, 0.0), (2.0, 1.0))
    # negative y truncates toward zero (NumCast), fpart from floor: y = -0.25 -> (0, 0) 0.25, lower (0, 1) 0.75
    assert pts((0.0, -0.25), (0.0, -0.25)) == [((0, 0), 0.25), ((0, 1), 0.75)]


def _blank(h):
    img = np.zeros((h, 2080, 4), np.uint8)
    img[..., 3] = 255
    return img


def test_band_edges_and_est_y():
    # est_y saturates, NaN -> 0
    assert mm.est_row(math.inf, 10) == 9 and mm.est_row(-math.inf, 10) == 0 and mm.est_row(math.nan, 10) == 0
    assert mm.est_row(3.99, 10) == 3 and mm.est_row(9.5, 10) == 9
    # fragments at y = 0 and y = h are never drawn, y = 1 .. h-1 are
    band = lambda x, y, h: x > -456 and x < 456 and y > 0 and y < h  # noqa: E731
    assert not band(0, 0, 10) and not band(0, 10, 10) and band(0, 1, 10) and band(0, 9, 10)
    assert not band(-456, 5, 10) and band(-455, 5, 10) and not band(456, 5, 10)


def test_far_side_clamped():
    # a vertex on the far side of the globe: distance is clamped to pi/3 before the projection
    sc = mm.Scalars([(0.0, 0.0), (0.01, 0.0)])
    x, y = mm.rel_px(sc, (0.0, PI * 0.9))
    x2, y2 = mm.rel_px(sc, (0.0, PI / 3))
    assert (x, y) == (x2, y2)
    assert x == -math.asin(math.sin(mm.azimuth((0.0, 0.0), (0.0, PI / 3)) - sc.ref_az) * math.sin(PI / 3)) / 0.0005


def test_blend_order_matters():
    bg = (10, 200, 30, 255)
    f1, f2 = (255, 0, 0, 100), (0, 0, 255, 180)
    a = mm.blend(mm.blend(bg, f1), f2)
    b = mm.blend(mm.blend(bg, f2), f1)
    assert a != b
    assert mm.blend(bg, (1, 2, 3, 0)) == bg and mm.blend(bg, (1, 2, 3, 255)) == (1, 2, 3, 255)
    # f32 by hand for one channel: 255 * ((fr*fa + br*ba*(1-fa)) / af), truncated
    f = np.float32
    fa, ba = f(100) / f(255), f(255) / f(255)
    af = ba + fa - ba * fa
    r = int(f(255) * ((f(255) / f(255) * fa + (f(10) / f(255) * ba) * (f(1) - fa)) / af))
    assert mm.blend(bg, f1)[0] == r
    # trunc(255 * fl(v / 255)) == v for every u8: over a background of alpha 255 the alpha 0 / 255 fast paths give what
    # the general formula gives (after a partial blend has left alpha 254 they need not)
    v = np.arange(256, dtype=np.float32)
    assert np.array_equal((f(255) * (v / f(255))).astype(np.int64), v.astype(np.int64))


def test_degenerate_track_draws_nothing():
    pos = np.tile([[math.radians(-30.0), math.radians(-60.0)]], (5, 1))
    layers = {"countries": [np.array([[-60.0, -30.0], [-59.0, -29.0], [-60.0, -29.5]])]}
    img = _blank(5)
    out, exc, info = mm.overlay(img, pos, layers)
    assert info["fragments"] == 0 and np.array_equal(out, img)


def test_rotate_model_edge_columns():
    img = np.zeros((4, 2080), np.uint8)
    img[1, 84] = img[1, 86] = img[1, 994] = 7
    r = mm.rotate_image(img)
    assert r[1, 84] == 7 and r[2, 994] == 7 and r[2, 86] == 7
