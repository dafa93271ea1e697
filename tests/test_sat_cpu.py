"""The satellite track on the CPU (apt.sat_track_host, apt.south_to_north_pass, the TLE reader) against
np_sgp4_model.py and against the reference's own known answers (tests/golden/tle/known_answers.json, the rows of
geo.rs:225-233, which the reference's author computed with `predict`).  No GPU involved.

libm: CPython's math module and the library both call the C library's sin / cos / atan2 / pow / fmod on this
platform, so the host track is compared bit for bit throughout (no case needed the 1e-13 rad fallback)."""
import ctypes as C
import datetime
import json
import math
import os

import numpy as np
import pytest

import noaa_apt_amd as apt
import np_sgp4_model as sm

HERE = os.path.dirname(os.path.abspath(__file__))
TLE_DIR = os.path.join(HERE, "golden", "tle")
TLE_2018 = open(os.path.join(TLE_DIR, "weather_2018.txt")).read()
TLE_2020 = open(os.path.join(TLE_DIR, "noaa_2020.txt")).read()
KNOWN = json.load(open(os.path.join(TLE_DIR, "known_answers.json")))
SATS = (apt.SatName.NOAA15, apt.SatName.NOAA18, apt.SatName.NOAA19)
DAY_MS = 86400000


def orbit(tle, name, kind, ms, draw_map=None):
    ref = apt.RefTime.Start(ms) if kind == "start" else apt.RefTime.End(ms)
    return apt.OrbitSettings(name, tle, ref, draw_map)


def model_track(tle, name, kind, ms, height):
    return np.array(sm.track(tle, name, kind, ms, height), np.float64).reshape(-1, 2)


def bit_cases():
    """(label, tle, name, kind, ms, height): the cases of the bit-for-bit comparison (and of the GPU test)"""
    cases = []
    for label, tle in (("2018", TLE_2018), ("2020", TLE_2020)):
        for name in SATS:
            t0 = sm.epoch_unix_ms(sm.find(tle, name))
            for days in (0, 10, 120):
                cases.append((f"{label} {name} +{days}d", tle, name, "start", t0 + days * DAY_MS, 1200))
    t15 = sm.epoch_unix_ms(sm.find(TLE_2020, "NOAA 15"))
    cases.append(("end", TLE_2020, "NOAA 18", "end", t15 + 5 * DAY_MS, 1200))
    cases.append(("milliseconds", TLE_2020, "NOAA 19", "start", t15 + 3 * DAY_MS + 123, 1200))
    cases.append(("antimeridian",) + _find_window(lambda tr: np.any(np.abs(np.diff(tr[:, 1])) > math.pi)))
    cases.append(("highest latitude",) + _find_window(
        lambda tr: 10 < int(np.argmax(tr[:, 0])) < len(tr) - 10 and tr[:, 0].max() > math.radians(80.0)))
    return cases


def _find_window(pred):
    t0 = sm.epoch_unix_ms(sm.find(TLE_2020, "NOAA 15"))
    for k in range(40):
        ms = t0 + k * 300000
        if pred(model_track(TLE_2020, "NOAA 15", "start", ms, 1200)):
            return TLE_2020, "NOAA 15", "start", ms, 1200
    raise AssertionError("no such window within 200 minutes of the epoch")


def _known(track_fn):
    worst = []
    for row in KNOWN["rows"]:
        lat, lon = track_fn(orbit(TLE_2020, row["satellite"], "start", row["timestamp"] * 1000), 1)[0]
        lat, lon = math.degrees(lat), (math.degrees(lon) + 360.0) % 360.0  # geo.rs:243-248
        print(f"{row['satellite']} {row['timestamp']}: lat {lat - row['latitude']:+.5f} lon "
              f"{lon - row['longitude']:+.5f} deg (tolerance {row['tolerance']})")
        assert abs(lat - row["latitude"]) <= row["tolerance"], row
        assert abs(lon - row["longitude"]) <= row["tolerance"], row
        worst.append(max(abs(lat - row["latitude"]), abs(lon - row["longitude"])))
    return worst


# ---------------------------------------------------------------- 1. the reference's known answers
def test_known_answers_model():
    assert len(KNOWN["rows"]) == 7
    _known(lambda o, h: model_track(o.custom_tle, o.sat_name, "start", o.ref_time.unix_ms, h))


def test_known_answers_host():
    _known(apt.sat_track_host)


# ---------------------------------------------------------------- 2. host == model, bit for bit
@pytest.mark.parametrize("case", bit_cases(), ids=lambda c: c[0])
def test_host_equals_model_bitwise(case):
    _, tle, name, kind, ms, height = case
    got = apt.sat_track_host(orbit(tle, name, kind, ms), height)
    want = model_track(tle, name, kind, ms, height)
    assert got.shape == want.shape == (height, 2)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.all(np.abs(got[:, 1]) <= math.pi) and np.all(np.abs(got[:, 0]) < math.radians(82.0))


def test_end_is_start_minus_half_a_second_per_row():
    t = sm.epoch_unix_ms(sm.find(TLE_2020, "NOAA 19")) + 7777
    a = apt.sat_track_host(orbit(TLE_2020, "NOAA 19", "end", t, None), 640)
    b = apt.sat_track_host(orbit(TLE_2020, "NOAA 19", "start", t - 500 * 640), 640)
    assert np.array_equal(a, b)
    assert not np.array_equal(a[0], a[1])  # successive rows differ: the Julian date carries the milliseconds


def test_ref_time_from_datetime():
    dt = datetime.datetime(2020, 1, 28, 13, 7, 51, 250000, tzinfo=datetime.timezone.utc)
    assert apt.RefTime.Start(dt).unix_ms == 1580216871250
    east = dt.astimezone(datetime.timezone(datetime.timedelta(hours=5, minutes=30)))
    assert apt.RefTime.End(east).unix_ms == 1580216871250
    with pytest.raises(apt.InvalidError):
        apt.RefTime.Start(dt.replace(tzinfo=None))
    with pytest.raises(apt.InvalidError):
        apt.RefTime.Start(1.5)
    assert sm.jday_unix_ms(1580216871250) == sm.jday(2020.0, 1.0, 28.0, 13.0, 7.0, 51.0, 250.0)
    # the calendar split, against datetime, across leap days and before 1970
    for ms in (0, -1, 951782400000, 951868799999, 1709164800000, 4107542400000, -86400001):
        d = datetime.datetime(1970, 1, 1, tzinfo=datetime.timezone.utc) + datetime.timedelta(milliseconds=ms)
        assert sm.civil_from_days(ms // DAY_MS) == (d.year, d.month, d.day)


# ---------------------------------------------------------------- 3. the TLE reader
def _pos(tle, name, ms=1580000000000):
    return apt.sat_track_host(orbit(tle, name, "start", ms), 1)[0]


def test_parser_padded_names_and_crlf():
    assert "NOAA 15                 \n" in TLE_2018  # the fixture pads its title lines
    want = _pos(TLE_2018, "NOAA 15")
    assert np.array_equal(_pos(TLE_2018.replace("\n", "\r\n"), "NOAA 15"), want)
    assert np.array_equal(_pos("\n\n" + TLE_2018, "NOAA 15"), want)
    assert [n for n, _ in sm.parse_multiple(TLE_2018)][:4] == ["NOAA 15", "METEOSAT-8 (MSG-1)", "KALPANA-1 (METSAT 1)",
                                                               "NOAA 18"]
    assert len(sm.parse_multiple(TLE_2018)) == 48


def test_parser_name_not_found():
    with pytest.raises(apt.InternalError, match='^Satellite "NOAA 17" not found in TLE$'):
        _pos(TLE_2020, "NOAA 17")
    with pytest.raises(apt.InternalError, match='Satellite "NOAA 15" not found in TLE'):
        _pos("", "NOAA 15")
    with pytest.raises(sm.TleError, match='Satellite "NOAA 17" not found in TLE'):
        sm.find(TLE_2020, "NOAA 17")


def test_parser_exponent_fields():
    # bstar `28923-4`, nddot `00000-0`; METEOSAT-8 has bstar `00000+0`, FENGYUN 2F `00000-0`, METEOR-M 2 `-90071-6`
    e = dict(sm.parse_multiple(TLE_2018))
    assert e["NOAA 15"]["bstar"] == 0.28923e-4
    assert e["METEOSAT-8 (MSG-1)"]["bstar"] == 0.0 and e["FENGYUN 2F"]["bstar"] == 0.0
    assert e["METEOR-M 2"]["bstar"] == -0.90071e-6
    # the same through the library: a bstar of +0 / -0 gives the same track as the model's, a changed one moves it
    plus = TLE_2018.replace("28923-4", "00000+0")
    minus = TLE_2018.replace("28923-4", "00000-0")
    ms = sm.epoch_unix_ms(sm.find(TLE_2018, "NOAA 15")) + 30 * DAY_MS
    a, b = _pos(plus, "NOAA 15", ms), _pos(minus, "NOAA 15", ms)
    assert np.array_equal(a, b)
    assert np.array_equal(a, np.array(sm.track(plus, "NOAA 15", "start", ms, 1)[0]))
    assert not np.array_equal(a, _pos(TLE_2018, "NOAA 15", ms))
    neg = TLE_2018.replace(" 28923-4", "-28923-4")
    assert np.array_equal(_pos(neg, "NOAA 15", ms), np.array(sm.track(neg, "NOAA 15", "start", ms, 1)[0]))
    # two-digit epoch year: 98 is 1998, 20 is 2020
    old = TLE_2020.replace("20028.53684332", "98028.53684332")
    assert sm.find(old, "NOAA 15")["jdsatepoch"] == sm.find(TLE_2020, "NOAA 15")["jdsatepoch"] - 8035.0


def test_parser_skips_a_truncated_record():
    lines = TLE_2020.split("\n")
    lines[4] = lines[4][:40]  # NOAA 18's line 1
    text = "\n".join(lines)
    assert [n for n, _ in sm.parse_multiple(text)] == ["NOAA 15", "NOAA 19"]
    assert np.array_equal(_pos(text, "NOAA 19"), _pos(TLE_2020, "NOAA 19"))
    assert np.array_equal(_pos(text, "NOAA 15"), _pos(TLE_2020, "NOAA 15"))
    with pytest.raises(apt.InternalError, match='Satellite "NOAA 18" not found in TLE'):
        _pos(text, "NOAA 18")
    garbled = TLE_2020.replace("99.0657", "99.O657")  # a letter in NOAA 18's inclination
    with pytest.raises(apt.InternalError, match="not found"):
        _pos(garbled, "NOAA 18")


# ---------------------------------------------------------------- 4. refusals and SGP4 errors
def test_deep_space_is_refused():
    for name in ("METEOSAT-8 (MSG-1)", "GOES 16"):
        with pytest.raises(apt.UnsupportedError, match="deep-space"):
            _pos(TLE_2018, name)
        with pytest.raises(sm.DeepSpace):
            sm.sgp4init(sm.find(TLE_2018, name))


def test_sgp4_errors_are_errors():
    ecc = TLE_2020.replace(" 0009655 ", " 9999999 ")
    assert ecc != TLE_2020
    with pytest.raises(apt.InternalError, match="SGP4 error"):
        apt.sat_track_host(orbit(ecc, "NOAA 15", "start", 1580000000000), 50)
    # a large drag term, two decades ahead
    drag = TLE_2020.replace(" 22730-4 ", " 50000-2 ")
    assert drag != TLE_2020
    ms = sm.epoch_unix_ms(sm.find(drag, "NOAA 15")) + 7300 * DAY_MS
    with pytest.raises(sm.Sgp4Error) as model_err:
        sm.track(drag, "NOAA 15", "start", ms, 5)
    assert model_err.value.code == 6
    with pytest.raises(apt.InternalError, match="SGP4 error 6: satellite has decayed"):
        apt.sat_track_host(orbit(drag, "NOAA 15", "start", ms), 5)
    # a TLE that decays in the middle of a track: the rows before it are fine, the call is an error
    tle, ms_ok = decaying_case()
    with pytest.raises(apt.InternalError, match="SGP4 error"):
        apt.sat_track_host(orbit(tle, "NOAA 15", "start", ms_ok), 1200)
    got = apt.sat_track_host(orbit(tle, "NOAA 15", "start", ms_ok), 100)
    assert np.all(np.isfinite(got))
    assert np.array_equal(got, model_track(tle, "NOAA 15", "start", ms_ok, 100))


def decaying_case():
    """(tle, start): NOAA 15 with a drag term of 0.099999, and a start time 300 rows before the model's first SGP4
    error (about 159 days after the epoch), found by stepping the model"""
    tle = TLE_2020.replace(" 22730-4 ", " 99999-1 ")
    assert tle != TLE_2020
    e = sm.find(tle, "NOAA 15")
    s = sm.sgp4init(e)

    def ok(ms):
        try:
            sm.position(s, ms)
            return True
        except sm.Sgp4Error:
            return False
    ms = sm.epoch_unix_ms(e)
    for step in (3600000, 500):
        while ok(ms):
            ms += step
        if step != 500:
            ms -= step
    return tle, ms - 300 * 500


# ---------------------------------------------------------------- 5. the pass direction
def _stretch(rising):
    """a time at which the model's latitude rises (or falls) across the next 2 s, well inside such a stretch"""
    e = sm.find(TLE_2020, "NOAA 19")
    s = sm.sgp4init(e)
    t0 = sm.epoch_unix_ms(e)
    for k in range(200):
        ms = t0 + k * 60000
        lat = [sm.position(s, ms + d)[0] for d in (-240000, 0, 2000, 240000)]
        if all((b > a) == rising for a, b in zip(lat, lat[1:])):
            return ms
    raise AssertionError("no stretch found")


@pytest.mark.parametrize("kind", ["start", "end"])
def test_south_to_north_pass_northbound(kind):
    ms = _stretch(True)
    assert apt.south_to_north_pass(orbit(TLE_2020, "NOAA 19", kind, ms)) is True
    assert sm.south_to_north_pass(TLE_2020, "NOAA 19", ms) is True


@pytest.mark.parametrize("kind", ["start", "end"])
def test_south_to_north_pass_southbound(kind):
    ms = _stretch(False)
    assert apt.south_to_north_pass(orbit(TLE_2020, "NOAA 19", kind, ms)) is False
    assert sm.south_to_north_pass(TLE_2020, "NOAA 19", ms) is False


def test_south_to_north_pass_follows_the_latitude_all_round_the_orbit():
    """Every 20 s over two orbits: the library, the model's rule and the sign of the model's latitude change over the
    2 s agree (the turning points, where the 2 s change is below 1e-7 rad, are left out).  And the finding that made
    the rule necessary: processing.rs:80 as written is true at every one of these times, because the azimuth of a
    retrograde orbit is always negative."""
    e = sm.find(TLE_2020, "NOAA 18")
    s = sm.sgp4init(e)
    t0 = sm.epoch_unix_ms(e)
    seen = set()
    for k in range(610):
        ms = t0 + 20000 * k
        dlat = sm.position(s, ms + 2000)[0] - sm.position(s, ms)[0]
        az = sm.pass_azimuth(TLE_2020, "NOAA 18", ms)
        assert az < 0.0 and sm.reference_predicate(az)
        if abs(dlat) < 1e-7:
            continue
        got = apt.south_to_north_pass(orbit(TLE_2020, "NOAA 18", "start", ms))
        assert got is sm.south_to_north_pass(TLE_2020, "NOAA 18", ms) is (dlat > 0.0), (k, az, dlat)
        assert apt.south_to_north_pass(orbit(TLE_2020, "NOAA 18", "end", ms)) is got  # End is taken as given
        seen.add(got)
    assert seen == {True, False}


# ---------------------------------------------------------------- 6. the C boundary
def _c_orbit(**kw):
    from noaa_apt_amd.api import _COrbitSettings
    f = dict(struct_size=C.sizeof(_COrbitSettings), flags=0, sat_name=b"NOAA 15", tle=TLE_2020.encode(), ref_kind=0,
             reserved=0, ref_unix_ms=1580000000000, draw_map=None)
    f.update(kw)
    return _COrbitSettings(**f)


def _c_track(c):
    out = (C.c_double * 2)()
    err = C.create_string_buffer(1024)
    rc = apt.lib().aptgpu_sat_track_host(C.byref(c), 1, out, err, 1024)
    return rc, err.value.decode()


def test_abi_refusals():
    from noaa_apt_amd.api import _COrbitSettings
    assert C.sizeof(_COrbitSettings) == 48
    assert _c_track(_c_orbit())[0] == 0
    rc, msg = _c_track(_c_orbit(struct_size=C.sizeof(_COrbitSettings) - 8))
    assert rc == 4 and "struct_size" in msg
    rc, msg = _c_track(_c_orbit(flags=1))
    assert rc == 4 and "flags" in msg
    rc, msg = _c_track(_c_orbit(tle=None))
    assert rc == 5 and "tle is NULL" in msg
    rc, msg = _c_track(_c_orbit(ref_kind=2))
    assert rc == 4 and "ref_kind" in msg
    with pytest.raises(apt.UnsupportedError):
        apt.sat_track_host(apt.OrbitSettings(apt.SatName.NOAA15, None, apt.RefTime.Start(0)), 1)
    out = C.c_int(7)
    err = C.create_string_buffer(1024)
    assert apt.lib().aptgpu_south_to_north_pass(C.byref(_c_orbit(flags=2)), C.byref(out), err, 1024) == 4
    assert apt.abi_version() == 2
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "aptgpu.h")).read()
    for name in ("aptgpu_sat_track", "aptgpu_sat_track_host", "aptgpu_south_to_north_pass",
                 "aptgpu_process_image_orbit", "aptgpu_plan_process_device_image_orbit"):
        assert name + "(" in hdr and hasattr(apt.lib(), name)
    assert "#define APTGPU_ROTATE_ORBIT 2" in hdr and "#define APTGPU_SAT_REASON_SGP4 10" in hdr
    assert apt.SAT_REASON_SGP4 == 10 and apt.Rotate.ORBIT == 2


def test_process_argument_checks_need_no_device():
    # (everything here is refused before the device is touched)
    sig = np.zeros(2080 * 4, np.float32)
    o = orbit(TLE_2020, "NOAA 15", "start", 1580000000000, apt.MapSettings())
    with pytest.raises(apt.InvalidError, match="layers"):
        apt.process(None, sig, apt.Contrast.MINMAX, orbit=o)
    with pytest.raises(apt.UnsupportedError):  # as before: Rotate.ORBIT needs an OrbitSettings
        apt.process(None, sig, apt.Contrast.MINMAX, rotate=apt.Rotate.ORBIT)
    with pytest.raises(apt.UnsupportedError):
        apt.process(None, sig, apt.Contrast.MINMAX, orbit=object())
    with pytest.raises(apt.InternalError, match='Satellite "NOAA 17" not found in TLE'):
        apt.process(None, sig, apt.Contrast.MINMAX, rotate=apt.Rotate.ORBIT,
                    orbit=orbit(TLE_2020, "NOAA 17", "start", 0))
