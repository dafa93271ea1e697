"""A restatement of the satellite track of the reference's map overlay (src/map.rs:28-58) for the tests.

The reference calls the `satellite` crate (a port of satellite.js, itself a port of Vallado's 2006 SGP4): TLE text ->
elements, `sgp4init` (WGS-72, "improved" mode), `sgp4` at `(jd - jdsatepoch) * 1440` minutes, `gstime` (IAU-82) and
`eci_to_geodedic` (WGS-84, 20 fixed iterations).  The crate's source is not available here; this model is written from
the published algorithm (Vallado, Crawford, Hujsak, Kelso, "Revisiting Spacetrack Report #3", AIAA 2006-6753) and has
not been run against the crate.  Two points are assumptions: the Julian date carries the timestamp's milliseconds,
and the longitude is wrapped into [-pi, pi] by adding / subtracting 2 pi until it is inside.  What anchors the model is
the reference's own known-answer test (tests/golden/tle/known_answers.json, geo.rs:225-233).

Only the near-earth branch exists (period < 225 min); velocity is not computed.  Scalar f64 with the `math` module, i.e.
the C library's libm (`math.fmod`, never `%`): the host code of the library calls the same functions, so its track
must equal this one bit for bit.
"""
import math

TWO_PI = 2.0 * math.pi
DEG2RAD = math.pi / 180.0
XPDOTP = 1440.0 / TWO_PI  # revolutions per day per (radian per minute)

# WGS-72
MU = 398600.8
RE = 6378.135
XKE = 60.0 / math.sqrt(RE * RE * RE / MU)
J2 = 0.001082616
J3 = -0.00000253881
J4 = -0.00000165597
J3OJ2 = J3 / J2
X2O3 = 2.0 / 3.0

LINE_MS = 500  # two image rows per second (map.rs:26)

ERRORS = {1: "mean eccentricity out of range", 2: "mean motion not positive", 4: "semi-latus rectum negative",
          6: "satellite has decayed"}


class TleError(Exception):
    pass


class DeepSpace(Exception):
    """period >= 225 min: needs SDP4, which is out of scope"""


class Sgp4Error(Exception):
    def __init__(self, code):
        super().__init__(f"SGP4 error {code}: {ERRORS[code]}")
        self.code = code


# ---------------------------------------------------------------- time
def civil_from_days(z):
    """days since 1970-01-01 -> (year, month, day), proleptic Gregorian, integers only"""
    z += 719468
    era = z // 146097
    doe = z - era * 146097
    yoe = (doe - doe // 1460 + doe // 36524 - doe // 146096) // 365
    doy = doe - (365 * yoe + yoe // 4 - yoe // 100)
    mp = (5 * doy + 2) // 153
    day = doy - (153 * mp + 2) // 5 + 1
    month = mp + 3 if mp < 10 else mp - 9
    year = yoe + era * 400 + (1 if month <= 2 else 0)
    return year, month, day


def jday(year, mon, day, hr, minute, sec, msec=0.0):
    return (367.0 * year - math.floor(7.0 * (year + math.floor((mon + 9.0) / 12.0)) * 0.25)
            + math.floor(275.0 * mon / 9.0) + day + 1721013.5
            + ((msec / 60000.0 + sec / 60.0 + minute) / 60.0 + hr) / 24.0)


def jday_unix_ms(ms):
    """Julian date of an integer count of milliseconds since 1970-01-01T00:00:00Z, from its calendar fields"""
    days, rem = divmod(ms, 86400000)
    year, mon, day = civil_from_days(days)
    hr, rem = divmod(rem, 3600000)
    minute, rem = divmod(rem, 60000)
    sec, msec = divmod(rem, 1000)
    return jday(float(year), float(mon), float(day), float(hr), float(minute), float(sec), float(msec))


def gstime(jd):
    t = (jd - 2451545.0) / 36525.0
    sec = -6.2e-6 * t * t * t + 0.093104 * t * t + (876600.0 * 3600.0 + 8640184.812866) * t + 67310.54841
    g = math.fmod(sec * DEG2RAD / 240.0, TWO_PI)
    if g < 0.0:
        g += TWO_PI
    return g


def days2mdhms(year, days):
    lmonth = [31, 29 if year % 4 == 0 else 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31]
    dayofyr = int(math.floor(days))
    i, acc = 1, 0
    while dayofyr > acc + lmonth[i - 1] and i < 12:
        acc += lmonth[i - 1]
        i += 1
    t = (days - dayofyr) * 24.0
    hr = math.floor(t)
    t = (t - hr) * 60.0
    minute = math.floor(t)
    sec = (t - minute) * 60.0
    return i, dayofyr - acc, hr, minute, sec


# ---------------------------------------------------------------- TLE text
def _num(s):
    s = s.strip()
    if not s or any(c not in "+-.0123456789" for c in s):
        raise TleError(s)
    try:
        return float(s)
    except ValueError:
        raise TleError(s)


def _implied(s):
    """`smmmmmxe`: sign or blank, five digits with the point in front, exponent sign, one digit"""
    if len(s) != 8 or s[0] not in " +-" or not s[1:6].isdigit() or s[6] not in "+-" or not s[7].isdigit():
        raise TleError(s)
    return float(("-" if s[0] == "-" else "") + "0." + s[1:6] + "e" + s[6:8])


def parse_record(l1, l2):
    if len(l1) < 61 or len(l2) < 63 or l1[:2] != "1 " or l2[:2] != "2 ":
        raise TleError("short line")
    if not l1[18:20].isdigit() or not l2[26:33].strip().isdigit():
        raise TleError("digits")
    e = {
        "epochyr": int(l1[18:20]),
        "epochdays": _num(l1[20:32]),
        "bstar": _implied(l1[53:61]),
        "inclo": _num(l2[8:16]) * DEG2RAD,
        "nodeo": _num(l2[17:25]) * DEG2RAD,
        "ecco": float("0." + l2[26:33].strip()),
        "argpo": _num(l2[34:42]) * DEG2RAD,
        "mo": _num(l2[43:51]) * DEG2RAD,
        "no_kozai": _num(l2[52:63]) / XPDOTP,
    }
    _num(l1[33:43])      # ndot, nddot: validated, unused by SGP4
    _implied(l1[44:52])
    year = e["epochyr"] + (2000 if e["epochyr"] < 57 else 1900)
    mon, day, hr, minute, sec = days2mdhms(year, e["epochdays"])
    e["jdsatepoch"] = jday(float(year), float(mon), float(day), hr, minute, sec)
    return e


def parse_multiple(text):
    """[(name, elements)] of every well-formed title / line 1 / line 2 group; malformed ones are skipped"""
    lines = [ln.rstrip("\r") for ln in text.split("\n")]
    out = []
    i = 0
    while i + 2 < len(lines):
        if lines[i + 1].startswith("1 ") and lines[i + 2].startswith("2 "):
            try:
                out.append((lines[i].strip(), parse_record(lines[i + 1], lines[i + 2])))
            except TleError:
                pass
            i += 3
        else:
            i += 1
    return out


def find(text, name):
    for n, e in parse_multiple(text):
        if n == name:
            return e
    raise TleError(f'Satellite "{name}" not found in TLE')


# ---------------------------------------------------------------- sgp4init (near earth)
def sgp4init(e):
    ecco, argpo, inclo, mo, bstar = e["ecco"], e["argpo"], e["inclo"], e["mo"], e["bstar"]
    no = e["no_kozai"]
    ss = 78.0 / RE + 1.0
    qzms2t = math.pow((120.0 - 78.0) / RE, 4.0)

    # initl
    eccsq = ecco * ecco
    omeosq = 1.0 - eccsq
    rteosq = math.sqrt(omeosq)
    cosio = math.cos(inclo)
    cosio2 = cosio * cosio
    ak = math.pow(XKE / no, X2O3)
    d1 = 0.75 * J2 * (3.0 * cosio2 - 1.0) / (rteosq * omeosq)
    del_ = d1 / (ak * ak)
    adel = ak * (1.0 - del_ * del_ - del_ * (1.0 / 3.0 + 134.0 * del_ * del_ / 81.0))
    del_ = d1 / (adel * adel)
    no = no / (1.0 + del_)
    ao = math.pow(XKE / no, X2O3)
    sinio = math.sin(inclo)
    po = ao * omeosq
    con42 = 1.0 - 5.0 * cosio2
    con41 = -con42 - cosio2 - cosio2
    posq = po * po
    rp = ao * (1.0 - ecco)

    if TWO_PI / no >= 225.0:
        raise DeepSpace()

    s = dict(e)
    s["no"] = no
    s["con41"] = con41
    s["isimp"] = 1 if rp < 220.0 / RE + 1.0 else 0
    sfour = ss
    qzms24 = qzms2t
    perige = (rp - 1.0) * RE
    if perige < 156.0:
        sfour = perige - 78.0
        if perige < 98.0:
            sfour = 20.0
        qzms24 = math.pow((120.0 - sfour) / RE, 4.0)
        sfour = sfour / RE + 1.0
    pinvsq = 1.0 / posq
    tsi = 1.0 / (ao - sfour)
    eta = ao * ecco * tsi
    etasq = eta * eta
    eeta = ecco * eta
    psisq = abs(1.0 - etasq)
    coef = qzms24 * math.pow(tsi, 4.0)
    coef1 = coef / math.pow(psisq, 3.5)
    cc2 = coef1 * no * (ao * (1.0 + 1.5 * etasq + eeta * (4.0 + etasq))
                        + 0.375 * J2 * tsi / psisq * con41 * (8.0 + 3.0 * etasq * (8.0 + etasq)))
    cc1 = bstar * cc2
    cc3 = 0.0
    if ecco > 1.0e-4:
        cc3 = -2.0 * coef * tsi * J3OJ2 * no * sinio / ecco
    x1mth2 = 1.0 - cosio2
    cc4 = 2.0 * no * coef1 * ao * omeosq * (
        eta * (2.0 + 0.5 * etasq) + ecco * (0.5 + 2.0 * etasq)
        - J2 * tsi / (ao * psisq) * (-3.0 * con41 * (1.0 - 2.0 * eeta + etasq * (1.5 - 0.5 * eeta))
                                     + 0.75 * x1mth2 * (2.0 * etasq - eeta * (1.0 + etasq)) * math.cos(2.0 * argpo)))
    cc5 = 2.0 * coef1 * ao * omeosq * (1.0 + 2.75 * (etasq + eeta) + eeta * etasq)
    cosio4 = cosio2 * cosio2
    temp1 = 1.5 * J2 * pinvsq * no
    temp2 = 0.5 * temp1 * J2 * pinvsq
    temp3 = -0.46875 * J4 * pinvsq * pinvsq * no
    s["mdot"] = (no + 0.5 * temp1 * rteosq * con41
                 + 0.0625 * temp2 * rteosq * (13.0 - 78.0 * cosio2 + 137.0 * cosio4))
    s["argpdot"] = (-0.5 * temp1 * con42 + 0.0625 * temp2 * (7.0 - 114.0 * cosio2 + 395.0 * cosio4)
                    + temp3 * (3.0 - 36.0 * cosio2 + 49.0 * cosio4))
    xhdot1 = -temp1 * cosio
    s["nodedot"] = xhdot1 + (0.5 * temp2 * (4.0 - 19.0 * cosio2) + 2.0 * temp3 * (3.0 - 7.0 * cosio2)) * cosio
    s["omgcof"] = bstar * cc3 * math.cos(argpo)
    s["xmcof"] = 0.0
    if ecco > 1.0e-4:
        s["xmcof"] = -X2O3 * coef * bstar / eeta
    s["nodecf"] = 3.5 * omeosq * xhdot1 * cc1
    s["t2cof"] = 1.5 * cc1
    if abs(cosio + 1.0) > 1.5e-12:
        s["xlcof"] = -0.25 * J3OJ2 * sinio * (3.0 + 5.0 * cosio) / (1.0 + cosio)
    else:
        s["xlcof"] = -0.25 * J3OJ2 * sinio * (3.0 + 5.0 * cosio) / 1.5e-12
    s["aycof"] = -0.5 * J3OJ2 * sinio
    dm = 1.0 + eta * math.cos(mo)
    s["delmo"] = dm * dm * dm
    s["sinmao"] = math.sin(mo)
    s["x7thm1"] = 7.0 * cosio2 - 1.0
    s["x1mth2"] = x1mth2
    s["eta"] = eta
    s["cc1"], s["cc4"], s["cc5"] = cc1, cc4, cc5
    s["d2"] = s["d3"] = s["d4"] = s["t3cof"] = s["t4cof"] = s["t5cof"] = 0.0
    if s["isimp"] != 1:
        cc1sq = cc1 * cc1
        d2 = 4.0 * ao * tsi * cc1sq
        temp = d2 * tsi * cc1 / 3.0
        d3 = (17.0 * ao + sfour) * temp
        d4 = 0.5 * temp * ao * tsi * (221.0 * ao + 31.0 * sfour) * cc1
        s["d2"], s["d3"], s["d4"] = d2, d3, d4
        s["t3cof"] = d2 + 2.0 * cc1sq
        s["t4cof"] = 0.25 * (3.0 * d3 + cc1 * (12.0 * d2 + 10.0 * cc1sq))
        s["t5cof"] = 0.2 * (3.0 * d4 + 12.0 * cc1 * d3 + 6.0 * d2 * d2 + 15.0 * cc1sq * (2.0 * d2 + cc1sq))
    return s


# ---------------------------------------------------------------- sgp4
def sgp4(s, t):
    """ECI position (km) `t` minutes after the epoch"""
    xmdf = s["mo"] + s["mdot"] * t
    argpdf = s["argpo"] + s["argpdot"] * t
    nodedf = s["nodeo"] + s["nodedot"] * t
    argpm = argpdf
    mm = xmdf
    t2 = t * t
    nodem = nodedf + s["nodecf"] * t2
    tempa = 1.0 - s["cc1"] * t
    tempe = s["bstar"] * s["cc4"] * t
    templ = s["t2cof"] * t2
    if s["isimp"] != 1:
        delomg = s["omgcof"] * t
        dm = 1.0 + s["eta"] * math.cos(xmdf)
        delm = s["xmcof"] * (dm * dm * dm - s["delmo"])
        temp = delomg + delm
        mm = xmdf + temp
        argpm = argpdf - temp
        t3 = t2 * t
        t4 = t3 * t
        tempa = tempa - s["d2"] * t2 - s["d3"] * t3 - s["d4"] * t4
        tempe = tempe + s["bstar"] * s["cc5"] * (math.sin(mm) - s["sinmao"])
        templ = templ + s["t3cof"] * t3 + t4 * (s["t4cof"] + t * s["t5cof"])
    nm = s["no"]
    em = s["ecco"]
    if nm <= 0.0:
        raise Sgp4Error(2)
    am = math.pow(XKE / nm, X2O3) * tempa * tempa
    nm = XKE / math.pow(am, 1.5)
    em = em - tempe
    if em >= 1.0 or em < -0.001:
        raise Sgp4Error(1)
    if em < 1.0e-6:
        em = 1.0e-6
    mm = mm + s["no"] * templ
    xlm = mm + argpm + nodem
    nodem = math.fmod(nodem, TWO_PI)
    argpm = math.fmod(argpm, TWO_PI)
    xlm = math.fmod(xlm, TWO_PI)
    mm = math.fmod(xlm - argpm - nodem, TWO_PI)
    sinip = math.sin(s["inclo"])
    cosip = math.cos(s["inclo"])

    axnl = em * math.cos(argpm)
    temp = 1.0 / (am * (1.0 - em * em))
    aynl = em * math.sin(argpm) + temp * s["aycof"]
    xl = mm + argpm + nodem + temp * s["xlcof"] * axnl

    u = math.fmod(xl - nodem, TWO_PI)
    eo1 = u
    tem5 = 9999.9
    ktr = 1
    sineo1 = coseo1 = 0.0
    while abs(tem5) >= 1.0e-12 and ktr <= 10:
        sineo1 = math.sin(eo1)
        coseo1 = math.cos(eo1)
        tem5 = 1.0 - coseo1 * axnl - sineo1 * aynl
        tem5 = (u - aynl * coseo1 + axnl * sineo1 - eo1) / tem5
        if abs(tem5) >= 0.95:
            tem5 = 0.95 if tem5 > 0.0 else -0.95
        eo1 = eo1 + tem5
        ktr += 1

    ecose = axnl * coseo1 + aynl * sineo1
    esine = axnl * sineo1 - aynl * coseo1
    el2 = axnl * axnl + aynl * aynl
    pl = am * (1.0 - el2)
    if pl < 0.0:
        raise Sgp4Error(4)
    rl = am * (1.0 - ecose)
    betal = math.sqrt(1.0 - el2)
    temp = esine / (1.0 + betal)
    sinu = am / rl * (sineo1 - aynl - axnl * temp)
    cosu = am / rl * (coseo1 - axnl + aynl * temp)
    su = math.atan2(sinu, cosu)
    sin2u = (cosu + cosu) * sinu
    cos2u = 1.0 - 2.0 * sinu * sinu
    temp = 1.0 / pl
    temp1 = 0.5 * J2 * temp
    temp2 = temp1 * temp
    mrt = rl * (1.0 - 1.5 * temp2 * betal * s["con41"]) + 0.5 * temp1 * s["x1mth2"] * cos2u
    su = su - 0.25 * temp2 * s["x7thm1"] * sin2u
    xnode = nodem + 1.5 * temp2 * cosip * sin2u
    xinc = s["inclo"] + 1.5 * temp2 * cosip * sinip * cos2u
    sinsu = math.sin(su)
    cossu = math.cos(su)
    snod = math.sin(xnode)
    cnod = math.cos(xnode)
    sini = math.sin(xinc)
    cosi = math.cos(xinc)
    xmx = -snod * cosi
    xmy = cnod * cosi
    ux = xmx * sinsu + cnod * cossu
    uy = xmy * sinsu + snod * cossu
    uz = sini * sinsu
    if mrt < 1.0:
        raise Sgp4Error(6)
    return mrt * ux * RE, mrt * uy * RE, mrt * uz * RE


# ---------------------------------------------------------------- ECI -> geodetic (WGS-84)
def eci_to_geodetic(x, y, z, gmst):
    a = 6378.137
    b = 6356.7523142
    r = math.sqrt(x * x + y * y)
    f = (a - b) / a
    e2 = 2.0 * f - f * f
    lon = math.atan2(y, x) - gmst
    while lon < -math.pi:
        lon += TWO_PI
    while lon > math.pi:
        lon -= TWO_PI
    lat = math.atan2(z, r)
    for _ in range(20):
        sl = math.sin(lat)
        c = 1.0 / math.sqrt(1.0 - e2 * (sl * sl))
        lat = math.atan2(z + a * c * e2 * sl, r)
    return lat, lon


def position(s, unix_ms):
    """(lat, lon) in rad of the sub-satellite point at an integer millisecond timestamp"""
    jd = jday_unix_ms(unix_ms)
    x, y, z = sgp4(s, (jd - s["jdsatepoch"]) * 1440.0)
    return eci_to_geodetic(x, y, z, gstime(jd))


def start_ms(ref_kind, ref_ms, height):
    """map.rs:43-46; ref_kind 'start' or 'end'"""
    return ref_ms if ref_kind == "start" else ref_ms - LINE_MS * height


def track(text, name, ref_kind, ref_ms, height):
    """[(lat, lon)] for the `height` rows of an image (map.rs:41-58)"""
    s = sgp4init(find(text, name))
    t0 = start_ms(ref_kind, ref_ms, height)
    return [position(s, t0 + LINE_MS * i) for i in range(height)]


def epoch_unix_ms(e):
    """the TLE epoch as integer milliseconds (rounded down): a convenient anchor for test times"""
    return int(math.floor((e["jdsatepoch"] - 2440587.5) * 86400000.0))


def pass_azimuth(text, name, ref_ms):
    """processing.rs:57-77: geo::azimuth between the sub-points at the reference time as given (Start or End alike)
    and 2 s later"""
    from np_map_model import azimuth
    s = sgp4init(find(text, name))
    return azimuth(position(s, ref_ms), position(s, ref_ms + 2000))


def reference_predicate(az):
    """processing.rs:80 as written.  True for every heading but the eastward quarter, so for a retrograde orbit
    (azimuth in (-pi, 0)) on northbound and southbound stretches alike."""
    return az < math.pi / 4.0 or az > 3.0 * math.pi / 4.0


def south_to_north_pass(text, name, ref_ms):
    """what processing::south_to_north_pass documents: the heading lies in the northward half"""
    return abs(pass_azimuth(text, name, ref_ms)) < math.pi / 2.0
