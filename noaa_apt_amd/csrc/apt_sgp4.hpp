// apt_sgp4.hpp — the satellite's sub-point for one image row (map.rs:51-58), shared by the host (apt_sat.cpp) and the
// gfx950 kernel (apt_kernels_track.hip): the same source text on both sides.
//
// The reference calls the `satellite` crate: propogate_datetime (SGP4 at (jd - jdsatepoch) * 1440 minutes),
// gstime_datetime (IAU-82) and eci_to_geodedic (WGS-84).  The crate is a port of satellite.js, itself a port of
// Vallado's 2006 code ("Revisiting Spacetrack Report #3", AIAA 2006-6753); this file is written from that algorithm:
// WGS-72 constants, "improved" mode, near-earth branch only, position only.
//
// With contraction off the f64 + - * /, sqrt, fmod and floor steps round alike on host and device; sin, cos, atan2 and
// pow are the C library's on the host and the device library's on the device and may differ by an ulp.
#pragma once

#include <cmath>
#include <cstdint>

#ifdef __HIP__
#include <hip/hip_runtime.h>
#define APT_HD __host__ __device__
#else
#define APT_HD
#endif

#pragma clang fp contract(off)

namespace apt::sat {

constexpr double kPi = 3.14159265358979323846;
constexpr double kTwoPi = 2.0 * kPi;
constexpr double kDeg2Rad = kPi / 180.0;
// WGS-72
constexpr double kMu = 398600.8;
constexpr double kRe = 6378.135;  // km
constexpr double kJ2 = 0.001082616;
constexpr double kJ3 = -0.00000253881;
constexpr double kJ4 = -0.00000165597;
constexpr double kJ3oJ2 = kJ3 / kJ2;
constexpr double kX2o3 = 2.0 / 3.0;
constexpr int64_t kLineMs = 500;  // two image rows per second (map.rs:26)

// The SGP4 error returns that can occur near earth (Vallado's numbering).
enum : int32_t { kErrEccentricity = 1, kErrMeanMotion = 2, kErrSemiLatus = 4, kErrDecayed = 6 };

// What sgp4init leaves for sgp4 (near earth): the elements and the secular / periodic coefficients.
struct Satrec {
    double jdsatepoch;
    double xke;  // 60 / sqrt(kRe^3 / kMu), computed once on the host
    double bstar, inclo, nodeo, ecco, argpo, mo, no;  // no: un-Kozai'd mean motion, rad / min
    double con41, x1mth2, x7thm1;
    double mdot, argpdot, nodedot, nodecf;
    double omgcof, xmcof, eta, delmo, sinmao;
    double cc1, cc4, cc5, t2cof, t3cof, t4cof, t5cof, d2, d3, d4;
    double xlcof, aycof;
    int32_t isimp;
    int32_t reserved;
};

// days since 1970-01-01 -> proleptic Gregorian (year, month, day); integers only
APT_HD inline void civil_from_days(int64_t z, int64_t &year, int64_t &month, int64_t &day)
{
    z += 719468;
    const int64_t era = (z >= 0 ? z : z - 146096) / 146097;
    const int64_t doe = z - era * 146097;
    const int64_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
    const int64_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
    const int64_t mp = (5 * doy + 2) / 153;
    day = doy - (153 * mp + 2) / 5 + 1;
    month = mp < 10 ? mp + 3 : mp - 9;
    year = yoe + era * 400 + (month <= 2 ? 1 : 0);
}

APT_HD inline double jday(double year, double mon, double day, double hr, double minute, double sec, double msec)
{
    return 367.0 * year - floor(7.0 * (year + floor((mon + 9.0) / 12.0)) * 0.25) + floor(275.0 * mon / 9.0) + day +
           1721013.5 + ((msec / 60000.0 + sec / 60.0 + minute) / 60.0 + hr) / 24.0;
}

// The Julian date of a chrono DateTime<Utc> held as integer milliseconds since the Unix epoch, from its calendar
// fields (assumed: the crate's jday carries the milliseconds; without them two rows would share a position).
APT_HD inline double jday_unix_ms(int64_t ms)
{
    int64_t days = ms / 86400000, rem = ms % 86400000;
    if (rem < 0) {
        rem += 86400000;
        days -= 1;
    }
    int64_t y, m, d;
    civil_from_days(days, y, m, d);
    const int64_t hr = rem / 3600000, r1 = rem % 3600000;
    const int64_t mi = r1 / 60000, r2 = r1 % 60000;
    return jday(static_cast<double>(y), static_cast<double>(m), static_cast<double>(d), static_cast<double>(hr),
                static_cast<double>(mi), static_cast<double>(r2 / 1000), static_cast<double>(r2 % 1000));
}

// Greenwich sidereal time, IAU-82, in [0, 2 pi)
APT_HD inline double gstime(double jd)
{
    const double t = (jd - 2451545.0) / 36525.0;
    const double sec = -6.2e-6 * t * t * t + 0.093104 * t * t + (876600.0 * 3600.0 + 8640184.812866) * t + 67310.54841;
    double g = fmod(sec * kDeg2Rad / 240.0, kTwoPi);
    if (g < 0.0) g += kTwoPi;
    return g;
}

// sgp4(satrec, tsince): ECI position in km, `t` minutes after the epoch.  Returns 0 or the SGP4 error.
APT_HD inline int32_t sgp4(const Satrec &s, double t, double &x, double &y, double &z)
{
    const double xmdf = s.mo + s.mdot * t;
    const double argpdf = s.argpo + s.argpdot * t;
    const double nodedf = s.nodeo + s.nodedot * t;
    double argpm = argpdf, mm = xmdf;
    const double t2 = t * t;
    double nodem = nodedf + s.nodecf * t2;
    double tempa = 1.0 - s.cc1 * t;
    double tempe = s.bstar * s.cc4 * t;
    double templ = s.t2cof * t2;
    if (s.isimp != 1) {
        const double delomg = s.omgcof * t;
        const double dm = 1.0 + s.eta * cos(xmdf);
        const double delm = s.xmcof * (dm * dm * dm - s.delmo);
        const double temp = delomg + delm;
        mm = xmdf + temp;
        argpm = argpdf - temp;
        const double t3 = t2 * t, t4 = t3 * t;
        tempa = tempa - s.d2 * t2 - s.d3 * t3 - s.d4 * t4;
        tempe = tempe + s.bstar * s.cc5 * (sin(mm) - s.sinmao);
        templ = templ + s.t3cof * t3 + t4 * (s.t4cof + t * s.t5cof);
    }
    double nm = s.no, em = s.ecco;
    if (nm <= 0.0) return kErrMeanMotion;
    const double am = pow(s.xke / nm, kX2o3) * tempa * tempa;
    nm = s.xke / pow(am, 1.5);
    em = em - tempe;
    if (em >= 1.0 || em < -0.001) return kErrEccentricity;
    if (em < 1.0e-6) em = 1.0e-6;
    mm = mm + s.no * templ;
    double xlm = mm + argpm + nodem;
    nodem = fmod(nodem, kTwoPi);
    argpm = fmod(argpm, kTwoPi);
    xlm = fmod(xlm, kTwoPi);
    mm = fmod(xlm - argpm - nodem, kTwoPi);
    const double sinip = sin(s.inclo), cosip = cos(s.inclo);

    // long-period periodics
    const double axnl = em * cos(argpm);
    double temp = 1.0 / (am * (1.0 - em * em));
    const double aynl = em * sin(argpm) + temp * s.aycof;
    const double xl = mm + argpm + nodem + temp * s.xlcof * axnl;

    // Kepler's equation
    const double u = fmod(xl - nodem, kTwoPi);
    double eo1 = u, tem5 = 9999.9, sineo1 = 0.0, coseo1 = 0.0;
    for (int ktr = 1; fabs(tem5) >= 1.0e-12 && ktr <= 10; ++ktr) {
        sineo1 = sin(eo1);
        coseo1 = cos(eo1);
        tem5 = 1.0 - coseo1 * axnl - sineo1 * aynl;
        tem5 = (u - aynl * coseo1 + axnl * sineo1 - eo1) / tem5;
        if (fabs(tem5) >= 0.95) tem5 = tem5 > 0.0 ? 0.95 : -0.95;
        eo1 = eo1 + tem5;
    }

    // short-period periodics
    const double ecose = axnl * coseo1 + aynl * sineo1;
    const double esine = axnl * sineo1 - aynl * coseo1;
    const double el2 = axnl * axnl + aynl * aynl;
    const double pl = am * (1.0 - el2);
    if (pl < 0.0) return kErrSemiLatus;
    const double rl = am * (1.0 - ecose);
    const double betal = sqrt(1.0 - el2);
    temp = esine / (1.0 + betal);
    const double sinu = am / rl * (sineo1 - aynl - axnl * temp);
    const double cosu = am / rl * (coseo1 - axnl + aynl * temp);
    double su = atan2(sinu, cosu);
    const double sin2u = (cosu + cosu) * sinu;
    const double cos2u = 1.0 - 2.0 * sinu * sinu;
    temp = 1.0 / pl;
    const double temp1 = 0.5 * kJ2 * temp;
    const double temp2 = temp1 * temp;
    const double mrt = rl * (1.0 - 1.5 * temp2 * betal * s.con41) + 0.5 * temp1 * s.x1mth2 * cos2u;
    su = su - 0.25 * temp2 * s.x7thm1 * sin2u;
    const double xnode = nodem + 1.5 * temp2 * cosip * sin2u;
    const double xinc = s.inclo + 1.5 * temp2 * cosip * sinip * cos2u;

    // orientation vectors
    const double sinsu = sin(su), cossu = cos(su);
    const double snod = sin(xnode), cnod = cos(xnode);
    const double sini = sin(xinc), cosi = cos(xinc);
    const double xmx = -snod * cosi, xmy = cnod * cosi;
    const double ux = xmx * sinsu + cnod * cossu;
    const double uy = xmy * sinsu + snod * cossu;
    const double uz = sini * sinsu;
    if (mrt < 1.0) return kErrDecayed;
    x = mrt * ux * kRe;
    y = mrt * uy * kRe;
    z = mrt * uz * kRe;
    return 0;
}

// satellite::transforms::eci_to_geodedic, latitude and longitude only (WGS-84; the wrap's exact form is assumed)
APT_HD inline void eci_to_geodetic(double x, double y, double z, double gmst, double &lat, double &lon)
{
    const double a = 6378.137, b = 6356.7523142;
    const double r = sqrt(x * x + y * y);
    const double f = (a - b) / a;
    const double e2 = 2.0 * f - f * f;
    lon = atan2(y, x) - gmst;
    while (lon < -kPi) lon += kTwoPi;
    while (lon > kPi) lon -= kTwoPi;
    lat = atan2(z, r);
    for (int k = 0; k < 20; ++k) {
        const double sl = sin(lat);
        const double c = 1.0 / sqrt(1.0 - e2 * (sl * sl));
        lat = atan2(z + a * c * e2 * sl, r);
    }
}

// (lat, lon) in rad at an integer millisecond timestamp.  Returns 0 or the SGP4 error (lat, lon then untouched).
APT_HD inline int32_t position(const Satrec &s, int64_t unix_ms, double &lat, double &lon)
{
    const double jd = jday_unix_ms(unix_ms);
    double x, y, z;
    const int32_t e = sgp4(s, (jd - s.jdsatepoch) * 1440.0, x, y, z);
    if (e) return e;
    eci_to_geodetic(x, y, z, gstime(jd), lat, lon);
    return 0;
}

// map.rs:43-46: RefTime::End(t) is `t - line_duration * height as i32`
APT_HD inline int64_t start_ms(bool ref_is_end, int64_t ref_ms, uint32_t height)
{
    return ref_is_end ? ref_ms - kLineMs * static_cast<int64_t>(static_cast<int32_t>(height)) : ref_ms;
}

}  // namespace apt::sat
