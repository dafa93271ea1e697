// apt_sat.cpp — host side of the satellite track (apt_sat.hpp): the TLE reader, sgp4init and the CPU entry points.
#include "apt_sat.hpp"

#include <cstdlib>
#include <mutex>

#include "apt_host.hpp"
#include "apt_map.hpp"

namespace apt::sat {

namespace {

struct Malformed {};

// a fixed-column decimal field: blanks around it, then only sign, digits and a point
double field(const std::string &line, size_t a, size_t b)
{
    std::string s = line.substr(a, b - a);
    const size_t i = s.find_first_not_of(' '), j = s.find_last_not_of(' ');
    if (i == std::string::npos) throw Malformed{};
    s = s.substr(i, j - i + 1);
    if (s.find_first_not_of("+-.0123456789") != std::string::npos) throw Malformed{};
    char *end = nullptr;
    const double v = std::strtod(s.c_str(), &end);
    if (end == s.c_str() || *end) throw Malformed{};
    return v;
}

bool digits(const std::string &s)
{
    return !s.empty() && s.find_first_not_of("0123456789") == std::string::npos;
}

// `smmmmmxe`: sign or blank, five digits with the decimal point in front of them, the exponent's sign and digit
// (`28923-4` = 0.28923e-4, `00000-0`, `00000+0`)
double implied(const std::string &line, size_t a)
{
    const std::string s = line.substr(a, 8);
    if (s.size() != 8 || (s[0] != ' ' && s[0] != '+' && s[0] != '-') || !digits(s.substr(1, 5)) ||
        (s[6] != '+' && s[6] != '-') || s[7] < '0' || s[7] > '9')
        throw Malformed{};
    const std::string text = std::string(s[0] == '-' ? "-" : "") + "0." + s.substr(1, 5) + "e" + s.substr(6, 2);
    return std::strtod(text.c_str(), nullptr);
}

void days2mdhms(int year, double days, int &mon, int &day, double &hr, double &minute, double &sec)
{
    const int lmonth[12] = {31, year % 4 == 0 ? 29 : 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
    const int dayofyr = static_cast<int>(std::floor(days));
    int i = 1, acc = 0;
    while (dayofyr > acc + lmonth[i - 1] && i < 12) {
        acc += lmonth[i - 1];
        ++i;
    }
    mon = i;
    day = dayofyr - acc;
    double t = (days - dayofyr) * 24.0;
    hr = std::floor(t);
    t = (t - hr) * 60.0;
    minute = std::floor(t);
    sec = (t - minute) * 60.0;
}

Elements record(const std::string &title, const std::string &l1, const std::string &l2)
{
    if (l1.size() < 61 || l2.size() < 63) throw Malformed{};
    if (!digits(l1.substr(18, 2))) throw Malformed{};
    Elements e;
    const size_t i = title.find_first_not_of(" \t"), j = title.find_last_not_of(" \t");
    e.name = i == std::string::npos ? std::string() : title.substr(i, j - i + 1);
    const int epochyr = std::atoi(l1.substr(18, 2).c_str());
    const double epochdays = field(l1, 20, 32);
    (void)field(l1, 33, 43);  // ndot and nddot: checked, not used by SGP4
    (void)implied(l1, 44);
    e.bstar = implied(l1, 53);
    e.inclo = field(l2, 8, 16) * kDeg2Rad;
    e.nodeo = field(l2, 17, 25) * kDeg2Rad;
    std::string ecc = l2.substr(26, 7);
    const size_t k = ecc.find_first_not_of(' ');
    if (k == std::string::npos || !digits(ecc.substr(k, ecc.find_last_not_of(' ') - k + 1))) throw Malformed{};
    ecc = ecc.substr(k, ecc.find_last_not_of(' ') - k + 1);
    e.ecco = std::strtod(("0." + ecc).c_str(), nullptr);
    e.argpo = field(l2, 34, 42) * kDeg2Rad;
    e.mo = field(l2, 43, 51) * kDeg2Rad;
    e.no_kozai = field(l2, 52, 63) / (1440.0 / kTwoPi);
    const int year = epochyr + (epochyr < 57 ? 2000 : 1900);
    int mon, day;
    double hr, minute, sec;
    days2mdhms(year, epochdays, mon, day, hr, minute, sec);
    e.jdsatepoch = jday(year, mon, day, hr, minute, sec, 0.0);
    return e;
}

struct Last {
    std::mutex m;
    std::string tle, name;
    Satrec rec;
    bool valid = false;
} g_last;

}  // namespace

std::vector<Elements> parse_multiple(const std::string &tle)
{
    std::vector<std::string> lines;
    for (size_t pos = 0; pos <= tle.size();) {
        size_t nl = tle.find('\n', pos);
        if (nl == std::string::npos) nl = tle.size();
        std::string ln = tle.substr(pos, nl - pos);
        while (!ln.empty() && ln.back() == '\r') ln.pop_back();
        lines.push_back(std::move(ln));
        pos = nl + 1;
    }
    std::vector<Elements> out;
    for (size_t i = 0; i + 2 < lines.size();) {
        if (lines[i + 1].compare(0, 2, "1 ") == 0 && lines[i + 2].compare(0, 2, "2 ") == 0) {
            try {
                out.push_back(record(lines[i], lines[i + 1], lines[i + 2]));
            } catch (const Malformed &) {
            }
            i += 3;
        } else {
            i += 1;
        }
    }
    return out;
}

Satrec sgp4init(const Elements &e)
{
    Satrec s{};
    s.jdsatepoch = e.jdsatepoch;
    s.xke = 60.0 / std::sqrt(kRe * kRe * kRe / kMu);
    s.bstar = e.bstar;
    s.inclo = e.inclo;
    s.nodeo = e.nodeo;
    s.ecco = e.ecco;
    s.argpo = e.argpo;
    s.mo = e.mo;
    const double ss = 78.0 / kRe + 1.0;
    const double qzms2t = std::pow((120.0 - 78.0) / kRe, 4.0);

    // initl: the un-Kozai'd mean motion and the auxiliary epoch quantities
    const double eccsq = s.ecco * s.ecco;
    const double omeosq = 1.0 - eccsq;
    const double rteosq = std::sqrt(omeosq);
    const double cosio = std::cos(s.inclo);
    const double cosio2 = cosio * cosio;
    const double ak = std::pow(s.xke / e.no_kozai, kX2o3);
    const double d1 = 0.75 * kJ2 * (3.0 * cosio2 - 1.0) / (rteosq * omeosq);
    double del = d1 / (ak * ak);
    const double adel = ak * (1.0 - del * del - del * (1.0 / 3.0 + 134.0 * del * del / 81.0));
    del = d1 / (adel * adel);
    s.no = e.no_kozai / (1.0 + del);
    const double ao = std::pow(s.xke / s.no, kX2o3);
    const double sinio = std::sin(s.inclo);
    const double po = ao * omeosq;
    const double con42 = 1.0 - 5.0 * cosio2;
    s.con41 = -con42 - cosio2 - cosio2;
    const double posq = po * po;
    const double rp = ao * (1.0 - s.ecco);

    if (kTwoPi / s.no >= 225.0)
        throw Error{ErrorKind::Unsupported,
                    "SGP4: \"" + e.name + "\" has a period of 225 minutes or more and needs the deep-space branch "
                    "(SDP4), which is not implemented"};

    s.isimp = rp < 220.0 / kRe + 1.0 ? 1 : 0;
    double sfour = ss, qzms24 = qzms2t;
    const double perige = (rp - 1.0) * kRe;
    if (perige < 156.0) {
        sfour = perige - 78.0;
        if (perige < 98.0) sfour = 20.0;
        qzms24 = std::pow((120.0 - sfour) / kRe, 4.0);
        sfour = sfour / kRe + 1.0;
    }
    const double pinvsq = 1.0 / posq;
    const double tsi = 1.0 / (ao - sfour);
    s.eta = ao * s.ecco * tsi;
    const double etasq = s.eta * s.eta;
    const double eeta = s.ecco * s.eta;
    const double psisq = std::fabs(1.0 - etasq);
    const double coef = qzms24 * std::pow(tsi, 4.0);
    const double coef1 = coef / std::pow(psisq, 3.5);
    const double cc2 = coef1 * s.no *
                       (ao * (1.0 + 1.5 * etasq + eeta * (4.0 + etasq)) +
                        0.375 * kJ2 * tsi / psisq * s.con41 * (8.0 + 3.0 * etasq * (8.0 + etasq)));
    s.cc1 = s.bstar * cc2;
    double cc3 = 0.0;
    if (s.ecco > 1.0e-4) cc3 = -2.0 * coef * tsi * kJ3oJ2 * s.no * sinio / s.ecco;
    s.x1mth2 = 1.0 - cosio2;
    s.cc4 = 2.0 * s.no * coef1 * ao * omeosq *
            (s.eta * (2.0 + 0.5 * etasq) + s.ecco * (0.5 + 2.0 * etasq) -
             kJ2 * tsi / (ao * psisq) *
                 (-3.0 * s.con41 * (1.0 - 2.0 * eeta + etasq * (1.5 - 0.5 * eeta)) +
                  0.75 * s.x1mth2 * (2.0 * etasq - eeta * (1.0 + etasq)) * std::cos(2.0 * s.argpo)));
    s.cc5 = 2.0 * coef1 * ao * omeosq * (1.0 + 2.75 * (etasq + eeta) + eeta * etasq);
    const double cosio4 = cosio2 * cosio2;
    const double temp1 = 1.5 * kJ2 * pinvsq * s.no;
    const double temp2 = 0.5 * temp1 * kJ2 * pinvsq;
    const double temp3 = -0.46875 * kJ4 * pinvsq * pinvsq * s.no;
    s.mdot = s.no + 0.5 * temp1 * rteosq * s.con41 + 0.0625 * temp2 * rteosq * (13.0 - 78.0 * cosio2 + 137.0 * cosio4);
    s.argpdot = -0.5 * temp1 * con42 + 0.0625 * temp2 * (7.0 - 114.0 * cosio2 + 395.0 * cosio4) +
                temp3 * (3.0 - 36.0 * cosio2 + 49.0 * cosio4);
    const double xhdot1 = -temp1 * cosio;
    s.nodedot = xhdot1 + (0.5 * temp2 * (4.0 - 19.0 * cosio2) + 2.0 * temp3 * (3.0 - 7.0 * cosio2)) * cosio;
    s.omgcof = s.bstar * cc3 * std::cos(s.argpo);
    s.xmcof = 0.0;
    if (s.ecco > 1.0e-4) s.xmcof = -kX2o3 * coef * s.bstar / eeta;
    s.nodecf = 3.5 * omeosq * xhdot1 * s.cc1;
    s.t2cof = 1.5 * s.cc1;
    // (the division is guarded for inclinations of 180 degrees)
    if (std::fabs(cosio + 1.0) > 1.5e-12) s.xlcof = -0.25 * kJ3oJ2 * sinio * (3.0 + 5.0 * cosio) / (1.0 + cosio);
    else s.xlcof = -0.25 * kJ3oJ2 * sinio * (3.0 + 5.0 * cosio) / 1.5e-12;
    s.aycof = -0.5 * kJ3oJ2 * sinio;
    const double dm = 1.0 + s.eta * std::cos(s.mo);
    s.delmo = dm * dm * dm;
    s.sinmao = std::sin(s.mo);
    s.x7thm1 = 7.0 * cosio2 - 1.0;
    if (s.isimp != 1) {
        const double cc1sq = s.cc1 * s.cc1;
        s.d2 = 4.0 * ao * tsi * cc1sq;
        const double temp = s.d2 * tsi * s.cc1 / 3.0;
        s.d3 = (17.0 * ao + sfour) * temp;
        s.d4 = 0.5 * temp * ao * tsi * (221.0 * ao + 31.0 * sfour) * s.cc1;
        s.t3cof = s.d2 + 2.0 * cc1sq;
        s.t4cof = 0.25 * (3.0 * s.d3 + s.cc1 * (12.0 * s.d2 + 10.0 * cc1sq));
        s.t5cof = 0.2 * (3.0 * s.d4 + 12.0 * s.cc1 * s.d3 + 6.0 * s.d2 * s.d2 + 15.0 * cc1sq * (2.0 * s.d2 + cc1sq));
    }
    return s;
}

Satrec satrec_for(const std::string &tle, const std::string &name)
{
    std::lock_guard<std::mutex> lock(g_last.m);
    if (g_last.valid && g_last.name == name && g_last.tle == tle) return g_last.rec;
    for (const Elements &e : parse_multiple(tle)) {
        if (e.name != name) continue;
        const Satrec rec = sgp4init(e);
        g_last.tle = tle;
        g_last.name = name;
        g_last.rec = rec;
        g_last.valid = true;
        return rec;
    }
    throw Error{ErrorKind::Internal, "Satellite \"" + name + "\" not found in TLE"};  // map.rs:37
}

std::string error_text(int32_t code)
{
    const char *what = code == kErrEccentricity ? "mean eccentricity out of range"
                       : code == kErrMeanMotion ? "mean motion not positive"
                       : code == kErrSemiLatus  ? "semi-latus rectum negative"
                       : code == kErrDecayed    ? "satellite has decayed"
                                                : "unknown";
    return "SGP4 error " + std::to_string(code) + ": " + what;
}

void track_host(const Satrec &s, bool ref_is_end, int64_t ref_ms, uint32_t height, double *out)
{
    const int64_t t0 = start_ms(ref_is_end, ref_ms, height);
    for (uint32_t i = 0; i < height; ++i) {
        const int32_t e = position(s, t0 + kLineMs * static_cast<int64_t>(i), out[2 * i], out[2 * i + 1]);
        if (e) throw Error{ErrorKind::Internal, error_text(e) + " (image row " + std::to_string(i) + ")"};
    }
}

bool south_to_north_pass(const Satrec &s, int64_t ref_ms)
{
    double lat0, lon0, lat1, lon1;
    int32_t e = position(s, ref_ms, lat0, lon0);
    if (!e) e = position(s, ref_ms + 2000, lat1, lon1);
    if (e) throw Error{ErrorKind::Internal, error_text(e)};
    const double azimuth = apt::map::geo_azimuth(lat0, lon0, lat1, lon1);
    // processing.rs:80 reads `azimuth < PI / 4. || azimuth > 3. * PI / 4.`, which an atan2 result in (-pi, pi] meets on
    // every stretch of a retrograde orbit (the NOAA sub-points always move west: azimuth about -0.24 rad northbound,
    // -2.90 rad southbound), so that test cannot tell the two apart.  What the function is documented to return
    // ("true if this was a south to north pass") is the heading's northward half:
    return std::fabs(azimuth) < kPi / 2.;
}

}  // namespace apt::sat
