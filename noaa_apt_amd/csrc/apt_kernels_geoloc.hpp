// apt_kernels_geoloc.hpp — the geolocation stage behind the decode: where on the Earth swath pixel (row, column)
// lies, the cosine of the solar zenith angle there, and the visible rows normalised by it (apt_kernels_geoloc.hip on
// the GPU, apt_geoloc.cpp on the CPU).  The reference has no such stage, so this is the definition
// (include/aptgpu.h states it in full; tests/np_geoloc_model.py in numpy).  The per-pixel and per-row arithmetic is
// written once, here, for both sides.
//
//  Frame   S, T, R from the overlay's scalars (start point and reference azimuth): the closed inverse of
//          latlon_to_rel_px (map.rs:71-100) is a rotation of the unit vector (cos b cos a, cos b sin a, sin b).
//  Point   x = x_rel + xoff[r], b = -x * x_res, a = (r - yaw * x) * y_res; valid iff acos(cos a cos b) < pi / 3.
//          The vector form keeps its precision at the pole, where asin / acos forms lose half the mantissa.
//  Sun     the Astronomical Almanac's low-precision series per row, f64: the unit vector of the sub-solar point.
//  Rows    f32: black + (x - black) / fmaxf(c, cmin) on the valid pixels, x elsewhere.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#include "apt_kernels_despeckle.hpp"  // key_of_bits / bits_of_key, APT_DSP_HD

namespace apt::geoloc {

constexpr int kPx = 2080;
constexpr int kHalfPx = 1040;
constexpr int kVideo0 = 86, kVideoN = 909;  // the video columns [base + 86, base + 995)
constexpr int kCentre = 453;                // video column of relative pixel 0 (image column 539 of channel A)
constexpr int kReasonCount = 7, kReasonSgp4 = 10, kReasonHeight = 15, kReasonDecode = 16;
constexpr double kPi = 3.14159265358979323846;
constexpr int64_t kLineMs = 500;
constexpr uint32_t kMaxRows = 1u << 22;  // rows of one recording the stage takes (36 minutes of APT are 4320)

// the overlay's per-call scalars as the pixel arithmetic reads them
struct Frame {
    double s[3], t[3], r[3];
    double x_res, y_res, yaw;
};

APT_DSP_HD Frame frame_of(double lat0, double lon0, double ref_az, double x_res, double y_res, double yaw)
{
    const double sp = sin(lat0), cp = cos(lat0), sl = sin(lon0), cl = cos(lon0);
    const double sa = sin(ref_az), ca = cos(ref_az);
    const double n[3] = {-sp * cl, -sp * sl, cp};
    const double e[3] = {-sl, cl, 0.};
    Frame f{};
    f.s[0] = cp * cl;
    f.s[1] = cp * sl;
    f.s[2] = sp;
    for (int i = 0; i < 3; ++i) {
        f.t[i] = ca * n[i] + sa * e[i];
        f.r[i] = -sa * n[i] + ca * e[i];
    }
    f.x_res = x_res;
    f.y_res = y_res;
    f.yaw = yaw;
    return f;
}

// xoff[r] as the stage reads it, from latlon_to_rel_px(track[r]).x as evaluated.  Row 0's is 0: track[0] is the start point, whose relative pixel is (0, 0), while
// latlon_to_rel_px evaluated there turns one ulp of the cosine of a zero distance into acos(1 - 2^-53) = 1.5e-8 rad,
// 3e-5 px at hscale 1, in a direction that atan2(0, +-0) picks.  Which of the two a library returns is its own
// rounding (glibc and the device library differ on the same track).
APT_DSP_HD double xoff_of(double evaluated, uint32_t r) { return r == 0 ? 0. : evaluated; }

struct Point {
    double x, y, z;
    bool valid;
};

// the forward point of row r, video column k (x_rel = k - kCentre)
APT_DSP_HD Point point_of(const Frame &f, double xoff, uint32_t r, int k)
{
    const double x = static_cast<double>(k - kCentre) + xoff;
    const double b = -x * f.x_res;
    const double a = (static_cast<double>(r) - f.yaw * x) * f.y_res;
    const double sb = sin(b), cb = cos(b), sa = sin(a), ca = cos(a);
    const double u = cb * ca, v = cb * sa;
    Point p;
    p.x = (u * f.s[0] + v * f.t[0]) + sb * f.r[0];
    p.y = (u * f.s[1] + v * f.t[1]) + sb * f.r[1];
    p.z = (u * f.s[2] + v * f.t[2]) + sb * f.r[2];
    p.valid = acos(ca * cb) < kPi / 3.;
    return p;
}

APT_DSP_HD void latlon_of(const Point &p, double &lat, double &lon)
{
    lat = atan2(p.z, hypot(p.x, p.y));
    lon = atan2(p.y, p.x);
}

// declination and right ascension minus sidereal time (the sub-solar longitude before wrapping) at t_ms
APT_DSP_HD void sun_angles(int64_t t_ms, double &delta, double &lon)
{
    const double rad = kPi / 180.;
    const double n = static_cast<double>(t_ms) / 86400000. + 2440587.5 - 2451545.0;
    const double l = fmod(280.460 + 0.9856474 * n, 360.);
    const double g = fmod(357.528 + 0.9856003 * n, 360.) * rad;
    const double lam = (l + 1.915 * sin(g) + 0.020 * sin(2. * g)) * rad;
    const double eps = (23.439 - 0.0000004 * n) * rad;
    const double alpha = atan2(cos(eps) * sin(lam), cos(lam));
    delta = asin(sin(eps) * sin(lam));
    const double theta = 15. * fmod(18.697374558 + 24.06570982441908 * n, 24.) * rad;
    lon = alpha - theta;
}

// the unit vector of the sub-solar point at t_ms
APT_DSP_HD void sun_of(int64_t t_ms, double (&u)[3])
{
    double delta, lon;
    sun_angles(t_ms, delta, lon);
    const double cd = cos(delta);
    u[0] = cd * cos(lon);
    u[1] = cd * sin(lon);
    u[2] = sin(delta);
}

APT_DSP_HD float cos_sun_of(const Point &p, const double *u)
{
    return static_cast<float>((p.x * u[0] + p.y * u[1]) + p.z * u[2]);
}

APT_DSP_HD float normalised(float x, float c, float black, float cmin, bool valid)
{
    const float d = c > cmin ? c : cmin;  // fmaxf(c, cmin): c is never NaN where valid
    return valid ? black + (x - black) / d : x;
}

// row 0's time: RefTime::End needs the height (map.rs:45)
APT_DSP_HD int64_t start_ms_of(bool ref_is_end, int64_t ref_ms, uint32_t h)
{
    return ref_is_end ? ref_ms - kLineMs * static_cast<int64_t>(h) : ref_ms;
}

APT_DSP_HD float quiet_nan() { return __builtin_nanf(""); }
APT_DSP_HD double quiet_nan64() { return __builtin_nan(""); }

// what a pixel adds to the record
struct Counters {
    unsigned long long n_outside = 0, n_capped = 0;
    uint32_t min_key = 0xFFFFFFFFu, max_key = 0u;  // totalOrder keys of cos_sun over the valid pixels
};

}  // namespace apt::geoloc

// ---- the host side (apt_geoloc.cpp; CPU only)
#include "../../include/aptgpu.h"
#include "apt_host.hpp"
#include "apt_map.hpp"

namespace apt::geoloc {

enum Out : unsigned { kOutLatLon = 1u, kOutCos = 2u, kOutRows = 4u };

struct Settings {
    int channel;  // 0 A, 1 B
    bool ref_is_end;
    int64_t ref_ms;
    float black, cmin;
};
// Required.  A struct_size that is too small, a flag, a channel other than 0 / 1, a time_kind other than START / END,
// a non-finite black level, max_zenith_deg outside (0, 90): Error{Invalid}.
Settings check_settings(const aptgpu_geoloc_settings *s);
// yaw, hscale, vscale of a nullable aptgpu_map_settings (0, 1, 1)
struct Geom {
    double yaw = 0., hscale = 1., vscale = 1.;
};
Geom check_geom(const aptgpu_map_settings *map);
// What every entry point refuses before it touches a device: both or neither of positions and orbit, rows asked for
// without a signal, more than kMaxRows rows.
void check_call(const void *positions, const void *orbit, bool want_rows, bool have_signal, size_t rows);
const char *reason_text(int reason);
// delta and the sub-solar longitude in (-pi, pi], radians
void sun_position(int64_t unix_ms, double out[2]);
// writes min(struct_size, sizeof) bytes of `r` (whose struct_size is then the caller's) into *out; null: nothing
void put_result(aptgpu_geoloc_result *out, aptgpu_geoloc_result r);
// The definition in plain C++.  track: `count` (lat, lon) pairs.  latlon (nullable) receives h * 909 pairs, cos_sun
// (nullable) h * 909 floats, rows (nullable; x required then, rows == x allowed) n floats.  *info is the record.  A
// failed record throws Error{Internal} after filling *info; nothing is written then.
void run_host(const float *x, size_t n, const double *track, size_t count, const Geom &g, const Settings &s,
              double *latlon, float *cos_sun, float *rows, aptgpu_geoloc_result *info);

}  // namespace apt::geoloc

#if defined(__HIPCC__)
#include "apt_kernels.hpp"
#include "apt_kernels_map.hpp"
#include "apt_kernels_track.hpp"

namespace apt::gpu {

// Device-side record: the head of aptgpu_geoloc_result, and the counters, which the pixel kernel's waves gather in
// kGeolocParts partial records, 64 bytes apart (a wave uses part[wave % kGeolocParts]; all waves on one record would
// queue their atomics on four addresses).  geoloc_record_to_public folds the parts on the host.
constexpr int kGeolocParts = 64;
struct GeolocPart {
    unsigned long long n_outside, n_capped;
    uint32_t min_key, max_key;
    uint32_t pad[10];
};
struct GeolocRecord {
    int32_t status, reason;
    uint32_t height, reserved;
    uint32_t pad[12];
    GeolocPart part[kGeolocParts];
};
void geoloc_record_to_public(const GeolocRecord &r, aptgpu_geoloc_result *out);

// Scratch of the stage per recording: the record, the frame, the height record the track launches read and, behind
// them, the per-row sun vectors of `rows` rows.
size_t geoloc_ws_bytes(size_t rows);
GeolocRecord *geoloc_ws_record(void *ws);
// the frame k_geoloc_rows wrote there (what a stage behind the track and row launches reads: apt_kernels_landmask.hpp)
const apt::geoloc::Frame *geoloc_ws_frame(void *ws);

// One recording's launches on s.  x (nullable unless out_rows), res, n, cap: as for the image stages (the sample count
// comes from the decode record on the device when res is set; cap bounds it and sizes the launches; cap / 2080 rows
// of room in every plane and in ws).  Exactly one of positions (host, n_positions pairs) and sat.
struct GeolocLaunch {
    const float *x;
    const Result *res;
    uint64_t n, cap;
    const double *positions;
    size_t n_positions;
    const apt::sat::TrackCall *sat;
    apt::geoloc::Geom geom;
    apt::geoloc::Settings st;
    double *latlon;  // nullable; 16-byte aligned
    float *cos_sun;  // nullable
    float *rows;     // nullable; == x: in place
};
// k_geoloc_head and the track's launches (apt_kernels_map.hpp: the track into dev.track, xoff[r] into dev.xoff, the
// call's checks into dev.ctl[1]; dev.prepare_track(s, cap / 2080) first)
void geoloc_track(hipStream_t s, const GeolocLaunch &l, apt::map::Device &dev, void *ws);
// k_geoloc_rows: the sun vector of every row, the frame and the record's head
void geoloc_rows(hipStream_t s, const GeolocLaunch &l, apt::map::Device &dev, void *ws);
// the copy of the rows when they are not normalised in place, then k_geoloc<OUT>
void geoloc_pixels(hipStream_t s, const GeolocLaunch &l, apt::map::Device &dev, void *ws);

}  // namespace apt::gpu
#endif
