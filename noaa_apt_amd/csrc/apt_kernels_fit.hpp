// apt_kernels_fit.hpp — the overlay fit: the search for the yaw, hscale, vscale and time offset under which the map's
// lines lie on the image's edges (apt_kernels_fit.hip on the GPU, apt_fit.cpp on the CPU).  The
// reference leaves these numbers to the user's eye, so this is the definition (include/aptgpu.h states it in full;
// tests/np_fit_model.py in numpy).  The per-point and per-candidate arithmetic is written once, here, for both sides.
//
//  Shift   s picks the h-row slice T[M + s ..] of the long track; its scalars are the overlay's (start, ref_az, D) and
//          its frame S, T, R is §25's frame_of.
//  Point   unit vector P; a = atan2(P.T, P.S), b = asin(P.R), valid iff P.S > 0.5: latlon_to_rel_px's (a, b).
//  Place   x0 = -b kx, y = a ky + yaw x0, x = x0 + bx[est_row(y)] kx; col = floor(x + .5) + 453, row = floor(y + .5).
//  Score   the sum of the box-summed gradient plane E_R at the places inside the image, and their number: integers.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include "apt_kernels_geoloc.hpp"  // Frame, frame_of, xoff_of, the video geometry, APT_DSP_HD

namespace apt::fit {

using apt::geoloc::kCentre;
using apt::geoloc::kHalfPx;
using apt::geoloc::kPi;
using apt::geoloc::kPx;
using apt::geoloc::kVideo0;
using apt::geoloc::kVideoN;

constexpr int kMaxRounds = 8;
constexpr int kMaxRadius = 64;                // R_0, the widest box
constexpr uint32_t kMaxPoints = 1u << 22;     // sample points of one call
constexpr uint64_t kMaxCandidates = 1u << 20; // per round
constexpr uint32_t kMinHeight = 16;
constexpr int kReasonNoCandidate = 17, kReasonFlat = 18;
constexpr int64_t kLineMs = 500;

// geo::distance and geo::azimuth (geo.rs:34-62), as apt_map.cpp and k_sat_scalars state them
APT_DSP_HD double distance(double lat1, double lon1, double lat2, double lon2)
{
    const double dl = lon2 - lon1;
    double c = sin(lat1) * sin(lat2) + cos(lat1) * cos(lat2) * cos(dl);
    c = fmin(fmax(c, -1.), 1.);
    return acos(c);
}
APT_DSP_HD double azimuth(double lat1, double lon1, double lat2, double lon2)
{
    const double dl = lon2 - lon1;
    return atan2(sin(dl), cos(lat1) * tan(lat2) - sin(lat1) * cos(dl));
}

// What a shift fixes: the frame of its slice and the angle D between the slice's two ends.
struct Shift {
    double s[3], t[3], r[3];
    double d;
};
APT_DSP_HD Shift shift_of(double lat0, double lon0, double lat1, double lon1)
{
    const double az = azimuth(lat0, lon0, lat1, lon1);
    const apt::geoloc::Frame f = apt::geoloc::frame_of(lat0, lon0, az, 0., 0., 0.);
    Shift o;
    for (int i = 0; i < 3; ++i) {
        o.s[i] = f.s[i];
        o.t[i] = f.t[i];
        o.r[i] = f.r[i];
    }
    o.d = distance(lat0, lon0, lat1, lon1);
    return o;
}

APT_DSP_HD void unit_of(double lat, double lon, double (&p)[3])
{
    const double cl = cos(lat);
    p[0] = cl * cos(lon);
    p[1] = cl * sin(lon);
    p[2] = sin(lat);
}
// a sample point (lon, lat in degrees) as the overlay turns it into radians (map.rs:150-151)
APT_DSP_HD void unit_of_deg(double lon_deg, double lat_deg, double (&p)[3])
{
    unit_of(lat_deg / 180. * kPi, lon_deg / 180. * kPi, p);
}

APT_DSP_HD double dot3(const double *u, const double *v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

// (a, b) of a unit vector in the shift's frame; false: beyond 60 degrees of arc from the start
APT_DSP_HD bool angles_of(const Shift &f, const double (&p)[3], double &a, double &b)
{
    const double ps = dot3(p, f.s), pt = dot3(p, f.t), pr = dot3(p, f.r);
    a = atan2(pt, ps);
    b = asin(fmin(fmax(pr, -1.), 1.));
    return ps > 0.5;
}

// the b of the track's row r in the shift's frame: the x offset of §25's xoff_of in angle units (x = -b kx)
APT_DSP_HD double bx_of(const Shift &f, double lat, double lon, uint32_t r)
{
    double p[3], a, b;
    unit_of(lat, lon, p);
    angles_of(f, p, a, b);
    return r == 0 ? 0. : b;
}

// value i of an axis: centre + i * step, one product and one sum
APT_DSP_HD double axis_value(double centre, int i, double step) { return centre + static_cast<double>(i) * step; }
APT_DSP_HD double kx_of(double hscale) { return hscale / 0.0005; }
APT_DSP_HD double ky_of(uint32_t h, double vscale, double d) { return static_cast<double>(h) * vscale / d; }

// (y.max(0.) as usize).min(height - 1), map.rs:110
APT_DSP_HD uint32_t est_row(double y, uint32_t h)
{
    const double m = fmax(y, 0.);
    return m >= static_cast<double>(h - 1) ? h - 1 : static_cast<uint32_t>(m);
}

// The place of a point under a candidate.  bx: the shift's h offsets.  Returns the index row * 909 + col into the edge
// plane, or -1 when the place is outside the image.
template <typename Bx>
APT_DSP_HD int64_t place_of(double a, double b, double yaw, double kx, double ky, uint32_t h, const Bx &bx)
{
    const double x0 = -b * kx;
    const double y = a * ky + yaw * x0;
    const double fr = floor(y + 0.5);
    if (!(fr >= 0. && fr < static_cast<double>(h))) return -1;
    const uint32_t e = est_row(y, h);
    const double x = x0 - (-bx[e] * kx);
    const double fc = floor(x + 0.5);
    if (!(fc >= static_cast<double>(-kCentre) && fc < static_cast<double>(kVideoN - kCentre))) return -1;
    return static_cast<int64_t>(fr) * kVideoN + (static_cast<int64_t>(fc) + kCentre);
}

// the order of two candidates: score / count as exact rationals (counts > 0); products below 2^68
APT_DSP_HD bool better(uint64_t s1, uint32_t c1, uint64_t s2, uint32_t c2)
{
    return static_cast<unsigned __int128>(s1) * c2 > static_cast<unsigned __int128>(s2) * c1;
}

// the grid of one round
struct Grid {
    int32_t n_shift, n_yaw, n_hscale, n_vscale;
    int32_t shift_step;
    double yaw_step, hscale_step, vscale_step;
    APT_DSP_HD uint32_t ns() const { return 2u * static_cast<uint32_t>(n_shift) + 1u; }
    APT_DSP_HD uint32_t ny() const { return 2u * static_cast<uint32_t>(n_yaw) + 1u; }
    APT_DSP_HD uint32_t nh() const { return 2u * static_cast<uint32_t>(n_hscale) + 1u; }
    APT_DSP_HD uint32_t nv() const { return 2u * static_cast<uint32_t>(n_vscale) + 1u; }
    APT_DSP_HD uint32_t per_shift() const { return ny() * nh() * nv(); }
    APT_DSP_HD uint32_t total() const { return ns() * per_shift(); }
};

// one candidate's sums as the trace carries them
struct Sum {
    uint64_t score;
    uint32_t count, zero;
};

}  // namespace apt::fit

// ---- the host side (apt_fit.cpp; CPU only)
namespace apt::fit {

struct Settings {
    int channel;
    uint32_t mask;  // bit k: layer k is sampled
    int32_t margin, rounds, radius;
    uint32_t min_points;
    double spacing;
    bool timing;
    Grid grid;  // round 0's
};
// Required.  Refused with Error{Invalid}: a struct_size that is too small, a flag, a channel other than 0 / 1, a layer
// mask with unknown bits, rounds outside 1..8, a negative step, count, margin or radius, shift_step or min_points below
// 1, radius << (rounds - 1) above 64, spacing_deg <= 0 or not finite, more than 2^20 candidates in a round.
Settings check_settings(const aptgpu_fit_settings *s);
// both or neither of positions and orbit; h < 16; more than 2^22 rows with the margins
void check_call(const void *positions, const void *orbit, size_t h, const Settings &st);
Grid grid_of_round(const Settings &st, int round);
int radius_of_round(const Settings &st, int round);
const char *reason_text(int reason);
void put_result(aptgpu_fit_result *out, aptgpu_fit_result r);
// the record before the first round: the head and round 0's centre
aptgpu_fit_result first_record(uint32_t h, const apt::geoloc::Geom &g, const Settings &st, uint32_t n_points);
// The sample points of the masked layers, (lon, lat) in degrees, in draw order.  More than 2^22: Error{Invalid}.
std::vector<double> sample_points(const apt::map::Layers &layers, uint32_t mask, double spacing_deg);
// The definition in plain C++.  image: h rows of 2080 bytes; track: h + 2 M pairs; scores (nullable): rounds * total
// sums.  *info is the record; a failed record throws Error{Internal} after filling it.
void run_host(const uint8_t *image, size_t h, const double *track, size_t count, const std::vector<double> &points,
              const apt::geoloc::Geom &g, const Settings &st, Sum *scores, aptgpu_fit_result *info);

}  // namespace apt::fit

#if defined(__HIPCC__)
#include "apt_kernels_track.hpp"

namespace apt::gpu {

// One fit's launches on s.  image: h rows of 2080 bytes in HBM.  Exactly one of positions (host, h + 2 M pairs) and sat
// (whose reference time is row -M's already, ref_is_end 0).  points: host, n_points (lon, lat) pairs.  The workspace
// holds the record (aptgpu_fit_result, its struct_size the library's) and every round's sums.
struct FitLaunch {
    const uint8_t *image;
    uint32_t h;
    const double *positions;
    size_t n_positions;
    const apt::sat::TrackCall *sat;
    const double *points;
    uint32_t n_points;
    apt::geoloc::Geom geom;
    apt::fit::Settings st;
};
struct FitWorkspace;
FitWorkspace *fit_ws_create(const FitLaunch &l);
void fit_ws_destroy(FitWorkspace *ws);
const aptgpu_fit_result *fit_ws_record(const FitWorkspace *ws);
const apt::fit::Sum *fit_ws_scores(const FitWorkspace *ws);
// uploads, then every round's launches; no launch waits on the host.  ms (nullable, 4 floats: edge, angles, score,
// pick) is filled after a host wait, from event pairs around the launches.
void fit_enqueue(hipStream_t s, const FitLaunch &l, FitWorkspace *ws, float *ms);

}  // namespace apt::gpu
#endif
