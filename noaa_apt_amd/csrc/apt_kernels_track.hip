// apt_kernels_track.hip — gfx950 kernels of the satellite track (apt_kernels_track.hpp; map.rs:41-69).
//
//   k_sat_track    one thread per image row: the row's time from the device height (RefTime::End needs it), SGP4,
//                  sidereal time and the geodetic sub-point, all f64 (apt_sgp4.hpp, the host's source text)
//   k_sat_scalars  one thread: start point, reference azimuth and the row pitch from the track's two ends
//                  (geo.rs:34-62 as apt_map.cpp states them, with the device library's sin / cos / tan / acos / atan2)
//
// Every row is independent; no LDS.  Both are bound by launch latency like the overlay's other launches.
#include "apt_kernels_track.hpp"

#pragma clang fp contract(off)

namespace apt::sat {

namespace {

using apt::gpu::ImageResult;
using apt::map::Scalars;

constexpr int kThreads = 64;

__global__ __launch_bounds__(kThreads) void k_sat_track(TrackCall call, const ImageResult *info, uint32_t height,
                                                        uint32_t rows_cap, double *track, uint32_t *err)
{
    const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t h = info ? info->height : height;
    if (r >= h || r >= rows_cap) return;
    const int64_t t0 = start_ms(call.ref_is_end != 0, call.ref_ms, h);
    double lat = 0., lon = 0.;
    const int32_t e = position(call.rec, t0 + kLineMs * static_cast<int64_t>(r), lat, lon);
    if (e) atomicMax(err, static_cast<uint32_t>(e));
    track[2 * r] = lat;
    track[2 * r + 1] = lon;
}

__global__ void k_sat_scalars(const double *track, const ImageResult *info, uint32_t rows_cap, double yaw,
                              double hscale, double vscale, Scalars *out, uint32_t *count)
{
    const uint32_t h = info->height;
    *count = h;
    Scalars s{};
    s.yaw = yaw;
    s.x_res = 0.0005 / hscale;
    if (h != 0 && h <= rows_cap) {
        const double lat0 = track[0], lon0 = track[1], lat1 = track[2 * (h - 1)], lon1 = track[2 * (h - 1) + 1];
        s.start_lat = lat0;
        s.start_lon = lon0;
        // geo::distance, geo.rs:34-46
        const double delta_lon = lon1 - lon0;
        double c = sin(lat0) * sin(lat1) + cos(lat0) * cos(lat1) * cos(delta_lon);
        c = fmin(fmax(c, -1.), 1.);
        s.y_res = acos(c) / static_cast<double>(h) / vscale;
        // geo::azimuth, geo.rs:54-62
        s.ref_az = atan2(sin(delta_lon), cos(lat0) * tan(lat1) - sin(lat0) * cos(delta_lon));
    }
    *out = s;
}

}  // namespace

void track(hipStream_t s, const TrackCall &call, const ImageResult *info, uint32_t height, uint32_t rows_cap,
           double *d_track, uint32_t *d_err)
{
    if (rows_cap == 0) return;
    k_sat_track<<<(rows_cap + kThreads - 1) / kThreads, kThreads, 0, s>>>(call, info, height, rows_cap, d_track, d_err);
}

void scalars(hipStream_t s, const double *d_track, const ImageResult *info, uint32_t rows_cap, double yaw,
             double hscale, double vscale, Scalars *d_scalars, uint32_t *d_count)
{
    k_sat_scalars<<<1, 1, 0, s>>>(d_track, info, rows_cap, yaw, hscale, vscale, d_scalars, d_count);
}

}  // namespace apt::sat
