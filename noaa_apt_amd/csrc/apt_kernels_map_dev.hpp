// apt_kernels_map_dev.hpp — device functions shared by the map overlay (apt_kernels_map.hip) and the reprojection
// (apt_kernels_project.hip): the reference's latlon_to_rel_px, its row estimate and image 0.24.7's blend.  Both
// translation units evaluate one source text, so a coastline drawn by the overlay and the same coastline found through
// the reprojection agree by construction.  Include only from a .hip file, under `#pragma clang fp contract(off)`.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "apt_map.hpp"

#pragma clang fp contract(off)

namespace apt::map {

namespace {

constexpr double kPi = 3.14159265358979323846;  // std::f64::consts::PI
constexpr uint32_t kSkip = 1;  // ctl[1]: the image stage failed before the overlay; nothing to draw or report

// latlon_to_rel_px (map.rs:71-100; geo::azimuth and geo::distance inlined, geo.rs:34-62) behind its transcendentals
// of one argument: those of the start point, of lat, and of the two longitude differences lon - start_lon (dl) and
// start_lon - lon (dl2).  dist is geo::distance(latlon, start) before map.rs clamps it to PI / 3.
__device__ inline void rel_px_from(const Scalars &s, double sin_slat, double cos_slat, double sin_lat, double cos_lat,
                                   double tan_lat, double sin_dl, double cos_dl, double cos_dl2, double &x, double &y,
                                   double &dist)
{
    const double az = atan2(sin_dl, cos_slat * tan_lat - sin_slat * cos_dl);
    const double B = az - s.ref_az;
    double cc = sin_lat * sin_slat + cos_lat * cos_slat * cos_dl2;
    cc = fmin(fmax(cc, -1.), 1.);
    dist = acos(cc);
    // f64::max / min ignore NaN, as fmax / fmin do
    const double c = fmin(fmax(dist, -kPi / 3.), kPi / 3.);
    const double a = atan(cos(B) * tan(c));
    const double b = asin(sin(B) * sin(c));
    x = -b / s.x_res;
    y = a / s.y_res + s.yaw * x;
}

// latlon_to_rel_px, map.rs:71-100
__device__ inline void rel_px(const Scalars &s, double lat, double lon, double &x, double &y)
{
    const double dl = lon - s.start_lon;
    const double dl2 = s.start_lon - lon;
    double dist;
    rel_px_from(s, sin(s.start_lat), cos(s.start_lat), sin(lat), cos(lat), tan(lat), sin(dl), cos(dl), cos(dl2), x, y,
                dist);
}

// (y.max(0.) as usize).min(height - 1): the cast saturates (inf -> usize::MAX), NaN -> 0
__device__ inline uint32_t est_row(double y, uint32_t h)
{
    const double m = fmax(y, 0.);
    return m >= static_cast<double>(h - 1) ? h - 1 : static_cast<uint32_t>(m);
}

// image 0.24.7's Rgba<u8>::blend (src-over in f32, truncating casts), with its alpha 0 / 255 fast paths
__device__ inline uint32_t blend(uint32_t bg, uint32_t fg)
{
    const uint32_t fa8 = fg >> 24;
    if (fa8 == 0) return bg;
    if (fa8 == 255) return fg;
    const float m = 255.f;
    const float br = static_cast<float>(bg & 255u) / m, bgc = static_cast<float>((bg >> 8) & 255u) / m;
    const float bb = static_cast<float>((bg >> 16) & 255u) / m, ba = static_cast<float>(bg >> 24) / m;
    const float fr = static_cast<float>(fg & 255u) / m, fgc = static_cast<float>((fg >> 8) & 255u) / m;
    const float fb = static_cast<float>((fg >> 16) & 255u) / m, fa = static_cast<float>(fa8) / m;
    const float af = ba + fa - ba * fa;
    if (af == 0.f) return bg;
    const float k = 1.f - fa;
    const float orr = (fr * fa + (br * ba) * k) / af;
    const float og = (fgc * fa + (bgc * ba) * k) / af;
    const float ob = (fb * fa + (bb * ba) * k) / af;
    const uint32_t r = static_cast<uint32_t>(m * orr), g = static_cast<uint32_t>(m * og);
    const uint32_t b = static_cast<uint32_t>(m * ob), a = static_cast<uint32_t>(m * af);
    return (r & 255u) | ((g & 255u) << 8) | ((b & 255u) << 16) | ((a & 255u) << 24);
}

}  // namespace

}  // namespace apt::map
