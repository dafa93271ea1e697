// apt_project.hpp — reprojection of process()'s swath image onto a north-up map grid: the host side (apt_project.cpp).
// The reference stops at the raw swath; its to-do list names this step (docs/development.md:112 "Draw image over
// mercator (or at least equirectangular) projection", :99 "Add latitude longitude grid").  The geometry is the map
// overlay's, inverted: every output pixel goes through the reference's latlon_to_rel_px (map.rs:71-100) and the
// x-offset correction of map.rs:105-111 back into the swath, so nothing is scattered.
// The gfx950 kernel: apt_kernels_project.hpp.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/aptgpu.h"

namespace apt::project {

constexpr int32_t kReasonCapacity = 11;   // APTGPU_PROJECT_REASON_CAPACITY
constexpr uint64_t kMaxPixels = 1ull << 26;

// What the kernel reads of a checked aptgpu_projection_settings (passed by value).  Pixel (i, j):
//   lon = (lon_west + j * step) / 180. * PI                       (degrees -> radians as map.rs:144)
//   equirectangular  lat = (lat_north - i * step) / 180. * PI
//   Mercator         lat = atan(sinh(y_north - i * step_rad))
struct Grid {
    int32_t kind, channel, sampling, graticule;
    uint32_t width, height;
    double lat_north, lon_west, step;  // degrees
    double y_north, step_rad;          // Mercator: asinh(tan(lat_north rad)) and step in radians (host libm)
    uint32_t grid_color;               // R | G<<8 | B<<16 | A<<24
};

// The checks of aptgpu_projection_settings (throws apt::Error, Invalid) and the per-call values.
Grid checked(const aptgpu_projection_settings *p);

// The graticule of a grid: flags[j] != 0 for the output columns and flags[width + i] != 0 for the rows nearest to a
// multiple of grid_deg (a Mercator row from its parallel's Y).  Empty when grid_deg is 0.
std::vector<uint8_t> graticule(const Grid &g, double grid_deg);

// aptgpu_projection_fit: a grid that covers the swath of `track` (count pairs lat, lon in radians).  Conservative.
void fit(const double *track, size_t count, double hscale, int kind, double step_deg, uint32_t max_width,
         aptgpu_projection_settings *out);
// aptgpu_projection_fit_many: the same for the union of several tracks' swaths, every track's longitudes unwrapped
// from the first track's first position.  One track gives fit()'s grid.
void fit_many(const double *const *tracks, const size_t *counts, size_t n_tracks, double hscale, int kind,
              double step_deg, uint32_t max_width, aptgpu_projection_settings *out);

}  // namespace apt::project
