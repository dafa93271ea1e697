// apt_kernels_track.hpp — the gfx950 side of the satellite track (apt_kernels_track.hip): SGP4 for every image row
// and the overlay's per-call scalars, computed where the image height is known.
#pragma once

#include <hip/hip_runtime.h>

#include "apt_kernels.hpp"
#include "apt_map.hpp"
#include "apt_sgp4.hpp"

namespace apt::sat {

// One call's satellite and reference time: travels to the kernels by value (no upload).
struct TrackCall {
    Satrec rec;
    int64_t ref_ms;
    int32_t ref_is_end;  // RefTime::End: the start is ref_ms - 500 ms * height, resolved on the device
    int32_t reserved;
};

// The reason an image record gets when a row's propagation fails (include/aptgpu.h: APTGPU_SAT_REASON_SGP4).
constexpr int32_t kReasonSgp4 = 10;

// (lat, lon) of rows [0, min(height, rows_cap)) into d_track, where height is info->height when info is given and
// `height` otherwise.  *d_err, which the caller hands over as 0, receives the largest SGP4 error of any row.
// One thread per row; rows_cap bounds the grid and the writes.
void track(hipStream_t s, const TrackCall &call, const apt::gpu::ImageResult *info, uint32_t height,
           uint32_t rows_cap, double *d_track, uint32_t *d_err);

// map.rs:59-69 from the device track: the Scalars record and the row count (d_count) the overlay's first two
// kernels read in their device-fed form.  One thread.
void scalars(hipStream_t s, const double *d_track, const apt::gpu::ImageResult *info, uint32_t rows_cap, double yaw,
             double hscale, double vscale, apt::map::Scalars *d_scalars, uint32_t *d_count);

}  // namespace apt::sat
