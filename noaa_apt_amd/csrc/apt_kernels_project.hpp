// apt_kernels_project.hpp — the gfx950 side of the reprojection (apt_kernels_project.hip; apt_project.hpp, DESIGN.md
// §15): process()'s swath image resampled onto a north-up equirectangular or Mercator grid, the step the reference's
// to-do list names after the overlay (docs/development.md:112, :99).  Every output pixel goes backwards through
// latlon_to_rel_px (map.rs:71-100) and the x-offset correction of map.rs:105-111; the track, its x offsets and the
// per-call scalars of map.rs:59-69 are the map overlay's (apt::map::Device), host-fed or left on the device by
// k_sat_scalars.
#pragma once

#include <hip/hip_runtime.h>

#include "apt_kernels.hpp"
#include "apt_kernels_map.hpp"
#include "apt_project.hpp"

namespace apt::project {

// Device-side state of one reprojection target (a one-shot call or a plan slot).  Grows, never shrinks.
struct Device {
    uint8_t *flags = nullptr;       // the graticule: width column flags, then height row flags
    uint8_t *flags_host = nullptr;  // pinned staging of the same
    hipEvent_t flags_ev = nullptr;  // behind the latest upload from flags_host
    size_t flags_cap = 0;
    apt::gpu::ImageResult *grid_info = nullptr;  // the record the PNG encoder reads: the grid's height, the call's status
    char *png_ws = nullptr;         // the encoder's scratch for a grid-sized image
    uint64_t png_stream_cap = 0;
    Device() = default;
    Device(const Device &) = delete;
    Device &operator=(const Device &) = delete;
    ~Device();
    // uploads the graticule of one call (empty: none) behind s; waits on the host only while the previous upload from
    // the staging buffer is still queued
    void upload_flags(hipStream_t s, const std::vector<uint8_t> &f);
};

// Reprojects src (info->height rows of 2080 px of src_channels bytes, unrotated) onto the grid into out (RGBA, out_cap
// bytes).  map.xoff and map.ctl hold what image_map_track / image_map_overlay (or their _sat forms) left there on the
// same stream; sc is the host-fed form's scalars, null for the device-fed form (map.scalars).  Errors found by those
// launches (count, SGP4) and an out_cap below width * height * 4 (kReasonCapacity) are written to info; with a status
// in info, set here or before, nothing is written to out.
void image_project(hipStream_t s, Device &dev, const apt::map::Device &map, const apt::map::Scalars *sc, const Grid &g,
                   const uint8_t *src, int src_channels, uint8_t *out, uint64_t out_cap, apt::gpu::ImageResult *info);

// The PNG file of the projected grid into d_png behind image_project: the encoder of apt_kernels_png.hpp between two
// single-thread launches that hand it the grid's height and take its length and status back into info (png_bytes;
// apt::png::kReasonCapacity).
void image_project_png(hipStream_t s, Device &dev, const Grid &g, const uint8_t *grid_rgba, uint8_t *d_png,
                       uint64_t png_cap, apt::gpu::ImageResult *info);

}  // namespace apt::project
