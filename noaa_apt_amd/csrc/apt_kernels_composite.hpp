// apt_kernels_composite.hpp — the gfx950 side of the composite (apt_kernels_composite.hip): up to
// kMaxPasses reprojected passes combined onto one north-up grid in one launch.  Every pass goes through steps 1-4 of
// the reprojection with the source text k_project evaluates (apt_kernels_project_dev.hpp); what is
// new is the choice among the covering passes, which needs the off-nadir distance x that k_project drops.
#pragma once

#include <hip/hip_runtime.h>

#include "apt_kernels_project.hpp"

namespace apt::composite {

constexpr int kMaxPasses = 16;       // APTGPU_COMPOSITE_MAX_PASSES
constexpr int32_t kReasonPass = 12;  // APTGPU_COMPOSITE_REASON_PASS

// One pass as the kernel reads it: what its track launch (image_map_track / image_map_track_sat) left on the device,
// its record and its unrotated image.
struct Pass {
    apt::map::Scalars sc;          // the host-fed form's scalars ...
    const apt::map::Scalars *scp;  // ... or, non-null, the device-fed form's (apt::map::Device::scalars)
    const double *xoff;
    const uint32_t *ctl;
    apt::gpu::ImageResult *info;
    const uint8_t *src;
    int32_t channels;              // 1 gray, 4 RGBA
    uint32_t reserved;
};

// Device-side state of one composite target (a one-shot call or a plan).  Grows, never shrinks.
struct Device {
    apt::project::Device grid;     // the graticule and the PNG scratch of the shared grid
    Pass *table = nullptr;         // kMaxPasses entries
    Pass *table_host = nullptr;    // pinned staging of the same
    hipEvent_t table_ev = nullptr; // behind the latest upload from table_host
    hipEvent_t pass_ev[kMaxPasses] = {};  // behind a pass's track stage, where that ran on another stream
    apt::gpu::ImageResult *info = nullptr;  // the composite's own record
    Device() = default;
    Device(const Device &) = delete;
    Device &operator=(const Device &) = delete;
    ~Device();
    // allocates the table and the record on first use
    void prepare();
    // uploads the pass table of one call behind s; waits on the host only while the previous upload from the staging
    // buffer is still queued
    void upload_table(hipStream_t s, const Pass *passes, int count);
};

// Orders s behind everything enqueued so far on `other` (the track stage of pass `p`), through the pass's event.
void wait_for_pass(hipStream_t s, Device &dev, int p, hipStream_t other);

// Resets the composite's record (the grid's height and pixel count under status 0), then combines the `count` passes
// of the uploaded table onto the grid into out (RGBA, out_cap bytes) and, when non-null, the number of covering
// passes per pixel into coverage (width * height bytes).  A pass whose track launch found an error, or whose record
// already carries a status, fails the composite: dev.info gets kReasonPass, that pass's record its own reason (as
// image_project leaves it), and nothing is written.  So does an out_cap below width * height * 4
// (apt::project::kReasonCapacity).
void image_composite(hipStream_t s, Device &dev, int count, int blend, const apt::project::Grid &g, uint8_t *out,
                     uint64_t out_cap, uint8_t *coverage);

}  // namespace apt::composite
