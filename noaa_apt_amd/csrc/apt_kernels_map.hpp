// apt_kernels_map.hpp — the gfx950 side of the map overlay (apt_kernels_map.hip): device state of one overlay
// target and the launch sequence that draws a layer set (apt_map.hpp) over process()'s RGBA image.
#pragma once

#include <hip/hip_runtime.h>

#include "apt_kernels.hpp"
#include "apt_map.hpp"

namespace apt {
void hip_check(hipError_t e, const char *what);
}

namespace apt::sat {
struct TrackCall;
}

namespace apt::map {

// Device-side state of one overlay target (a one-shot call or a plan slot): the uploaded layer set, the per-vertex
// projection and segment scan, the track, the fragments and their per-pixel runs.  Grows, never shrinks.
struct Device {
    double *verts = nullptr;    // 2 per vertex (lon°, lat°)
    int32_t *meta = nullptr;    // 2 per vertex
    double *proj = nullptr;     // 2 per vertex (x, y) relative pixels
    uint64_t *seg = nullptr;    // fragments per segment, then their exclusive scan (n_vert + 1)
    uint64_t *sums = nullptr;   // scan block sums
    double *track = nullptr;    // 2 per row (lat, lon) rad
    double *xoff = nullptr;     // per row
    uint64_t *frags = nullptr;  // kMaxFragments packed fragments, in draw order
    uint32_t *slot = nullptr;   // 2 * kMaxFragments: each copy's arrival slot at its pixel
    uint32_t *runs = nullptr;   // 2 * kMaxFragments: the copies grouped into one contiguous run per pixel
    uint32_t *cnt = nullptr;    // per pixel of rows_cap rows: copies landing there (zero between calls)
    uint32_t *base = nullptr;   // per pixel: start of its run in `runs` (valid where cnt != 0)
    uint32_t *ctl = nullptr;    // [0] fragment total, [1] error / skip, [2] run allocator; the device-fed form:
                                // [3] SGP4 error of the track, [4] row count
    Scalars *scalars = nullptr; // the device-fed form's per-call scalars (k_sat_scalars)
    static constexpr size_t kCtlWords = 8;
    static constexpr int kTrackRing = 8;
    double *track_host[kTrackRing] = {};  // pinned staging of the track (rows_cap rows each), used in turn
    hipEvent_t track_ev[kTrackRing] = {}; // behind the latest upload from track_host[k]
    int track_next = 0;
    size_t n_vert = 0, vert_cap = 0, rows_cap = 0;
    uint64_t gen = 0;           // layer-set generation held in verts/meta
    bool frag_ready = false;
    Device() = default;
    Device(const Device &) = delete;
    Device &operator=(const Device &) = delete;
    ~Device();
    // (re)allocates for rows_cap rows and uploads the layer set when its generation differs, on stream s
    void prepare(hipStream_t s, const Layers &layers, size_t rows_cap);
    // the control words and the scalars alone (both prepare forms call it)
    void prepare_control(hipStream_t s);
    // the part of prepare() the reprojection needs when no overlay is drawn: control words, track and x offsets
    void prepare_track(hipStream_t s, size_t rows_cap);
    // copies min(count, rows_cap) positions to the device through the next staging buffer of the ring; waits on the
    // host only while that buffer's upload of kTrackRing calls ago is still queued
    void upload_track(hipStream_t s, const double *positions, size_t count);
};

// The overlay on the RGBA image `img` (height rows of 2080 px, from info->height on the device), which image_color
// wrote, with the rotation folded in when `rotate` (each fragment goes through the same permutation).  d_track holds
// min(count, rows_cap) positions; count != height is an error in info (reason kReasonCount), as are the bounds
// above.  An info record whose status is already set is left alone and nothing is drawn.
void image_map_overlay(hipStream_t s, Device &dev, const Scalars &sc, const Colors &colors, uint32_t count,
                       bool rotate, uint8_t *img, apt::gpu::ImageResult *info);

// The same with the track computed on the device (apt_kernels_track.hpp): SGP4 for info->height rows into dev.track,
// the scalars of map.rs:59-69 from its two ends into device memory, then the overlay reading both from there.  No
// upload and no host wait.  A propagation error in any row is reported in info (apt::sat::kReasonSgp4) and nothing
// is drawn.
void image_map_overlay_sat(hipStream_t s, Device &dev, const apt::sat::TrackCall &call, double yaw, double hscale,
                           double vscale, const Colors &colors, bool rotate, uint8_t *img,
                           apt::gpu::ImageResult *info);

// The first launch of either form alone, for a consumer that needs the track's x offsets but no overlay (the
// reprojection, apt_kernels_project.hpp): dev.xoff for every row and the call's checks in dev.ctl[1] (kReasonCount,
// apt::sat::kReasonSgp4, or 1 when info already carries a status).  The record itself is not written.
void image_map_track(hipStream_t s, Device &dev, const Scalars &sc, uint32_t count, apt::gpu::ImageResult *info);
void image_map_track_sat(hipStream_t s, Device &dev, const apt::sat::TrackCall &call, double yaw, double hscale,
                         double vscale, apt::gpu::ImageResult *info);

}  // namespace apt::map
