// apt_capi_stream_handle.hpp — the handle behind aptgpu_stream: the design, `finished` and exactly one engine.  The host
// engine is a twin behind apt::stream::HostLive (apt_stream.cpp, apt_stream_track.cpp); the device engine is DeviceLive
// (apt_capi_stream.hip), whose row finder — the picker's three kernels or the tracker's — is chosen once at creation.
// What the tracker adds on the device is DeviceTracker (apt_capi_stream_track.hip): a plain stream has none.
#pragma once

#include <memory>
#include <vector>

#include "apt_capi_stream_parts.hpp"
#include "apt_capi_util.hpp"
#include "apt_kernels_stream.hpp"
#include "apt_kernels_stream_track.hpp"

namespace apt::capi {

using stream_parts::Target;

// The tracker's device state (include/aptgpu.h §4e).
struct DeviceTracker {
    const apt::stream_track::Params T;
    apt::DeviceBuffer<char> mem;  // the tracker's record and rings: fixed at creation
    apt::gpu::StreamTrackBuffers b{};
    uint64_t m = 0;                         // positions final so far: a function of the sample count alone
    float *d_scores = nullptr;              // the caller's, device-resident form (nullable)
    apt::DeviceBuffer<char> score_scratch;  // ... or the stream's own, grown to the call's rows_cap

    explicit DeviceTracker(const apt::stream_track::Params &t) : T(t) {}
    // creation (behind the plain stream's): the record and the rings
    void create(hipStream_t s);
    // the record back to its first state (enqueued and waited for)
    void reset(hipStream_t s);
    // aptgpu_stream_rows_bound when the sample count comes to n_after
    uint32_t rows_bound(const apt::stream::Params &P, uint64_t n_after) const;
    // where a device-resident call's lock indicators go: the caller's buffer, or the scratch grown to rows_cap
    float *scores_target(hipStream_t s, uint32_t rows_cap);
};

// The device engine: the HIP stream, the record, the rings and the staging, and the counts the host keeps.
struct DeviceLive {
    // the row finder of one launch sequence, behind k_stream_front: the work samples [w0, w1) are final
    using RowFinder = void (*)(DeviceLive &e, const Target &t, uint64_t w0, uint64_t w1, bool first, bool finish);

    const apt::stream::Params P;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    apt::DeviceBuffer<char> mem;  // the record, the rings and the taps: one allocation, fixed at creation
    apt::gpu::StreamBuffers b{};
    // the host-fed form's staging: stage_cap positions, then as many rows (a tracked stream: then as many lock indicators);
    // kStageRows at creation, grown only when one push can release more (rows_bound)
    apt::DeviceBuffer<char> stage;
    uint32_t stage_cap = 0;
    // what the host knows without asking the device: both are functions of the sample count alone
    uint64_t n_in = 0, work_len = 0;
    uint64_t rows_seen = 0;  // rows_total of the last record read back (a lower bound of the device's)
    const std::unique_ptr<DeviceTracker> tracker;  // null: the picker
    const RowFinder find_rows;

    DeviceLive(const apt::stream::Params &p, const apt::stream_track::Params *t);  // (t null: the picker)
    ~DeviceLive();
    void create(const apt::stream::Design &d, const aptgpu_context *ctx);
    void reset();
    void set_device() const { apt::hip_check(hipSetDevice(device), "hipSetDevice"); }
    uint32_t rows_bound(size_t n) const;
    uint64_t bytes() const { return mem.count + stage.count + (tracker ? tracker->mem.count : 0); }
    Target stage_target(size_t n);  // the staging, grown to the bound of a push of n samples
    Target caller_target(float *d_rows, uint64_t *d_positions, size_t rows_cap);
    // n samples (host or device memory) into the ring and the launch sequences, in segments of at most max_push; nothing waits
    void enqueue(const void *samples, size_t n, bool first, bool finish, const Target &t);
    apt::stream::State read_record();  // (waits)
};

// the tracker's row finder (apt_capi_stream_track.hip)
void track_rows(DeviceLive &e, const Target &t, uint64_t w0, uint64_t w1, bool first, bool finish);

}  // namespace apt::capi

struct aptgpu_stream {
    apt::stream::Design d;
    bool finished = false;
    // exactly one engine
    std::unique_ptr<apt::stream::HostLive> host;
    std::unique_ptr<apt::capi::DeviceLive> dev;
    std::vector<float> last_scores;  // host-fed form of a tracked stream: the lock indicators of the last call's rows

    bool tracked() const { return host ? host->track_record() != nullptr : dev->tracker != nullptr; }
};
