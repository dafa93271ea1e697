// apt_capi_stream_handle.hpp — the handle behind aptgpu_stream (apt_capi_stream.hip) and what a tracked stream
// (apt_capi_stream_track.hip; include/aptgpu.h §4e) adds to it: one handle type, one set of entry points.
#pragma once

#include <memory>
#include <vector>

#include "apt_capi_util.hpp"
#include "apt_kernels_stream.hpp"
#include "apt_kernels_stream_track.hpp"

struct aptgpu_stream {
    bool host = false;
    apt::stream::Design d;
    std::unique_ptr<apt::stream::HostStream> twin;
    // ---- the device form
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
    bool finished = false;
    // ---- a tracked stream (apt_capi_stream_track.hip; include/aptgpu.h §4e)
    bool tracked = false;
    apt::stream_track::Params tp{};
    std::unique_ptr<apt::stream_track::HostTrackStream> ttwin;
    apt::DeviceBuffer<char> tmem;  // the tracker's record and rings: fixed at creation
    apt::gpu::StreamTrackBuffers tb{};
    float *d_scores = nullptr;              // the caller's, device-resident form (nullable)
    apt::DeviceBuffer<char> score_scratch;  // ... or the stream's own, grown to the call's rows_cap
    std::vector<float> last_scores;         // host-fed form: the lock indicators of the last call's rows
    uint64_t m = 0;                         // positions final so far: a function of the sample count alone

    ~aptgpu_stream()
    {
        if (!host && stream) {
            (void)hipSetDevice(device);
            (void)hipStreamSynchronize(stream);
            if (own_stream) (void)hipStreamDestroy(stream);
        }
    }
};

namespace apt::capi::stream_track_parts {

// creation (behind the plain stream's): the tracker's record and rings
void create_device(aptgpu_stream *s);
// the tracker's record back to its first state (enqueued on the stream; the caller waits)
void reset_device(aptgpu_stream *s);
// one launch sequence behind k_stream_front: the work samples [w0, w1) are final
void enqueue_segment(aptgpu_stream *s, float *d_rows, uint64_t *d_pos, float *d_scores, uint32_t rows_cap, uint64_t w1, bool first,
                     bool finish);
uint32_t bound_of(const aptgpu_stream *s, size_t n);
// where a device-resident call's lock indicators go: the caller's buffer, or the stream's scratch grown to rows_cap
float *scores_target(aptgpu_stream *s, uint32_t rows_cap);

}  // namespace apt::capi::stream_track_parts
