// apt_capi_stream_track.hip — extern "C" surface of include/aptgpu.h §4e: a live stream whose rows are found by the
// flywheel tracker.  The handle and the push / finish / reset / info entry points are §4d's (apt_capi_stream.hip); this
// unit holds what the tracker adds to the device engine (DeviceTracker and its row finder: apt_capi_stream_handle.hpp)
// and its own three entry points.  Every refusal is made by design_tracked before a device is touched.
#include <algorithm>

#include "apt_capi_stream_handle.hpp"

namespace st = apt::stream;
namespace tk = apt::stream_track;

static_assert(sizeof(aptgpu_stream_track_result) == sizeof(tk::Record), "Record mirrors aptgpu_stream_track_result");
static_assert(offsetof(tk::Record, last_position) == offsetof(aptgpu_stream_track_result, last_position), "Record mirrors aptgpu_stream_track_result");
static_assert(sizeof(aptgpu_live_track_settings) == 16, "aptgpu_live_track_settings is part of the ABI");

namespace apt::capi {

void DeviceTracker::create(hipStream_t s)
{
    const size_t o_rec = 0;
    const size_t o_s = o_rec + align256(sizeof(tk::Record));
    const size_t o_best = o_s + align256(static_cast<size_t>(T.cap_s) * 4);
    const size_t o_bp = o_best + align256(static_cast<size_t>(T.cap_best) * 4);
    const size_t total = o_bp + align256(T.cap_bp);
    mem.alloc(total);
    char *base = mem.ptr;
    b.record = reinterpret_cast<tk::Record *>(base + o_rec);
    b.ring_s = reinterpret_cast<float *>(base + o_s);
    b.ring_best = reinterpret_cast<float *>(base + o_best);
    b.ring_bp = reinterpret_cast<int8_t *>(base + o_bp);
    apt::hip_check(hipMemsetAsync(base, 0, total, s), "hipMemsetAsync");
}

void DeviceTracker::reset(hipStream_t s)
{
    tk::Record z{};
    z.struct_size = sizeof(aptgpu_stream_track_result);
    tk::record_reset(z, T);
    apt::hip_check(hipMemcpyAsync(b.record, &z, sizeof z, hipMemcpyHostToDevice, s), "hipMemcpyAsync H2D");
    apt::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");  // z leaves scope
    m = 0;
    d_scores = nullptr;
}

uint32_t DeviceTracker::rows_bound(const st::Params &P, uint64_t n_after) const { return tk::rows_bound_after(T, P, m, n_after); }

float *DeviceTracker::scores_target(hipStream_t s, uint32_t rows_cap)
{
    if (d_scores) return d_scores;
    const size_t need = static_cast<size_t>(std::max<uint32_t>(rows_cap, 1u)) * 4;
    if (score_scratch.count < need) {
        apt::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        score_scratch.alloc(need);
    }
    return reinterpret_cast<float *>(score_scratch.ptr);
}

// (the tracker in the picker's place)
void track_rows(DeviceLive &e, const Target &t, uint64_t, uint64_t w1, bool first, bool finish)
{
    DeviceTracker &k = *e.tracker;
    const uint64_t m0 = k.m, m1 = tk::positions_final(k.T, w1);
    apt::gpu::stream_track_score(e.stream, e.P, k.T, e.b, k.b, m0, m1, w1);
    apt::gpu::stream_track_dp(e.stream, e.P, k.T, e.b, k.b, t.positions, t.scores, t.cap, e.n_in, m0, m1, w1, first, finish);
    apt::gpu::stream_track_rows(e.stream, e.P, e.b, t.positions, t.rows, t.cap, std::min<uint32_t>(t.cap, 32u));
    k.m = m1;
}

namespace {

// the record of a tracked stream, host or device
tk::Record track_record_of(aptgpu_stream *s)
{
    if (s->host) return *s->host->track_record();
    tk::Record rec{};
    s->dev->set_device();
    apt::hip_check(hipMemcpyAsync(&rec, s->dev->tracker->b.record, sizeof rec, hipMemcpyDeviceToHost, s->dev->stream), "hipMemcpyAsync D2H");
    apt::hip_check(hipStreamSynchronize(s->dev->stream), "hipStreamSynchronize");
    return rec;
}

}  // namespace

}  // namespace apt::capi

using namespace apt::capi;

extern "C" {

int aptgpu_stream_create_tracked(const aptgpu_context *ctx, const aptgpu_settings *settings, const aptgpu_stream_settings *stream_settings,
                                 const aptgpu_live_track_settings *track, aptgpu_stream **out, char *err, size_t err_cap)
{
    return stream_parts::create(ctx, settings, stream_settings, true, track, false, out, err, err_cap);
}

int aptgpu_stream_create_tracked_host(const aptgpu_context *ctx, const aptgpu_settings *settings,
                                      const aptgpu_stream_settings *stream_settings, const aptgpu_live_track_settings *track,
                                      aptgpu_stream **out, char *err, size_t err_cap)
{
    return stream_parts::create(ctx, settings, stream_settings, true, track, true, out, err, err_cap);
}

int aptgpu_stream_track_scores(aptgpu_stream *stream, float *scores, size_t cap, size_t *n, char *err, size_t err_cap)
{
    if (!stream || (!scores && cap) || !n) return null_argument(err, err_cap, "stream");
    return guarded(err, err_cap, [&] {
        if (!stream->tracked()) throw Error{ErrorKind::Invalid, "stream: not a tracked stream"};
        *n = stream->last_scores.size();
        const size_t k = std::min(cap, stream->last_scores.size());
        if (k) std::memcpy(scores, stream->last_scores.data(), k * sizeof(float));
        return APTGPU_OK;
    });
}

int aptgpu_stream_track_scores_device(aptgpu_stream *stream, float *d_scores, char *err, size_t err_cap)
{
    if (!stream) return null_argument(err, err_cap, "stream");
    return guarded(err, err_cap, [&] {
        if (!stream->tracked()) throw Error{ErrorKind::Invalid, "stream: not a tracked stream"};
        if (stream->host) throw Error{ErrorKind::Invalid, "stream: a host handle has no device entry points"};
        stream->dev->tracker->d_scores = d_scores;
        return APTGPU_OK;
    });
}

int aptgpu_stream_track_results(aptgpu_stream *stream, aptgpu_stream_track_result *result, char *err, size_t err_cap)
{
    if (!stream || !result) return null_argument(err, err_cap, "stream");
    return guarded(err, err_cap, [&] {
        if (!stream->tracked()) throw Error{ErrorKind::Invalid, "stream: not a tracked stream"};
        if (result->struct_size < sizeof(aptgpu_stream_track_result))
            throw Error{ErrorKind::Invalid, "aptgpu_stream_track_result: struct_size not set"};
        const tk::Record rec = track_record_of(stream);
        const uint32_t size = result->struct_size;
        std::memcpy(result, &rec, sizeof(aptgpu_stream_track_result));
        result->struct_size = size;
        return APTGPU_OK;
    });
}

}  // extern "C"
