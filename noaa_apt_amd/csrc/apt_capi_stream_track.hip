// apt_capi_stream_track.hip — extern "C" surface of include/aptgpu.h §4e: a live stream whose rows are found by the
// flywheel tracker.  The handle and the push / finish / reset / info entry points are §4d's (apt_capi_stream.hip); this
// unit holds what the tracker adds: its device state, its launches, its bound and its own three entry points.  Every
// refusal is made by design_tracked before a device is touched.
#include <algorithm>

#include "apt_capi_stream_handle.hpp"
#include "apt_capi_stream_parts.hpp"

namespace st = apt::stream;
namespace tk = apt::stream_track;

static_assert(sizeof(aptgpu_stream_track_result) == sizeof(tk::Record), "Record mirrors aptgpu_stream_track_result");
static_assert(offsetof(tk::Record, last_position) == offsetof(aptgpu_stream_track_result, last_position), "Record mirrors aptgpu_stream_track_result");
static_assert(sizeof(aptgpu_live_track_settings) == 16, "aptgpu_live_track_settings is part of the ABI");

namespace apt::capi::stream_track_parts {

namespace {
size_t align256(size_t v) { return (v + 255u) & ~static_cast<size_t>(255u); }
}  // namespace

void create_device(aptgpu_stream *s)
{
    const tk::Params &T = s->tp;
    const size_t o_rec = 0;
    const size_t o_s = o_rec + align256(sizeof(tk::Record));
    const size_t o_best = o_s + align256(static_cast<size_t>(T.cap_s) * 4);
    const size_t o_bp = o_best + align256(static_cast<size_t>(T.cap_best) * 4);
    const size_t total = o_bp + align256(T.cap_bp);
    s->tmem.alloc(total);
    char *base = s->tmem.ptr;
    s->tb.record = reinterpret_cast<tk::Record *>(base + o_rec);
    s->tb.ring_s = reinterpret_cast<float *>(base + o_s);
    s->tb.ring_best = reinterpret_cast<float *>(base + o_best);
    s->tb.ring_bp = reinterpret_cast<int8_t *>(base + o_bp);
    apt::hip_check(hipMemsetAsync(base, 0, total, s->stream), "hipMemsetAsync");
}

void reset_device(aptgpu_stream *s)
{
    tk::Record z{};
    z.struct_size = sizeof(aptgpu_stream_track_result);
    tk::record_reset(z, s->tp);
    apt::hip_check(hipMemcpyAsync(s->tb.record, &z, sizeof z, hipMemcpyHostToDevice, s->stream), "hipMemcpyAsync H2D");
    apt::hip_check(hipStreamSynchronize(s->stream), "hipStreamSynchronize");  // z leaves scope
}

void enqueue_segment(aptgpu_stream *s, float *d_rows, uint64_t *d_pos, float *d_scores, uint32_t rows_cap, uint64_t w1, bool first,
                     bool finish)
{
    const st::Params &P = s->d.P;
    const tk::Params &T = s->tp;
    const uint64_t m0 = s->m, m1 = tk::positions_final(T, w1);
    apt::gpu::stream_track_score(s->stream, P, T, s->b, s->tb, m0, m1, w1);
    apt::gpu::stream_track_dp(s->stream, P, T, s->b, s->tb, d_pos, d_scores, rows_cap, s->n_in, m0, m1, w1, first, finish);
    apt::gpu::stream_track_rows(s->stream, P, s->b, d_pos, d_rows, rows_cap, std::min<uint32_t>(rows_cap, 32u));
    s->m = m1;
}

uint32_t bound_of(const aptgpu_stream *s, size_t n)
{
    const st::Params &P = s->d.P;
    const uint64_t n_in = s->host ? s->ttwin->state().n_in : s->n_in;
    const uint64_t m0 = s->host ? s->ttwin->record().m : s->m;
    // (a finish makes more work samples final than a push of the same samples: the bound serves both)
    return tk::rows_bound(s->tp, m0, tk::positions_final(s->tp, st::work_count(P, n_in + n, true)));
}

float *scores_target(aptgpu_stream *s, uint32_t rows_cap)
{
    if (s->d_scores) return s->d_scores;
    const size_t need = static_cast<size_t>(std::max<uint32_t>(rows_cap, 1u)) * 4;
    if (s->score_scratch.count < need) {
        apt::hip_check(hipStreamSynchronize(s->stream), "hipStreamSynchronize");
        s->score_scratch.alloc(need);
    }
    return reinterpret_cast<float *>(s->score_scratch.ptr);
}

}  // namespace apt::capi::stream_track_parts

using namespace apt::capi;

extern "C" {

int aptgpu_stream_create_tracked(const aptgpu_context *ctx, const aptgpu_settings *settings, const aptgpu_stream_settings *stream_settings,
                                 const aptgpu_live_track_settings *track, aptgpu_stream **out, char *err, size_t err_cap)
{
    return stream_parts::create_tracked(ctx, settings, stream_settings, track, false, out, err, err_cap);
}

int aptgpu_stream_create_tracked_host(const aptgpu_context *ctx, const aptgpu_settings *settings,
                                      const aptgpu_stream_settings *stream_settings, const aptgpu_live_track_settings *track,
                                      aptgpu_stream **out, char *err, size_t err_cap)
{
    return stream_parts::create_tracked(ctx, settings, stream_settings, track, true, out, err, err_cap);
}

int aptgpu_stream_track_scores(aptgpu_stream *stream, float *scores, size_t cap, size_t *n, char *err, size_t err_cap)
{
    if (!stream || (!scores && cap) || !n) {
        put_err(err, err_cap, "stream: null argument");
        return APTGPU_ERR_INVALID;
    }
    return guarded(err, err_cap, [&] {
        if (!stream->tracked) throw Error{ErrorKind::Invalid, "stream: not a tracked stream"};
        *n = stream->last_scores.size();
        const size_t k = std::min(cap, stream->last_scores.size());
        if (k) std::memcpy(scores, stream->last_scores.data(), k * sizeof(float));
        return APTGPU_OK;
    });
}

int aptgpu_stream_track_scores_device(aptgpu_stream *stream, float *d_scores, char *err, size_t err_cap)
{
    if (!stream) {
        put_err(err, err_cap, "stream: null argument");
        return APTGPU_ERR_INVALID;
    }
    return guarded(err, err_cap, [&] {
        if (!stream->tracked) throw Error{ErrorKind::Invalid, "stream: not a tracked stream"};
        if (stream->host) throw Error{ErrorKind::Invalid, "stream: a host handle has no device entry points"};
        stream->d_scores = d_scores;
        return APTGPU_OK;
    });
}

int aptgpu_stream_track_results(aptgpu_stream *stream, aptgpu_stream_track_result *result, char *err, size_t err_cap)
{
    if (!stream || !result) {
        put_err(err, err_cap, "stream: null argument");
        return APTGPU_ERR_INVALID;
    }
    return guarded(err, err_cap, [&] {
        if (!stream->tracked) throw Error{ErrorKind::Invalid, "stream: not a tracked stream"};
        if (result->struct_size < sizeof(aptgpu_stream_track_result))
            throw Error{ErrorKind::Invalid, "aptgpu_stream_track_result: struct_size not set"};
        tk::Record rec{};
        if (stream->host) {
            rec = stream->ttwin->record();
        } else {
            apt::hip_check(hipSetDevice(stream->device), "hipSetDevice");
            apt::hip_check(hipMemcpyAsync(&rec, stream->tb.record, sizeof rec, hipMemcpyDeviceToHost, stream->stream), "hipMemcpyAsync D2H");
            apt::hip_check(hipStreamSynchronize(stream->stream), "hipStreamSynchronize");
        }
        const uint32_t size = result->struct_size;
        std::memcpy(result, &rec, sizeof(aptgpu_stream_track_result));
        result->struct_size = size;
        return APTGPU_OK;
    });
}

}  // extern "C"
