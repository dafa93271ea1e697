// apt_capi_stream.hip — extern "C" surface of include/aptgpu.h §4d: live decode.  One handle type serves the kernels
// and the host twin (apt_stream.cpp); every refusal is made by design_stream before a device is touched.
#include <algorithm>
#include <memory>
#include <vector>

#include "apt_capi_stream_handle.hpp"
#include "apt_capi_stream_parts.hpp"

namespace st = apt::stream;

static_assert(sizeof(aptgpu_stream_result) == 56, "aptgpu_stream_result is part of the ABI");
static_assert(offsetof(st::State, p) == sizeof(aptgpu_stream_result), "State's head must mirror aptgpu_stream_result");
static_assert(offsetof(st::State, scan_pos) == offsetof(aptgpu_stream_result, scan_pos), "State's head must mirror aptgpu_stream_result");

namespace {

using namespace apt::capi;
using apt::capi::stream_parts::Target;

constexpr uint32_t kStageRows = 64;

namespace tparts = apt::capi::stream_track_parts;

size_t align256(size_t v) { return (v + 255u) & ~static_cast<size_t>(255u); }

// bytes of the staging per row: its position, its pixels and, on a tracked stream, its lock indicator
size_t stage_row_bytes(const aptgpu_stream *s) { return 8 + st::kPx * 4 + (s->tracked ? 4 : 0); }
float *stage_scores(const aptgpu_stream *s)
{
    return s->tracked ? reinterpret_cast<float *>(s->stage.ptr + static_cast<size_t>(s->stage_cap) * (8 + st::kPx * 4)) : nullptr;
}
const st::State &host_state(const aptgpu_stream *s) { return s->tracked ? s->ttwin->state() : s->twin->state(); }

st::Design design_of(const aptgpu_context *ctx, const aptgpu_settings *settings, const aptgpu_stream_settings *ss)
{
    return st::design_stream(settings, ss, ctx ? ctx->mode : APTGPU_MODE_STRICT, apt::gpu::read_plan_switches().fast_mfma == '1');
}

void create_device(aptgpu_stream *s, const aptgpu_context *ctx)
{
    const st::Params &P = s->d.P;
    s->device = ctx ? ctx->device : 0;
    apt::hip_check(hipSetDevice(s->device), "hipSetDevice");
    if (ctx && ctx->stream) {
        s->stream = static_cast<hipStream_t>(ctx->stream);
    } else {
        apt::hip_check(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking), "hipStreamCreate");
        s->own_stream = true;
    }
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += align256(bytes);
        return at;
    };
    const size_t o_state = take(sizeof(st::State));
    const size_t o_in = take(static_cast<size_t>(P.cap_in) * (P.s16 ? 2 : 4));
    const size_t o_f = take(static_cast<size_t>(P.cap_f) * 4);
    const size_t o_c = take(P.sync ? static_cast<size_t>(P.cap_c) * 4 : 0);
    const size_t o_tab = take(s->d.table.size() * 4);
    const size_t o_h2 = take(s->d.h2.size() * 4);
    s->mem.alloc(off);
    char *base = s->mem.ptr;
    s->b.state = reinterpret_cast<st::State *>(base + o_state);
    s->b.ring_in = base + o_in;
    s->b.ring_f = reinterpret_cast<float *>(base + o_f);
    s->b.ring_c = reinterpret_cast<float *>(base + o_c);
    s->b.table = reinterpret_cast<const float *>(base + o_tab);
    s->b.h2 = reinterpret_cast<const float *>(base + o_h2);
    s->stage_cap = kStageRows;
    // (a tracked stream: what a push of max_push samples or a finish can release, so that only longer pushes grow it)
    if (s->tracked) s->stage_cap = std::max(kStageRows, apt::stream_track::rows_bound(s->tp, 0, st::new_work_max(P, P.max_push) + s->tp.L));
    s->stage.alloc(static_cast<size_t>(s->stage_cap) * stage_row_bytes(s));
    if (s->tracked) tparts::create_device(s);
    apt::hip_check(hipMemsetAsync(base, 0, off, s->stream), "hipMemsetAsync");
    apt::hip_check(hipMemcpyAsync(base + o_tab, s->d.table.data(), s->d.table.size() * 4, hipMemcpyHostToDevice, s->stream), "hipMemcpyAsync H2D");
    apt::hip_check(hipMemcpyAsync(base + o_h2, s->d.h2.data(), s->d.h2.size() * 4, hipMemcpyHostToDevice, s->stream), "hipMemcpyAsync H2D");
    apt::hip_check(hipStreamSynchronize(s->stream), "hipStreamSynchronize");  // the taps' host copies may go
}

void reset_device(aptgpu_stream *s)
{
    st::State z{};
    z.struct_size = sizeof(aptgpu_stream_result);
    st::state_reset(z);
    if (s->tracked) z.n_sync = 0;  // (positions committed, not the picker's peaks)
    apt::hip_check(hipSetDevice(s->device), "hipSetDevice");
    if (s->tracked) tparts::reset_device(s);
    apt::hip_check(hipMemcpyAsync(s->b.state, &z, sizeof z, hipMemcpyHostToDevice, s->stream), "hipMemcpyAsync H2D");
    apt::hip_check(hipStreamSynchronize(s->stream), "hipStreamSynchronize");  // z leaves scope
}

// n samples (host or device memory) into the ring and the four kernels, in segments of at most max_push; nothing waits
// (first: this call opens a push; false continues one whose samples arrive in pieces)
void enqueue(aptgpu_stream *s, const void *samples, size_t n, bool finish, float *d_rows, uint64_t *d_pos, uint32_t rows_cap,
             bool first = true, float *d_scores = nullptr)
{
    const st::Params &P = s->d.P;
    const size_t es = P.s16 ? 2 : 4;
    const char *src = static_cast<const char *>(samples);
    size_t done = 0;
    do {
        const size_t seg = std::min<size_t>(n - done, P.max_push);
        if (seg) {
            const size_t q = static_cast<size_t>(s->n_in & (P.cap_in - 1));
            const size_t c1 = std::min<size_t>(seg, P.cap_in - q);
            char *ring = static_cast<char *>(s->b.ring_in);
            apt::hip_check(hipMemcpyAsync(ring + q * es, src + done * es, c1 * es, hipMemcpyDefault, s->stream), "hipMemcpyAsync");
            if (seg > c1)
                apt::hip_check(hipMemcpyAsync(ring, src + (done + c1) * es, (seg - c1) * es, hipMemcpyDefault, s->stream), "hipMemcpyAsync");
        }
        done += seg;
        const bool fin = finish && done == n;
        const uint64_t w0 = s->work_len;
        s->n_in += seg;
        const uint64_t w1 = st::work_count(P, s->n_in, fin);
        apt::gpu::stream_front(s->stream, P, s->b, w0, w1, s->n_in);
        if (s->tracked) {  // (the tracker in the picker's place: §4e)
            tparts::enqueue_segment(s, d_rows, d_pos, d_scores, rows_cap, w1, first, fin);
            s->work_len = w1;
            first = false;
            continue;
        }
        apt::gpu::stream_corr(s->stream, P, s->b, w0, w1);
        apt::gpu::stream_sync(s->stream, P, s->b, d_pos, rows_cap, s->n_in, w1, first, fin);
        apt::gpu::stream_rows(s->stream, P, s->b, d_pos, d_rows, rows_cap, std::min<uint32_t>(rows_cap, 32u));
        s->work_len = w1;
        first = false;
    } while (done < n);
    if (finish) s->finished = true;
    apt::hip_check(hipGetLastError(), "kernel launch (stream)");
}

void copy_result(const st::State &r, aptgpu_stream_result *out)
{
    const uint32_t size = out->struct_size;
    std::memcpy(out, &r, sizeof(aptgpu_stream_result));
    out->struct_size = size;
}

void fail_record(const aptgpu_stream_result &r)
{
    if (r.status != 0) throw Error{ErrorKind::Internal, st::reason_text(r.reason)};
}

// aptgpu_stream_rows_bound: from the sample count after the push and the rows the host knows to be out
uint32_t bound_of(const aptgpu_stream *s, size_t n)
{
    if (s->tracked) return tparts::bound_of(s, n);
    if (s->host) return st::rows_bound(s->d.P, s->twin->state().n_in + n, s->twin->state().rows_total);
    return st::rows_bound(s->d.P, s->n_in + n, s->rows_seen);
}

void check_call(const aptgpu_stream *s, size_t n, size_t rows_cap, const aptgpu_stream_result *result, bool want_result)
{
    if (s->finished) throw Error{ErrorKind::Invalid, "stream: finished; only reset and destroy are accepted"};
    if (want_result && result->struct_size < sizeof(aptgpu_stream_result))
        throw Error{ErrorKind::Invalid, "aptgpu_stream_result: struct_size not set"};
    if (rows_cap < bound_of(s, n)) throw Error{ErrorKind::Invalid, "stream: rows_cap is below aptgpu_stream_rows_bound"};
}

// The host-fed form in three parts (apt_capi_stream_parts.hpp): where the rows of the push go, its samples in one or
// more pieces, then ONE record and the rows it counts.
Target begin_host_fed(aptgpu_stream *s, size_t n, float *rows, uint64_t *positions, size_t rows_cap)
{
    if (s->host) {
        const uint32_t cap = static_cast<uint32_t>(std::min<size_t>(rows_cap, 0xFFFFFFFFu));
        if (s->tracked) s->last_scores.assign(std::max<uint32_t>(bound_of(s, n), 1u), 0.f);
        return Target{rows, positions, s->tracked ? std::min<uint32_t>(cap, static_cast<uint32_t>(s->last_scores.size())) : cap};
    }
    apt::hip_check(hipSetDevice(s->device), "hipSetDevice");
    const uint32_t need = bound_of(s, n);
    if (need > s->stage_cap) {
        apt::hip_check(hipStreamSynchronize(s->stream), "hipStreamSynchronize");
        s->stage.alloc(static_cast<size_t>(need) * stage_row_bytes(s));
        s->stage_cap = need;
    }
    return Target{reinterpret_cast<float *>(s->stage.ptr + static_cast<size_t>(s->stage_cap) * 8),
                  reinterpret_cast<uint64_t *>(s->stage.ptr), need};
}

void piece_of_push(aptgpu_stream *s, const void *samples, size_t n, bool first, bool finish, const Target &t)
{
    if (!s->host) {
        // a tracked stream's lock indicators go beside the rows: into the staging when the rows do (the host-fed form),
        // else where the device-resident form puts them
        float *scores = nullptr;
        if (s->tracked)
            scores = t.positions == reinterpret_cast<uint64_t *>(s->stage.ptr) ? stage_scores(s) : tparts::scores_target(s, t.cap);
        enqueue(s, samples, n, finish, t.rows, t.positions, t.cap, first, scores);
        return;
    }
    const st::Params &P = s->d.P;
    const size_t es = P.s16 ? 2 : 4;
    size_t done = 0;
    do {
        const size_t seg = std::min<size_t>(n - done, P.max_push);
        const bool head = first && done == 0;
        done += seg;
        const char *src = static_cast<const char *>(samples) + (done - seg) * es;
        if (s->tracked) s->ttwin->push_segment(src, seg, finish && done == n, head, t.rows, t.positions, s->last_scores.data(), t.cap);
        else s->twin->push_segment(src, seg, finish && done == n, head, t.rows, t.positions, t.cap);
    } while (done < n);
    if (finish) s->finished = true;
}

void end_host_fed(aptgpu_stream *s, const Target &t, float *rows, uint64_t *positions, aptgpu_stream_result *result)
{
    if (s->host) {
        copy_result(host_state(s), result);
        if (s->tracked) s->last_scores.resize(result->n_rows);
        fail_record(*result);
        return;
    }
    st::State rec{};
    apt::hip_check(hipMemcpyAsync(&rec, s->b.state, sizeof rec, hipMemcpyDeviceToHost, s->stream), "hipMemcpyAsync D2H");
    apt::hip_check(hipStreamSynchronize(s->stream), "hipStreamSynchronize");
    s->rows_seen = rec.rows_total;
    if (rec.n_rows > t.cap) throw Error{ErrorKind::Internal, st::reason_text(st::kReasonOverflow)};
    if (rec.n_rows) {
        apt::hip_check(hipMemcpyAsync(rows, t.rows, static_cast<size_t>(rec.n_rows) * st::kPx * 4, hipMemcpyDeviceToHost, s->stream),
                       "hipMemcpyAsync D2H");
        apt::hip_check(hipMemcpyAsync(positions, t.positions, static_cast<size_t>(rec.n_rows) * 8, hipMemcpyDeviceToHost, s->stream),
                       "hipMemcpyAsync D2H");
        if (s->tracked) {
            s->last_scores.resize(rec.n_rows);
            apt::hip_check(hipMemcpyAsync(s->last_scores.data(), stage_scores(s), static_cast<size_t>(rec.n_rows) * 4, hipMemcpyDeviceToHost,
                                          s->stream),
                           "hipMemcpyAsync D2H");
        }
        apt::hip_check(hipStreamSynchronize(s->stream), "hipStreamSynchronize");
    } else {
        s->last_scores.clear();
    }
    copy_result(rec, result);
    fail_record(*result);
}

// host-fed: rows and positions in host memory
void push_host_fed(aptgpu_stream *s, const void *samples, size_t n, bool finish, float *rows, uint64_t *positions, size_t rows_cap,
                   aptgpu_stream_result *result)
{
    const Target t = begin_host_fed(s, n, rows, positions, rows_cap);
    piece_of_push(s, samples, n, true, finish, t);
    end_host_fed(s, t, rows, positions, result);
}

int create(const aptgpu_context *ctx, const aptgpu_settings *settings, const aptgpu_stream_settings *ss, bool host, aptgpu_stream **out,
           char *err, size_t err_cap, bool tracked = false, const aptgpu_live_track_settings *track = nullptr)
{
    if (!out) {
        put_err(err, err_cap, "stream: null argument");
        return APTGPU_ERR_INVALID;
    }
    *out = nullptr;
    return guarded(err, err_cap, [&] {
        auto s = std::make_unique<aptgpu_stream>();
        s->host = host;
        s->tracked = tracked;
        if (tracked) {
            apt::stream_track::Design td = apt::stream_track::design_tracked(settings, ss, track, ctx ? ctx->mode : APTGPU_MODE_STRICT,
                                                                             apt::gpu::read_plan_switches().fast_mfma == '1');
            s->d = td.stream;
            s->tp = td.T;
            if (host) s->ttwin = std::make_unique<apt::stream_track::HostTrackStream>(std::move(td));
        } else {
            s->d = design_of(ctx, settings, ss);
            if (host) s->twin = std::make_unique<st::HostStream>(s->d);
        }
        if (!host) {
            create_device(s.get(), ctx);
            reset_device(s.get());
        }
        *out = s.release();
        return APTGPU_OK;
    });
}

}  // namespace

namespace apt::capi::stream_parts {

bool is_host(const aptgpu_stream *s) { return s->host; }
void check(const aptgpu_stream *s, size_t n, size_t rows_cap, const aptgpu_stream_result *result, bool want_result)
{
    check_call(s, n, rows_cap, result, want_result);
}
Target begin(aptgpu_stream *s, size_t n, float *rows, uint64_t *positions, size_t rows_cap)
{
    return begin_host_fed(s, n, rows, positions, rows_cap);
}
void piece(aptgpu_stream *s, const void *samples, size_t n, bool first, bool finish, const Target &t)
{
    if (!s->host) apt::hip_check(hipSetDevice(s->device), "hipSetDevice");
    piece_of_push(s, samples, n, first, finish, t);
}
void end(aptgpu_stream *s, const Target &t, float *rows, uint64_t *positions, aptgpu_stream_result *result)
{
    end_host_fed(s, t, rows, positions, result);
}
int create_tracked(const aptgpu_context *ctx, const aptgpu_settings *settings, const aptgpu_stream_settings *ss,
                   const aptgpu_live_track_settings *track, bool host, aptgpu_stream **out, char *err, size_t err_cap)
{
    return create(ctx, settings, ss, host, out, err, err_cap, true, track);
}

}  // namespace apt::capi::stream_parts

extern "C" {

int aptgpu_stream_create(const aptgpu_context *ctx, const aptgpu_settings *settings, const aptgpu_stream_settings *stream_settings,
                         aptgpu_stream **out, char *err, size_t err_cap)
{
    return create(ctx, settings, stream_settings, false, out, err, err_cap);
}

int aptgpu_stream_create_host(const aptgpu_context *ctx, const aptgpu_settings *settings, const aptgpu_stream_settings *stream_settings,
                              aptgpu_stream **out, char *err, size_t err_cap)
{
    return create(ctx, settings, stream_settings, true, out, err, err_cap);
}

void aptgpu_stream_destroy(aptgpu_stream *stream) { delete stream; }

int aptgpu_stream_get_info(const aptgpu_stream *stream, aptgpu_stream_info *info)
{
    if (!stream || !info || info->struct_size < sizeof(aptgpu_stream_info)) return APTGPU_ERR_INVALID;
    const uint64_t host_bytes = !stream->host ? 0 : stream->tracked ? stream->ttwin->bytes() : stream->twin->bytes();
    st::fill_info(stream->d, stream->host ? host_bytes : stream->mem.count + stream->stage.count + stream->tmem.count, info);
    return APTGPU_OK;
}

int aptgpu_stream_reset(aptgpu_stream *stream, char *err, size_t err_cap)
{
    if (!stream) {
        put_err(err, err_cap, "stream: null argument");
        return APTGPU_ERR_INVALID;
    }
    return guarded(err, err_cap, [&] {
        if (stream->host && stream->tracked) stream->ttwin->reset();
        else if (stream->host) stream->twin->reset();
        else reset_device(stream);
        stream->m = 0;
        stream->d_scores = nullptr;
        stream->last_scores.clear();
        stream->n_in = 0;
        stream->work_len = 0;
        stream->rows_seen = 0;
        stream->finished = false;
        return APTGPU_OK;
    });
}

size_t aptgpu_stream_rows_bound(const aptgpu_stream *stream, size_t n) { return stream ? bound_of(stream, n) : 0; }

int aptgpu_stream_push(aptgpu_stream *stream, const void *samples, size_t n, float *rows, uint64_t *positions, size_t rows_cap,
                       aptgpu_stream_result *result, char *err, size_t err_cap)
{
    if (!stream || (!samples && n) || !rows || !positions || !result) {
        put_err(err, err_cap, "stream: null argument");
        return APTGPU_ERR_INVALID;
    }
    return guarded(err, err_cap, [&] {
        check_call(stream, n, rows_cap, result, true);
        push_host_fed(stream, samples, n, false, rows, positions, rows_cap, result);
        return APTGPU_OK;
    });
}

int aptgpu_stream_finish(aptgpu_stream *stream, float *rows, uint64_t *positions, size_t rows_cap, aptgpu_stream_result *result,
                         char *err, size_t err_cap)
{
    if (!stream || !rows || !positions || !result) {
        put_err(err, err_cap, "stream: null argument");
        return APTGPU_ERR_INVALID;
    }
    return guarded(err, err_cap, [&] {
        check_call(stream, 0, rows_cap, result, true);
        push_host_fed(stream, nullptr, 0, true, rows, positions, rows_cap, result);
        return APTGPU_OK;
    });
}

int aptgpu_stream_push_device(aptgpu_stream *stream, const void *d_samples, size_t n, float *d_rows, uint64_t *d_positions,
                              size_t rows_cap, char *err, size_t err_cap)
{
    if (!stream || (!d_samples && n) || !d_rows || !d_positions) {
        put_err(err, err_cap, "stream: null argument");
        return APTGPU_ERR_INVALID;
    }
    return guarded(err, err_cap, [&] {
        if (stream->host) throw Error{ErrorKind::Invalid, "stream: a host handle has no device entry points"};
        check_call(stream, n, rows_cap, nullptr, false);
        apt::hip_check(hipSetDevice(stream->device), "hipSetDevice");
        const uint32_t cap = static_cast<uint32_t>(std::min<size_t>(rows_cap, 0xFFFFFFFFu));
        enqueue(stream, d_samples, n, false, d_rows, d_positions, cap, true, stream->tracked ? tparts::scores_target(stream, cap) : nullptr);
        return APTGPU_OK;
    });
}

int aptgpu_stream_finish_device(aptgpu_stream *stream, float *d_rows, uint64_t *d_positions, size_t rows_cap, char *err, size_t err_cap)
{
    if (!stream || !d_rows || !d_positions) {
        put_err(err, err_cap, "stream: null argument");
        return APTGPU_ERR_INVALID;
    }
    return guarded(err, err_cap, [&] {
        if (stream->host) throw Error{ErrorKind::Invalid, "stream: a host handle has no device entry points"};
        check_call(stream, 0, rows_cap, nullptr, false);
        apt::hip_check(hipSetDevice(stream->device), "hipSetDevice");
        const uint32_t cap = static_cast<uint32_t>(std::min<size_t>(rows_cap, 0xFFFFFFFFu));
        enqueue(stream, nullptr, 0, true, d_rows, d_positions, cap, true, stream->tracked ? tparts::scores_target(stream, cap) : nullptr);
        return APTGPU_OK;
    });
}

int aptgpu_stream_results(aptgpu_stream *stream, aptgpu_stream_result *result, char *err, size_t err_cap)
{
    if (!stream || !result) {
        put_err(err, err_cap, "stream: null argument");
        return APTGPU_ERR_INVALID;
    }
    return guarded(err, err_cap, [&] {
        if (result->struct_size < sizeof(aptgpu_stream_result)) throw Error{ErrorKind::Invalid, "aptgpu_stream_result: struct_size not set"};
        if (stream->host) {
            copy_result(host_state(stream), result);
        } else {
            st::State rec{};
            apt::hip_check(hipSetDevice(stream->device), "hipSetDevice");
            apt::hip_check(hipMemcpyAsync(&rec, stream->b.state, sizeof rec, hipMemcpyDeviceToHost, stream->stream), "hipMemcpyAsync D2H");
            apt::hip_check(hipStreamSynchronize(stream->stream), "hipStreamSynchronize");
            stream->rows_seen = rec.rows_total;
            copy_result(rec, result);
        }
        fail_record(*result);
        return APTGPU_OK;
    });
}

}  // extern "C"
