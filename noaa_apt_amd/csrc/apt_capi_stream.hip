// apt_capi_stream.hip — extern "C" surface of include/aptgpu.h §4d: live decode.  One handle type serves the kernels
// and the host twin (apt_stream.cpp); every refusal is made by design_stream before a device is touched.
#include <algorithm>
#include <memory>
#include <vector>

#include "apt_capi_stream_parts.hpp"
#include "apt_capi_util.hpp"
#include "apt_kernels_stream.hpp"

namespace st = apt::stream;

static_assert(sizeof(aptgpu_stream_result) == 56, "aptgpu_stream_result is part of the ABI");
static_assert(offsetof(st::State, p) == sizeof(aptgpu_stream_result), "State's head must mirror aptgpu_stream_result");
static_assert(offsetof(st::State, scan_pos) == offsetof(aptgpu_stream_result, scan_pos), "State's head must mirror aptgpu_stream_result");

struct aptgpu_stream {
    bool host = false;
    st::Design d;
    std::unique_ptr<st::HostStream> twin;
    // ---- the device form
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    apt::DeviceBuffer<char> mem;  // the record, the rings and the taps: one allocation, fixed at creation
    apt::gpu::StreamBuffers b{};
    // the host-fed form's staging: stage_cap positions, then as many rows; kStageRows at creation, grown only when one
    // push can release more (rows_bound)
    apt::DeviceBuffer<char> stage;
    uint32_t stage_cap = 0;
    // what the host knows without asking the device: both are functions of the sample count alone
    uint64_t n_in = 0, work_len = 0;
    uint64_t rows_seen = 0;  // rows_total of the last record read back (a lower bound of the device's)
    bool finished = false;

    ~aptgpu_stream()
    {
        if (!host && stream) {
            (void)hipSetDevice(device);
            (void)hipStreamSynchronize(stream);
            if (own_stream) (void)hipStreamDestroy(stream);
        }
    }
};

namespace {

using namespace apt::capi;
using apt::capi::stream_parts::Target;

constexpr uint32_t kStageRows = 64;

size_t align256(size_t v) { return (v + 255u) & ~static_cast<size_t>(255u); }

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
    s->stage.alloc(static_cast<size_t>(s->stage_cap) * (8 + st::kPx * 4));
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
    apt::hip_check(hipSetDevice(s->device), "hipSetDevice");
    apt::hip_check(hipMemcpyAsync(s->b.state, &z, sizeof z, hipMemcpyHostToDevice, s->stream), "hipMemcpyAsync H2D");
    apt::hip_check(hipStreamSynchronize(s->stream), "hipStreamSynchronize");  // z leaves scope
}

// n samples (host or device memory) into the ring and the four kernels, in segments of at most max_push; nothing waits
// (first: this call opens a push; false continues one whose samples arrive in pieces)
void enqueue(aptgpu_stream *s, const void *samples, size_t n, bool finish, float *d_rows, uint64_t *d_pos, uint32_t rows_cap,
             bool first = true)
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
    if (s->host) return Target{rows, positions, static_cast<uint32_t>(std::min<size_t>(rows_cap, 0xFFFFFFFFu))};
    apt::hip_check(hipSetDevice(s->device), "hipSetDevice");
    const uint32_t need = bound_of(s, n);
    if (need > s->stage_cap) {
        apt::hip_check(hipStreamSynchronize(s->stream), "hipStreamSynchronize");
        s->stage.alloc(static_cast<size_t>(need) * (8 + st::kPx * 4));
        s->stage_cap = need;
    }
    return Target{reinterpret_cast<float *>(s->stage.ptr + static_cast<size_t>(s->stage_cap) * 8),
                  reinterpret_cast<uint64_t *>(s->stage.ptr), need};
}

void piece_of_push(aptgpu_stream *s, const void *samples, size_t n, bool first, bool finish, const Target &t)
{
    if (!s->host) {
        enqueue(s, samples, n, finish, t.rows, t.positions, t.cap, first);
        return;
    }
    const st::Params &P = s->d.P;
    const size_t es = P.s16 ? 2 : 4;
    size_t done = 0;
    do {
        const size_t seg = std::min<size_t>(n - done, P.max_push);
        const bool head = first && done == 0;
        done += seg;
        s->twin->push_segment(static_cast<const char *>(samples) + (done - seg) * es, seg, finish && done == n, head, t.rows,
                              t.positions, t.cap);
    } while (done < n);
    if (finish) s->finished = true;
}

void end_host_fed(aptgpu_stream *s, const Target &t, float *rows, uint64_t *positions, aptgpu_stream_result *result)
{
    if (s->host) {
        copy_result(s->twin->state(), result);
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
        apt::hip_check(hipStreamSynchronize(s->stream), "hipStreamSynchronize");
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
           char *err, size_t err_cap)
{
    if (!out) {
        put_err(err, err_cap, "stream: null argument");
        return APTGPU_ERR_INVALID;
    }
    *out = nullptr;
    return guarded(err, err_cap, [&] {
        auto s = std::make_unique<aptgpu_stream>();
        s->host = host;
        s->d = design_of(ctx, settings, ss);
        if (host) s->twin = std::make_unique<st::HostStream>(s->d);
        else {
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
    st::fill_info(stream->d, stream->host ? stream->twin->bytes() : stream->mem.count + stream->stage.count, info);
    return APTGPU_OK;
}

int aptgpu_stream_reset(aptgpu_stream *stream, char *err, size_t err_cap)
{
    if (!stream) {
        put_err(err, err_cap, "stream: null argument");
        return APTGPU_ERR_INVALID;
    }
    return guarded(err, err_cap, [&] {
        if (stream->host) stream->twin->reset();
        else reset_device(stream);
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
        enqueue(stream, d_samples, n, false, d_rows, d_positions, static_cast<uint32_t>(std::min<size_t>(rows_cap, 0xFFFFFFFFu)));
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
        enqueue(stream, nullptr, 0, true, d_rows, d_positions, static_cast<uint32_t>(std::min<size_t>(rows_cap, 0xFFFFFFFFu)));
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
            copy_result(stream->twin->state(), result);
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
