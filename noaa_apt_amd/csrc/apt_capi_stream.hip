// apt_capi_stream.hip — extern "C" surface of include/aptgpu.h §4d: live decode.  One handle type (the design,
// `finished`, one engine: apt_capi_stream_handle.hpp) serves the kernels (DeviceLive, below) and the host twins (behind
// apt::stream::HostLive); every entry point picks the engine once.  Every refusal is made by design_stream /
// design_tracked before a device is touched.
#include <algorithm>
#include <memory>
#include <vector>

#include "apt_capi_stream_handle.hpp"

namespace st = apt::stream;
namespace tk = apt::stream_track;

static_assert(sizeof(aptgpu_stream_result) == 56, "aptgpu_stream_result is part of the ABI");
static_assert(offsetof(st::State, p) == sizeof(aptgpu_stream_result), "State's head must mirror aptgpu_stream_result");
static_assert(offsetof(st::State, scan_pos) == offsetof(aptgpu_stream_result, scan_pos), "State's head must mirror aptgpu_stream_result");

namespace apt::capi {

namespace {

constexpr uint32_t kStageRows = 64;
constexpr size_t kStageRowHead = 8 + st::kPx * 4;  // bytes of the staging per row: its position and its pixels

// the picker's row finder
void pick_rows(DeviceLive &e, const Target &t, uint64_t w0, uint64_t w1, bool first, bool finish)
{
    apt::gpu::stream_corr(e.stream, e.P, e.b, w0, w1);
    apt::gpu::stream_sync(e.stream, e.P, e.b, t.positions, t.cap, e.n_in, w1, first, finish);
    apt::gpu::stream_rows(e.stream, e.P, e.b, t.positions, t.rows, t.cap, std::min<uint32_t>(t.cap, 32u));
}

}  // namespace

DeviceLive::DeviceLive(const st::Params &p, const tk::Params *t)
    : P(p), tracker(t ? std::make_unique<DeviceTracker>(*t) : nullptr), find_rows(t ? track_rows : pick_rows)
{
}

DeviceLive::~DeviceLive()
{
    if (stream) {
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(stream);
        if (own_stream) (void)hipStreamDestroy(stream);
    }
}

void DeviceLive::create(const st::Design &d, const aptgpu_context *ctx)
{
    device = ctx ? ctx->device : 0;
    set_device();
    if (ctx && ctx->stream) {
        stream = static_cast<hipStream_t>(ctx->stream);
    } else {
        apt::hip_check(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "hipStreamCreate");
        own_stream = true;
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
    const size_t o_tab = take(d.table.size() * 4);
    const size_t o_h2 = take(d.h2.size() * 4);
    mem.alloc(off);
    char *base = mem.ptr;
    b.state = reinterpret_cast<st::State *>(base + o_state);
    b.ring_in = base + o_in;
    b.ring_f = reinterpret_cast<float *>(base + o_f);
    b.ring_c = reinterpret_cast<float *>(base + o_c);
    b.table = reinterpret_cast<const float *>(base + o_tab);
    b.h2 = reinterpret_cast<const float *>(base + o_h2);
    stage_cap = kStageRows;
    // (a tracked stream: what a push of max_push samples or a finish can release, so that only longer pushes grow it)
    if (tracker) stage_cap = std::max(kStageRows, tk::rows_bound(tracker->T, 0, st::new_work_max(P, P.max_push) + tracker->T.L));
    stage.alloc(static_cast<size_t>(stage_cap) * (kStageRowHead + (tracker ? 4 : 0)));
    if (tracker) tracker->create(stream);
    apt::hip_check(hipMemsetAsync(base, 0, off, stream), "hipMemsetAsync");
    apt::hip_check(hipMemcpyAsync(base + o_tab, d.table.data(), d.table.size() * 4, hipMemcpyHostToDevice, stream), "hipMemcpyAsync H2D");
    apt::hip_check(hipMemcpyAsync(base + o_h2, d.h2.data(), d.h2.size() * 4, hipMemcpyHostToDevice, stream), "hipMemcpyAsync H2D");
    apt::hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");  // the taps' host copies may go
}

void DeviceLive::reset()
{
    st::State z{};
    z.struct_size = sizeof(aptgpu_stream_result);
    st::state_reset(z);
    if (tracker) z.n_sync = 0;  // (positions committed, not the picker's peaks)
    set_device();
    if (tracker) tracker->reset(stream);
    apt::hip_check(hipMemcpyAsync(b.state, &z, sizeof z, hipMemcpyHostToDevice, stream), "hipMemcpyAsync H2D");
    apt::hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");  // z leaves scope
    n_in = work_len = rows_seen = 0;
}

// from the sample count after the push and the rows the host knows to be out
uint32_t DeviceLive::rows_bound(size_t n) const
{
    return tracker ? tracker->rows_bound(P, n_in + n) : st::rows_bound(P, n_in + n, rows_seen);
}

Target DeviceLive::stage_target(size_t n)
{
    const size_t row_bytes = kStageRowHead + (tracker ? 4 : 0);
    const uint32_t need = rows_bound(n);
    if (need > stage_cap) {
        apt::hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
        stage.alloc(static_cast<size_t>(need) * row_bytes);
        stage_cap = need;
    }
    const size_t cap = stage_cap;
    return Target{reinterpret_cast<float *>(stage.ptr + cap * 8), reinterpret_cast<uint64_t *>(stage.ptr),
                  tracker ? reinterpret_cast<float *>(stage.ptr + cap * kStageRowHead) : nullptr, need};
}

Target DeviceLive::caller_target(float *d_rows, uint64_t *d_positions, size_t rows_cap)
{
    const uint32_t cap = clamp_cap(rows_cap);
    return Target{d_rows, d_positions, tracker ? tracker->scores_target(stream, cap) : nullptr, cap};
}

void DeviceLive::enqueue(const void *samples, size_t n, bool first, bool finish, const Target &t)
{
    const size_t es = P.s16 ? 2 : 4;
    const char *src = static_cast<const char *>(samples);
    size_t done = 0;
    do {
        const size_t seg = std::min<size_t>(n - done, P.max_push);
        if (seg) {
            const size_t q = static_cast<size_t>(n_in & (P.cap_in - 1));
            const size_t c1 = std::min<size_t>(seg, P.cap_in - q);
            char *ring = static_cast<char *>(b.ring_in);
            apt::hip_check(hipMemcpyAsync(ring + q * es, src + done * es, c1 * es, hipMemcpyDefault, stream), "hipMemcpyAsync");
            if (seg > c1)
                apt::hip_check(hipMemcpyAsync(ring, src + (done + c1) * es, (seg - c1) * es, hipMemcpyDefault, stream), "hipMemcpyAsync");
        }
        done += seg;
        const bool fin = finish && done == n;
        const uint64_t w0 = work_len;
        n_in += seg;
        const uint64_t w1 = st::work_count(P, n_in, fin);
        apt::gpu::stream_front(stream, P, b, w0, w1, n_in);
        find_rows(*this, t, w0, w1, first, fin);
        work_len = w1;
        first = false;
    } while (done < n);
    apt::hip_check(hipGetLastError(), "kernel launch (stream)");
}

st::State DeviceLive::read_record()
{
    st::State rec{};
    apt::hip_check(hipMemcpyAsync(&rec, b.state, sizeof rec, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync D2H");
    apt::hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
    rows_seen = rec.rows_total;
    return rec;
}

namespace {

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

uint32_t bound_of(const aptgpu_stream *s, size_t n) { return s->host ? s->host->rows_bound(n) : s->dev->rows_bound(n); }

void piece_of_push(aptgpu_stream *s, const void *samples, size_t n, bool first, bool finish, const Target &t)
{
    if (s->host) s->host->push(samples, n, first, finish, t.rows, t.positions, t.scores, t.cap);
    else s->dev->enqueue(samples, n, first, finish, t);
    if (finish) s->finished = true;
}

// the device-resident form: one piece into the caller's buffers
void push_device(aptgpu_stream *s, const void *d_samples, size_t n, bool finish, float *d_rows, uint64_t *d_positions, size_t rows_cap)
{
    if (s->host) throw Error{ErrorKind::Invalid, "stream: a host handle has no device entry points"};
    stream_parts::check(s, n, rows_cap, nullptr, false);
    s->dev->set_device();
    const Target t = s->dev->caller_target(d_rows, d_positions, rows_cap);
    piece_of_push(s, d_samples, n, true, finish, t);
}

}  // namespace

// The host-fed form in three parts (apt_capi_stream_parts.hpp): where the rows of the push go, its samples in one or
// more pieces, then ONE record and the rows it counts.
namespace stream_parts {

int create(const aptgpu_context *ctx, const aptgpu_settings *settings, const aptgpu_stream_settings *ss, bool tracked,
           const aptgpu_live_track_settings *track, bool host, aptgpu_stream **out, char *err, size_t err_cap)
{
    if (!out) return null_argument(err, err_cap, "stream");
    *out = nullptr;
    return guarded(err, err_cap, [&] {
        const int mode = ctx ? ctx->mode : APTGPU_MODE_STRICT;
        const bool mfma = apt::gpu::read_plan_switches().fast_mfma == '1';
        auto s = std::make_unique<aptgpu_stream>();
        tk::Design td;
        if (tracked) td = tk::design_tracked(settings, ss, track, mode, mfma);
        else td.stream = st::design_stream(settings, ss, mode, mfma);
        s->d = td.stream;
        if (host) {
            if (tracked) s->host = std::make_unique<tk::HostTrackStream>(std::move(td));
            else s->host = std::make_unique<st::HostStream>(std::move(td.stream));
        } else {
            s->dev = std::make_unique<DeviceLive>(s->d.P, tracked ? &td.T : nullptr);
            s->dev->create(s->d, ctx);
            s->dev->reset();
        }
        *out = s.release();
        return APTGPU_OK;
    });
}

void check(const aptgpu_stream *s, size_t n, size_t rows_cap, const aptgpu_stream_result *result, bool want_result)
{
    if (s->finished) throw Error{ErrorKind::Invalid, "stream: finished; only reset and destroy are accepted"};
    if (want_result && result->struct_size < sizeof(aptgpu_stream_result))
        throw Error{ErrorKind::Invalid, "aptgpu_stream_result: struct_size not set"};
    if (rows_cap < bound_of(s, n)) throw Error{ErrorKind::Invalid, "stream: rows_cap is below aptgpu_stream_rows_bound"};
}

Target begin(aptgpu_stream *s, size_t n, float *rows, uint64_t *positions, size_t rows_cap)
{
    if (!s->host) {
        s->dev->set_device();
        return s->dev->stage_target(n);
    }
    Target t{rows, positions, nullptr, clamp_cap(rows_cap)};
    if (s->host->track_record()) {
        s->last_scores.assign(std::max<uint32_t>(s->host->rows_bound(n), 1u), 0.f);
        t.scores = s->last_scores.data();
        t.cap = std::min<uint32_t>(t.cap, static_cast<uint32_t>(s->last_scores.size()));
    }
    return t;
}

Target device_target(aptgpu_stream *s, float *d_rows, uint64_t *d_positions, size_t rows_cap)
{
    return s->dev->caller_target(d_rows, d_positions, rows_cap);
}

void piece(aptgpu_stream *s, const void *samples, size_t n, bool first, bool finish, const Target &t)
{
    if (!s->host) s->dev->set_device();
    piece_of_push(s, samples, n, first, finish, t);
}

void end(aptgpu_stream *s, const Target &t, float *rows, uint64_t *positions, aptgpu_stream_result *result)
{
    if (s->host) {
        copy_result(s->host->state(), result);
        if (t.scores) s->last_scores.resize(result->n_rows);
        fail_record(*result);
        return;
    }
    const hipStream_t q = s->dev->stream;
    const st::State rec = s->dev->read_record();
    if (rec.n_rows > t.cap) throw Error{ErrorKind::Internal, st::reason_text(st::kReasonOverflow)};
    s->last_scores.resize(t.scores ? rec.n_rows : 0);
    if (rec.n_rows) {
        apt::hip_check(hipMemcpyAsync(rows, t.rows, static_cast<size_t>(rec.n_rows) * st::kPx * 4, hipMemcpyDeviceToHost, q), "hipMemcpyAsync D2H");
        apt::hip_check(hipMemcpyAsync(positions, t.positions, static_cast<size_t>(rec.n_rows) * 8, hipMemcpyDeviceToHost, q), "hipMemcpyAsync D2H");
        if (t.scores)
            apt::hip_check(hipMemcpyAsync(s->last_scores.data(), t.scores, static_cast<size_t>(rec.n_rows) * 4, hipMemcpyDeviceToHost, q),
                           "hipMemcpyAsync D2H");
        apt::hip_check(hipStreamSynchronize(q), "hipStreamSynchronize");
    }
    copy_result(rec, result);
    fail_record(*result);
}

}  // namespace stream_parts

}  // namespace apt::capi

using namespace apt::capi;

namespace {

// host-fed: rows and positions in host memory
void push_host_fed(aptgpu_stream *s, const void *samples, size_t n, bool finish, float *rows, uint64_t *positions, size_t rows_cap,
                   aptgpu_stream_result *result)
{
    stream_parts::check(s, n, rows_cap, result, true);
    const Target t = stream_parts::begin(s, n, rows, positions, rows_cap);
    piece_of_push(s, samples, n, true, finish, t);
    stream_parts::end(s, t, rows, positions, result);
}

}  // namespace

extern "C" {

int aptgpu_stream_create(const aptgpu_context *ctx, const aptgpu_settings *settings, const aptgpu_stream_settings *stream_settings,
                         aptgpu_stream **out, char *err, size_t err_cap)
{
    return stream_parts::create(ctx, settings, stream_settings, false, nullptr, false, out, err, err_cap);
}

int aptgpu_stream_create_host(const aptgpu_context *ctx, const aptgpu_settings *settings, const aptgpu_stream_settings *stream_settings,
                              aptgpu_stream **out, char *err, size_t err_cap)
{
    return stream_parts::create(ctx, settings, stream_settings, false, nullptr, true, out, err, err_cap);
}

void aptgpu_stream_destroy(aptgpu_stream *stream) { delete stream; }

int aptgpu_stream_get_info(const aptgpu_stream *stream, aptgpu_stream_info *info)
{
    if (!stream || !info || info->struct_size < sizeof(aptgpu_stream_info)) return APTGPU_ERR_INVALID;
    st::fill_info(stream->d, stream->host ? stream->host->bytes() : stream->dev->bytes(), info);
    return APTGPU_OK;
}

int aptgpu_stream_reset(aptgpu_stream *stream, char *err, size_t err_cap)
{
    if (!stream) return null_argument(err, err_cap, "stream");
    return guarded(err, err_cap, [&] {
        if (stream->host) stream->host->reset();
        else stream->dev->reset();
        stream->last_scores.clear();
        stream->finished = false;
        return APTGPU_OK;
    });
}

size_t aptgpu_stream_rows_bound(const aptgpu_stream *stream, size_t n) { return stream ? bound_of(stream, n) : 0; }

int aptgpu_stream_push(aptgpu_stream *stream, const void *samples, size_t n, float *rows, uint64_t *positions, size_t rows_cap,
                       aptgpu_stream_result *result, char *err, size_t err_cap)
{
    if (!stream || (!samples && n) || !rows || !positions || !result) return null_argument(err, err_cap, "stream");
    return guarded(err, err_cap, [&] {
        push_host_fed(stream, samples, n, false, rows, positions, rows_cap, result);
        return APTGPU_OK;
    });
}

int aptgpu_stream_finish(aptgpu_stream *stream, float *rows, uint64_t *positions, size_t rows_cap, aptgpu_stream_result *result,
                         char *err, size_t err_cap)
{
    if (!stream || !rows || !positions || !result) return null_argument(err, err_cap, "stream");
    return guarded(err, err_cap, [&] {
        push_host_fed(stream, nullptr, 0, true, rows, positions, rows_cap, result);
        return APTGPU_OK;
    });
}

int aptgpu_stream_push_device(aptgpu_stream *stream, const void *d_samples, size_t n, float *d_rows, uint64_t *d_positions,
                              size_t rows_cap, char *err, size_t err_cap)
{
    if (!stream || (!d_samples && n) || !d_rows || !d_positions) return null_argument(err, err_cap, "stream");
    return guarded(err, err_cap, [&] {
        push_device(stream, d_samples, n, false, d_rows, d_positions, rows_cap);
        return APTGPU_OK;
    });
}

int aptgpu_stream_finish_device(aptgpu_stream *stream, float *d_rows, uint64_t *d_positions, size_t rows_cap, char *err, size_t err_cap)
{
    if (!stream || !d_rows || !d_positions) return null_argument(err, err_cap, "stream");
    return guarded(err, err_cap, [&] {
        push_device(stream, nullptr, 0, true, d_rows, d_positions, rows_cap);
        return APTGPU_OK;
    });
}

int aptgpu_stream_results(aptgpu_stream *stream, aptgpu_stream_result *result, char *err, size_t err_cap)
{
    if (!stream || !result) return null_argument(err, err_cap, "stream");
    return guarded(err, err_cap, [&] {
        if (result->struct_size < sizeof(aptgpu_stream_result)) throw Error{ErrorKind::Invalid, "aptgpu_stream_result: struct_size not set"};
        if (stream->host) {
            copy_result(stream->host->state(), result);
        } else {
            stream->dev->set_device();
            copy_result(stream->dev->read_record(), result);
        }
        fail_record(*result);
        return APTGPU_OK;
    });
}

}  // extern "C"
