// apt_capi_track.hip — extern "C" surface of include/aptgpu.h §4c: the flywheel sync stage behind the front end.
#include <algorithm>
#include <memory>
#include <vector>

#include "apt_capi_util.hpp"
#include "apt_kernels_track_sync.hpp"
#include "apt_session.hpp"

namespace {

using namespace apt::capi;
using apt::gpu::TrackCall;
using apt::gpu::TrackRec;
using apt::gpu::TrackResult;

static_assert(sizeof(TrackResult) == sizeof(aptgpu_track_result), "TrackResult must mirror aptgpu_track_result");

// The stage's scratch for a recording of up to n_cap samples, one allocation: the record, s, the back-pointers, the
// position list, the back-track's scratch and the positions' scores.  The lists hold the longest path any allowed
// jitter admits.
struct TrackWs {
    TrackResult *rec;
    float *score;
    int8_t *bp;
    uint32_t *pos, *tmp;
    float *pscore;
    uint32_t pos_cap;
};
size_t align16(size_t v) { return (v + 15u) & ~static_cast<size_t>(15u); }
size_t track_ws_layout(void *base, uint64_t n_cap, uint32_t L, TrackWs *out)
{
    const uint32_t pos_cap = apt::track::positions_bound(n_cap, L, apt::track::kMaxJitter);
    const uintptr_t p = reinterpret_cast<uintptr_t>(base);  // (null: the size alone is wanted)
    size_t off = 0;
    auto take = [&](size_t bytes) {
        void *q = reinterpret_cast<void *>(p + off);
        off += align16(bytes);
        return q;
    };
    TrackWs w{};
    w.rec = reinterpret_cast<TrackResult *>(take(64));
    w.score = reinterpret_cast<float *>(take(n_cap * sizeof(float)));
    w.bp = reinterpret_cast<int8_t *>(take(n_cap));
    w.pos = reinterpret_cast<uint32_t *>(take(pos_cap * sizeof(uint32_t)));
    w.tmp = reinterpret_cast<uint32_t *>(take(pos_cap * sizeof(uint32_t)));
    w.pscore = reinterpret_cast<float *>(take(pos_cap * sizeof(float)));
    w.pos_cap = pos_cap;
    if (out) *out = w;
    return off;
}

TrackRec make_rec(const TrackWs &w, const float *x, const apt::gpu::Result *res, uint64_t n, uint32_t f_stride, float *rows,
                  uint32_t rows_cap)
{
    TrackRec r{};
    r.x = x;
    r.res = res;
    r.n = n;
    r.f_stride = f_stride;
    r.pos_cap = w.pos_cap;
    r.score = w.score;
    r.bp = w.bp;
    r.pos = w.pos;
    r.tmp = w.tmp;
    r.pscore = w.pscore;
    r.rows = rows;
    r.rows_cap = rows_cap;
    r.rec = w.rec;
    return r;
}

// (a path whose every step is the shortest allowed has more rows than n / L: the list's bound is the rows' bound)
uint32_t rows_bound(uint64_t, uint32_t, const TrackWs &w) { return w.pos_cap; }

// the recordings of one plan call: one launch per kernel and chunk of kTrackMaxCall, behind the decode on its stream
void enqueue_plan(aptgpu_plan *plan, int count, const apt::track::Settings &st, float *const *d_rows, const size_t *rows_cap)
{
    const uint32_t pw = plan->pw, L = plan->spr;
    const uint64_t n_cap = plan->max_work_len;
    hipStream_t s = plan->stream_of(0);
    for (int from = 0; from < count; from += apt::gpu::kTrackMaxCall) {
        const int to = std::min(count, from + apt::gpu::kTrackMaxCall);
        TrackCall call{};
        call.count = static_cast<uint32_t>(to - from);
        uint32_t max_rows = 0;
        for (int i = from; i < to; ++i) {
            aptgpu_plan::Slot &sl = plan->slot_of(i);
            if (!sl.track_ws.ptr) sl.track_ws.alloc(track_ws_layout(nullptr, n_cap, L, nullptr));
            TrackWs w;
            track_ws_layout(sl.track_ws.ptr, n_cap, L, &w);
            const uint32_t cap = static_cast<uint32_t>(std::min<size_t>(rows_cap[i], rows_bound(n_cap, L, w)));
            call.rec[i - from] = make_rec(w, sl.filtered.ptr, plan->result_of(i), n_cap, sl.f_stride, d_rows[i], cap);
            max_rows = std::max(max_rows, cap);
        }
        plan->timed(s, "track_score", [&] { apt::gpu::track_score(s, call, pw, n_cap); });
        plan->timed(s, "track_dp", [&] { apt::gpu::track_dp(s, call, pw, st.w, st.lam); });
        plan->timed(s, "track_rows", [&] { apt::gpu::track_rows(s, call, pw, max_rows); });
    }
    apt::hip_check(hipGetLastError(), "kernel launch (track stage)");
}

uint64_t *positions_malloc(const std::vector<uint32_t> &p)
{
    uint64_t *out = host_alloc<uint64_t>(p.size());
    for (size_t k = 0; k < p.size(); ++k) out[k] = p[k];
    return out;
}

// the record into the caller's struct, whose struct_size stays the caller's
void put_record(aptgpu_track_result *out, const TrackResult &r)
{
    const uint32_t size = out->struct_size;
    std::memcpy(out, &r, sizeof r);
    out->struct_size = size;
}

void fail_record(const TrackResult &r)
{
    if (r.status != 0) throw Error{ErrorKind::Internal, apt::track::reason_text(r.reason)};
}

// host arrays through the kernels: scores only (want_track false), or the whole stage
void run_host_arrays(const aptgpu_context *ctx, int count, const float *const *signals, const size_t *n, uint32_t work_rate_hz,
                     const aptgpu_track_settings *settings, bool want_track, uint64_t **positions, float **scores,
                     float **rows, aptgpu_track_result *results)
{
    // every refusal first: Scratch touches the device
    const apt::track::Settings st = apt::track::check_settings(settings);
    const uint32_t pw = apt::track::pixel_width(work_rate_hz, st);
    if (count < 1) throw Error{ErrorKind::Invalid, "track: count must be >= 1"};
    std::vector<apt::track::Geometry> geo(static_cast<size_t>(count));
    for (int i = 0; i < count; ++i) {
        if (!signals[i]) throw Error{ErrorKind::Invalid, "track: a null signal"};
        geo[static_cast<size_t>(i)] = apt::track::geometry_of(n[i], pw, st);
        if (want_track) apt::track::check_result_struct(results + i);
    }
    for (int i = 0; i < count; ++i) {
        if (positions) positions[i] = nullptr;
        if (scores) scores[i] = nullptr;
        if (rows) rows[i] = nullptr;
    }
    Scratch sc(ctx);
    hipStream_t s = sc.stream;
    const uint32_t L = geo[0].L;
    std::vector<apt::DeviceBuffer<float>> d_x(static_cast<size_t>(count)), d_rows(static_cast<size_t>(count));
    std::vector<apt::DeviceBuffer<char>> d_ws(static_cast<size_t>(count));
    std::vector<TrackWs> ws(static_cast<size_t>(count));
    std::vector<uint32_t> caps(static_cast<size_t>(count), 0u);
    for (int i = 0; i < count; ++i) {
        const size_t k = static_cast<size_t>(i);
        d_x[k] = sc.upload(signals[i], n[i]);
        d_ws[k].alloc(track_ws_layout(nullptr, n[i], L, nullptr));
        track_ws_layout(d_ws[k].ptr, n[i], L, &ws[k]);
        if (want_track && rows) {
            caps[k] = rows_bound(n[i], L, ws[k]);
            d_rows[k].alloc(static_cast<size_t>(caps[k]) * 2080u + 16);
        }
    }
    for (int from = 0; from < count; from += apt::gpu::kTrackMaxCall) {
        const int to = std::min(count, from + apt::gpu::kTrackMaxCall);
        TrackCall call{};
        call.count = static_cast<uint32_t>(to - from);
        uint64_t max_n = 0;
        uint32_t max_rows = 0;
        for (int i = from; i < to; ++i) {
            const size_t k = static_cast<size_t>(i);
            call.rec[i - from] = make_rec(ws[k], d_x[k].ptr, nullptr, n[i], 0u, d_rows[k].ptr, caps[k]);
            max_n = std::max<uint64_t>(max_n, n[i]);
            max_rows = std::max(max_rows, caps[k]);
        }
        apt::gpu::track_score(s, call, pw, max_n);
        if (want_track) {
            apt::gpu::track_dp(s, call, pw, st.w, st.lam);
            apt::gpu::track_rows(s, call, pw, max_rows);
        }
        apt::hip_check(hipGetLastError(), "kernel launch (track stage)");
    }
    // (every recording's outputs are handed out together, once the last one is on the host)
    std::vector<HostPtr<uint64_t>> out_pos(static_cast<size_t>(count));
    std::vector<HostSignal> out_scores(static_cast<size_t>(count)), out_rows(static_cast<size_t>(count));
    for (int i = 0; i < count; ++i) {
        const size_t k = static_cast<size_t>(i);
        if (!want_track) {
            out_scores[k].reset(sc.download_malloc(ws[k].score, geo[k].M));
            continue;
        }
        const TrackResult r = read_record(s, ws[k].rec);
        put_record(results + i, r);
        fail_record(r);
        std::vector<uint32_t> p(r.n_positions);
        if (!p.empty())
            apt::hip_check(hipMemcpyAsync(p.data(), ws[k].pos, p.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s),
                           "hipMemcpyAsync D2H");
        out_scores[k].reset(sc.download_malloc(ws[k].pscore, r.n_positions));
        apt::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        out_pos[k].reset(positions_malloc(p));
        if (rows) out_rows[k].reset(sc.download_malloc(d_rows[k].ptr, static_cast<size_t>(r.n_rows) * 2080u));
    }
    apt::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
    for (int i = 0; i < count; ++i) {
        const size_t k = static_cast<size_t>(i);
        if (positions) positions[i] = out_pos[k].release();
        scores[i] = out_scores[k].release();
        if (rows) rows[i] = out_rows[k].release();
    }
}

}  // namespace

extern "C" {

int aptgpu_track_sync(const aptgpu_context *ctx, int count, const float *const *signals, const size_t *n,
                      uint32_t work_rate_hz, const aptgpu_track_settings *settings, uint64_t **positions, float **scores,
                      float **rows, aptgpu_track_result *results, char *err, size_t err_cap)
{
    if (!signals || !n || !positions || !scores || !results) {
        put_err(err, err_cap, "track: null argument");
        return APTGPU_ERR_INVALID;
    }
    return guarded(err, err_cap, [&] {
        run_host_arrays(ctx, count, signals, n, work_rate_hz, settings, true, positions, scores, rows, results);
        return APTGPU_OK;
    });
}

int aptgpu_sync_score(const aptgpu_context *ctx, int count, const float *const *signals, const size_t *n,
                      uint32_t work_rate_hz, float **scores, char *err, size_t err_cap)
{
    if (!signals || !n || !scores) {
        put_err(err, err_cap, "track: null argument");
        return APTGPU_ERR_INVALID;
    }
    return guarded(err, err_cap, [&] {
        run_host_arrays(ctx, count, signals, n, work_rate_hz, nullptr, false, nullptr, scores, nullptr, nullptr);
        return APTGPU_OK;
    });
}

int aptgpu_track_sync_host(const float *signal, size_t n, uint32_t work_rate_hz, const aptgpu_track_settings *settings,
                           uint64_t **positions, float **scores, float **rows, float **score_out,
                           aptgpu_track_result *info, char *err, size_t err_cap)
{
    if (!signal || !positions || !scores) {
        put_err(err, err_cap, "track: null argument");
        return APTGPU_ERR_INVALID;
    }
    *positions = nullptr;
    *scores = nullptr;
    if (rows) *rows = nullptr;
    if (score_out) *score_out = nullptr;
    return guarded(err, err_cap, [&] {
        const apt::track::Settings st = apt::track::check_settings(settings);
        const uint32_t pw = apt::track::pixel_width(work_rate_hz, st);
        const apt::track::Geometry g = apt::track::geometry_of(n, pw, st);
        apt::track::check_result_struct(info);
        std::vector<float> s(g.M), ps, rw;
        std::vector<uint32_t> p;
        apt::track::score_host(signal, g, s.data());
        apt::track::track_host(signal, n, g, st, s.data(), p, ps, rows ? &rw : nullptr, info);
        HostPtr<uint64_t> out_p(positions_malloc(p));
        HostSignal out_s(host_alloc<float>(ps.size()));
        HostSignal out_r(rows ? host_alloc<float>(rw.size()) : nullptr);
        HostSignal out_all(score_out ? host_alloc<float>(s.size()) : nullptr);
        if (!ps.empty()) std::memcpy(out_s.get(), ps.data(), ps.size() * sizeof(float));
        if (out_r && !rw.empty()) std::memcpy(out_r.get(), rw.data(), rw.size() * sizeof(float));
        if (out_all) std::memcpy(out_all.get(), s.data(), s.size() * sizeof(float));
        *positions = out_p.release();
        *scores = out_s.release();
        if (rows) *rows = out_r.release();
        if (score_out) *score_out = out_all.release();
        return APTGPU_OK;
    });
}

int aptgpu_plan_track_device(aptgpu_plan *plan, int count, const aptgpu_track_settings *settings, float *const *d_rows,
                             const size_t *rows_cap, char *err, size_t err_cap)
{
    if (!plan || count < 0 || (count && (!d_rows || !rows_cap))) {
        put_err(err, err_cap, "track: null argument");
        return APTGPU_ERR_INVALID;
    }
    return guarded(err, err_cap, [&] {
        const apt::track::Settings st = apt::track::check_settings(settings);
        if (!plan->work_is_multiple) throw Error{ErrorKind::Invalid, "track: work_rate must be a multiple of 4160 Hz"};
        (void)apt::track::pixel_width(plan->settings.work_rate, st);
        if (static_cast<size_t>(count) > plan->last_slots.size())
            throw Error{ErrorKind::Invalid, "count exceeds the recordings of the last decode call"};
        if (plan->max_work_len >= (1ull << 31)) throw Error{ErrorKind::Invalid, "track: the plan's signals are too long"};
        for (int i = 0; i < count; ++i)
            if (!d_rows[i] && rows_cap[i]) throw Error{ErrorKind::Invalid, "null device pointer"};
        apt::hip_check(hipSetDevice(plan->device), "hipSetDevice");
        enqueue_plan(plan, count, st, d_rows, rows_cap);
        return APTGPU_OK;
    });
}

int aptgpu_plan_track_results(aptgpu_plan *plan, int count, aptgpu_track_result *results)
{
    // (the record heads the slot's scratch; a struct too short for it is refused like a stage that never ran)
    return plan_results(
        plan, count, results,
        [&](int i) -> TrackResult * {
            if (results[i].struct_size < sizeof(aptgpu_track_result)) return nullptr;
            return reinterpret_cast<TrackResult *>(plan->slot_of(i).track_ws.ptr);
        },
        [&](int i, const TrackResult &r) { put_record(results + i, r); });
}

int aptgpu_plan_track_positions(aptgpu_plan *plan, int i, uint64_t *pos, float *scores, size_t cap, size_t *n_positions)
{
    if (!plan || i < 0 || static_cast<size_t>(i) >= plan->last_slots.size() || !n_positions) return APTGPU_ERR_INVALID;
    aptgpu_plan::Slot &sl = plan->slot_of(i);
    if (!sl.track_ws.ptr) return APTGPU_ERR_INVALID;
    try {
        apt::hip_check(hipSetDevice(plan->device), "hipSetDevice");
        plan->sync_all();
        TrackWs w;
        track_ws_layout(sl.track_ws.ptr, plan->max_work_len, plan->spr, &w);
        TrackResult r{};
        apt::hip_check(hipMemcpy(&r, w.rec, sizeof r, hipMemcpyDeviceToHost), "hipMemcpy");
        *n_positions = r.n_positions;
        const size_t take = std::min<size_t>(std::min<size_t>(cap, r.n_positions), w.pos_cap);
        if (take && pos) {
            std::vector<uint32_t> tmp(take);
            apt::hip_check(hipMemcpy(tmp.data(), w.pos, take * sizeof(uint32_t), hipMemcpyDeviceToHost), "hipMemcpy");
            for (size_t k = 0; k < take; ++k) pos[k] = tmp[k];
        }
        if (take && scores)
            apt::hip_check(hipMemcpy(scores, w.pscore, take * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy");
    } catch (const apt::Error &) {
        return APTGPU_ERR_HIP;
    }
    return APTGPU_OK;
}

int aptgpu_decode_tracked(const aptgpu_context *ctx, const aptgpu_settings *settings, const float *signal, size_t n,
                          uint32_t input_rate_hz, const aptgpu_track_settings *track, float **rows_out, size_t *n_out,
                          uint64_t **positions, float **scores, aptgpu_track_result *info, char *err, size_t err_cap)
{
    if (!settings || (!signal && n) || !rows_out || !n_out) {
        put_err(err, err_cap, "null argument");
        return APTGPU_ERR_INVALID;
    }
    *rows_out = nullptr;
    *n_out = 0;
    if (positions) *positions = nullptr;
    if (scores) *scores = nullptr;
    return guarded(err, err_cap, [&] {
        const apt::track::Settings st = apt::track::check_settings(track);
        (void)apt::track::pixel_width(settings->work_rate, st);
        apt::track::check_result_struct(info);
        aptgpu_context c{};
        if (ctx) c = *ctx;
        c.step = nullptr;
        std::unique_ptr<aptgpu_plan, PlanDeleter> plan(apt::plan_create(&c, *settings, input_rate_hz, false, n, 1, /*depth*/ 1));
        const uint64_t w = plan->work_len_for(n);
        if (w < 10ull * plan->spr) throw Error{ErrorKind::Internal, kTooShort};  // decode.rs:79-83
        hipStream_t s = plan->stream;
        apt::DeviceBuffer<float> d_in, d_plain, d_rows;
        d_in.alloc(n + 16);
        const uint64_t plain_cap = plan->out_len_nosync(w) + 16;
        d_plain.alloc(plain_cap);
        const size_t rows_cap = apt::track::positions_bound(plan->max_work_len, plan->spr, apt::track::kMaxJitter);
        d_rows.alloc(rows_cap * 2080u + 16);
        apt::hip_check(hipMemcpyAsync(d_in.ptr, signal, n * sizeof(float), hipMemcpyHostToDevice, s), "hipMemcpyAsync H2D");
        aptgpu_plan::Input in;
        in.ptr = d_in.ptr;
        in.n = n;
        float *plain = d_plain.ptr;
        plan->run_call(1, &in, &plain, &plain_cap, false);
        float *rp = d_rows.ptr;
        enqueue_plan(plan.get(), 1, st, &rp, &rows_cap);
        plan->sync_all();
        TrackWs ws;
        track_ws_layout(plan->slot_of(0).track_ws.ptr, plan->max_work_len, plan->spr, &ws);
        const TrackResult r = read_record(s, ws.rec);
        if (info) put_record(info, r);
        fail_record(r);
        Scratch sc(&c);
        std::vector<uint32_t> p(r.n_positions);
        if (!p.empty()) apt::hip_check(hipMemcpy(p.data(), ws.pos, p.size() * sizeof(uint32_t), hipMemcpyDeviceToHost), "hipMemcpy");
        HostSignal out_rows(sc.download_malloc(d_rows.ptr, static_cast<size_t>(r.n_rows) * 2080u));
        HostSignal out_scores(scores ? sc.download_malloc(ws.pscore, r.n_positions) : nullptr);
        HostPtr<uint64_t> out_pos(positions ? positions_malloc(p) : nullptr);
        *rows_out = out_rows.release();
        *n_out = static_cast<size_t>(r.n_rows) * 2080u;
        if (scores) *scores = out_scores.release();
        if (positions) *positions = out_pos.release();
        return APTGPU_OK;
    });
}

}  // extern "C"
