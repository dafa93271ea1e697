// apt_capi.hip — the extern "C" surface declared in include/aptgpu.h.
// No exception crosses the ABI; apt::Error maps to status code + message.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "apt_capi_util.hpp"
#include "apt_kernels_fused_variants.hpp"
#include "apt_session.hpp"

using namespace apt::capi;

extern "C" {

const char *aptgpu_version(void) { return "aptgpu 0.2.0 (gfx950)"; }
int aptgpu_abi_version(void) { return APTGPU_ABI_VERSION; }

int aptgpu_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void aptgpu_free(void *p) { std::free(p); }

void aptgpu_cache_clear(void) { apt::capi::session_cache_clear(); }

void aptgpu_cache_info(int32_t *entries, uint64_t *device_bytes)
{
    int e = 0;
    uint64_t b = 0;
    apt::capi::session_cache_info(&e, &b);
    if (entries) *entries = e;
    if (device_bytes) *device_bytes = b;
}

// ------------------------------------------------------------------ plans
int aptgpu_plan_create(const aptgpu_context *ctx, const aptgpu_settings *settings,
                       uint32_t input_rate_hz, int sync, size_t max_samples, int max_batch,
                       aptgpu_plan **plan_out, char *err, size_t err_cap)
{
    if (!settings || !plan_out) {
        put_err(err, err_cap, "null argument");
        return APTGPU_ERR_INVALID;
    }
    return guarded(err, err_cap, [&] {
        *plan_out = apt::plan_create(ctx, *settings, input_rate_hz, sync != 0, max_samples, max_batch);
        return APTGPU_OK;
    });
}

void aptgpu_plan_destroy(aptgpu_plan *plan)
{
    if (!plan) return;
    (void)hipSetDevice(plan->device);
    for (hipStream_t st : plan->streams) (void)hipStreamSynchronize(st);
    if (plan->ev_user) (void)hipEventDestroy(plan->ev_user);
    for (hipStream_t st : plan->streams) (void)hipStreamDestroy(st);
    for (hipEvent_t ev : plan->ev_front) (void)hipEventDestroy(ev);
    delete plan;
}

int aptgpu_plan_get_info(const aptgpu_plan *plan, aptgpu_plan_info *info)
{
    if (!plan || !info) return APTGPU_ERR_INVALID;
    info->l = plan->l;
    info->m = plan->m;
    info->n_resample_taps = static_cast<uint32_t>(plan->taps_resample.size());
    info->n_lowpass_taps = static_cast<uint32_t>(plan->taps_lowpass.size());
    info->n_sync_taps = plan->n_sync_taps;
    info->samples_per_work_row = plan->spr;
    info->min_distance = plan->md;
    info->max_samples = plan->max_samples;
    info->max_work_len = plan->max_work_len;
    info->max_rows = plan->max_rows;
    info->fused = plan->fused();
    info->max_batch = plan->max_batch;
    return APTGPU_OK;
}

int aptgpu_plan_decode_device(aptgpu_plan *plan, int count, const float *const *d_signals,
                              const size_t *n, float *const *d_rows, const size_t *rows_cap,
                              char *err, size_t err_cap)
{
    if (!plan || !d_signals || !n || !d_rows || !rows_cap || count < 0 ||
        count > plan->max_batch) {
        put_err(err, err_cap, "bad argument to aptgpu_plan_decode_device");
        return APTGPU_ERR_INVALID;
    }
    return guarded(err, err_cap, [&] {
        apt::hip_check(hipSetDevice(plan->device), "hipSetDevice");
        for (int i = 0; i < count; ++i)
            if (n[i] > plan->max_samples)
                throw Error{ErrorKind::Invalid, "recording longer than the plan's max_samples"};
        std::vector<aptgpu_plan::Input> ins(static_cast<size_t>(count));
        std::vector<uint64_t> caps(static_cast<size_t>(count));
        for (int i = 0; i < count; ++i) {
            ins[static_cast<size_t>(i)].ptr = d_signals[i];
            ins[static_cast<size_t>(i)].n = n[i];
            caps[static_cast<size_t>(i)] = static_cast<uint64_t>(rows_cap[i]) * 2080u;
        }
        plan->run_call(count, ins.data(), d_rows, caps.data(), false);
        return APTGPU_OK;
    });
}

int aptgpu_plan_synchronize(aptgpu_plan *plan)
{
    if (!plan) return APTGPU_ERR_INVALID;
    (void)hipSetDevice(plan->device);
    try {
        plan->sync_all();
    } catch (const Error &) {
        return APTGPU_ERR_HIP;
    }
    return APTGPU_OK;
}

int aptgpu_plan_join(aptgpu_plan *plan)
{
    if (!plan) return APTGPU_ERR_INVALID;
    if (!plan->user_stream) return aptgpu_plan_synchronize(plan);
    (void)hipSetDevice(plan->device);
    // ctx.stream waits (on the device) for everything enqueued so far on the internal streams
    for (hipStream_t st : plan->streams) {
        if (hipEventRecord(plan->ev_user, st) != hipSuccess ||
            hipStreamWaitEvent(plan->user_stream, plan->ev_user, 0) != hipSuccess)
            return APTGPU_ERR_HIP;
    }
    return APTGPU_OK;
}

int aptgpu_plan_results(aptgpu_plan *plan, int count, aptgpu_result *results)
{
    if (!plan || !results || count < 0 || static_cast<size_t>(count) > plan->last_slots.size())
        return APTGPU_ERR_INVALID;
    static_assert(sizeof(aptgpu_result) == sizeof(apt::gpu::Result), "result layout");
    (void)hipSetDevice(plan->device);
    try {
        plan->sync_all();
    } catch (const Error &) {
        return APTGPU_ERR_HIP;
    }
    for (int i = 0; i < count; ++i)
        if (hipMemcpy(results + i, plan->result_of(i), sizeof(aptgpu_result), hipMemcpyDeviceToHost) !=
            hipSuccess)
            return APTGPU_ERR_HIP;
    return APTGPU_OK;
}

int aptgpu_plan_sync_positions(aptgpu_plan *plan, int i, uint64_t *pos, size_t cap, size_t *n_sync)
{
    if (!plan || i < 0 || static_cast<size_t>(i) >= plan->last_slots.size() || !n_sync)
        return APTGPU_ERR_INVALID;
    aptgpu_result r{};
    (void)hipSetDevice(plan->device);
    try {
        plan->sync_all();
    } catch (const Error &) {
        return APTGPU_ERR_HIP;
    }
    if (hipMemcpy(&r, plan->result_of(i), sizeof r, hipMemcpyDeviceToHost) != hipSuccess)
        return APTGPU_ERR_HIP;
    *n_sync = r.n_sync;
    size_t take = r.n_sync < cap ? r.n_sync : cap;
    if (!plan->sync || !pos || take == 0) return APTGPU_OK;
    if (take > plan->slot_of(i).peaks.count) take = plan->slot_of(i).peaks.count;
    std::vector<uint32_t> tmp(take);
    if (hipMemcpy(tmp.data(), plan->slot_of(i).peaks.ptr, take * sizeof(uint32_t),
                  hipMemcpyDeviceToHost) != hipSuccess)
        return APTGPU_ERR_HIP;
    for (size_t k = 0; k < take; ++k) pos[k] = tmp[k];
    return APTGPU_OK;
}

int aptgpu_plan_enable_timing(aptgpu_plan *plan, int on)
{
    if (!plan) return APTGPU_ERR_INVALID;
    plan->timer.enable(on < 0 ? 0 : (on > 2 ? 2 : on));
    return APTGPU_OK;
}

int aptgpu_plan_collect_timing(aptgpu_plan *plan, aptgpu_kernel_time *out, size_t cap, size_t *n_out)
{
    if (!plan || !n_out) return APTGPU_ERR_INVALID;
    try {
        (void)hipSetDevice(plan->device);
        plan->sync_all();
        plan->sync_all();  // the event pairs live on both streams
        auto v = plan->timer.collect(plan->stream);
        *n_out = v.size();
        for (size_t i = 0; i < v.size() && i < cap && out; ++i) out[i] = v[i];
        return APTGPU_OK;
    } catch (const Error &) {
        return APTGPU_ERR_HIP;
    }
}

int aptgpu_plan_read_internal(aptgpu_plan *plan, int i, const char *name, void *host_out,
                              size_t bytes, size_t *size_out)
{
    if (!plan || !name || i < 0 || static_cast<size_t>(i) >= plan->last_slots.size())
        return APTGPU_ERR_INVALID;
    aptgpu_plan::Slot &sl = plan->slot_of(i);
    const void *src = nullptr;
    size_t size = 0;
    const std::string n(name);
    if (n == "inv_sinphi") {  // host-side constant: RN(1/sin(phi)) when the fast exact divide is on, else 0
        if (size_out) *size_out = sizeof(float);
        if (host_out && bytes >= sizeof(float)) std::memcpy(host_out, &plan->inv_sinphi, sizeof(float));
        return APTGPU_OK;
    }
    if (n == "fused_variant") {  // host-side: "<row of apt_kernels_fused_variants.hpp>_f32" / "..._i16", "" where none ran
        std::string v;
        if (sl.fused_variant >= 0 && sl.fused_variant < apt::gpu::kFusedVariantCount)
            v = std::string(apt::gpu::kFusedVariants[sl.fused_variant].name) + (sl.fused_variant_i16 ? "_i16" : "_f32");
        if (size_out) *size_out = v.size();
        if (host_out && bytes) std::memcpy(host_out, v.data(), bytes < v.size() ? bytes : v.size());
        return APTGPU_OK;
    }
    if (n == "filtered") { src = sl.filtered.ptr; size = sl.filtered.count * sizeof(float); }
    else if (n == "correlation") { src = sl.correlation.ptr; size = sl.correlation.count * sizeof(float); }
    else if (n == "group_max") { src = sl.gm.ptr; size = sl.gm.count * sizeof(apt::gpu::GroupMax); }
    else if (n == "terminal_words") { src = sl.words.ptr; size = sl.words.count * sizeof(uint64_t); }
    else if (n == "peaks") { src = sl.peaks.ptr; size = sl.peaks.count * sizeof(uint32_t); }
    else if (n == "picker_flags") { src = sl.flags.ptr; size = sl.flags.count * sizeof(uint32_t); }
    else if (n == "eqfloat_thresholds") {  // T_1..T_255 of half A, then of half B (apt_kernels_eqfloat.hpp)
        src = sl.eqfloat_ws.ptr ? apt::gpu::eqfloat_ws_thresholds(sl.eqfloat_ws.ptr) : nullptr;
        size = sl.eqfloat_ws.ptr ? 2 * 255 * sizeof(uint32_t) : 0;
    }
    else return APTGPU_ERR_INVALID;
    if (size_out) *size_out = size;
    (void)hipSetDevice(plan->device);
    try {
        plan->sync_all();
    } catch (const Error &) {
        return APTGPU_ERR_HIP;
    }
    const size_t take = bytes < size ? bytes : size;
    if (n == "filtered" && sl.f_stride != 0 && plan->pw != 0) {
        // F in pixel-phase planes (apt::gpu::f_index): returned in natural order all the same — of every plane the
        // floats the caller's `bytes` reach, interleaved on the host
        if (!take || !host_out || !src) return APTGPU_OK;
        try {
            const uint32_t pw = plan->pw;
            const uint64_t want = take / sizeof(float);
            const uint64_t limit = static_cast<uint64_t>(pw) * sl.f_stride;  // samples the planes hold
            const uint64_t have = want < limit ? want : limit;
            const uint64_t per = (have + pw - 1) / pw;  // <= f_stride
            std::vector<float> plane(per);
            float *out = static_cast<float *>(host_out);
            for (uint32_t p = 0; p < pw && per; ++p) {
                if (hipMemcpy(plane.data(), static_cast<const float *>(src) + static_cast<uint64_t>(p) * sl.f_stride,
                              per * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
                    return APTGPU_ERR_HIP;
                for (uint64_t k = p, j = 0; k < have; k += pw, ++j) out[k] = plane[j];
            }
            for (uint64_t k = have; k < want; ++k) out[k] = 0.f;
        } catch (const std::exception &) {
            return APTGPU_ERR_INTERNAL;
        }
        return APTGPU_OK;
    }
    if (take && host_out && src &&
        hipMemcpy(host_out, src, take, hipMemcpyDeviceToHost) != hipSuccess)
        return APTGPU_ERR_HIP;
    return APTGPU_OK;
}

// ------------------------------------------------------------------ building blocks
int aptgpu_filter_design(const aptgpu_filter *f, float **coeff_out, size_t *n_out)
{
    if (!f || !coeff_out || !n_out) return APTGPU_ERR_INVALID;
    auto flt = apt::make_filter(f->kind, f->cutout_pi_rad, f->atten, f->delta_w_pi_rad);
    if (!flt) return APTGPU_ERR_INVALID;
    try {
        apt::Signal c = flt->design();
        float *p = host_alloc<float>(c.size());
        std::memcpy(p, c.data(), c.size() * sizeof(float));
        *coeff_out = p;
        *n_out = c.size();
        return APTGPU_OK;
    } catch (...) {
        return APTGPU_ERR_INVALID;
    }
}

void aptgpu_filter_resample(aptgpu_filter *f, uint32_t input_rate_hz, uint32_t output_rate_hz)
{
    if (!f || f->kind == APTGPU_FILTER_NOFILTER) return;
    auto flt = apt::make_filter(f->kind, f->cutout_pi_rad, f->atten, f->delta_w_pi_rad);
    if (!flt) return;
    flt->resample(apt::Rate::hz(input_rate_hz), apt::Rate::hz(output_rate_hz));
    if (auto *lp = dynamic_cast<apt::Lowpass *>(flt.get())) {
        f->cutout_pi_rad = lp->cutout.get_pi_rad();
        f->delta_w_pi_rad = lp->delta_w.get_pi_rad();
    } else if (auto *dc = dynamic_cast<apt::LowpassDcRemoval *>(flt.get())) {
        f->cutout_pi_rad = dc->cutout.get_pi_rad();
        f->delta_w_pi_rad = dc->delta_w.get_pi_rad();
    }
}

int aptgpu_generate_sync_frame(uint32_t work_rate_hz, int8_t **frame_out, size_t *n_out, char *err,
                               size_t err_cap)
{
    if (!frame_out || !n_out) return APTGPU_ERR_INVALID;
    return guarded(err, err_cap, [&] {
        std::vector<int8_t> g;
        std::string msg;
        if (!apt::generate_sync_frame(apt::Rate::hz(work_rate_hz), &g, &msg))
            throw Error{ErrorKind::Internal, msg};
        int8_t *p = host_alloc<int8_t>(g.size());
        std::memcpy(p, g.data(), g.size());
        *frame_out = p;
        *n_out = g.size();
        return APTGPU_OK;
    });
}

namespace {

// resample_with_filter, dsp.rs:62-126, on host buffers.
int resample_with_filter_impl(const aptgpu_context *ctx, const float *signal, size_t n,
                              uint32_t in_hz, uint32_t out_hz, apt::Filter &filt, float **out,
                              size_t *n_out)
{
    if (out_hz == 0) throw Error{ErrorKind::Internal, "Can't resample to 0Hz"};
    if (in_hz == 0) throw Error{ErrorKind::Invalid, "input_rate is 0"};
    Scratch sc(ctx);
    auto d_x = sc.upload(signal, n);
    apt::DeviceBuffer<float> d_y;
    const uint64_t w = resample_device(sc, d_x.ptr, n, in_hz, out_hz, filt, d_y);
    *out = sc.download_malloc(d_y.ptr, w);
    *n_out = w;
    return APTGPU_OK;
}

}  // namespace

int aptgpu_resample_with_filter(const aptgpu_context *ctx, const float *signal, size_t n,
                                uint32_t input_rate_hz, uint32_t output_rate_hz,
                                aptgpu_filter filt, float **out, size_t *n_out, char *err,
                                size_t err_cap)
{
    if ((!signal && n) || !out || !n_out) return APTGPU_ERR_INVALID;
    return guarded(err, err_cap, [&] {
        auto f = apt::make_filter(filt.kind, filt.cutout_pi_rad, filt.atten, filt.delta_w_pi_rad);
        if (!f) throw Error{ErrorKind::Invalid, "unknown filter kind"};
        return resample_with_filter_impl(ctx, signal, n, input_rate_hz, output_rate_hz, *f, out,
                                         n_out);
    });
}

int aptgpu_resample(const aptgpu_context *ctx, const float *signal, size_t n,
                    uint32_t input_rate_hz, uint32_t output_rate_hz, float atten,
                    float delta_w_pi_rad, float **out, size_t *n_out, char *err, size_t err_cap)
{
    if ((!signal && n) || !out || !n_out) return APTGPU_ERR_INVALID;
    return guarded(err, err_cap, [&] {
        if (input_rate_hz == 0) throw Error{ErrorKind::Invalid, "input_rate is 0"};
        const apt::Rate in_rate = apt::Rate::hz(input_rate_hz);
        // dsp.rs:140-150
        const apt::Freq cutout =
            output_rate_hz > input_rate_hz
                ? apt::Freq::hz(static_cast<float>(input_rate_hz) / 2.f, in_rate)
                : apt::Freq::hz(static_cast<float>(output_rate_hz) / 2.f, in_rate);
        apt::Lowpass f(cutout, atten, apt::Freq::pi_rad(delta_w_pi_rad));
        return resample_with_filter_impl(ctx, signal, n, input_rate_hz, output_rate_hz, f, out, n_out);
    });
}

int aptgpu_demodulate(const aptgpu_context *ctx, const float *signal, size_t n,
                      float carrier_pi_rad, float **out, char *err, size_t err_cap)
{
    if ((!signal && n) || !out) return APTGPU_ERR_INVALID;
    return guarded(err, err_cap, [&] {
        if (n == 0) throw Error{ErrorKind::Invalid, "empty signal (the reference panics)"};
        Scratch sc(ctx);
        const float phi = 2.f * apt::Freq::pi_rad(carrier_pi_rad).get_rad();  // dsp.rs:360
        auto d_x = sc.upload(signal, n);
        apt::DeviceBuffer<float> d_y;
        d_y.alloc(n + 16);
        apt::gpu::demodulate(sc.stream, d_x.ptr, n, cosf(phi) * 2.f, sinf(phi), d_y.ptr);
        *out = sc.download_malloc(d_y.ptr, n);
        return APTGPU_OK;
    });
}

int aptgpu_filter_signal(const aptgpu_context *ctx, const float *signal, size_t n,
                         aptgpu_filter filt, float **out, char *err, size_t err_cap)
{
    if ((!signal && n) || !out) return APTGPU_ERR_INVALID;
    return guarded(err, err_cap, [&] {
        auto f = apt::make_filter(filt.kind, filt.cutout_pi_rad, filt.atten, filt.delta_w_pi_rad);
        if (!f) throw Error{ErrorKind::Invalid, "unknown filter kind"};
        const apt::Signal coeff = f->design();
        Scratch sc(ctx);
        auto d_x = sc.upload(signal, n);
        auto d_c = sc.upload(coeff.data(), coeff.size());
        apt::DeviceBuffer<float> d_y;
        d_y.alloc(n + 16);
        apt::gpu::fir_decimate(sc.stream, d_x.ptr, n, d_c.ptr, static_cast<uint32_t>(coeff.size()), 1,
                               d_y.ptr, n);
        *out = sc.download_malloc(d_y.ptr, n);
        return APTGPU_OK;
    });
}

int aptgpu_find_sync(const aptgpu_context *ctx, const float *signal, size_t n,
                     uint32_t work_rate_hz, uint64_t **pos_out, size_t *n_pos,
                     float **correlation_out, size_t *n_corr_out, char *err, size_t err_cap)
{
    if ((!signal && n) || !pos_out || !n_pos) return APTGPU_ERR_INVALID;
    return guarded(err, err_cap, [&] {
        if (work_rate_hz % apt::FINAL_RATE != 0) throw Error{ErrorKind::Internal, kNotMultiple};
        const uint32_t pw = work_rate_hz / apt::FINAL_RATE;
        const uint64_t spr64 = static_cast<uint64_t>(apt::PX_PER_ROW) * work_rate_hz / apt::FINAL_RATE;
        const uint32_t spr = static_cast<uint32_t>(spr64);
        const uint32_t md = static_cast<uint32_t>(static_cast<uint64_t>(spr) * 8 / 10);
        const uint32_t g = 38 * pw;
        if (pw == 0 || n < g)
            throw Error{ErrorKind::Invalid, "signal shorter than the sync frame (the reference panics)"};
        if (static_cast<uint64_t>(md) * 8 > 160u * 1024u)
            throw Error{ErrorKind::Unsupported, "work_rate too large for the sync search (LDS)"};
        const uint64_t n_corr = n - g;
        Scratch sc(ctx);
        auto d_f = sc.upload(signal, n);
        apt::DeviceBuffer<float> d_c;
        d_c.alloc(n_corr + 64);
        apt::DeviceBuffer<uint64_t> d_bits;
        d_bits.alloc(n_corr / 64 + md / 64 + 4);
        const uint32_t cap = static_cast<uint32_t>(n / spr + 4);
        apt::DeviceBuffer<uint32_t> d_peaks;
        d_peaks.alloc(cap);
        apt::DeviceBuffer<apt::gpu::Result> d_res;
        d_res.alloc(1);
        apt::gpu::correlate(sc.stream, d_f.ptr, n_corr, pw, d_c.ptr);
        if (ctx && ctx->mode == APTGPU_MODE_GENERIC) {
            apt::gpu::terminals(sc.stream, d_c.ptr, n_corr, md, d_bits.ptr);
            apt::gpu::orbit_walk(sc.stream, d_bits.ptr, d_c.ptr, n_corr, n, spr, md, d_peaks.ptr, cap, d_res.ptr);
        } else {
            const uint64_t ng = n_corr / apt::gpu::sync_group_size() + 2;
            const uint64_t chunks = ng / apt::gpu::sync_chunk_groups() + 2;
            apt::DeviceBuffer<apt::gpu::GroupMax> d_gm;
            d_gm.alloc(ng + 64);
            apt::DeviceBuffer<uint64_t> d_words, d_nanw;
            d_words.alloc(ng + 64);
            d_nanw.alloc(ng + 64);
            apt::DeviceBuffer<uint32_t> d_slot, d_cnt, d_flags;
            d_slot.alloc(chunks * apt::gpu::sync_slot_cap());
            d_cnt.alloc(chunks);
            d_flags.alloc(32);
            apt::hip_check(hipMemsetAsync(d_flags.ptr, 0, 32 * sizeof(uint32_t), sc.stream), "hipMemsetAsync");
            apt::DeviceBuffer<uint32_t> d_ws;
            d_ws.alloc(apt::gpu::sync_orbit_ws_words(n, spr));
            // a one-recording "call" over a one-entry slot table
            apt::gpu::SlotPtrs sp{};
            sp.f = d_f.ptr;
            sp.gm = d_gm.ptr;
            sp.corr = d_c.ptr;
            sp.words = d_words.ptr;
            sp.nanw = d_nanw.ptr;
            sp.slot_nt = d_slot.ptr;
            sp.slot_cnt = d_cnt.ptr;
            sp.flags = d_flags.ptr;
            sp.orbit_ws = d_ws.ptr;
            sp.peaks = d_peaks.ptr;
            sp.res = d_res.ptr;
            sp.peaks_cap = cap;
            apt::DeviceBuffer<apt::gpu::SlotPtrs> d_sp;
            d_sp.alloc(1);
            apt::hip_check(hipMemcpyAsync(d_sp.ptr, &sp, sizeof sp, hipMemcpyHostToDevice, sc.stream), "hipMemcpyAsync");
            apt::gpu::CallArgs call{};
            call.count = 1;
            call.rec[0].x = nullptr;
            call.rec[0].n = 0;
            call.rec[0].w = n;
            call.rec[0].rows = nullptr;
            call.rec[0].rows_cap = 0;
            call.rec[0].slot = 0;
            apt::gpu::group_max(sc.stream, d_c.ptr, n_corr, d_gm.ptr);
            const apt::gpu::LaunchSwitches sw = apt::gpu::read_launch_switches();  // (once per API call)
            apt::gpu::sync_nodes(sc.stream, call, d_sp.ptr, n, pw, spr, md, false, true, sw);
            apt::gpu::sync_orbit(sc.stream, call, d_sp.ptr, spr, md, pw, apt::gpu::read_plan_switches().force_walk == '1', sw);  // (no plan here: the same reader)
            apt::hip_check(hipGetLastError(), "kernel launch (find_sync)");
            apt::hip_check(hipStreamSynchronize(sc.stream), "hipStreamSynchronize");
        }
        apt::gpu::Result r{};
        apt::hip_check(hipMemcpyAsync(&r, d_res.ptr, sizeof r, hipMemcpyDeviceToHost, sc.stream),
                       "hipMemcpyAsync");
        apt::hip_check(hipStreamSynchronize(sc.stream), "hipStreamSynchronize");
        std::vector<uint32_t> tmp(r.n_sync);
        if (r.n_sync)
            apt::hip_check(hipMemcpy(tmp.data(), d_peaks.ptr, r.n_sync * sizeof(uint32_t),
                                     hipMemcpyDeviceToHost),
                           "hipMemcpy peaks");
        uint64_t *pos = host_alloc<uint64_t>(r.n_sync);
        for (size_t k = 0; k < r.n_sync; ++k) pos[k] = tmp[k];
        *pos_out = pos;
        *n_pos = r.n_sync;
        if (correlation_out) {
            *correlation_out = sc.download_malloc(d_c.ptr, n_corr);
            if (n_corr_out) *n_corr_out = n_corr;
        }
        return APTGPU_OK;
    });
}

}  // extern "C"
