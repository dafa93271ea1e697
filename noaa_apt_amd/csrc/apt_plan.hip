// apt_plan.hip — plan construction (host-side design, HBM workspace) and the
// kernel pipeline of decode() (reference: src/decode.rs:43-162).
#include "apt_plan.hpp"

#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace apt {

void hip_check(hipError_t e, const char *what)
{
    if (e != hipSuccess) {
        throw Error{ErrorKind::Hip, std::string(what) + ": " + hipGetErrorString(e), static_cast<int>(e)};
    }
}

// ---------------------------------------------------------------- KernelTimer
KernelTimer::~KernelTimer()
{
    for (auto &p : pairs_) {
        (void)hipEventDestroy(p.a);
        (void)hipEventDestroy(p.b);
    }
    for (auto e : pool_) (void)hipEventDestroy(e);
}

void KernelTimer::enable(int mode) { mode_ = mode; }

hipEvent_t KernelTimer::take()
{
    if (!pool_.empty()) {
        hipEvent_t e = pool_.back();
        pool_.pop_back();
        return e;
    }
    hipEvent_t e;
    hip_check(hipEventCreate(&e), "hipEventCreate");
    return e;
}

void KernelTimer::begin(hipStream_t s, const char *name, bool dominant)
{
    // mode 1 samples: every 8th dominant launch is bracketed, so the markers (which serialise
    // the stream for ~6 us each) cost ~1.5 us per recording instead of ~12
    open_ = mode_ == 2 || (mode_ == 1 && dominant && (sampled_++ % 8) == 0);
    if (!open_) return;
    Pair p{name, take(), take()};
    hip_check(hipEventRecord(p.a, s), "hipEventRecord");
    pairs_.push_back(p);
}

void KernelTimer::end(hipStream_t s)
{
    if (!open_) return;
    open_ = false;
    hip_check(hipEventRecord(pairs_.back().b, s), "hipEventRecord");
}

std::vector<aptgpu_kernel_time> KernelTimer::collect(hipStream_t s)
{
    hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
    std::vector<aptgpu_kernel_time> out;
    for (auto &p : pairs_) {
        float ms = 0.f;
        hip_check(hipEventElapsedTime(&ms, p.a, p.b), "hipEventElapsedTime");
        aptgpu_kernel_time *slot = nullptr;
        for (auto &o : out)
            if (std::strcmp(o.name, p.name) == 0) slot = &o;
        if (!slot) {
            aptgpu_kernel_time t{};
            std::snprintf(t.name, sizeof t.name, "%s", p.name);
            out.push_back(t);
            slot = &out.back();
        }
        slot->avg_ms += ms;
        slot->launches += 1;
        pool_.push_back(p.a);
        pool_.push_back(p.b);
    }
    pairs_.clear();
    for (auto &o : out)
        if (o.launches) o.avg_ms /= static_cast<double>(o.launches);
    return out;
}

// ---------------------------------------------------------------- plan_create
namespace {

// the source is a temporary of the caller, so wait for the copy before returning (on the plan's own stream: the null
// stream would serialise against other plans' work)
void upload(aptgpu_plan *plan, DeviceBuffer<float> &dst, const float *src, size_t n)
{
    dst.alloc(n);
    hip_check(hipMemcpyAsync(dst.ptr, src, n * sizeof(float), hipMemcpyHostToDevice, plan->stream), "hipMemcpy taps");
    hip_check(hipStreamSynchronize(plan->stream), "hipStreamSynchronize");
}
void upload(aptgpu_plan *plan, DeviceBuffer<float> &dst, const Signal &src) { upload(plan, dst, src.data(), src.size()); }

// Calls in flight = streams (call j runs on stream j % depth and owns that stream's slots), and the events that order
// the front ends of consecutive calls.
void create_streams(aptgpu_plan *plan, const aptgpu_context *ctx, int depth)
{
    const gpu::PlanSwitches &sw = plan->psw;
    const int max_batch = plan->max_batch;
    if (ctx && ctx->stream) {
        plan->user_stream = static_cast<hipStream_t>(ctx->stream);
        hip_check(hipEventCreateWithFlags(&plan->ev_user, hipEventDisableTiming), "hipEventCreate");
    }
    if (depth <= 0) depth = sw.streams ? sw.streams : (max_batch >= 4 ? 3 : 6);
    depth = std::max(1, std::min(depth, 16));
    plan->streams.resize(static_cast<size_t>(depth));
    for (auto &st : plan->streams) hip_check(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "hipStreamCreate");
    plan->stream = plan->streams[0];
    // (not with a user stream: such plans may be captured into a HIP graph, call by call, and an event
    // recorded before the capture cannot be waited for inside it)
    plan->front_serial = max_batch >= 4 && !plan->user_stream && depth > 1;
    if (plan->front_serial) {
        plan->ev_front.resize(static_cast<size_t>(depth));
        for (auto &ev : plan->ev_front) hip_check(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate");
    }
}

// A plan whose resampling factors have a specialised kernel but whose tap COUNT differs (a tuned
// resample_atten / resample_delta_freq) lands on a slower kernel — the count fixes which window samples each
// polyphase branch uses, a compile-time pattern.  Same results; say so once instead of leaving it to
// stats.fused (APTGPU_QUIET=1 silences it).
void note_unspecialised(const aptgpu_plan *plan)
{
    const bool specialisable = (plan->mode == APTGPU_MODE_STRICT || plan->mode == APTGPU_MODE_FAST) && plan->l > 1 &&
                               plan->work_is_multiple && !plan->export_filtered && plan->psw.fused_any != '1';
    if (!specialisable || plan->fe.kind == gpu::FrontEndKind::Split || plan->l != 13 || (plan->m != 50 && plan->m != 100) ||
        plan->pw != 3)
        return;
    static std::atomic<bool> told{false};
    if (plan->psw.quiet != '1' && !told.exchange(true))
        std::fprintf(stderr,
                     "aptgpu: %u -> %u Hz with %zu resample / %zu low-pass taps has no compile-time specialised front end "
                     "(those exist for up to 1079 / 2145 resample taps and up to 45 low-pass taps at 48 / 96 kHz); using kernel path %d "
                     "(same results, lower throughput)\n",
                     plan->input_rate, plan->settings.work_rate, plan->taps_resample.size(), plan->taps_lowpass.size(), plan->fused());
}

// The tables of the plan's front end (plan->fe), in the layouts its kernel reads.
void upload_front_end_tables(aptgpu_plan *plan)
{
    using gpu::FrontEndKind;
    const gpu::FrontEnd &fe = plan->fe;
    const uint32_t t1 = static_cast<uint32_t>(plan->taps_resample.size());
    if (plan->mode == APTGPU_MODE_FP16_TAPS && plan->l > 1) {  // (also the unfused step-export path of the fused fp16 mode)
        std::vector<uint16_t> tab(static_cast<size_t>(plan->l) * gpu::f16taps_pairs_per_phase(plan->l, t1) * 2 + 8, 0);
        plan->f16_unscale = gpu::f16taps_pack(plan->l, plan->taps_resample.data(), t1, tab.data());
        plan->d_taps_f16.alloc(tab.size());
        hip_check(hipMemcpyAsync(plan->d_taps_f16.ptr, tab.data(), tab.size() * 2, hipMemcpyHostToDevice, plan->stream),
                  "hipMemcpy f16 taps");
        hip_check(hipStreamSynchronize(plan->stream), "hipStreamSynchronize");  // `tab` dies here
    }
    if (fe.kind == FrontEndKind::Unfused) return;
    {
        // division by sin(phi) through its reciprocal: only if it is exactly rounded for every x
        const float rc = 1.0f / plan->sinphi;
        if (fe.fast) plan->inv_sinphi = rc;  // a plain multiplication by the rounded reciprocal
        else if (plan->psw.general_envelope != '1' && gpu::verify_fast_divide(plan->device, plan->sinphi, rc)) plan->inv_sinphi = rc;
    }
    if (fe.kind == FrontEndKind::Split) {
        // (the kernel that will read it: fast plans run the fast instantiation, whose chunks may differ)
        const int ch = gpu::fused_chunk_of(plan->m, fe.fast);
        const uint32_t t1_layout = fe.pad_t1 ? fe.pad_t1 : t1;
        Signal hs(static_cast<size_t>(gpu::fused_tap_table_floats(plan->l, plan->m, t1_layout, ch)) + 16, 0.f);
        if (fe.mfma || fe.f16) {
            // same buffer, different content: the bf16 fragments of the resampler's Toeplitz matrix / half2 tap pairs as raw dwords
            std::vector<uint32_t> tab((fe.mfma ? gpu::fused_mfma_table_dwords(plan->l, plan->m) : gpu::fused_f16_table_dwords(plan->l, plan->m, t1)) + 16, 0u);
            if (fe.mfma) gpu::fused_mfma_table(plan->l, plan->m, plan->taps_resample.data(), t1, tab.data());
            else plan->f16_unscale = gpu::fused_f16_branch_taps(plan->l, plan->m, plan->taps_resample.data(), t1, tab.data());
            hs.assign(tab.size(), 0.f);
            std::memcpy(hs.data(), tab.data(), tab.size() * sizeof(uint32_t));
        } else {
            gpu::fused_branch_taps(plan->l, plan->m, plan->taps_resample.data(), t1, ch, hs.data(), t1_layout);
        }
        upload(plan, plan->d_taps_branch, hs);
    } else {
        const bool phase = fe.kind == FrontEndKind::Phase;
        Signal tab(static_cast<size_t>(phase ? gpu::fused_phase_table_floats(fe.geom) : gpu::fused_any_table_floats(plan->l, t1)) + 16, 0.f);
        if (phase) {
            const gpu::FusedVariantRow &row = gpu::kFusedVariants[fe.variant[0]];  // (the tile is the kernel's: its own T2)
            gpu::fused_phase_table(fe.geom, static_cast<uint32_t>(row.t2), plan->pw, plan->taps_resample.data(), tab.data(), plan->psw);
        } else gpu::fused_any_table(plan->l, plan->taps_resample.data(), t1, tab.data());
        upload(plan, plan->d_taps_any, tab);
    }
    // the low-pass taps in pairs, and (kModeStrictPad2) laid out for the kernel's bound: zeros behind the filter's last tap
    Signal lp(plan->taps_lowpass);
    if (fe.pad_t2) {
        lp.resize(fe.pad_t2, 0.f);
        Signal padded(lp);
        padded.resize(lp.size() + 16, 0.f);
        upload(plan, plan->d_taps_lowpass_pad, padded);
    }
    Signal h2p(2 * (lp.size() + 1) + 16, 0.f);
    gpu::fused_lowpass_pairs(lp.data(), static_cast<uint32_t>(lp.size()), h2p.data());
    upload(plan, plan->d_taps_lowpass_pairs, h2p);
}

// workspace: one set of max_batch slots per stream
void alloc_workspace(aptgpu_plan *plan)
{
    plan->slots.resize(plan->streams.size() * static_cast<size_t>(plan->max_batch));
    const uint64_t w = plan->max_work_len;
    // (F in pixel-phase planes where a k_fused instantiation writes it: pw planes of f_plane_stride floats)
    plan->plane_stride = plan->writes_planes() ? gpu::f_plane_stride(w, plan->pw) : 0u;  // (then pw >= 1)
    for (auto &sl : plan->slots) {
        // (resampled / demodulated / correlation are only needed by the unfused kernels: allocated on first use)
        sl.filtered.alloc(std::max<uint64_t>(w, static_cast<uint64_t>(plan->pw) * plan->plane_stride) + 64);
        sl.f_stride = plan->plane_stride;  // (what a call without step export leaves: run_call)
        if (plan->sync) {
            sl.peaks.alloc(plan->max_rows + 2);
            const uint64_t ng = w / gpu::sync_group_size() + 2;
            const uint64_t chunks = ng / gpu::sync_chunk_groups() + 2;
            sl.gm.alloc(ng + 64);
            sl.words.alloc(ng + 64);
            sl.nanw.alloc(ng + 64);
            sl.slot_nt.alloc(chunks * gpu::sync_slot_cap());
            sl.slot_cnt.alloc(chunks);
            sl.orbit_ws.alloc(gpu::sync_orbit_ws_words(w, plan->spr));
            sl.flags.alloc(32);
            hip_check(hipMemsetAsync(sl.flags.ptr, 0, 32 * sizeof(uint32_t), plan->stream), "hipMemset flags");
            if (plan->fe.kind == gpu::FrontEndKind::Unfused) sl.correlation.alloc(w + 64);
            if (plan->mode == APTGPU_MODE_GENERIC) sl.bits.alloc(w / 64 + plan->md / 64 + 4);
        }
    }
    plan->d_results.alloc(plan->slots.size());
    hip_check(hipMemsetAsync(plan->d_results.ptr, 0, sizeof(gpu::Result) * plan->slots.size(), plan->stream),
              "hipMemset");
    plan->d_slots.alloc(plan->slots.size());
    // the uploads and memsets above ran on the plan's first stream: make them land before a decode can
    // be enqueued on any of the others (a stream sync, not a device sync — other plans of this process,
    // e.g. concurrent aptgpu_decode calls on other host threads, keep running)
    plan->upload_slot_table();
}

}  // namespace

aptgpu_plan *plan_create(const aptgpu_context *ctx, const aptgpu_settings &settings,
                         uint32_t input_rate, bool sync, size_t max_samples, int max_batch, int depth)
{
    if (input_rate == 0) throw Error{ErrorKind::Invalid, "input_rate is 0"};
    if (max_batch < 1) max_batch = 1;

    auto plan = std::make_unique<aptgpu_plan>();
    plan->device = ctx ? ctx->device : 0;
    plan->mode = ctx ? ctx->mode : APTGPU_MODE_STRICT;
    plan->settings = settings;
    plan->input_rate = input_rate;
    plan->sync = sync;
    plan->max_samples = max_samples;
    plan->max_batch = max_batch;
    plan->sw = gpu::read_launch_switches();
    plan->psw = gpu::read_plan_switches();
    plan->export_filtered = settings.export_resample_filtered != 0;
    plan->force_walk = plan->psw.force_walk == '1';

    // the filters, factors and sync geometry (pure host code: apt_front_end.cpp)
    static_cast<PlanDesign &>(*plan) = design_plan(settings, input_rate, sync);

    hip_check(hipSetDevice(plan->device), "hipSetDevice");
    create_streams(plan.get(), ctx, depth);

    plan->max_work_len = plan->work_len_for(max_samples);
    const uint64_t rows = plan->spr ? plan->max_work_len / plan->spr + 2 : 2;
    plan->max_rows = static_cast<uint32_t>(rows);

    upload(plan.get(), plan->d_taps_resample, plan->taps_resample);
    upload(plan.get(), plan->d_taps_lowpass, plan->taps_lowpass);
    upload(plan.get(), plan->d_one, Signal{1.f});
    plan->fe = gpu::select_front_end(plan->l, plan->m, static_cast<uint32_t>(plan->taps_resample.size()),
                                     static_cast<uint32_t>(plan->taps_lowpass.size()), plan->pw, plan->mode,
                                     plan->work_is_multiple, plan->export_filtered, plan->psw);
    note_unspecialised(plan.get());
    upload_front_end_tables(plan.get());
    alloc_workspace(plan.get());
    return plan.release();
}

}  // namespace apt

void aptgpu_plan::upload_slot_table()
{
    std::vector<apt::gpu::SlotPtrs> tab(slots.size());
    for (size_t k = 0; k < slots.size(); ++k) {
        Slot &sl = slots[k];
        apt::gpu::SlotPtrs &t = tab[k];
        t.f = sl.filtered.ptr;
        t.gm = sl.gm.ptr;
        t.corr = sl.correlation.ptr;
        t.words = sl.words.ptr;
        t.nanw = sl.nanw.ptr;
        t.slot_nt = sl.slot_nt.ptr;
        t.slot_cnt = sl.slot_cnt.ptr;
        t.flags = sl.flags.ptr;
        t.orbit_ws = sl.orbit_ws.ptr;
        t.peaks = sl.peaks.ptr;
        t.res = d_results.ptr + k;
        t.peaks_cap = static_cast<uint32_t>(sl.peaks.count);
        t.f_stride = sl.f_stride;
    }
    apt::hip_check(hipMemcpyAsync(d_slots.ptr, tab.data(), tab.size() * sizeof(apt::gpu::SlotPtrs),
                                  hipMemcpyHostToDevice, stream),
                   "hipMemcpy slot table");
    apt::gpu::FusedParams prm{};
    if (writes_planes()) {
        prm.hs = d_taps_branch.ptr;
        prm.table = d_taps_any.ptr;
        prm.tab = fe.geom;
        prm.h2 = fe.pad_t2 ? d_taps_lowpass_pad.ptr : d_taps_lowpass.ptr;
        prm.h2p = d_taps_lowpass_pairs.ptr;
        prm.t2 = static_cast<uint32_t>(taps_lowpass.size());
        prm.slots = d_slots.ptr;
        prm.cosphi2 = cosphi2;
        prm.sinphi = sinphi;
        prm.inv_sinphi = inv_sinphi;
        prm.f16_unscale = fe.f16 ? f16_unscale : 0.f;
        prm.coeff = d_taps_resample.ptr;
        prm.t1 = static_cast<uint32_t>(taps_resample.size());
        prm.want_gm = (sync && work_is_multiple) ? 1 : 0;
        prm.gm_slack = apt::gpu::fused_gm_slack(pw, sw.gm_slack_scale);
        if (!d_fused_params.ptr) d_fused_params.alloc(1);
        apt::hip_check(hipMemcpyAsync(d_fused_params.ptr, &prm, sizeof prm, hipMemcpyHostToDevice, stream),
                       "hipMemcpy fused params");
    }
    apt::hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
}

// ------------------------------------------------------- export_resample_filtered
// fast_resampling (dsp.rs:186-289) evaluated at t = off + d0 + k*step of the interpolated axis: the window of
// such a t starts at the first multiple of l at or after t - off = d (:237-248), input x0 = ceil(d / l), tap
// p = x0*l - d, then taps p + i*l while they stay <= 2*off (:254); inputs at or beyond n are skipped (:257).
// step == m, d0 == 0 is the normal branch (k_resample_generic); the export branch (:265-273) needs d0 =
// ResampleGeom::d0 for the output and step == 1 for the expanded signal.  Only this mode uses the
// kernel, which is why it lives beside the plan and not with the hot kernels.
namespace {
__global__ void __launch_bounds__(256)
k_resample_at(const float *__restrict__ x, uint64_t n, const float *__restrict__ coeff, uint32_t jlim, uint32_t l,
              uint64_t d0, uint32_t step, float *__restrict__ out, uint64_t w)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; k < w; k += stride) {
        const uint64_t d = d0 + k * step;
        uint64_t xi = (d + l - 1) / l;
        const uint32_t p = static_cast<uint32_t>(xi * l - d);
        float sum = 0.f;
        for (uint32_t j = p; j < jlim; j += l, ++xi)
            if (xi < n) sum = __fadd_rn(sum, __fmul_rn(coeff[j], x[xi]));
        out[k] = sum;
    }
}

}  // namespace

namespace apt {
void resample_at(hipStream_t s, const float *x, uint64_t n, const float *coeff, uint32_t ntaps, uint32_t l, uint64_t d0,
                 uint32_t step, float *out, uint64_t w)
{
    if (w == 0) return;
    const uint32_t jlim = 2 * ((ntaps - 1) / 2) + 1;  // n <= t + offset  <=>  j <= 2*offset
    const uint64_t blocks = std::min<uint64_t>((w + 255) / 256, 256u * 64u);
    hipLaunchKernelGGL(k_resample_at, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, x, n, coeff, jlim, l, d0, step,
                       out, w);
}
}  // namespace apt

// ------------------------------------------------------- one resample_with_filter stage
namespace apt {
// resample_with_filter's choice (dsp.rs:77-124) among the kernels that compute it
ResampleStage::Kernel ResampleStage::kernel() const
{
    if (g.l == 1) return kFirDecimate;  // filter + decimate
    if (g.flagged) return kResampleAt;  // fast_resampling's other decimation phase (dsp.rs:265-273)
    return d_taps_f16 ? kResampleF16Taps : kResampleGeneric;
}

const char *ResampleStage::label(bool final_stage) const
{
    static const char *const first[] = {"resample_generic", "resample_f16taps", "resample_generic", "fir_decimate"};
    static const char *const last[] = {"final_resample", "final_resample", "final_resample", "final_decimate"};
    return (final_stage ? last : first)[kernel()];
}

void ResampleStage::enqueue(hipStream_t s, const float *d_x, uint64_t n, float *d_out, uint64_t w) const
{
    const uint32_t t = static_cast<uint32_t>(g.ntaps);
    switch (kernel()) {
        case kResampleAt: resample_at(s, d_x, n, d_taps, t, g.l, g.d0(n), g.m, d_out, w); break;
        case kResampleF16Taps: gpu::resample_f16taps(s, d_x, n, d_taps_f16, t, g.l, g.m, f16_unscale, d_out, w); break;
        case kResampleGeneric: gpu::resample_generic(s, d_x, n, d_taps, t, g.l, g.m, d_out, w); break;
        case kFirDecimate: gpu::fir_decimate(s, d_x, n, d_taps, t, g.m, d_out, w); break;
    }
}

void ResampleStage::enqueue_filtered(hipStream_t s, const float *d_x, uint64_t n, float *d_out) const
{
    const uint32_t t = static_cast<uint32_t>(g.ntaps);
    if (g.l > 1) resample_at(s, d_x, n, d_taps, t, g.l, 0, 1, d_out, g.expanded_len(n));
    else gpu::fir_decimate(s, d_x, n, d_taps, t, 1, d_out, n);
    hip_check(hipGetLastError(), "kernel launch (resample_filtered step)");
}
}  // namespace apt

void aptgpu_plan::sync_all()
{
    for (hipStream_t st : streams) apt::hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
}

// ------------------------------------------------------------------ pipeline
// The kernel sequence of decode() for the recordings of one call, all already in HBM.
void aptgpu_plan::run_call(int count, const Input *ins, float *const *d_rows, const uint64_t *rows_cap_floats,
                           bool keep_steps)
{
    using namespace apt::gpu;
    if (count < 0 || count > max_batch) throw apt::Error{apt::ErrorKind::Invalid, "more recordings than max_batch"};
    last_stream = static_cast<int>(calls++ % streams.size());
    hipStream_t cur = streams[static_cast<size_t>(last_stream)];
    const int slot0 = last_stream * max_batch;
    last_slots.assign(static_cast<size_t>(count), 0);
    for (int i = 0; i < count; ++i) last_slots[static_cast<size_t>(i)] = slot0 + i;
    composite_count = -1;
    // the call's stream waits for what is already enqueued on ctx.stream (inputs may be produced there)
    if (user_stream) {
        apt::hip_check(hipEventRecord(ev_user, user_stream), "hipEventRecord");
        apt::hip_check(hipStreamWaitEvent(cur, ev_user, 0), "hipStreamWaitEvent");
    }
    auto timed = [&](const char *name, auto &&launch) {
        const bool dominant = !std::strcmp(name, "fused_front_end") || !std::strcmp(name, "resample_generic") ||
                              !std::strcmp(name, "resample_f16taps");
        timer.begin(cur, name, dominant);
        launch();
        timer.end(cur);
    };

    const bool use_fused = fe.kind != FrontEndKind::Unfused && !keep_steps;
    const bool want_sync = sync && work_is_multiple;
    // The layout of F this call leaves in its slots: pixel-phase planes from the k_fused instantiations, contiguous from
    // k_fused_any and the unfused kernels (a fused plan that exports steps).  Every consumer reads it from the slot table.
    const uint32_t f_stride = use_fused ? plane_stride : 0u;
    {
        bool changed = false;
        for (int i = 0; i < count; ++i) {
            Slot &sl = slots[static_cast<size_t>(slot0 + i)];
            // the unfused kernels keep the full correlation; a fused plan that exports steps gets the
            // buffers (and their entry in the slot table) on first use
            if (!use_fused && sync && !sl.correlation.ptr) {
                sl.correlation.alloc(max_work_len + 64);
                changed = true;
            }
            if (sl.f_stride != f_stride) {
                sl.f_stride = f_stride;
                changed = true;
            }
        }
        if (changed) {
            sync_all();  // (no launch in flight may be reading the table while it is rewritten)
            upload_slot_table();
        }
    }

    // recordings that go through the kernels; the error paths of decode() are settled per recording
    std::vector<int> live;
    std::vector<uint64_t> wlen(static_cast<size_t>(count));
    std::vector<const void *> xin(static_cast<size_t>(count));
    std::vector<char> is_pcm(static_cast<size_t>(count), 0);
    for (int i = 0; i < count; ++i) {
        const Input &in = ins[i];
        Slot &sl = slots[static_cast<size_t>(slot0 + i)];
        Result *res = d_results.ptr + slot0 + i;
        sl.fused_variant = -1;  // (until a k_fused instantiation serves this call)
        const uint64_t w = work_len_for(in.n);
        wlen[static_cast<size_t>(i)] = w;
        // decode.rs:79-83 — fewer than 10 rows of samples
        if (w < 10ull * spr) {
            set_result(cur, res, Result{APTGPU_ERR_INTERNAL, 1, 0, 0, w, 0});
            continue;
        }
        // WAV ingest (wav.rs:30-51): mono PCM16 goes straight into the fused front end, anything
        // else is converted into the slot's f32 staging buffer first
        // (a k_fused instantiation for f32 input only — odd m: no dword reads of sample pairs — gets the payload staged)
        const bool pcm16 = in.codec == static_cast<int>(apt::WavCodec::I16) && in.channels == 1 && use_fused &&
                           (reinterpret_cast<uintptr_t>(in.ptr) & (fe.kind == FrontEndKind::Split ? 3u : 1u)) == 0 &&
                           (!writes_planes() || fe.variant[1] != kFusedNone);
        xin[static_cast<size_t>(i)] = in.ptr;
        is_pcm[static_cast<size_t>(i)] = pcm16 ? 1 : 0;
        if (in.codec >= 0 && !pcm16) {
            if (!sl.ingest.ptr) sl.ingest.alloc(max_samples + 16);
            timed("wav_to_signal", [&] {
                wav_to_signal(cur, in.ptr, in.n, in.channels, in.bytes_per_sample, in.codec, sl.ingest.ptr);
            });
            xin[static_cast<size_t>(i)] = sl.ingest.ptr;
        }
        live.push_back(i);
    }
    // the fused front ends take one launch per input kind: the live recordings that are f32 Signals [0] / mono PCM16 [1]
    std::vector<int> by_kind[2];
    if (use_fused)
        for (int i : live) by_kind[is_pcm[static_cast<size_t>(i)] ? 1 : 0].push_back(i);

    // per-stage launches cover up to kMaxCall recordings each
    auto make_call = [&](const std::vector<int> &idx, size_t from, size_t to, uint64_t *max_w, uint32_t *max_cap) {
        CallArgs c{};
        c.count = static_cast<uint32_t>(to - from);
        *max_w = 0;
        *max_cap = 0;
        for (size_t k = from; k < to; ++k) {
            const int i = idx[k];
            RecArgs &r = c.rec[k - from];
            r.x = xin[static_cast<size_t>(i)];
            r.n = ins[i].n;
            r.w = wlen[static_cast<size_t>(i)];
            r.rows = d_rows[i];
            uint64_t rc = rows_cap_floats[i] / 2080u;
            if (rc > max_rows) rc = max_rows;
            r.rows_cap = static_cast<uint32_t>(rc);
            r.slot = static_cast<uint32_t>(slot0 + i);
            *max_w = std::max(*max_w, r.w);
            *max_cap = std::max(*max_cap, r.rows_cap);
        }
        return c;
    };
    auto for_chunks = [&](const std::vector<int> &idx, auto &&fn) {
        for (size_t from = 0; from < idx.size(); from += static_cast<size_t>(kMaxCall)) {
            const size_t to = std::min(idx.size(), from + static_cast<size_t>(kMaxCall));
            uint64_t max_w = 0;
            uint32_t max_cap = 0;
            const CallArgs c = make_call(idx, from, to, &max_w, &max_cap);
            fn(c, max_w, max_cap);
        }
    };

    const uint32_t t1 = static_cast<uint32_t>(taps_resample.size());
    const uint32_t t2 = static_cast<uint32_t>(taps_lowpass.size());
    if (use_fused && writes_planes()) {
        // 1-3 fused: resample -> envelope -> low-pass (-> correlation maxima) in one launch per input
        // kind (apt_kernels_fused.hip), behind the previous call's front end (see front_serial, apt_plan.hpp)
        if (front_serial && !live.empty() && prev_front >= 0 && prev_front != last_stream)
            apt::hip_check(hipStreamWaitEvent(cur, ev_front[static_cast<size_t>(prev_front)], 0), "hipStreamWaitEvent");
        for (int kind = 0; kind < 2; ++kind) {
#if defined(APT_WITH_PROBES) || defined(APT_DEBUG_SKIP)
            const int rep_f = [] { const char *e = std::getenv("APTGPU_DEBUG_REPEAT_FRONT"); return e ? std::max(1, std::atoi(e)) : 1; }();
#else
            constexpr int rep_f = 1;
#endif
            for (int rf = 0; rf < rep_f; ++rf)
            for_chunks(by_kind[kind], [&](const CallArgs &c, uint64_t max_w, uint32_t) {
                timed("fused_front_end", [&] {
                    int variant = -1;
                    const bool ok = fused_front_end(cur, fe, kind == 1, c, d_fused_params.ptr, max_w, &variant);
                    for (uint32_t k = 0; k < c.count; ++k) {
                        slots[c.rec[k].slot].fused_variant = variant;
                        slots[c.rec[k].slot].fused_variant_i16 = kind == 1;
                    }
                    if (!ok)
                        throw apt::Error{apt::ErrorKind::Internal, "fused front end: no kernel for this geometry"};
                });
            });
        }
        if (front_serial && !live.empty()) {
            apt::hip_check(hipEventRecord(ev_front[static_cast<size_t>(last_stream)], cur), "hipEventRecord");
            prev_front = last_stream;
        }
    } else if (use_fused) {
        // the run-time front end (k_fused_any: fast / slow profiles, odd rates): one launch per input kind too
        for (int kind = 0; kind < 2; ++kind) {
            for_chunks(by_kind[kind], [&](const CallArgs &c, uint64_t max_w, uint32_t) {
                timed("fused_front_end", [&] {
                    if (!fused_any_front_end(cur, l, m, t1, t2, pw, kind == 1, c, d_slots.ptr, max_w, d_taps_any.ptr,
                                             d_taps_lowpass.ptr, d_taps_lowpass_pairs.ptr, cosphi2, sinphi, inv_sinphi,
                                             want_sync, sw.gm_slack_scale))
                        throw apt::Error{apt::ErrorKind::Internal, "fused front end: no kernel for this geometry"};
                });
            });
        }
    } else {
        for (int i : live) {
            Slot &sl = slots[static_cast<size_t>(slot0 + i)];
            const uint64_t w = wlen[static_cast<size_t>(i)];
            const uint64_t n = ins[i].n;
            const float *d_signal = static_cast<const float *>(xin[static_cast<size_t>(i)]);
            if (!sl.resampled.ptr) {
                sl.resampled.alloc(max_work_len + 64);
                sl.demodulated.alloc(max_work_len + 64);
            }
            // 1. resample to work_rate (dsp.rs:62-126)
            const apt::ResampleStage st = first_stage();
            timed(st.label(false), [&] { st.enqueue(cur, d_signal, n, sl.resampled.ptr, w); });
            // 2. AM envelope (dsp.rs:350-383)
            timed("demodulate", [&] { demodulate(cur, sl.resampled.ptr, w, cosphi2, sinphi, sl.demodulated.ptr); });
            // 3. low-pass (dsp.rs:386-410)
            timed("lowpass", [&] {
                fir_decimate(cur, sl.demodulated.ptr, w, d_taps_lowpass.ptr, t2, 1, sl.filtered.ptr, w);
            });
            // 4a. the full correlation of find_sync (decode.rs:225-233) and its group maxima
            if (want_sync) {
                const uint64_t n_corr = w - n_sync_taps;  // w >= 10*spr > 38*pw
                timed("correlate", [&] { correlate(cur, sl.filtered.ptr, n_corr, pw, sl.correlation.ptr); });
                if (mode != APTGPU_MODE_GENERIC)
                    timed("group_max", [&] { group_max(cur, sl.correlation.ptr, n_corr, sl.gm.ptr); });
            }
        }
    }

    if (sync && !work_is_multiple) {
        // generate_sync_frame, decode.rs:172-176
        for (int i : live)
            set_result(cur, d_results.ptr + slot0 + i, Result{APTGPU_ERR_INTERNAL, 3, 0, 0, wlen[static_cast<size_t>(i)], 0});
    } else if (sync) {
        bool gather_wanted = true;
        int gather_reps = 1;
        // 4. find_sync (decode.rs:204-263): terminal flags, orbit
        if (mode == APTGPU_MODE_GENERIC) {
            // reference-shaped picker: full sliding-window terminals + sequential orbit
            for (int i : live) {
                Slot &sl = slots[static_cast<size_t>(slot0 + i)];
                const uint64_t w = wlen[static_cast<size_t>(i)];
                const uint64_t n_corr = w - n_sync_taps;
                timed("terminals", [&] { terminals(cur, sl.correlation.ptr, n_corr, md, sl.bits.ptr); });
                timed("orbit_walk", [&] {
                    orbit_walk(cur, sl.bits.ptr, sl.correlation.ptr, n_corr, w, spr, md, sl.peaks.ptr,
                               static_cast<uint32_t>(sl.peaks.count),
                               d_results.ptr + slot0 + i);
                });
            }
        } else {
            // (probe builds only — make PROBES=1, or libaptgpu_probe.so of `make probe-lib` — APTGPU_DEBUG_SKIP, a bit mask: 1 words + slots, 2 orbit,
            // 4 gather.  Timing experiments: what each kernel behind the front end costs a pipelined step; the results
            // are then garbage, so a product build does not even read the variable.)
#if defined(APT_WITH_PROBES) || defined(APT_DEBUG_SKIP)
            const int skip = [] {
                const char *e = std::getenv("APTGPU_DEBUG_SKIP");
                return e ? std::atoi(e) : 0;
            }();
            // APTGPU_DEBUG_REPEAT_WORDS / _ORBIT / _GATHER = n: the kernel is launched n times instead of once (each is
            // idempotent: same inputs, same outputs) — what ONE more launch of it costs a pipelined step, with every
            // result still valid
            const int rep_w = [] { const char *e = std::getenv("APTGPU_DEBUG_REPEAT_WORDS"); return e ? std::max(1, std::atoi(e)) : 1; }();
            const int rep_o = [] { const char *e = std::getenv("APTGPU_DEBUG_REPEAT_ORBIT"); return e ? std::max(1, std::atoi(e)) : 1; }();
            const int rep_g = [] { const char *e = std::getenv("APTGPU_DEBUG_REPEAT_GATHER"); return e ? std::max(1, std::atoi(e)) : 1; }();
#else
            constexpr int skip = 0, rep_w = 1, rep_o = 1, rep_g = 1;
#endif
            gather_reps = rep_g;
            for_chunks(live, [&](const CallArgs &c, uint64_t max_w, uint32_t) {
                if (!(skip & 1))
                    for (int r = 0; r < rep_w; ++r)
                        timed("sync_nodes", [&] { sync_nodes(cur, c, d_slots.ptr, max_w, pw, spr, md, use_fused && fe.fast, !use_fused, sw); });
                if (!(skip & 2))
                    for (int r = 0; r < rep_o; ++r)
                        timed("sync_orbit", [&] { sync_orbit(cur, c, d_slots.ptr, spr, md, pw, force_walk, sw); });
            });
            gather_wanted = !(skip & 4);
        }
        // 5. aligned rows + final /pw (decode.rs:120-134,158-159)
        if (gather_wanted)
            for (int r = 0; r < gather_reps; ++r)
                for_chunks(live, [&](const CallArgs &c, uint64_t, uint32_t max_cap) {
                    timed("gather_rows", [&] { gather_rows_call(cur, c, d_slots.ptr, spr, pw, max_cap); });
                });
    } else {
        // decode.rs:135-159 — crop to whole rows, resample_with_filter(NoFilter).  Where that is a pure decimation
        // (every stock profile: l2 == 1) the recordings of the call share ONE launch, result records included
        if (l2 == 1 && !keep_steps) {
            for (size_t from = 0; from < live.size(); from += static_cast<size_t>(kMaxCall)) {
                const size_t to = std::min(live.size(), from + static_cast<size_t>(kMaxCall));
                uint64_t max_w = 0;
                uint32_t max_cap = 0;
                CallArgs c = make_call(live, from, to, &max_w, &max_cap);
                for (size_t k = from; k < to; ++k)  // (floats, not rows, in this launch)
                    c.rec[k - from].rows_cap = static_cast<uint32_t>(std::min<uint64_t>(rows_cap_floats[live[k]], 0xFFFFFFFFull));
                timed("final_decimate", [&] { nosync_rows_call(cur, c, d_slots.ptr, spr, m2, max_w); });
            }
        } else
        for (int i : live) {
            Slot &sl = slots[static_cast<size_t>(slot0 + i)];
            // (the kernels below read F as one contiguous signal: step exports run unfused, and l2 > 1 — a work rate
            // that is no multiple of 4160 Hz — has no k_fused instantiation)
            if (sl.f_stride != 0) throw apt::Error{apt::ErrorKind::Internal, "no-sync tail: F is in pixel-phase planes"};
            const uint64_t w = wlen[static_cast<size_t>(i)];
            uint64_t n_out = out_len_nosync(w);
            if (n_out > rows_cap_floats[i]) n_out = rows_cap_floats[i];
            const apt::ResampleStage st = final_stage();
            timed(st.label(true), [&] { st.enqueue(cur, sl.filtered.ptr, whole_rows(w), d_rows[i], n_out); });
            set_result(cur, d_results.ptr + slot0 + i,
                       Result{APTGPU_OK, 0, static_cast<uint32_t>(n_out / 2080u), 0, w, n_out});
        }
    }
    // a launch that failed (bad grid / LDS size, an earlier fault) would otherwise leave a stale or
    // zeroed — i.e. "OK" — result record behind
    apt::hip_check(hipGetLastError(), "kernel launch (decode chain)");
}

// ------------------------------------------------------------------ image stage
aptgpu_plan::ImageTarget aptgpu_plan::image_target(int i, uint64_t rows_cap_floats)
{
    using namespace apt::gpu;
    const size_t slot = static_cast<size_t>(last_slots[static_cast<size_t>(i)]);
    Slot &sl = slots[slot];
    uint64_t cap = static_cast<uint64_t>(max_rows) * 2080u;
    if (!sync) cap = out_len_nosync(work_len_for(max_samples)) + 16;
    if (rows_cap_floats < cap) cap = rows_cap_floats;
    const uint64_t ws_cap = std::max<uint64_t>(static_cast<uint64_t>(max_rows) * 2080u,
                                               out_len_nosync(work_len_for(max_samples)) + 16);
    if (!d_image_results.ptr) {
        // (no memset: the first kernel of every variant resets its record)
        d_image_results.alloc(slots.size());
    }
    if (!sl.image_ws.ptr) sl.image_ws.alloc(image_ws_bytes(ws_cap));
    return ImageTarget{sl, stream_of(i), cap, sl.image_ws.ptr, d_image_results.ptr + slot, d_results.ptr + slot};
}

// A plan brackets the launch with its timer and checks each stage's launches under the stage's own label; a one-shot
// call (plan == null) does neither.
template <typename Fn>
static void launch_timed(aptgpu_plan *plan, hipStream_t s, const char *name, Fn &&launch)
{
    plan ? plan->timed(s, name, launch) : launch();
}
static void stage_done(aptgpu_plan *plan, const char *label)
{
    if (plan) apt::hip_check(hipGetLastError(), label);
}

void apt::enqueue_image_limits(aptgpu_plan *plan, const ImageJob &j, int contrast, float percent)
{
    using namespace apt::gpu;
    hipStream_t s = j.stream;
    if (contrast == APTGPU_CONTRAST_TELEMETRY)
        launch_timed(plan, s, "image_telemetry", [&] { image_telemetry(s, j.rows, j.res, j.n, j.cap, j.ws, j.info, true); });
    else if (contrast == APTGPU_CONTRAST_PERCENT)
        launch_timed(plan, s, "image_percent", [&] { image_percent(s, j.rows, j.res, j.n, j.cap, percent, j.ws, j.info); });
    else  // MinMax, and Histogram's limits (noaa_apt.rs:158-164)
        launch_timed(plan, s, "image_minmax", [&] { image_minmax(s, j.rows, j.res, j.n, j.cap, j.ws, j.info); });
}

void aptgpu_plan::enqueue_image(int i, const float *d_rows, uint64_t rows_cap_floats, int contrast,
                                float percent, bool rotate, uint8_t *d_image)
{
    using namespace apt::gpu;
    const ImageTarget t = image_target(i, rows_cap_floats);
    apt::enqueue_image_limits(this, image_job(t, d_rows), contrast, percent);
    timed(t.stream, "image_map_u8", [&] { image_map_u8(t.stream, d_rows, t.res, 0, t.cap, t.ws, rotate, d_image, t.out); });
    apt::hip_check(hipGetLastError(), "kernel launch (image stage)");
}

void apt::enqueue_despeckle(aptgpu_plan *plan, const ImageJob &j, int radius, float threshold, float *d_out,
                            apt::gpu::DespeckleResult *rec)
{
    using namespace apt::gpu;
    hipStream_t s = j.stream;
    if (threshold != 0.f && (j.res || j.n >= 2080))  // (the limits of the unfiltered signal, as Percent(0.98) reports them)
        enqueue_image_limits(plan, j, APTGPU_CONTRAST_PERCENT, 0.98f);
    launch_timed(plan, s, "image_despeckle", [&] {
        apt::gpu::despeckle(s, j.rows, j.res, j.n, j.cap, radius, threshold, image_ws_pointers(j.ws, j.cap).limits, j.info,
                            d_out, rec);
    });
    apt::hip_check(hipGetLastError(), "kernel launch (despeckle stage)");
}

void apt::enqueue_thermal(aptgpu_plan *plan, const ImageJob &j, apt::gpu::ThermalLaunch l,
                          const apt::gpu::ThermalCoeffs &coeffs, const apt::gpu::ThermalTable &table, void *ws)
{
    using namespace apt::gpu;
    hipStream_t s = j.stream;
    l.res = j.res;
    l.n = j.n;
    l.cap = j.cap;
    launch_timed(plan, s, "image_telemetry",
                 [&] { image_telemetry(s, j.rows, j.res, j.n, j.cap, j.ws, thermal_ws_telemetry(ws), false); });
    launch_timed(plan, s, "image_thermal_space", [&] { thermal_space(s, l, ws); });
    launch_timed(plan, s, "image_thermal_setup", [&] { thermal_setup(s, l, coeffs, ws); });
    launch_timed(plan, s, "image_thermal_map", [&] { thermal_map(s, l, table, ws); });
    apt::hip_check(hipGetLastError(), "kernel launch (thermal stage)");
}

void apt::enqueue_geoloc(aptgpu_plan *plan, const ImageJob &j, apt::gpu::GeolocLaunch l, apt::map::Device &dev, void *ws)
{
    using namespace apt::gpu;
    hipStream_t s = j.stream;
    l.res = j.res;
    l.n = j.n;
    l.cap = j.cap;
    dev.prepare_track(s, static_cast<size_t>(j.cap / 2080u));
    launch_timed(plan, s, "image_geoloc_track", [&] { geoloc_track(s, l, dev, ws); });
    launch_timed(plan, s, "image_geoloc_rows", [&] { geoloc_rows(s, l, dev, ws); });
    launch_timed(plan, s, "image_geoloc", [&] { geoloc_pixels(s, l, dev, ws); });
    apt::hip_check(hipGetLastError(), "kernel launch (geolocation stage)");
}

void aptgpu_plan::enqueue_despeckle(int i, const float *d_rows, uint64_t rows_cap_floats, int radius, float threshold,
                                    float *d_out)
{
    using namespace apt::gpu;
    const ImageTarget t = image_target(i, rows_cap_floats);
    Slot &sl = t.slot;
    if (!sl.despeckle_ws.ptr) sl.despeckle_ws.alloc(despeckle_ws_bytes());
    apt::ImageJob j = image_job(t, d_rows);
    j.info = despeckle_ws_limits_info(sl.despeckle_ws.ptr);  // (the limits' record; the image stage's stays as it is)
    apt::enqueue_despeckle(this, j, radius, threshold, d_out, despeckle_ws_record(sl.despeckle_ws.ptr));
}

void aptgpu_plan::enqueue_thermal(int i, uint64_t rows_cap_floats, const apt::gpu::ThermalLaunch &l,
                                  const apt::gpu::ThermalCoeffs &coeffs, const apt::gpu::ThermalTable &table)
{
    const ImageTarget t = image_target(i, rows_cap_floats);
    Slot &sl = t.slot;
    if (!sl.thermal_ws.ptr) sl.thermal_ws.alloc(apt::gpu::thermal_ws_bytes());
    apt::enqueue_thermal(this, image_job(t, l.x), l, coeffs, table, sl.thermal_ws.ptr);
}

void aptgpu_plan::enqueue_geoloc(int i, uint64_t rows_cap_floats, const apt::gpu::GeolocLaunch &l)
{
    const ImageTarget t = image_target(i, rows_cap_floats);
    Slot &sl = t.slot;
    const size_t rows = static_cast<size_t>(t.cap / 2080u);
    if (!sl.geoloc_ws.ptr || sl.geoloc_rows < rows) {
        sl.geoloc_ws.alloc(apt::gpu::geoloc_ws_bytes(rows));
        sl.geoloc_rows = rows;
    }
    if (!sl.map) sl.map = std::make_unique<apt::map::Device>();
    apt::enqueue_geoloc(this, image_job(t, l.x), l, *sl.map, sl.geoloc_ws.ptr);
}

aptgpu_plan::Palette::~Palette()
{
    for (hipEvent_t ev : uploaded)
        if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : lab_uploaded)
        if (ev) (void)hipEventDestroy(ev);
    if (pinned) (void)hipHostFree(pinned);
    if (lab_pinned) (void)hipHostFree(lab_pinned);
}

void aptgpu_plan::set_palette(const uint8_t *rgb, bool lab)
{
    constexpr size_t kBytes = 256 * 256 * 3;
    if (palette.gen == 0 || std::memcmp(palette.rgb.data(), rgb, kBytes) != 0) new_palette(rgb);
    if (!lab || palette.lab_gen == palette.gen) return;
    if (!palette.lab_pinned) {
        apt::hip_check(hipHostMalloc(reinterpret_cast<void **>(&palette.lab_pinned), sizeof(apt::lab::Tables)),
                       "hipHostMalloc");
        palette.lab_uploaded.assign(streams.size(), nullptr);
    }
    for (hipEvent_t ev : palette.lab_uploaded)  // as for `pinned` below
        if (ev) apt::hip_check(hipEventSynchronize(ev), "hipEventSynchronize");
    std::memcpy(palette.lab_pinned, apt::lab::tables_for(rgb).get(), sizeof(apt::lab::Tables));
    palette.lab_gen = palette.gen;
}

void aptgpu_plan::new_palette(const uint8_t *rgb)
{
    constexpr size_t kBytes = 256 * 256 * 3;
    if (!palette.pinned) {
        apt::hip_check(hipHostMalloc(reinterpret_cast<void **>(&palette.pinned), 65536 * sizeof(uint32_t)),
                       "hipHostMalloc");
        palette.uploaded.assign(streams.size(), nullptr);
    }
    // the slots' uploads of the previous generation read `pinned`: wait for them (only when the palette
    // changes; a plan that keeps one palette never waits here)
    for (hipEvent_t ev : palette.uploaded)
        if (ev) apt::hip_check(hipEventSynchronize(ev), "hipEventSynchronize");
    palette.rgb.assign(rgb, rgb + kBytes);
    apt::gpu::color_pack_palette(rgb, palette.pinned);
    ++palette.gen;
}

void aptgpu_plan::enqueue_images(const apt::ImageRequest &q, int count, const float *const *d_rows,
                                 const size_t *rows_cap)
{
    using namespace apt::gpu;
    // (sized for the plan's largest image with 4 bytes per pixel, so one allocation serves every call)
    uint64_t stream_cap = 0;
    if (q.png && !q.project)
        stream_cap = apt::png::stream_bytes(
            2080, std::max<uint64_t>(max_rows, out_len_nosync(work_len_for(max_samples)) / 2080u + 1), 4);
    auto upload = [&](void *dst, const void *pinned, size_t bytes, hipEvent_t &ev, hipStream_t s, const char *what) {
        apt::hip_check(hipMemcpyAsync(dst, pinned, bytes, hipMemcpyHostToDevice, s), what);
        if (!ev) apt::hip_check(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate");
        apt::hip_check(hipEventRecord(ev, s), "hipEventRecord");
    };
    std::vector<apt::ImageJob> jobs(static_cast<size_t>(count));
    for (int i = 0; i < count; ++i) {
        const ImageTarget t = image_target(i, static_cast<uint64_t>(rows_cap[i]) * 2080u);
        Slot &sl = t.slot;
        if (!sl.color_ws.ptr) {
            sl.color_ws.alloc(color_ws_bytes());
            apt::hip_check(color_ws_init(t.stream, sl.color_ws.ptr), "hipMemsetAsync");
        }
        if (q.colored && sl.palette_gen != palette.gen) {
            upload(color_ws_palette(sl.color_ws.ptr), palette.pinned, 65536 * sizeof(uint32_t),
                   palette.uploaded[static_cast<size_t>(last_stream)], t.stream, "hipMemcpyAsync H2D (palette)");
            sl.palette_gen = palette.gen;
        }
        if (q.lab) {
            if (!sl.lab_ws.ptr) sl.lab_ws.alloc(lab_ws_bytes());
            if (sl.lab_gen != palette.lab_gen) {
                upload(sl.lab_ws.ptr, palette.lab_pinned, sizeof(apt::lab::Tables),
                       palette.lab_uploaded[static_cast<size_t>(last_stream)], t.stream, "hipMemcpyAsync H2D (Lab tables)");
                sl.lab_gen = palette.lab_gen;
            }
        }
        if (q.contrast == APTGPU_CONTRAST_HISTOGRAM_FLOAT && !sl.eqfloat_ws.ptr) sl.eqfloat_ws.alloc(eqfloat_ws_bytes());
        if ((q.overlay || q.project) && !sl.map) sl.map = std::make_unique<apt::map::Device>();
        if (q.project && !sl.project) sl.project = std::make_unique<apt::project::Device>();
        if (q.png && !q.project && t.cap >= 2080u && !sl.png_ws.ptr) sl.png_ws.alloc(apt::png::ws_bytes(stream_cap));
        apt::ImageJob &j = jobs[static_cast<size_t>(i)];
        j = image_job(t, d_rows[i]);
        j.color_ws = sl.color_ws.ptr;
        j.lab_ws = sl.lab_ws.ptr;
        j.eqfloat_ws = sl.eqfloat_ws.ptr;
        j.png_ws = sl.png_ws.ptr;
        j.map = sl.map.get();
        j.project = sl.project.get();
        j.stream_cap = stream_cap;
        // Histogram with colour takes the 98 % limits; the zero-length error of get_min / get_max is the same
        // record (reason 1) as percent's (noaa_apt.rs:158-175)
        apt::enqueue_image_limits(this, j, q.lab ? APTGPU_CONTRAST_PERCENT : q.contrast, q.lab ? 0.98f : q.percent);
        apt::enqueue_image_color(this, q, q.rec[static_cast<size_t>(i)], j);
    }
    apt::enqueue_image_outputs(this, q, jobs.data(), count);
}

void aptgpu_plan::enqueue_composite(apt::ImageRequest &q, int count, const uint32_t *heights)
{
    if (composite.size() < streams.size()) composite.resize(streams.size());
    std::unique_ptr<apt::composite::Device> &dev = composite[static_cast<size_t>(last_stream)];
    if (!dev) dev = std::make_unique<apt::composite::Device>();
    q.comp.dev = dev.get();
    std::vector<apt::ImageJob> jobs(static_cast<size_t>(count));
    for (int i = 0; i < count; ++i) {
        const ImageTarget t = image_target(i, static_cast<uint64_t>(heights[i]) * 2080u);
        if (!t.slot.map) t.slot.map = std::make_unique<apt::map::Device>();
        apt::ImageJob &j = jobs[static_cast<size_t>(i)];
        j = image_job(t, nullptr);
        j.map = t.slot.map.get();
    }
    composite_count = count;
    apt::enqueue_image_outputs(this, q, jobs.data(), count);
}

namespace apt {

using Recording = ImageRequest::Recording;

static uint32_t count32(size_t count) { return count < 0xffffffffu ? static_cast<uint32_t>(count) : 0xffffffffu; }

void enqueue_image_color(aptgpu_plan *plan, const ImageRequest &q, const Recording &r, const ImageJob &j)
{
    using namespace apt::gpu;
    hipStream_t s = j.stream;
    if (q.contrast == APTGPU_CONTRAST_HISTOGRAM_FLOAT) {  // (no palette: the entry points refuse it)
        launch_timed(plan, s, "image_equalize_float",
                     [&] { image_equalize_float(s, j.rows, j.res, j.n, j.cap, j.eqfloat_ws); });
        launch_timed(plan, s, "image_color_float", [&] {
            image_color_float(s, j.rows, j.res, j.n, j.cap, j.ws, j.eqfloat_ws, q.channels, r.rotate, r.d_image, j.info);
        });
    } else {
        const bool equalize = q.contrast == APTGPU_CONTRAST_HISTOGRAM;
        if (q.lab)
            launch_timed(plan, s, "image_equalize_lab", [&] {
                image_equalize_lab(s, j.rows, j.res, j.n, j.cap, j.ws, j.color_ws, j.lab_ws, q.tune);
            });
        else if (equalize)
            launch_timed(plan, s, "image_equalize", [&] { image_equalize(s, j.rows, j.res, j.n, j.cap, j.ws, j.color_ws); });
        launch_timed(plan, s, "image_color", [&] {
            image_color(s, j.rows, j.res, j.n, j.cap, j.ws, j.color_ws, equalize, q.colored ? &q.tune : nullptr,
                        q.channels, r.rotate, r.d_image, j.info, q.lab ? j.lab_ws : nullptr);
        });
    }
    stage_done(plan, "kernel launch (image stage)");
}

static void enqueue_image_overlay(aptgpu_plan *plan, const ImageRequest &q, const Recording &r, const ImageJob &j)
{
    const apt::map::Colors colors{{q.layers->color[0], q.layers->color[1], q.layers->color[2]}};
    j.map->prepare(j.stream, *q.layers, j.cap / 2080u);
    if (r.track == ImageRequest::Track::Sat) {
        launch_timed(plan, j.stream, "image_map_overlay_sat", [&] {
            apt::map::image_map_overlay_sat(j.stream, *j.map, r.sat, r.geom.yaw, r.geom.hscale, r.geom.vscale, colors,
                                            r.rotate, r.d_image, j.info);
        });
    } else {
        j.map->upload_track(j.stream, r.positions, r.n_positions);
        const apt::map::Scalars sc = apt::map::scalars(r.positions, r.n_positions, r.geom.yaw, r.geom.hscale, r.geom.vscale);
        launch_timed(plan, j.stream, "image_map_overlay", [&] {
            apt::map::image_map_overlay(j.stream, *j.map, sc, colors, count32(r.n_positions), r.rotate, r.d_image, j.info);
        });
    }
    stage_done(plan, "kernel launch (map overlay)");
}

// The track's x offsets and scalars in the job's map device, for a consumer that inverts the geometry (an overlay left
// them there; without one they are computed first).  Returns the host-fed form's scalars.
static apt::map::Scalars enqueue_image_track(aptgpu_plan *plan, const ImageRequest &q, const Recording &r,
                                             const ImageJob &j, const char *name)
{
    const bool sat = r.track == ImageRequest::Track::Sat;
    apt::map::Scalars sc{};
    if (!sat) sc = apt::map::scalars(r.positions, r.n_positions, r.geom.yaw, r.geom.hscale, r.geom.vscale);
    if (!q.overlay) {
        j.map->prepare_track(j.stream, j.cap / 2080u);
        launch_timed(plan, j.stream, name, [&] {
            if (sat) {
                apt::map::image_map_track_sat(j.stream, *j.map, r.sat, r.geom.yaw, r.geom.hscale, r.geom.vscale, j.info);
            } else {
                j.map->upload_track(j.stream, r.positions, r.n_positions);
                apt::map::image_map_track(j.stream, *j.map, sc, count32(r.n_positions), j.info);
            }
        });
    }
    return sc;
}

static void enqueue_image_project(aptgpu_plan *plan, const ImageRequest &q, const Recording &r, const ImageJob &j)
{
    const bool sat = r.track == ImageRequest::Track::Sat;
    const apt::map::Scalars sc = enqueue_image_track(plan, q, r, j, "image_project_track");
    j.project->upload_flags(j.stream, r.flags);
    launch_timed(plan, j.stream, "image_project", [&] {
        apt::project::image_project(j.stream, *j.project, *j.map, sat ? nullptr : &sc, r.grid, r.d_image, q.channels,
                                    r.d_out, r.out_cap, j.info);
    });
    if (q.png)
        launch_timed(plan, j.stream, "image_project_png", [&] {
            apt::project::image_project_png(j.stream, *j.project, r.grid, r.d_out, r.d_png, r.png_cap, j.info);
        });
    stage_done(plan, "kernel launch (reprojection)");
}

static void enqueue_image_png(aptgpu_plan *plan, const ImageRequest &q, const Recording &r, const ImageJob &j)
{
    const uint32_t rows = static_cast<uint32_t>(j.cap / 2080u);  // the launch grids cover the capacity
    if (rows == 0) return;
    launch_timed(plan, j.stream, "image_png_filter", [&] {
        apt::png::encode_filter(j.stream, r.d_image, 2080, rows, q.channels, j.png_ws, j.stream_cap, j.info);
    });
    launch_timed(plan, j.stream, "image_png_deflate", [&] {
        apt::png::encode_deflate(j.stream, 2080, rows, q.channels, j.png_ws, j.stream_cap, j.info);
    });
    launch_timed(plan, j.stream, "image_png_place", [&] {
        apt::png::encode_place(j.stream, 2080, rows, q.channels, j.png_ws, j.stream_cap, r.d_png, r.png_cap, j.info, nullptr);
    });
    stage_done(plan, "kernel launch (PNG encoder)");
}

// The composite of the request's passes: every pass's track stage on its own job's stream, the pass
// table through the composite's pinned staging buffer, then the one launch (and the PNG of the grid) on the first
// job's stream behind an event per pass that ran on another.
static void enqueue_image_composite(aptgpu_plan *plan, const ImageRequest &q, const ImageJob *jobs, int count)
{
    using apt::composite::Pass;
    apt::composite::Device &dev = *q.comp.dev;
    hipStream_t s = jobs[0].stream;
    const apt::project::Grid &g = q.rec[0].grid;
    Pass table[apt::composite::kMaxPasses] = {};
    for (int i = 0; i < count; ++i) {
        const Recording &r = q.rec[static_cast<size_t>(i)];
        const ImageJob &j = jobs[i];
        Pass &p = table[i];
        p.sc = enqueue_image_track(plan, q, r, j, "image_composite_track");
        p.scp = r.track == ImageRequest::Track::Sat ? j.map->scalars : nullptr;
        p.xoff = j.map->xoff;
        p.ctl = j.map->ctl;
        p.info = j.info;
        p.src = r.d_image;
        p.channels = r.channels;
        apt::composite::wait_for_pass(s, dev, i, j.stream);
    }
    dev.upload_table(s, table, count);
    dev.grid.upload_flags(s, q.rec[0].flags);
    launch_timed(plan, s, "image_composite", [&] {
        apt::composite::image_composite(s, dev, count, q.comp.blend, g, q.comp.d_out, q.comp.out_cap, q.comp.d_coverage);
    });
    if (q.png)
        launch_timed(plan, s, "image_composite_png", [&] {
            apt::project::image_project_png(s, dev.grid, g, q.comp.d_out, q.comp.d_png, q.comp.png_cap, dev.info);
        });
    stage_done(plan, "kernel launch (composite)");
}

void enqueue_image_outputs(aptgpu_plan *plan, const ImageRequest &q, const ImageJob *jobs, int count)
{
    auto each = [&](auto stage) {
        for (int i = 0; i < count; ++i) stage(plan, q, q.rec[static_cast<size_t>(i)], jobs[i]);
    };
    if (q.overlay) each(enqueue_image_overlay);
    if (q.composite)
        enqueue_image_composite(plan, q, jobs, count);
    else if (q.project)
        each(enqueue_image_project);
    else if (q.png)
        each(enqueue_image_png);
}

}  // namespace apt
