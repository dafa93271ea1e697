// apt_capi_decode.hip — decode() on a host buffer (aptgpu_decode, aptgpu_decode_wav): where the plan and the buffers
// come from, the upload and the launch, the status and step narration in the reference's order, the rows and stats.
// No exception crosses the ABI; apt::Error maps to status code + message.
#include <cstdlib>
#include <memory>
#include <string>

#include "apt_capi_util.hpp"
#include "apt_session.hpp"

using namespace apt::capi;

namespace apt::capi {

namespace {

// What one decode() call runs on: the plan (designed taps, HBM workspace, streams) and the device input / output
// buffers.  They come from the process-wide session cache (apt_session.hpp; SURVEY.md §8(b), threading row) unless the
// caller wants the step export (unfused kernels, every intermediate kept) or runs on a stream of their own: building
// and tearing them down cost 2 ms per call, as much as the PCIe time of a ten-minute recording.
struct DecodeRun {
    SessionLease lease;
    std::unique_ptr<aptgpu_plan, PlanDeleter> own_plan;
    apt::DeviceBuffer<uint8_t> own_in;
    apt::DeviceBuffer<float> own_rows;
    aptgpu_plan *plan = nullptr;
    void *d_in = nullptr;
    float *d_rows = nullptr;
    uint64_t rows_cap = 0;
    bool ok = false;  // a session that an exception left half-way through a call is not reused
    ~DecodeRun() { if (!ok && lease) lease.poison(); }

    // (not the constructor: a failure in here poisons a session already leased, like any other)
    void acquire(const aptgpu_context &ctx, const aptgpu_settings &settings, uint32_t input_rate_hz, bool sync, size_t n,
                 size_t in_bytes, bool cached)
    {
        if (cached) {
            lease = session_acquire(SessionKey::of_decode(ctx.device, ctx.mode, input_rate_hz, sync, 1, 1, settings), n);
            plan = lease->plan.get();
        } else {
            own_plan.reset(apt::plan_create(&ctx, settings, input_rate_hz, sync, n, 1, /*depth*/ 1));
            plan = own_plan.get();
        }
        if (plan->spr == 0) throw Error{ErrorKind::Invalid, "work_rate too small"};
        rows_cap = plan->rows_bound(n);
        if (cached) {
            lease->ensure_set(0, in_bytes + 64, rows_cap);
            d_in = lease->sets[0].in[0].ptr;
            d_rows = lease->sets[0].out[0].ptr;
        } else {
            own_in.alloc(in_bytes + 64);
            own_rows.alloc(rows_cap);
            d_in = own_in.ptr;
            d_rows = own_rows.ptr;
        }
    }
    // decode()'s own per-recording errors (decode.rs:79-83,112-118,172-176) leave the GPU state perfectly valid: wait
    // for what the call enqueued and hand the session back to the cache — only a HIP failure or an unknown exception
    // poisons it
    Error decode_error(const char *msg)
    {
        if (hipStreamSynchronize(plan->stream) == hipSuccess) ok = true;
        return Error{ErrorKind::Internal, msg};
    }
};

// H2D of the recording and the whole decode() behind it, on the plan's one stream (streams[0] == stream).  Returns the
// recording as the first stage reads it: the f32 Signal in HBM.
const float *upload_and_run(DecodeRun &r, const void *host, size_t in_bytes, aptgpu_plan::Input in, bool steps)
{
    aptgpu_plan *plan = r.plan;
    if (in_bytes)
        apt::hip_check(hipMemcpyAsync(r.d_in, host, in_bytes, hipMemcpyHostToDevice, plan->stream), "hipMemcpyAsync H2D");
    in.ptr = r.d_in;
    const uint64_t cap = r.rows_cap;
    plan->run_call(1, &in, &r.d_rows, &cap, steps);
    if (!steps) return nullptr;  // (nobody reads it)
    plan->sync_all();  // the step exports read the slot's buffers
    // (... F among them, as one contiguous signal: run_call's unfused kernels leave it so, never a k_fused launch)
    if (plan->slot_of(0).f_stride != 0) throw Error{ErrorKind::Internal, "step export: F is in pixel-phase planes"};
    return in.codec >= 0 ? plan->slot_of(0).ingest.ptr : static_cast<const float *>(r.d_in);
}

// decode.rs:59-63: the "input" step and the first status
void narrate_input(const aptgpu_context *ctx, const aptgpu_context *steps_ctx, hipStream_t s, StepSignal x,
                   uint32_t input_rate_hz, uint32_t work_rate)
{
    step_signal(steps_ctx, s, "input", x, input_rate_hz);
    status(ctx, 0.1f, "Resampling to " + std::to_string(work_rate));
}

void read_result(aptgpu_plan *plan, aptgpu_result *res)
{
    if (aptgpu_plan_results(plan, 1, res) != APTGPU_OK) throw Error{ErrorKind::Hip, "could not read the result record"};
}

// decode.rs:65-159 as the caller sees it: every status, and (steps_ctx != null) every Context::step, in the reference's
// order, over what run_call left in the slot; d_x: the recording in HBM (steps only).  Fills *res.
void narrate(const aptgpu_context *ctx, const aptgpu_context *steps_ctx, DecodeRun &r, const float *d_x, size_t n,
             uint32_t input_rate_hz, bool sync, aptgpu_result *res)
{
    aptgpu_plan *plan = r.plan;
    hipStream_t s = plan->stream;
    aptgpu_plan::Slot &sl = plan->slot_of(0);
    const uint32_t work = plan->settings.work_rate;
    const uint64_t w = plan->work_len_for(n);
    if (w < 10ull * plan->spr) {  // decode.rs:79-83 (run_call resampled nothing: of the stage's steps, the filter alone)
        step(steps_ctx, true, "resample_filter", 1, plan->taps_resample.data(), plan->taps_resample.size(), 0);
        throw r.decode_error(kTooShort);
    }
    export_stage_steps(steps_ctx, s, plan->first_stage(), plan->taps_resample, input_rate_hz, work, StepSignal::device(d_x, n),
                       StepSignal::device(sl.resampled.ptr, w), /*filter_steps*/ false);
    status(ctx, 0.4f, "Demodulating");  // decode.rs:87
    step_signal(steps_ctx, s, "demodulation_result", StepSignal::device(sl.demodulated.ptr, w), 0);
    status(ctx, 0.42f, "Filtering");  // decode.rs:93
    step(steps_ctx, true, "filter_filter", 1, plan->taps_lowpass.data(), plan->taps_lowpass.size(), 0);
    const HostSignal filtered(steps_ctx ? download_malloc(sl.filtered.ptr, w, s) : nullptr);
    step(steps_ctx, true, "filter_result", 0, filtered.get(), w, 0);

    // the input of the final resample_with_filter(NoFilter) (decode.rs:158-159), as export_stage_steps takes it
    StepSignal final_in;
    apt::DeviceBuffer<float> d_al;
    HostSignal al;
    if (sync) {
        status(ctx, 0.5f, "Syncing");  // decode.rs:107
        if (!plan->work_is_multiple) throw r.decode_error(kNotMultiple);
        step_signal(steps_ctx, s, "sync_correlation", StepSignal::device(sl.correlation.ptr, w - plan->n_sync_taps), 0);
        read_result(plan, res);
        if (res->n_sync < 5) throw r.decode_error(kFewSync);  // decode.rs:112-118
        if (steps_ctx) {
            // "sync_result": the aligned rows at work_rate (decode.rs:150); then the same rows as filter([1.]) leaves them
            // (0.0 + x*1.0, and nothing at all for sample 0: the `i > j` guard), the l == 1 branch of the final stage
            const uint64_t count = static_cast<uint64_t>(res->n_rows) * plan->spr;
            d_al.alloc(count + 16);
            apt::gpu::gather_rows(s, sl.filtered.ptr, sl.peaks.ptr, plan->result_of(0), plan->spr, 1, true, d_al.ptr, res->n_rows);
            step_signal(steps_ctx, s, "sync_result", StepSignal::device(d_al.ptr, count), work);
            apt::gpu::gather_rows(s, sl.filtered.ptr, sl.peaks.ptr, plan->result_of(0), plan->spr, 1, false, d_al.ptr, res->n_rows);
            al.reset(download_malloc(d_al.ptr, count, s));
            final_in = StepSignal::on_host(al.get(), count);
        }
    } else {
        status(ctx, 0.5f, "Skipping Syncing");  // decode.rs:136
        step(steps_ctx, true, "sync_correlation", 0, nullptr, 0, work);  // decode.rs:139
        read_result(plan, res);
        final_in = StepSignal::device(sl.filtered.ptr, plan->whole_rows(w));
        step(steps_ctx, true, "sync_result", 0, filtered.get(), final_in.n, work);
    }
    status(ctx, 0.90f, "Resampling to 4160");  // decode.rs:154
    if (res->status != APTGPU_OK)
        throw r.decode_error(res->reason == 2 ? kFewSync : res->reason == 3 ? kNotMultiple : kTooShort);
    export_stage_steps(steps_ctx, s, plan->final_stage(), apt::Signal{1.f}, work, apt::FINAL_RATE, final_in,
                       StepSignal::device(r.d_rows, res->n_out), /*filter_steps*/ true);
}

// the rows on the host (malloc'd: the caller's) and the call's stats
void collect(DecodeRun &r, const aptgpu_result &res, size_t n, float **rows_out, size_t *n_out, aptgpu_stats *stats)
{
    const aptgpu_plan *plan = r.plan;
    *rows_out = download_malloc(r.d_rows, res.n_out, plan->stream);
    *n_out = res.n_out;
    if (!stats) return;
    stats->work_len = plan->work_len_for(n);
    stats->n_sync = res.n_sync;
    stats->n_rows = res.n_rows;
    stats->l = plan->l;
    stats->m = plan->m;
    stats->n_resample_taps = static_cast<uint32_t>(plan->taps_resample.size());
    stats->n_lowpass_taps = static_cast<uint32_t>(plan->taps_lowpass.size());
    stats->fused = plan->fused();
    stats->orbit_path = 1;
}

}  // namespace

// decode() on a host buffer: the f32 Signal, or (wav != nullptr) the payload of a WAV data chunk
// that is uploaded as it is and converted on the device (wav.rs:30-51).
int decode_host(const aptgpu_context *ctx_in, const aptgpu_settings *settings, const float *signal,
                const uint8_t *wav_data, const apt::WavInfo *wav, size_t n, uint32_t input_rate_hz, int sync,
                float **rows_out, size_t *n_out, aptgpu_stats *stats, char *err, size_t err_cap)
{
    *rows_out = nullptr;
    *n_out = 0;
    const aptgpu_context ctx = ctx_in ? *ctx_in : aptgpu_context{};
    const bool steps = settings->export_wav != 0 && ctx.step != nullptr;
    const aptgpu_context *steps_ctx = steps ? &ctx : nullptr;

    return guarded(err, err_cap, [&]() -> int {
        // a WAV input is exported after its conversion on the device
        const bool input_from_device = wav && steps;
        if (!input_from_device)
            narrate_input(&ctx, steps_ctx, nullptr, StepSignal::on_host(signal, n), input_rate_hz, settings->work_rate);
        const size_t in_bytes = wav ? wav->data_len : n * sizeof(float);
        DecodeRun r;
        r.acquire(ctx, *settings, input_rate_hz, sync != 0, n, in_bytes, /*cached*/ !steps && ctx.stream == nullptr);
        const aptgpu_plan::Input in = wav ? aptgpu_plan::Input::wav(nullptr, n, *wav) : aptgpu_plan::Input{nullptr, n};
        const float *d_x = upload_and_run(r, wav ? static_cast<const void *>(wav_data) : signal, in_bytes, in, steps);
        if (input_from_device)
            narrate_input(&ctx, steps_ctx, r.plan->stream, StepSignal::device(d_x, n), input_rate_hz, settings->work_rate);
        aptgpu_result res{};
        narrate(&ctx, steps_ctx, r, d_x, n, input_rate_hz, sync != 0, &res);
        collect(r, res, n, rows_out, n_out, stats);
        r.ok = true;
        return APTGPU_OK;
    });
}

}  // namespace apt::capi

extern "C" {

int aptgpu_decode(const aptgpu_context *ctx_in, const aptgpu_settings *settings,
                  const float *signal, size_t n, uint32_t input_rate_hz, int sync,
                  float **rows_out, size_t *n_out, aptgpu_stats *stats, char *err, size_t err_cap)
{
    if (!settings || (!signal && n) || !rows_out || !n_out) {
        put_err(err, err_cap, "null argument");
        return APTGPU_ERR_INVALID;
    }
    return apt::capi::decode_host(ctx_in, settings, signal, nullptr, nullptr, n, input_rate_hz, sync, rows_out,
                                  n_out, stats, err, err_cap);
}

}  // extern "C"
