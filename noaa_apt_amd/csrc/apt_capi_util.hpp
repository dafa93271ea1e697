// apt_capi_util.hpp — helpers shared by the extern "C" translation units (apt_capi.hip,
// apt_capi_image.hip, the stream units): error mapping, the null-argument refusal, malloc'd outputs, context callbacks,
// a per-call stream, the readback of a stage's record (one-shot and plan), the buffer-overlap predicate.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>

#include "apt_kernels_track.hpp"
#include "apt_plan.hpp"
#include "apt_sat.hpp"

// the opaque layer-set handle of include/aptgpu.h (apt_capi_image.hip creates and fills it)
struct aptgpu_map_layers {
    apt::map::Layers layers;
    // the land mask's acceleration table of `layers` (apt_kernels_landmask.hpp), built on first use and again when the
    // layers' generation or the band count change; type-erased so that only the land mask's unit needs its header
    mutable std::shared_ptr<const void> land_table;
    mutable std::mutex land_mutex;
};

namespace apt::capi {

using apt::Error;
using apt::ErrorKind;

inline void put_err(char *err, size_t cap, const std::string &msg)
{
    if (err && cap) std::snprintf(err, cap, "%s", msg.c_str());
}

inline int fail(const Error &e, char *err, size_t cap)
{
    put_err(err, cap, e.message);
    return static_cast<int>(e.kind);
}

template <typename Fn>
int guarded(char *err, size_t cap, Fn &&fn)
{
    try {
        return fn();
    } catch (const Error &e) {
        return fail(e, err, cap);
    } catch (const std::bad_alloc &) {
        put_err(err, cap, "out of host memory");
        return APTGPU_ERR_INVALID;
    } catch (const std::exception &e) {
        put_err(err, cap, e.what());
        return APTGPU_ERR_INTERNAL;
    }
}

// the refusal of a null argument by the stream, fm-stream and iq-live entry points: "<who>: null argument"
inline int null_argument(char *err, size_t cap, const char *who)
{
    put_err(err, cap, std::string(who) + ": null argument");
    return APTGPU_ERR_INVALID;
}

inline size_t align256(size_t v) { return (v + 255u) & ~static_cast<size_t>(255u); }
// a caller's rows_cap as the kernels take it
inline uint32_t clamp_cap(size_t cap) { return cap > 0xFFFFFFFFu ? 0xFFFFFFFFu : static_cast<uint32_t>(cap); }

template <typename T>
T *host_alloc(size_t n)
{
    T *p = static_cast<T *>(std::malloc((n ? n : 1) * sizeof(T)));
    if (!p) throw std::bad_alloc();
    return p;
}

inline void status(const aptgpu_context *ctx, float progress, const std::string &text)
{
    if (ctx && ctx->status) ctx->status(progress, text.c_str(), ctx->user);
}

// Context::step through the C callback; a nonzero return aborts like `?` in the reference.
inline void step(const aptgpu_context *ctx, bool on, const char *id, int variant, const float *data,
          size_t n, uint32_t rate)
{
    if (!on || !ctx || !ctx->step) return;
    if (ctx->step(id, variant, data, n, rate, ctx->user) != 0)
        throw Error{ErrorKind::Internal, std::string("step callback failed at \"") + id + "\""};
}

// D2H into malloc'd memory, waited for: what the ABI hands out (aptgpu_free) and what a step callback reads
inline float *download_malloc(const float *d, size_t n, hipStream_t s)
{
    float *p = host_alloc<float>(n);
    if (n) {
        if (hipMemcpyAsync(p, d, n * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess) {
            std::free(p);
            throw Error{ErrorKind::Hip, "D2H copy failed"};
        }
    }
    return p;
}
// A malloc'd output until the call has everything it hands out: released into the out-parameters last.
struct HostFree {
    void operator()(void *p) const { std::free(p); }
};
template <typename T>
using HostPtr = std::unique_ptr<T, HostFree>;
using HostSignal = HostPtr<float>;

// One record of a one-shot call: copied behind everything on s, waited for.
template <typename T>
T read_record(hipStream_t s, const T *d)
{
    T r{};
    apt::hip_check(hipMemcpyAsync(&r, d, sizeof r, hipMemcpyDeviceToHost, s), "hipMemcpyAsync D2H");
    apt::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
    return r;
}

// The aptgpu_plan_*_results entry points: one record per recording of the first `count` of the last decode call, read
// once every stream of the plan is idle.  record_of(i): where recording i's record is in HBM (null: its stage never ran
// on that slot, which is refused before anything is waited for); publish(i, r): the record into results[i].
template <typename RecordOf, typename Publish>
int plan_results(aptgpu_plan *plan, int count, const void *results, RecordOf &&record_of, Publish &&publish)
{
    if (!plan || count < 0 || (!results && count)) return APTGPU_ERR_INVALID;
    if (static_cast<size_t>(count) > plan->last_slots.size()) return APTGPU_ERR_INVALID;
    for (int i = 0; i < count; ++i)
        if (!record_of(i)) return APTGPU_ERR_INVALID;
    try {
        apt::hip_check(hipSetDevice(plan->device), "hipSetDevice");
        plan->sync_all();
        for (int i = 0; i < count; ++i) {
            std::remove_cv_t<std::remove_pointer_t<decltype(record_of(i))>> r;
            apt::hip_check(hipMemcpy(&r, record_of(i), sizeof r, hipMemcpyDeviceToHost), "hipMemcpy");
            publish(i, r);
        }
    } catch (const Error &) {
        return APTGPU_ERR_HIP;
    }
    return APTGPU_OK;
}

// base .. base + bytes of two buffers overlap: the half-open ranges intersect, or the starts are equal (an empty range
// still has its place).  A null buffer overlaps nothing.
inline bool overlaps(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    if (!a0 || !b0) return false;
    return (a0 < b0 + b_bytes && b0 < a0 + a_bytes) || a0 == b0;
}
// ... with any rows buffer of a plan call: rows_cap[j] rows of 2080 floats at d_rows[j]
inline bool overlaps_rows(const void *p, size_t bytes, int count, const float *const *d_rows, const size_t *rows_cap)
{
    for (int j = 0; j < count; ++j)
        if (overlaps(p, bytes, d_rows[j], rows_cap[j] * 2080u * sizeof(float))) return true;
    return false;
}

// A signal that a step carries: in HBM (downloaded for the callback) or on the host already.
struct StepSignal {
    const float *dev = nullptr, *host = nullptr;
    uint64_t n = 0;
    static StepSignal device(const float *d, uint64_t n) { return {d, nullptr, n}; }
    static StepSignal on_host(const float *h, uint64_t n) { return {nullptr, h, n}; }
};

// Step::signal (context.rs) of such a signal
inline void step_signal(const aptgpu_context *ctx, hipStream_t s, const char *id, StepSignal x, uint32_t rate)
{
    if (!ctx || !ctx->step) return;
    HostSignal h(x.dev ? download_malloc(x.dev, x.n, s) : nullptr);
    step(ctx, true, id, 0, x.dev ? h.get() : x.host, x.n, rate);
}

struct Scratch {
    int device;
    hipStream_t stream = nullptr;
    bool own = false;
    explicit Scratch(const aptgpu_context *ctx) : device(ctx ? ctx->device : 0)
    {
        apt::hip_check(hipSetDevice(device), "hipSetDevice");
        if (ctx && ctx->stream) {
            stream = static_cast<hipStream_t>(ctx->stream);
        } else {
            apt::hip_check(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking),
                           "hipStreamCreate");
            own = true;
        }
    }
    ~Scratch()
    {
        if (own && stream) {
            (void)hipStreamSynchronize(stream);
            (void)hipStreamDestroy(stream);
        }
    }
    apt::DeviceBuffer<float> upload(const float *h, size_t n, size_t pad = 16)
    {
        apt::DeviceBuffer<float> d;
        d.alloc(n + pad);
        if (n)
            apt::hip_check(hipMemcpyAsync(d.ptr, h, n * sizeof(float), hipMemcpyHostToDevice, stream),
                           "hipMemcpyAsync H2D");
        return d;
    }
    float *download_malloc(const float *d, size_t n) { return apt::capi::download_malloc(d, n, stream); }
};

// The Context::step calls of one resample_with_filter stage, in the reference's order: "resample_filter" (dsp.rs:96 /
// :106), "resample_filtered" (l > 1: fast_resampling's expanded signal, empty unless export_resample_filtered,
// dsp.rs:269,281-285; l == 1: the filtered signal before its decimation, dsp.rs:108-114), "resample_decimated"
// (dsp.rs:100-104,118-122).  The only place that delivers them: decode()'s two stages and the WAV tool's come here.
//   x  the stage's input in HBM, from which one auxiliary launch computes the signal of "resample_filtered" — or, on
//      the host, that signal itself where the caller has it already (decode()'s sync branch: gather_rows writes the rows
//      as filter([1.]) leaves them)
//   y  the stage's output, in HBM or on the host
//   filter_steps  at l == 1 the reference's filter() also delivers "filter_filter" / "filter_result" (dsp.rs:407-408)
//      ahead of "resample_filtered".  Here only decode()'s final stage does; its first stage and the WAV tool never have
//      (a known deviation, pinned by test_first_resample_with_l_equal_1_delivers_the_filtered_signal and
//      test_resample_tool_steps_and_flag).  Passing true there is the whole correction.
inline void export_stage_steps(const aptgpu_context *ctx, hipStream_t s, const apt::ResampleStage &st, const apt::Signal &taps,
                               uint32_t in_hz, uint32_t out_hz, StepSignal x, StepSignal y, bool filter_steps)
{
    if (!ctx || !ctx->step) return;
    const apt::ResampleGeom &g = st.g;
    step(ctx, true, "resample_filter", 1, taps.data(), taps.size(), 0);
    HostSignal own;
    StepSignal filtered = StepSignal::on_host(x.host, x.host ? x.n : 0);  // (empty: l > 1 without the flag)
    if (x.dev && (g.l == 1 || g.flagged)) {
        const uint64_t count = g.expanded_len(x.n);
        auto compute = [&] {
            apt::DeviceBuffer<float> d_f;
            d_f.alloc(count + 16);
            st.enqueue_filtered(s, x.dev, x.n, d_f.ptr);
            own.reset(download_malloc(d_f.ptr, count, s));
            filtered = StepSignal::on_host(own.get(), count);
        };
        // The expanded signal is n * l floats (gigabytes for a whole pass) on the device and on the host.  Where either
        // allocation fails the step is delivered empty and the work goes on — the reference logs "Expanded filtered
        // signal can't fit in memory, skipping step" and does the same (dsp.rs:211-220).  Nothing of the caller's runs
        // inside the try: an exception from the step callback is the callback's.
        if (g.l > 1) {
            try {
                compute();
            } catch (const Error &e) {
                if (e.kind != ErrorKind::Hip || e.hip_code != static_cast<int>(hipErrorOutOfMemory)) throw;
                (void)hipGetLastError();
            } catch (const std::bad_alloc &) {
            }
            if (!own)
                std::fprintf(stderr, "aptgpu: expanded filtered signal (%llu samples) can't fit in memory, skipping step\n",
                             static_cast<unsigned long long>(count));
        } else {
            compute();
        }
    }
    if (g.l == 1 && filter_steps) {
        step(ctx, true, "filter_filter", 1, taps.data(), taps.size(), 0);
        step(ctx, true, "filter_result", 0, filtered.host, filtered.n, 0);
    }
    step(ctx, true, "resample_filtered", 0, filtered.host, filtered.n, g.filtered_rate(in_hz));
    step_signal(ctx, s, "resample_decimated", y, out_hz);
}

// resample_with_filter (dsp.rs:62-126) on a signal already in HBM; returns the output length.
// steps_ctx (nullable; used when it has a step callback): the stage's Context::step calls.  export_filtered:
// context.export_resample_filtered — the other decimation phase of fast_resampling (dsp.rs:265-273) and, with steps, the
// expanded signal.
inline uint64_t resample_device(Scratch &sc, const float *d_x, size_t n, uint32_t in_hz, uint32_t out_hz,
                                apt::Filter &filt, apt::DeviceBuffer<float> &d_y, bool export_filtered = false,
                                const aptgpu_context *steps_ctx = nullptr)
{
    if (out_hz == 0) throw Error{ErrorKind::Internal, "Can't resample to 0Hz"};  // dsp.rs:69-71
    const apt::Rate in_rate = apt::Rate::hz(in_hz), out_rate = apt::Rate::hz(out_hz);
    const apt::LM lm = apt::interpolation_factors(in_rate, out_rate);
    if (lm.l > 1) {
        apt::Rate interpolated{};
        if (!in_rate.checked_mul(lm.l, &interpolated)) {
            char buf[512];
            std::snprintf(buf, sizeof buf,
                          "Can't resample, looks like the sample rates do not have a big\n"
                          "                divisor in common. input_rate: %u, output_rate: %u, "
                          "l: %u, m: %u",
                          in_hz, out_hz, lm.l, lm.m);
            throw Error{ErrorKind::RateOverflow, buf};
        }
        filt.resample(in_rate, interpolated);
    }
    const apt::Signal coeff = filt.design();
    auto d_c = sc.upload(coeff.data(), coeff.size());
    const apt::ResampleStage st{{lm.l, lm.m, coeff.size(), export_filtered}, d_c.ptr};
    const uint64_t w = st.g.out_len(n);
    d_y.alloc(w + 16);
    st.enqueue(sc.stream, d_x, n, d_y.ptr, w);
    export_stage_steps(steps_ctx, sc.stream, st, coeff, in_hz, out_hz, StepSignal::device(d_x, n),
                       StepSignal::device(d_y.ptr, w), /*filter_steps*/ false);
    apt::hip_check(hipStreamSynchronize(sc.stream), "hipStreamSynchronize");  // d_c goes out of scope
    return w;
}

// One recording's aptgpu_orbit_settings after its checks: the initialised satellite and the reference time for the
// kernels, the map settings (null: no overlay) and Rotate::Orbit's outcome.
struct SatCall {
    apt::sat::TrackCall call;
    const aptgpu_map_settings *draw_map;
};

// The checks of aptgpu_orbit_settings, then parse + sgp4init (cached for the last TLE and name).
inline SatCall orbit_args(const aptgpu_orbit_settings *orbit)
{
    if (!orbit || orbit->struct_size < sizeof(aptgpu_orbit_settings))
        throw Error{ErrorKind::Invalid, "aptgpu_orbit_settings: struct_size not set"};
    if (orbit->flags) throw Error{ErrorKind::Invalid, "aptgpu_orbit_settings: unknown flags"};
    if (!orbit->sat_name) throw Error{ErrorKind::Invalid, "aptgpu_orbit_settings: sat_name not set"};
    if (orbit->ref_kind != APTGPU_REF_TIME_START && orbit->ref_kind != APTGPU_REF_TIME_END)
        throw Error{ErrorKind::Invalid, "aptgpu_orbit_settings: unknown ref_kind"};
    if (!orbit->tle)
        throw Error{ErrorKind::Unsupported,
                    "aptgpu_orbit_settings: tle is NULL (the reference then downloads the current TLE, "
                    "misc::get_current_tle; pass the text)"};
    if (orbit->draw_map && orbit->draw_map->struct_size < sizeof(aptgpu_map_settings))
        throw Error{ErrorKind::Invalid, "aptgpu_map_settings: struct_size not set"};
    SatCall c{};
    c.call.rec = apt::sat::satrec_for(orbit->tle, orbit->sat_name);
    c.call.ref_ms = orbit->ref_unix_ms;
    c.call.ref_is_end = orbit->ref_kind == APTGPU_REF_TIME_END;
    c.draw_map = orbit->draw_map;
    return c;
}

// decode()'s own errors (decode.rs:79-83,112-118,172-176)
inline constexpr const char *kTooShort = "Got less than 10 rows of samples, audio file is too short";
inline constexpr const char *kFewSync = "Found less than 5 sync frames, audio file is too short or too noisy";
inline constexpr const char *kNotMultiple = "work_rate is not multiple of FINAL_RATE";

// apt_capi_decode.hip
int decode_host(const aptgpu_context *ctx_in, const aptgpu_settings *settings, const float *signal,
                const uint8_t *wav_data, const apt::WavInfo *wav, size_t n, uint32_t input_rate_hz, int sync,
                float **rows_out, size_t *n_out, aptgpu_stats *stats, char *err, size_t err_cap);

}  // namespace apt::capi
