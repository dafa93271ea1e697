/*
 * aptgpu.h — C ABI of libaptgpu.so: the MI355X (gfx950) implementation of
 * martinber/noaa-apt's signal-to-image hot path, i.e. the body of
 * noaa_apt::decode()  (reference: src/decode.rs:43-162, re-exported at
 * src/noaa_apt.rs:5) and the dsp.rs / filters.rs functions it calls.
 *
 * This is the drop-in boundary: plain C types, plain pointers and sizes, no
 * C++/torch types.  A Rust `extern "C"` block binds exactly these symbols
 * (see INTEGRATION.md for the shim that gives them the reference's Rust
 * signatures).  Every entry point names the reference interface it replaces.
 *
 * Conventions
 *  - all functions return an APTGPU_* status code; on error `err` (if given)
 *    receives the same message string the reference puts in its err::Error.
 *  - "host" pointers are ordinary process memory; "d_" pointers are device
 *    (HBM) memory on the plan's GPU.
 *  - thread-safe and re-entrant; a plan must not be used from two threads at
 *    once (make one plan per thread / per stream).  The only process-global
 *    mutable state is the mutex-guarded session cache behind the host-array
 *    entry points (aptgpu_cache_clear / aptgpu_cache_info) and per-device
 *    caches of kernel attributes and of the envelope's divide check.
 *  - numerics: f32 throughout, every product and sum rounded separately and
 *    accumulated in the reference's order, so outputs are bit-identical to
 *    the reference's scalar loops (APTGPU_MODE_STRICT, the default).
 */
#ifndef APTGPU_H
#define APTGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------ */
#define APTGPU_OK 0
#define APTGPU_ERR_INTERNAL 1      /* err::Error::Internal(String)      src/err.rs:27   */
#define APTGPU_ERR_RATE_OVERFLOW 2 /* err::Error::RateOverflow(String)  src/err.rs:31   */
#define APTGPU_ERR_HIP 3           /* HIP runtime / device failure (Rust shim: Internal) */
#define APTGPU_ERR_INVALID 4       /* FFI misuse: null pointer, capacity too small, ...  */
#define APTGPU_ERR_UNSUPPORTED 5   /* reference feature not offered on the GPU path      */
#define APTGPU_ERR_WAV_OPEN 6      /* err::Error::WavOpen(String)       src/err.rs:14   */
#define APTGPU_ERR_IO 7            /* err::Error::Io(std::io::Error)    src/err.rs:11   */

/* ---- filters (src/filters.rs:22-46) ------------------------------------ */
#define APTGPU_FILTER_NOFILTER 0          /* filters::NoFilter          */
#define APTGPU_FILTER_LOWPASS 1           /* filters::Lowpass           */
#define APTGPU_FILTER_LOWPASS_DC_REMOVAL 2 /* filters::LowpassDcRemoval */

/* A `impl filters::Filter` value: frequencies are Freq.pi_rad (fractions of
 * pi rad/sample, src/frequency.rs:30-32), atten in positive dB. */
typedef struct aptgpu_filter {
    int32_t kind;
    float cutout_pi_rad;
    float atten;
    float delta_w_pi_rad;
} aptgpu_filter;

/* ---- config::Settings, the fields decode() reads (src/config.rs:76-106;
 *      read at src/decode.rs:55,57,68,70,75,98) ---------------------------- */
typedef struct aptgpu_settings {
    uint32_t work_rate;         /* Hz, intermediate processing rate            */
    float resample_atten;       /* dB                                          */
    float resample_delta_freq;  /* Hz                                          */
    float resample_cutout;      /* Hz                                          */
    float demodulation_atten;   /* dB                                          */
    int32_t export_wav;         /* Settings.export_wav: deliver steps via step */
    int32_t export_resample_filtered; /* Settings.export_resample_filtered (src/config.rs:83 ->
                                   context.rs:113).  As in the reference it moves the decimation
                                   phase of fast_resampling (src/dsp.rs:265-273) -- other rows,
                                   exported or not -- and with export_wav the "resample_filtered"
                                   step carries the expanded signal (n*l floats).  Served by the
                                   unfused kernels: a debugging aid, not a fast path            */
} aptgpu_settings;

/* ---- context::Context (src/context.rs:100-133) -------------------------- */
/* Context::status(progress, description)  src/context.rs:127-129 */
typedef void (*aptgpu_status_fn)(float progress, const char *description, void *user);
/* Context::step(Step{id, variant, data, rate})  src/context.rs:132-211.
 * variant: 0 = Variant::Signal, 1 = Variant::Filter; rate_hz 0 = None.
 * `data` is host memory valid only during the call.  Return nonzero to abort
 * the decode with APTGPU_ERR_INTERNAL (the reference propagates step errors). */
typedef int (*aptgpu_step_fn)(const char *id, int variant, const float *data, size_t n,
                              uint32_t rate_hz, void *user);

typedef struct aptgpu_context {
    aptgpu_status_fn status; /* nullable */
    aptgpu_step_fn step;     /* nullable; only called when settings.export_wav != 0 */
    void *user;
    int32_t device;          /* HIP device ordinal */
    int32_t mode;            /* APTGPU_MODE_* */
    void *stream;            /* hipStream_t to run on, NULL = the plan's own stream */
} aptgpu_context;

#define APTGPU_MODE_STRICT 0 /* bit-exact with the reference's f32 loops; fused kernels when
                                the (L, M, taps) combination has a specialisation          */
#define APTGPU_MODE_GENERIC 1 /* force the unfused generic kernels (any rate combination)   */
#define APTGPU_MODE_FP16_TAPS 2 /* first resample with fp16 taps + fp16 samples through
                                   v_dot2_f32_f16, f32 accumulate (BASELINE.json config 5).  NOT
                                   bit-exact: pixels within ~2e-3 of the row peak (of the peak, not
                                   of the pixel: the error does not shrink with the pixel's own
                                   value; measured 2.2e-4 max / 3.9e-5 rms of the signal's peak), sync positions unchanged on
                                   APT data; every other stage as in STRICT.  Input domain: the
                                   samples are converted to fp16 UNSCALED (only the taps are
                                   prescaled) — 16-bit PCM and +-1 float data fit, a sample beyond
                                   +-65504 becomes an infinity, and samples below 6.1e-5 in
                                   magnitude fall into fp16's subnormals and lose precision      */
#define APTGPU_MODE_FAST 3 /* f32 throughout with the same taps in the same order, but fused
                              multiply-adds in the two FIR stages, the native square root and a
                              reciprocal multiplication in the envelope, and the +-1 sync correlation
                              evaluated from pulse sums: about a third of the strict arithmetic.  NOT
                              bit-exact, deterministic; tolerance (enforced by the tests):
                              same row count, sync positions identical for >= 99.9 % of the rows and
                              never off by more than one work-rate sample, |d px| <= 1e-4 * max|px| on
                              rows with identical position.  Rates / profiles without a fast kernel
                              are served by the strict kernels.  With a user-tuned resample filter (a
                              tap count other than the stock profiles') at 48 / 96 kHz the resampler
                              runs on the matrix cores from bf16 pieces of the f32 taps (three: exact)
                              and samples (two truncated planes: exact for samples of at most 16
                              significant bits, the remainder of any other sample is dropped), f32
                              accumulation: the same tolerance (measured 5e-7 of full scale on 16-bit
                              data, 1.3e-5 max / 3.7e-6 rms on full-mantissa f32 samples). */

/* What find_sync()/decode() learned; the reference only logs it
 * (`info!("Found {} sync frames")` src/decode.rs:260). */
typedef struct aptgpu_stats {
    uint64_t work_len;      /* samples after the first resample                 */
    uint64_t n_sync;        /* peaks.len() of find_sync (0 when sync == 0)      */
    uint64_t n_rows;        /* image rows returned                              */
    uint32_t l, m;          /* interpolation / decimation factors dsp.rs:73-75  */
    uint32_t n_resample_taps, n_lowpass_taps;
    int32_t fused;          /* front end used: 0 unfused generic kernels, 1 compile-time
                               specialised fused kernel, 2 run-time fused kernel, 3 table-driven
                               stage 1 in front of the specialised work-rate stages (11 025 Hz),
                               4 phase-resident taps in stage 1, same work-rate stages (44 100 Hz) */
    int32_t orbit_path;     /* peak-picker path: 0 doubling (LDS), 1 bitmask walk */
} aptgpu_stats;

/* ====================================================================== */
/* 1. decode()                                                             */
/* ====================================================================== */

/* Replaces  pub fn decode(context: &mut Context, settings: &config::Settings,
 *                         signal: &Signal, input_rate: Rate, sync: bool)
 *                         -> err::Result<Signal>        src/decode.rs:43-49
 * signal: host f32 samples exactly as wav::load_wav produces them (unscaled,
 * first channel; src/wav.rs:30-51).  On success *rows_out is a malloc'd
 * buffer of *n_out = rows*2080 floats (release with aptgpu_free).
 * Errors and their messages are the reference's (src/decode.rs:79-83,112-118,
 * 172-176; src/dsp.rs:69-71,82-91). */
int aptgpu_decode(const aptgpu_context *ctx, const aptgpu_settings *settings,
                  const float *signal, size_t n, uint32_t input_rate_hz, int sync,
                  float **rows_out, size_t *n_out, aptgpu_stats *stats /* nullable */,
                  char *err, size_t err_cap);

/* Releases any buffer this library returned (Vec<f32> drop). */
void aptgpu_free(void *p);

/* The host-array entry points (aptgpu_decode, aptgpu_decode_wav, aptgpu_decode_batch[_wav]) keep what a call
 * needs on the device between calls — the plan (designed taps, HBM workspace, streams), input / output buffers,
 * pinned staging — in a process-wide, mutex-guarded, least-recently-used cache keyed by (device, the five
 * settings decode() reads, input rate, sync, mode, recordings per call): SURVEY.md section 8(b), threading
 * row.  A cached session serves one call at a time (concurrent callers with the same key each get their own);
 * at most 8 idle sessions / APTGPU_SESSION_CACHE_MB (default: a quarter of the device's memory; 0 = no caching)
 * of device memory are kept, and a session that cannot be built for lack of device memory empties the cache and
 * tries once more.  Calls that export steps or run on a caller's stream do not use it.
 * aptgpu_cache_clear() releases every idle session; aptgpu_cache_info() reports what is idle. */
void aptgpu_cache_clear(void);
void aptgpu_cache_info(int32_t *entries /* nullable */, uint64_t *device_bytes /* nullable */);

/* ====================================================================== */
/* 2. plans: device-resident and batched decode                            */
/* ====================================================================== */

/* A plan owns the designed taps, the HBM workspace and a stream for decode()
 * calls of one (settings, input_rate, sync) combination on one GPU.  It is
 * what a long-running caller (GUI worker thread src/gui/work.rs:174-197, or a
 * batch driver over independent recordings) keeps between calls. */
typedef struct aptgpu_plan aptgpu_plan;

typedef struct aptgpu_plan_info {
    uint32_t l, m;
    uint32_t n_resample_taps, n_lowpass_taps, n_sync_taps;
    uint32_t samples_per_work_row; /* PX_PER_ROW * work_rate / FINAL_RATE  decode.rs:55 */
    uint32_t min_distance;         /* samples_per_work_row * 8 / 10        decode.rs:216 */
    uint64_t max_samples;          /* capacity the plan was created for                  */
    uint64_t max_work_len;         /* work-rate samples at max_samples                   */
    uint64_t max_rows;             /* upper bound on rows for max_samples                */
    int32_t fused;                 /* front end: 0 unfused, 1 specialised fused, 2 run-time fused,
                                      3 table-driven / 4 phase-resident stage 1 + specialised
                                      work-rate stages */
    int32_t max_batch;
} aptgpu_plan_info;

/* Result record the device fills per recording (also readable from the host
 * with aptgpu_plan_results). */
typedef struct aptgpu_result {
    int32_t status;    /* APTGPU_OK, or APTGPU_ERR_INTERNAL (<10 rows / <5 sync frames) */
    int32_t reason;    /* 0 ok, 1 "<10 rows", 2 "<5 sync frames", 3 work_rate not a multiple of
                          4160, 4 ok but rows truncated to the caller's rows_cap; -1 while the
                          recording's kernels have not finished                              */
    uint32_t n_rows;   /* image rows written (n_out / 2080 when sync != 0; never more than rows_cap) */
    uint32_t n_sync;   /* peaks.len() of find_sync, 0 when sync == 0                         */
    uint64_t work_len; /* samples after the first resample                                   */
    uint64_t n_out;    /* floats written to d_rows                                           */
} aptgpu_result;

int aptgpu_plan_create(const aptgpu_context *ctx, const aptgpu_settings *settings,
                       uint32_t input_rate_hz, int sync, size_t max_samples, int max_batch,
                       aptgpu_plan **plan_out, char *err, size_t err_cap);
void aptgpu_plan_destroy(aptgpu_plan *plan);
int aptgpu_plan_get_info(const aptgpu_plan *plan, aptgpu_plan_info *info);

/* Enqueue decode() of `count` independent recordings already resident in HBM.
 * d_signals[i] points to n[i] device floats; d_rows[i] receives up to
 * rows_cap[i]*2080 device floats.  Asynchronous, no host synchronisation.
 * The recordings of one call go through ONE launch per stage (front end, sync words, sync slots, orbit,
 * row gather), in order on one of the plan's `depth` internal streams; consecutive calls go round-robin
 * over those streams (depth = 3 for plans created with max_batch >= 4, else 6; APTGPU_STREAMS overrides),
 * so the front end of call j+1 overlaps the latency-bound peak picker and the row gather of call j.
 * Stream k owns the workspace slots [k*max_batch, (k+1)*max_batch) — depth*max_batch slots in all — and a
 * slot is only reused by a later call on its own stream.  Plans with max_batch >= 4 (and no ctx.stream)
 * additionally order the front end of call j+1 behind the front end of call j with an event, so that each
 * front end has the whole GPU.  If
 * ctx.stream was given at plan creation the work is ordered AFTER what is
 * already enqueued on ctx.stream (inputs may be produced there); to order
 * ctx.stream after the decode, call aptgpu_plan_join().  Recordings of different
 * calls run on different internal streams: a call that reuses the output buffers of
 * an earlier call is only ordered after it if aptgpu_plan_join() / _synchronize() /
 * _results() came in between.  Outcome per recording lands in the plan's result
 * records. */
int aptgpu_plan_decode_device(aptgpu_plan *plan, int count, const float *const *d_signals,
                              const size_t *n, float *const *d_rows, const size_t *rows_cap,
                              char *err, size_t err_cap);
/* Waits for the stream and copies the `count` result records to the host. */
int aptgpu_plan_results(aptgpu_plan *plan, int count, aptgpu_result *results);
/* Sync-frame positions found by the last decode of recording i (find_sync()'s
 * return value, src/decode.rs:262); writes min(cap, n_sync) entries. */
int aptgpu_plan_sync_positions(aptgpu_plan *plan, int i, uint64_t *pos, size_t cap,
                               size_t *n_sync);
int aptgpu_plan_synchronize(aptgpu_plan *plan);
/* Makes ctx.stream wait, on the device, for everything the plan has enqueued
 * so far (host does not block).  Without a ctx.stream: same as synchronize. */
int aptgpu_plan_join(aptgpu_plan *plan);

/* Kernel timing with HIP events recorded on the plan's stream.  on = 0: off;
 * 1: the dominant (first-stage) kernel of every 8th decode is bracketed (sampling keeps the
 * markers, which serialise the stream, cheap); 2: every
 * kernel launch is.  Enable, run decodes, then collect: averages are over all
 * bracketed launches since the last collect. */
typedef struct aptgpu_kernel_time {
    char name[48];
    double avg_ms;
    uint64_t launches;
} aptgpu_kernel_time;
int aptgpu_plan_enable_timing(aptgpu_plan *plan, int on);
int aptgpu_plan_collect_timing(aptgpu_plan *plan, aptgpu_kernel_time *out, size_t cap,
                               size_t *n_out);

/* Introspection: copies one of the plan's internal HBM buffers of recording slot i to the
 * host after synchronising — the device-side counterpart of the intermediate signals the
 * reference exports through Context::step (src/context.rs:132-211).  Names: "filtered"
 * (f32, "filter_result"), "correlation" (f32, "sync_correlation"), "group_max" (f32, maxima
 * of the correlation over groups of 52 positions), "terminal_words" (u64), "peaks" (u32,
 * find_sync positions), "picker_flags" (u32[32]: [0] list overflow, [1] 1 = sequential
 * fallback ran, [8..] cycle stamps of the picker kernels), "eqfloat_thresholds" (u32[2][255]: the
 * sorted threshold keys T_1..T_255 of half A, then of half B, of the slot's last
 * APTGPU_CONTRAST_HISTOGRAM_FLOAT image; size 0 before the first one).  Writes min(bytes, size) bytes
 * and returns the buffer's size in *size_out.  Two names are host-side constants with no device copy:
 * "inv_sinphi" (f32) and "fused_variant" (chars, not NUL-terminated: the row name in
 * csrc/apt_kernels_fused_variants.hpp of the front-end kernel the slot's last decode launched, with "_f32" or
 * "_i16" appended for its input type; size 0 where k_fused_any or the unfused kernels ran). */
int aptgpu_plan_read_internal(aptgpu_plan *plan, int i, const char *name, void *host_out,
                              size_t bytes, size_t *size_out);

/* ====================================================================== */
/* 2b. host-fed batch decode over one or more GPUs                          */
/* ====================================================================== */
/* The batch variant of decode(): what a driver that loops `load(); decode();` over many recordings
 * (the reference's CLI does it for one, src/main.rs:102-104) binds instead of the loop.  Recordings are
 * independent, so they are sharded over `devices` (ordinals, repeats allowed: {0, 0} = two workers on
 * GPU 0; n_devices == 0 = ctx->device) longest-first onto the least loaded entry, with NO collective of
 * any kind; every entry gets a host thread and a cached session (plan, device buffers, copy streams) and keeps
 * the uploads of calls k+1 / k+2, the kernels of call k and the download of call k-1 in flight together
 * (recordings_per_call recordings per call, <= 0 = 16); rows are DMA'd straight into the returned buffers.
 * Every worker thread pins itself to the CPUs of its GPU's NUMA node first (sysfs: the device's numa_node and
 * that node's cpulist; APTGPU_NUMA_PIN=0 turns it off), so the buffers it allocates and the staging copies it
 * drives stay on the socket the GPU hangs off.  (Throughput figures: DESIGN.md section 7, profiles/.)  All
 * recordings of a batch share (settings, input_rate_hz, sync); ctx supplies mode (and the device when
 * n_devices == 0), callbacks are not used.
 *   rows_out[i] / n_out[i]: malloc'd rows of recording i (aptgpu_free), NULL / 0 when status[i] != 0;
 *   status[i]: APTGPU_OK, or the error decode() would have returned for that recording
 *              (APTGPU_ERR_INTERNAL: too short / too few sync frames; for WAV images also the
 *              reference's WAV errors, and APTGPU_ERR_INVALID for a rate other than input_rate_hz);
 *   results[i] (nullable): the device-side record (rows, sync frames found, work length).
 * Returns APTGPU_OK when every worker ran (per-recording failures are in status[]), else the first
 * worker-level error (HIP failure, bad argument).  Host buffers may be pageable; pinned ones
 * (aptgpu_host_alloc) are DMA'd directly. */
/* ABI note (0.2.0): `struct_size` is the caller's sizeof(aptgpu_batch_stats), set BEFORE the call; the library fills
 * at most that many bytes, so a caller built against this header keeps working when fields are appended.  A
 * struct_size below 8 (a zero-initialised struct; the bytes a 0.1.0 caller's `double seconds` starts with) is refused
 * with APTGPU_ERR_INVALID before anything runs.  The struct had no such field in 0.1.0 and grew twice: a binding
 * checks aptgpu_abi_version() at load time. */
typedef struct aptgpu_batch_stats {
    uint32_t struct_size;  /* in: sizeof(aptgpu_batch_stats) as the caller was compiled              */
    uint32_t reserved;
    double seconds;        /* wall time of the whole call                                   */
    uint64_t samples;      /* input samples of the recordings that were handed to a worker  */
    uint64_t h2d_bytes, d2h_bytes;
    double h2d_seconds;    /* host time inside the H2D copy calls, summed over the workers  */
    double d2h_seconds;
    int32_t workers;
    int32_t recordings_per_call;
    double gate_wait_seconds; /* summed over the workers: time spent waiting for the per-device upload gate    */
    double setup_seconds;     /* summed: leasing (or building) the session and sizing its buffers, before the
                                 first upload — a session built inside the call shows here                      */
    int32_t sessions_created; /* sessions that were not in the cache (0 in a warmed-up process)                 */
    int32_t workers_pinned;   /* workers that found their GPU's NUMA node and pinned themselves to its CPUs     */
} aptgpu_batch_stats;

int aptgpu_decode_batch(const aptgpu_context *ctx, const aptgpu_settings *settings,
                        uint32_t input_rate_hz, int sync, int count, const float *const *signals,
                        const size_t *n, const int32_t *devices, int n_devices, int recordings_per_call,
                        float **rows_out, size_t *n_out, int32_t *status,
                        aptgpu_result *results /* nullable */, aptgpu_batch_stats *stats /* nullable */,
                        char *err, size_t err_cap);
/* The same on WAV file images (noaa_apt::load + decode per file): the data chunk is uploaded as it
 * is — 2 bytes per sample for PCM16 — and converted on the device (wav.rs:30-51). */
int aptgpu_decode_batch_wav(const aptgpu_context *ctx, const aptgpu_settings *settings,
                            uint32_t input_rate_hz, int sync, int count, const void *const *wav_images,
                            const size_t *wav_bytes, const int32_t *devices, int n_devices,
                            int recordings_per_call, float **rows_out, size_t *n_out, int32_t *status,
                            aptgpu_result *results, aptgpu_batch_stats *stats, char *err, size_t err_cap);
/* Pinned host memory (hipHostMalloc) for inputs that should cross PCIe by direct DMA; NULL on failure. */
void *aptgpu_host_alloc(size_t bytes);
void aptgpu_host_free(void *p);
/* Which host CPUs a worker of `device` pins itself to: the device's PCI address (hipDeviceGetPCIBusId), its NUMA
 * node and that node's CPU list as sysfs prints it ("0-63,128-191").  numa_node = -1 and an empty list when the
 * platform does not say (single-socket hosts, containers without sysfs): no pinning then.  The second form is the
 * same lookup on a given PCI address under a given sysfs root ("/sys" on a real host) and needs no GPU. */
int aptgpu_host_affinity(int device, char *pci_bdf /* >= 16 bytes, nullable */, int32_t *numa_node,
                         char *cpulist, size_t cpulist_cap);
int aptgpu_host_affinity_from_sysfs(const char *sysfs_root, const char *pci_bdf, int32_t *numa_node,
                                    char *cpulist, size_t cpulist_cap);

/* ====================================================================== */
/* 3. the dsp.rs / filters.rs / decode.rs building blocks (host buffers)    */
/* ====================================================================== */
/* These mirror the reference functions one-to-one so stage-level parity    */
/* tests read like the reference's own unit tests.  Outputs are malloc'd.   */

/* Filter::design()                     src/filters.rs:48-54,57-88,98-132 (host math) */
int aptgpu_filter_design(const aptgpu_filter *f, float **coeff_out, size_t *n_out);
/* Filter::resample(input_rate, output_rate)   src/filters.rs:90-94,134-138 */
void aptgpu_filter_resample(aptgpu_filter *f, uint32_t input_rate_hz, uint32_t output_rate_hz);
/* generate_sync_frame(work_rate)       src/decode.rs:171-199 */
int aptgpu_generate_sync_frame(uint32_t work_rate_hz, int8_t **frame_out, size_t *n_out,
                               char *err, size_t err_cap);
/* dsp::resample_with_filter(context, signal, input_rate, output_rate, filt)  src/dsp.rs:62-126 */
int aptgpu_resample_with_filter(const aptgpu_context *ctx, const float *signal, size_t n,
                                uint32_t input_rate_hz, uint32_t output_rate_hz,
                                aptgpu_filter filt, float **out, size_t *n_out, char *err,
                                size_t err_cap);
/* dsp::resample(context, signal, input_rate, output_rate, atten, delta_w)   src/dsp.rs:132-162
 * (the WAV->WAV tool path, src/resample.rs:36) */
int aptgpu_resample(const aptgpu_context *ctx, const float *signal, size_t n,
                    uint32_t input_rate_hz, uint32_t output_rate_hz, float atten,
                    float delta_w_pi_rad, float **out, size_t *n_out, char *err, size_t err_cap);
/* dsp::demodulate(context, signal, carrier_freq)   src/dsp.rs:350-383 */
int aptgpu_demodulate(const aptgpu_context *ctx, const float *signal, size_t n,
                      float carrier_pi_rad, float **out, char *err, size_t err_cap);
/* dsp::filter(context, signal, filter)             src/dsp.rs:386-410 */
int aptgpu_filter_signal(const aptgpu_context *ctx, const float *signal, size_t n,
                         aptgpu_filter filt, float **out, char *err, size_t err_cap);
/* lab 0.11.0's Lab::from_rgb / Lab::to_rgb (Cargo.lock:991) as the Lab path of aptgpu_process_image
 * runs them (CPU only): rgb holds n (R, G, B) u8 triples, lab n (L, a, b) f32 triples.  from_rgb calls
 * the C library's powf; to_rgb is f32 arithmetic plus a threshold quantiser that stands in for the
 * crate's final powf + round + clamp.  Restated from the crate's published source. */
int aptgpu_lab_from_rgb(const uint8_t *rgb, size_t n, float *lab);
int aptgpu_lab_to_rgb(const float *lab, size_t n, uint8_t *rgb);
/* find_sync(context, signal, work_rate)            src/decode.rs:204-263
 * correlation_out nullable (the "sync_correlation" step). */
int aptgpu_find_sync(const aptgpu_context *ctx, const float *signal, size_t n,
                     uint32_t work_rate_hz, uint64_t **pos_out, size_t *n_pos,
                     float **correlation_out, size_t *n_corr, char *err, size_t err_cap);

/* ====================================================================== */
/* 4. consumers of the pixel rows                 */
/* ====================================================================== */
/* noaa_apt::process() (src/noaa_apt.rs:132-235): contrast limits                           */
/* -> map_signal_u8, plus telemetry.rs, histogram equalisation (imageext.rs:21-45), palette */
/* false colour (processing.rs:113-165) and the 180-degree channel rotation.  Equalisation */
/* of a false-colour image (CIE Lab, imageext.rs:51-64) is opt-in                        */
/* (APTGPU_COLOR_EQUALIZE_LAB); the map overlay from a caller-computed track or from a TLE  */
/* (below).                                                                                  */
/* aptgpu_process_gray / aptgpu_plan_process_device: the grayscale image of the first     */
/* three contrasts; aptgpu_process_image / aptgpu_plan_process_device_image and their     */
/* *_map / *_png / *_orbit / *_project forms: every contrast (APTGPU_CONTRAST_HISTOGRAM   */
/* and APTGPU_CONTRAST_HISTOGRAM_FLOAT too), optional false colour (not with               */
/* HISTOGRAM_FLOAT), gray or RGBA output.                                                   */

#define APTGPU_CONTRAST_TELEMETRY 0 /* Contrast::Telemetry   src/noaa_apt.rs:141-150 */
#define APTGPU_CONTRAST_PERCENT 1   /* Contrast::Percent(p)  src/noaa_apt.rs:151-157 */
#define APTGPU_CONTRAST_MINMAX 2    /* Contrast::MinMax      src/noaa_apt.rs:158-164 (Histogram
                                       takes the same limits before its equalisation) */
#define APTGPU_CONTRAST_HISTOGRAM 3 /* Contrast::Histogram: MinMax limits, then per-channel equalisation
                                       (aptgpu_process_image / aptgpu_plan_process_device_image only) */
/* Histogram equalisation on the f32 signal, before the pixel values become integers (the reference's to-do list,
 * docs/development.md:105-106; not a reference Contrast).  The image's two halves (columns [0, 1040) and [1040, 2080)
 * of the n / 2080 whole rows, N = 1040 * height samples each) are equalised on their own.  Samples are ordered by
 * IEEE totalOrder on their bits: key = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000) as u32, so -NaN < -Inf < ... <
 * -0 < +0 < ... < +Inf < +NaN and every input has a place.  cum(p) = samples of p's half with key <= key(p), and
 * out(p) = (255f32 * (cum as f32 / N as f32)) as u8 (imageext.rs:33,38 with one bin per representable value).  low /
 * high of aptgpu_image_result and the zero-length error are Histogram's (MinMax limits); they do not enter the
 * pixels.  Gray or RGBA (R = G = B, A = 255); with a palette (color != NULL) APTGPU_ERR_UNSUPPORTED before any
 * callback.  aptgpu_process_image / aptgpu_plan_process_device_image and their *_map / *_png / *_orbit / *_project
 * forms only; aptgpu_process_gray / aptgpu_plan_process_device refuse it.  DESIGN.md §16. */
#define APTGPU_CONTRAST_HISTOGRAM_FLOAT 4
#define APTGPU_ROTATE_NO 0          /* Rotate::No  */
#define APTGPU_ROTATE_YES 1         /* Rotate::Yes  src/noaa_apt.rs:228-231, processing.rs:21-37 */
#define APTGPU_ROTATE_ORBIT 2       /* Rotate::Orbit: the *_orbit entry points only (they decide from the satellite's
                                       pass, processing.rs:40-81); everywhere else APTGPU_ERR_UNSUPPORTED */

/* What the image stage found; also the telemetry::Telemetry values (src/telemetry.rs:19-23). */
typedef struct aptgpu_image_result {
    int32_t status;          /* APTGPU_OK or APTGPU_ERR_INTERNAL */
    int32_t reason;          /* 1 zero-length signal (dsp.rs:40-44), 2 too short for telemetry
                                (telemetry.rs:199-203), 3 no low bucket (misc.rs:172 panics),
                                4 the decode before it failed, 5-8 the map overlay's limits
                                (APTGPU_MAP_REASON_*), 9 APTGPU_PNG_REASON_CAPACITY, 10 APTGPU_SAT_REASON_SGP4,
                                11 APTGPU_PROJECT_REASON_CAPACITY, 12 APTGPU_COMPOSITE_REASON_PASS */
    uint32_t height;         /* rows of 2080 px */
    uint32_t telemetry_row;  /* best frame start, telemetry.rs:196,228-230 */
    float low, high;         /* the contrast limits used by map_signal_u8 */
    float telemetry_quality;
    int32_t channel_a, channel_b; /* index for aptgpu_channel_name(), -1 = not computed */
    uint32_t png_bytes;      /* the *_png entry points: length of the PNG file (with APTGPU_PNG_REASON_CAPACITY
                                the length it needs); 0 from every other call (this was `reserved`) */
    uint64_t n_px;           /* u8 pixels written */
    float values_a[16], values_b[16]; /* wedges 1-16 of each band */
} aptgpu_image_result;

/* dsp::get_min / dsp::get_max          src/dsp.rs:20-54 */
int aptgpu_get_min(const aptgpu_context *ctx, const float *signal, size_t n, float *out, char *err,
                   size_t err_cap);
int aptgpu_get_max(const aptgpu_context *ctx, const float *signal, size_t n, float *out, char *err,
                   size_t err_cap);
/* misc::percent(signal, percent)       src/misc.rs:119-175 */
int aptgpu_percent(const aptgpu_context *ctx, const float *signal, size_t n, float percent,
                   float *low, float *high, char *err, size_t err_cap);
/* map_signal_u8(signal, low, high)     src/noaa_apt.rs:249-259; *out malloc'd, n bytes */
int aptgpu_map_signal_u8(const aptgpu_context *ctx, const float *signal, size_t n, float low,
                         float high, uint8_t **out, char *err, size_t err_cap);
/* telemetry::read_telemetry(context, signal)   src/telemetry.rs:125-243; fills values_*,
 * telemetry_row/quality, channel_*.  With ctx->step set, the five "telemetry_*" steps are
 * exported in the reference's order (telemetry.rs:234-238). */
int aptgpu_read_telemetry(const aptgpu_context *ctx, const float *signal, size_t n,
                          aptgpu_image_result *telemetry, char *err, size_t err_cap);
/* Telemetry::get_channel_name table    src/telemetry.rs:104-106 */
const char *aptgpu_channel_name(int index);
/* process() up to the GrayImage (+ rotate): contrast limits, status callbacks at 0.1 / 0.3 /
 * 0.90 with the reference's texts, u8 image rows*2080 (malloc'd).  src/noaa_apt.rs:132-235 */
int aptgpu_process_gray(const aptgpu_context *ctx, const float *signal, size_t n, int contrast,
                        float percent, int rotate, uint8_t **image_out, size_t *n_out,
                        aptgpu_image_result *info, char *err, size_t err_cap);
/* Device-resident: the same stage chained behind the most recent aptgpu_plan_decode_device
 * call, recording i of that call, on the recording's own stream (no host round trip; the
 * pixel count comes from the decode result on the device).  d_rows[i] must be the rows
 * buffer given to the decode call (same rows_cap[i]); d_images[i] has room for
 * rows_cap[i]*2080 bytes. */
int aptgpu_plan_process_device(aptgpu_plan *plan, int count, const float *const *d_rows,
                               const size_t *rows_cap, int contrast, float percent, int rotate,
                               uint8_t *const *d_images, char *err, size_t err_cap);

/* noaa_apt::ColorSettings (src/noaa_apt.rs:63-71) with the palette already decoded by the caller
 * (`image::open(..).into_rgb8()`, 256 x 256, alpha dropped). */
typedef struct aptgpu_color_settings {
    uint32_t struct_size;        /* sizeof(aptgpu_color_settings) */
    uint32_t flags;              /* APTGPU_COLOR_* bits; 0 = the behaviour of ABI 2 before flags */
    const uint8_t *palette_rgb;  /* host, 256*256*3: pixel (a, b) at (b*256 + a)*3 */
    float ch_a_tune_start, ch_a_tune_end, ch_b_tune_start, ch_b_tune_end;
} aptgpu_color_settings;
/* With APTGPU_CONTRAST_HISTOGRAM: equalise the false-colour image as the reference does, channel A in
 * CIE Lab (98 % limits, false colour, then L equalised over 101 bins, imageext.rs:50-64; channel B as
 * the gray equalisation).  Bit-exact against tests/np_lab_model.py, a restatement of the lab crate
 * 0.11.0.  No effect with the other contrasts; any other bit is APTGPU_ERR_INVALID. */
#define APTGPU_COLOR_EQUALIZE_LAB (1u << 0)
/* process() for every contrast incl. APTGPU_CONTRAST_HISTOGRAM, with optional false colour (color
 * nullable).  channels 1 = the gray image (no colour allowed), 4 = the reference's RgbaImage (A = 255).
 * The image has height = n / 2080 whole rows; *image_out malloc'd, *n_out = height*2080*channels
 * bytes, info->n_px = height*2080.  Status callbacks as aptgpu_process_gray (Histogram: "Mapping
 * values").  Histogram with false colour needs color->flags & APTGPU_COLOR_EQUALIZE_LAB (the reference
 * equalises channel A in CIE Lab then); without it, and for Rotate::Orbit, the call is refused with
 * APTGPU_ERR_UNSUPPORTED before any callback. */
int aptgpu_process_image(const aptgpu_context *ctx, const float *signal, size_t n, int contrast,
                         float percent, int rotate, const aptgpu_color_settings *color, int channels,
                         uint8_t **image_out, size_t *n_out, aptgpu_image_result *info, char *err,
                         size_t err_cap);
/* Device-resident, chained behind the last aptgpu_plan_decode_device call like
 * aptgpu_plan_process_device; d_images[i] holds rows_cap[i]*2080*channels bytes (16-byte aligned
 * for channels 4, 4-byte for channels 1).  The palette is uploaded once per workspace slot and
 * again only when its bytes change.  Results through aptgpu_plan_image_results. */
int aptgpu_plan_process_device_image(aptgpu_plan *plan, int count, const float *const *d_rows,
                                     const size_t *rows_cap, int contrast, float percent, int rotate,
                                     const aptgpu_color_settings *color, int channels,
                                     uint8_t *const *d_images, char *err, size_t err_cap);
/* Waits for the image stage of the last call and copies the records. */
int aptgpu_plan_image_results(aptgpu_plan *plan, int count, aptgpu_image_result *results);

/* ---- the map overlay (map.rs:14-200) ----
 * The caller passes the satellite's (lat, lon) for every image row, in radians, as map.rs:41-58 computes them; or
 * it passes the TLE and the time and the track is computed on the GPU ("the satellite track" below).  The overlay draws over the RGBA image before the rotation, as the reference does.  Errors found on
 * the device land in aptgpu_image_result (status APTGPU_ERR_INTERNAL) with these reasons; the image is then left
 * without the overlay: */
#define APTGPU_MAP_REASON_OVERFLOW 5  /* more than APTGPU_MAP_MAX_FRAGMENTS fragments in one image */
#define APTGPU_MAP_REASON_WALK 6      /* a segment's walk is longer than APTGPU_MAP_MAX_WALK steps or has a
                                         non-finite end (the reference loops for ages or panics there) */
#define APTGPU_MAP_REASON_COUNT 7     /* the position count differs from the image height */
#define APTGPU_MAP_REASON_PIXEL 8     /* more than APTGPU_MAP_MAX_PIXEL_FRAGMENTS fragments on one pixel (tiny
                                         hscale / vscale squeeze the whole map into a few pixels) */
#define APTGPU_MAP_MAX_FRAGMENTS (1u << 21)
#define APTGPU_MAP_MAX_PIXEL_FRAGMENTS (1u << 16)
#define APTGPU_MAP_MAX_WALK (1u << 20)

/* noaa_apt::MapSettings minus the colours (src/noaa_apt.rs:84-91); the CLI's defaults are yaw 0, hscale 1, vscale 1
 * (config.rs:646-648). */
typedef struct aptgpu_map_settings {
    uint32_t struct_size; /* sizeof(aptgpu_map_settings) */
    uint32_t reserved;    /* 0 */
    double yaw, hscale, vscale;
} aptgpu_map_settings;

/* The shapefile layers in the reference's draw order, with their RGBA colours.  Parsed once; uploaded once per
 * device workspace and again only after the layer set changes. */
typedef struct aptgpu_map_layers aptgpu_map_layers;
#define APTGPU_MAP_STATES 0    /* states.shp, read as Polyline; default colour (255, 255, 0, 150)  */
#define APTGPU_MAP_COUNTRIES 1 /* countries.shp, Polygon; (255, 255, 0, 255)                       */
#define APTGPU_MAP_LAKES 2     /* lakes.shp, Polygon; (50, 200, 200, 255)  (default_settings.toml:72-74) */
/* An empty layer set with the default colours. */
int aptgpu_map_layers_create(aptgpu_map_layers **out);
void aptgpu_map_layers_destroy(aptgpu_map_layers *layers);
/* Reads <dir>/states.shp, countries.shp and lakes.shp (all three must exist: "Could not load {:?}",
 * APTGPU_ERR_INTERNAL, as map.rs:136-137).  Shapefile errors: a record of another type than its layer's is
 * APTGPU_ERR_INTERNAL, a layer type other than Polyline / Polygon APTGPU_ERR_UNSUPPORTED, an empty part
 * APTGPU_ERR_INVALID.  On error the set is unchanged. */
int aptgpu_map_layers_load_dir(aptgpu_map_layers *layers, const char *dir, char *err, size_t err_cap);
/* Sets one layer from arrays: xy holds n_points (x = lon°, y = lat°) pairs, part k is points
 * [part_offsets[k], part_offsets[k + 1]) with part_offsets[0] = 0 and part_offsets[n_parts] = n_points, no part
 * empty.  n_parts = 0 removes the layer (it is then not drawn). */
int aptgpu_map_layers_set(aptgpu_map_layers *layers, int layer, const double *xy, size_t n_points,
                          const uint32_t *part_offsets, size_t n_parts, char *err, size_t err_cap);
int aptgpu_map_layers_set_color(aptgpu_map_layers *layers, int layer, const uint8_t rgba[4]);
/* The reader alone (CPU): the parts of one .shp file read as shape_type 3 (Polyline) or 5 (Polygon).  *xy and
 * *part_offsets malloc'd (free with aptgpu_free), *n_parts + 1 offsets. */
int aptgpu_map_read_shapefile(const char *path, int shape_type, double **xy, size_t *n_points,
                              uint32_t **part_offsets, size_t *n_parts, char *err, size_t err_cap);

/* aptgpu_process_image followed by the map overlay.  channels must be 4 (APTGPU_ERR_INVALID otherwise);
 * Rotate::Orbit stays APTGPU_ERR_UNSUPPORTED.  sat_positions: height = n / 2080 pairs (lat, lon) in
 * radians.  Status callback 0.5 "Drawing map" (noaa_apt.rs:205). */
int aptgpu_process_image_map(const aptgpu_context *ctx, const float *signal, size_t n, int contrast,
                             float percent, int rotate, const aptgpu_color_settings *color, int channels,
                             const aptgpu_map_settings *map, const aptgpu_map_layers *layers,
                             const double *sat_positions, uint8_t **image_out, size_t *n_out,
                             aptgpu_image_result *info, char *err, size_t err_cap);
/* aptgpu_plan_process_device_image followed by the map overlay, on each recording's stream without a host round
 * trip.  sat_positions[i] holds n_positions[i] pairs; the height is known only on the device, so a count that
 * differs from it is reported through aptgpu_plan_image_results (APTGPU_MAP_REASON_COUNT). */
int aptgpu_plan_process_device_image_map(aptgpu_plan *plan, int count, const float *const *d_rows,
                                         const size_t *rows_cap, int contrast, float percent, int rotate,
                                         const aptgpu_color_settings *color, int channels,
                                         const aptgpu_map_settings *map, const aptgpu_map_layers *layers,
                                         const double *const *sat_positions, const size_t *n_positions,
                                         uint8_t *const *d_images, char *err, size_t err_cap);

/* ---- PNG encoding (main.rs, the Decode arm: `img.save(&output_filename)`) ----
 * The file is the signature, IHDR, one IDAT and IEND: 8 bits per sample, no interlace, colour type 0 (gray) for
 * channels 1 and 6 (RGBA, what the reference's RgbaImage saves as) for channels 4.  Decoding it gives the input bytes
 * exactly; its bytes are a function of the pixels and the settings alone (not of the batch, the slot or the run) but
 * are not those of the `png` crate.  Filter, deflate (matches, Huffman codes, bit packing), Adler-32 and CRC-32 all
 * run on the GPU; only the encoded bytes cross to the host. */
#define APTGPU_PNG_REASON_CAPACITY 9 /* aptgpu_image_result.reason: png_cap[i] is below the file's length, which
                                        png_bytes then holds; nothing was written to d_png[i] */
typedef struct aptgpu_png_settings {
    uint32_t struct_size; /* sizeof(aptgpu_png_settings) */
    uint32_t flags;       /* 0; any set bit is APTGPU_ERR_INVALID */
} aptgpu_png_settings;
/* The largest file the encoder can emit for such an image (every deflate chunk stored): pure host arithmetic.  0 for
 * a zero width or height, channels other than 1 or 4, or an image past 2^31 filtered bytes. */
size_t aptgpu_png_bound(uint32_t width, uint32_t height, int channels);
/* Any host u8 image (height rows of width pixels of `channels` bytes) through the GPU encoder; settings nullable
 * (= flags 0).  *png_out malloc'd, *n_out bytes.  A zero width or height and channels other than 1 or 4 are
 * APTGPU_ERR_INVALID. */
int aptgpu_encode_png(const aptgpu_context *ctx, const uint8_t *image, uint32_t width, uint32_t height, int channels,
                      const aptgpu_png_settings *settings, uint8_t **png_out, size_t *n_out, char *err,
                      size_t err_cap);
/* aptgpu_process_image_map returning the PNG file instead of the pixels.  map, layers and sat_positions are nullable
 * together (then no overlay, and channels may be 1).  info->png_bytes = *n_out.  A signal shorter than one row has
 * no image to encode: APTGPU_ERR_INVALID. */
int aptgpu_process_image_png(const aptgpu_context *ctx, const float *signal, size_t n, int contrast, float percent,
                             int rotate, const aptgpu_color_settings *color, int channels,
                             const aptgpu_map_settings *map, const aptgpu_map_layers *layers,
                             const double *sat_positions, const aptgpu_png_settings *png, uint8_t **png_out,
                             size_t *n_out, aptgpu_image_result *info, char *err, size_t err_cap);
/* aptgpu_plan_process_device_image_map (map, layers, sat_positions and n_positions nullable together) followed by the
 * encoder on each recording's stream: d_images[i] receives the pixels as before, d_png[i] (png_cap[i] bytes;
 * aptgpu_png_bound(2080, rows_cap[i], channels) always suffices) the file.  Its length arrives in
 * aptgpu_plan_image_results' png_bytes.  A capacity below the file's length is reported there (status
 * APTGPU_ERR_INTERNAL, reason APTGPU_PNG_REASON_CAPACITY, png_bytes = the length needed) and d_png[i] is left
 * untouched: nothing is truncated. */
int aptgpu_plan_process_device_image_png(aptgpu_plan *plan, int count, const float *const *d_rows,
                                         const size_t *rows_cap, int contrast, float percent, int rotate,
                                         const aptgpu_color_settings *color, int channels,
                                         const aptgpu_map_settings *map, const aptgpu_map_layers *layers,
                                         const double *const *sat_positions, const size_t *n_positions,
                                         uint8_t *const *d_images, const aptgpu_png_settings *png,
                                         uint8_t *const *d_png, const size_t *png_cap, char *err, size_t err_cap);

/* ---- the satellite track (map.rs:28-58, processing.rs:40-81) ----
 * noaa_apt::OrbitSettings: the satellite's name, the TLE text and the reference time.  SGP4 (near earth, WGS-72), the
 * sidereal time and the geodetic sub-point of every image row, t = start + 500 ms * row, are computed in f64: by a
 * kernel, one thread per row, where the image height is known, and by the same source text on the CPU.  The
 * algorithm is Vallado's 2006 SGP4 as the `satellite` crate ports it; the parity statement is the reference's own
 * known-answer test (geo.rs:225-233), not bit equality with the crate. */
#define APTGPU_REF_TIME_START 0 /* RefTime::Start(t): row 0 is at t */
#define APTGPU_REF_TIME_END 1   /* RefTime::End(t): row 0 is at t - 500 ms * height (map.rs:45) */
#define APTGPU_SAT_REASON_SGP4 10 /* aptgpu_image_result.reason: SGP4 returned an error for a row of the image (the
                                     satellite decayed, eccentricity out of range: the reference panics there); the
                                     image is left without the overlay */
typedef struct aptgpu_orbit_settings {
    uint32_t struct_size;  /* sizeof(aptgpu_orbit_settings) */
    uint32_t flags;        /* 0; any set bit is APTGPU_ERR_INVALID */
    const char *sat_name;  /* SatName::to_string(): "NOAA 15", "NOAA 18", "NOAA 19" (any title line of the text) */
    const char *tle;       /* custom_tle: title / line 1 / line 2 per satellite.  NULL is APTGPU_ERR_UNSUPPORTED: the
                              reference then downloads the current TLE, which this library does not do */
    int32_t ref_kind;      /* APTGPU_REF_TIME_START / APTGPU_REF_TIME_END */
    int32_t reserved;      /* 0 */
    int64_t ref_unix_ms;   /* the DateTime<Utc> as milliseconds since 1970-01-01T00:00:00Z */
    const aptgpu_map_settings *draw_map; /* nullable: then no map, only the rotation decision */
} aptgpu_orbit_settings;
/* Errors of every entry point that takes the struct: a name that is not in the text is APTGPU_ERR_INTERNAL with the
 * reference's `Satellite "NAME" not found in TLE` (a malformed record is skipped, as the reference ignores
 * parse_multiple's errors); an orbit with a period of 225 minutes or more needs the deep-space branch:
 * APTGPU_ERR_UNSUPPORTED; an SGP4 error return is APTGPU_ERR_INTERNAL with its number and meaning. */
/* The track of an image of `height` rows, computed by the kernel and copied back: latlon_out receives height pairs
 * (lat, lon) in radians, longitude in [-pi, pi]. */
int aptgpu_sat_track(const aptgpu_context *ctx, const aptgpu_orbit_settings *orbit, uint32_t height,
                     double *latlon_out, char *err, size_t err_cap);
/* The same on the CPU (no GPU needed): the values a caller of aptgpu_process_image_map would compute itself. */
int aptgpu_sat_track_host(const aptgpu_orbit_settings *orbit, uint32_t height, double *latlon_out, char *err,
                          size_t err_cap);
/* processing::south_to_north_pass (CPU): the sub-points at the reference time as given (Start and End alike, as the
 * reference) and 2 s later, geo::azimuth between them, *out = |azimuth| < pi/2: the satellite is heading north.  (The
 * reference compares `azimuth < PI/4 || azimuth > 3*PI/4`, which an atan2 result meets on the northbound and the
 * southbound stretches of a retrograde orbit alike; this returns what that function documents.  DESIGN.md §14.) */
int aptgpu_south_to_north_pass(const aptgpu_orbit_settings *orbit, int *out, char *err, size_t err_cap);

#define APTGPU_OUTPUT_PIXELS 0 /* *out: the image, height*2080*channels bytes */
#define APTGPU_OUTPUT_PNG 1    /* *out: the PNG file (png nullable = flags 0) */
/* process() with the reference's OrbitSettings: aptgpu_process_image, then the map overlay when orbit->draw_map is set
 * (layers required then, channels 4; status 0.5 "Drawing map"), then optionally the PNG encoder.  rotate may be
 * APTGPU_ROTATE_ORBIT: decided by aptgpu_south_to_north_pass before anything is launched (status 0.90 "Rotating
 * output image" only when it rotates). */
int aptgpu_process_image_orbit(const aptgpu_context *ctx, const float *signal, size_t n, int contrast, float percent,
                               int rotate, const aptgpu_color_settings *color, int channels,
                               const aptgpu_orbit_settings *orbit, const aptgpu_map_layers *layers, int output,
                               const aptgpu_png_settings *png, uint8_t **out, size_t *n_out,
                               aptgpu_image_result *info, char *err, size_t err_cap);
/* aptgpu_plan_process_device_image_png with the track computed on each recording's stream: orbit[i] is recording i's
 * satellite and time (RefTime::End is resolved on the device, where the height is known).  draw_map must be set for
 * every recording or for none; layers is shared.  d_png (with png and png_cap) is nullable: then no PNG.  A
 * propagation error in any row is reported through aptgpu_plan_image_results (APTGPU_SAT_REASON_SGP4). */
int aptgpu_plan_process_device_image_orbit(aptgpu_plan *plan, int count, const float *const *d_rows,
                                           const size_t *rows_cap, int contrast, float percent, int rotate,
                                           const aptgpu_color_settings *color, int channels,
                                           const aptgpu_orbit_settings *const *orbit, const aptgpu_map_layers *layers,
                                           uint8_t *const *d_images, const aptgpu_png_settings *png,
                                           uint8_t *const *d_png, const size_t *png_cap, char *err, size_t err_cap);

/* ---- reprojection onto a north-up map grid ----
 * The reference's image is the raw swath; its to-do list names the next step (docs/development.md:112 "Draw image over
 * mercator (or at least equirectangular) projection", :99 "Add latitude longitude grid").  Every output pixel goes
 * backwards through the reference's own latlon_to_rel_px (map.rs:71-100) and the x-offset correction of map.rs:105-111
 * into one channel of the unrotated swath image, so the projected coastlines agree with the overlay's by construction.
 * The settings struct is the georeference of the output: the centre of pixel (i, j) lies at
 *   longitude lon_west + j * step                                   (degrees; may pass 180, never wrapped)
 *   latitude  lat_north - i * step                                  (equirectangular)
 *             atan(sinh(asinh(tan(lat_north)) - i * step in rad))   (Mercator: step is the longitude step)
 * A pixel is painted only where the swath covers it: the band of map.rs:116-121 (-456 < x < 456, 0 < y < height) and
 * less than 60 degrees of arc from the track's first point (latlon_to_rel_px clamps its distance there; beyond it every
 * point would alias onto one image row).  Every other pixel is (0, 0, 0, 0).  The output is always RGBA; a gray source
 * reads as (g, g, g, 255). */
#define APTGPU_PROJECTION_EQUIRECTANGULAR 0
#define APTGPU_PROJECTION_MERCATOR 1
#define APTGPU_PROJECTION_CHANNEL_A 0 /* columns x + 539 of the swath  */
#define APTGPU_PROJECTION_CHANNEL_B 1 /* columns x + 1579              */
#define APTGPU_SAMPLING_NEAREST 0     /* the pixel at floor(x + 0.5), floor(y + 0.5) */
#define APTGPU_SAMPLING_BILINEAR 1    /* the four neighbours in f64, every channel, rounded half up */
#define APTGPU_PROJECT_REASON_CAPACITY 11 /* aptgpu_image_result.reason: out_cap[i] is below width * height * 4 bytes;
                                             nothing was written to d_out[i] */
#define APTGPU_PROJECTION_MAX_PIXELS (1u << 26)
typedef struct aptgpu_projection_settings {
    uint32_t struct_size; /* sizeof(aptgpu_projection_settings) */
    int32_t kind;         /* APTGPU_PROJECTION_* */
    uint32_t width, height;      /* >= 1, width * height <= APTGPU_PROJECTION_MAX_PIXELS */
    double lat_north, lon_west;  /* degrees: the centre of pixel (0, 0); |lat_north| <= 90 (and the last row's for
                                    the equirectangular grid) */
    double step;          /* degrees per pixel, finite and > 0 */
    int32_t channel;      /* APTGPU_PROJECTION_CHANNEL_* */
    int32_t sampling;     /* APTGPU_SAMPLING_* */
    double grid_deg;      /* 0: no graticule; otherwise >= step: the rows and columns nearest to every multiple of it are
                             blended with grid_color (image 0.24.7's blend, once where they cross), over painted and
                             empty pixels alike */
    uint8_t grid_color[4]; /* RGBA */
    uint32_t reserved;    /* 0 */
} aptgpu_projection_settings;
/* Host only (no GPU): a grid of `kind` that covers the swath of a track of `count` (lat, lon) pairs in radians: the
 * track's bounding box (longitudes unwrapped so that consecutive rows differ by less than pi), grown by the swath's
 * half angle 456 * 0.0005 / hscale in latitude and by that / cos(max |lat|) in longitude, latitudes clamped to +-85
 * degrees for Mercator and +-90 otherwise, the longitude span to 360.  Conservative, not tight.  step_deg > 0 is the
 * step; otherwise max_width >= 2 columns span the box.  channel A, nearest sampling and no graticule are filled in. */
int aptgpu_projection_fit(const double *track, size_t count, double hscale, int kind, double step_deg,
                          uint32_t max_width, aptgpu_projection_settings *out, char *err, size_t err_cap);
/* Reprojects a host image: height rows of 2080 px of `channels` (1 or 4) bytes, unrotated, with its track (n_positions
 * = height pairs).  map gives yaw / hscale / vscale (nullable: 0, 1, 1).  output APTGPU_OUTPUT_PIXELS: *out is the
 * RGBA grid, proj->width * proj->height * 4 bytes; APTGPU_OUTPUT_PNG: the PNG file of it (png nullable). */
int aptgpu_project_image(const aptgpu_context *ctx, const uint8_t *image, uint32_t height, int channels,
                         const double *sat_positions, size_t n_positions, const aptgpu_map_settings *map,
                         const aptgpu_projection_settings *proj, int output, const aptgpu_png_settings *png,
                         uint8_t **out, size_t *n_out, char *err, size_t err_cap);
/* process() with the reprojection at its end: the image stage, the map overlay when `layers` is given (drawn on the
 * swath by the overlay's own launches; channels 4 then), the reprojection, optionally the PNG encoder, all on one
 * stream.  Exactly one of sat_positions (height pairs) and orbit (the track is then computed on the GPU) must be
 * given.  map gives yaw / hscale / vscale (nullable: orbit->draw_map when that is set, else 0, 1, 1).  The projection
 * reads the unrotated image and north is up by construction: any rotate but APTGPU_ROTATE_NO is APTGPU_ERR_INVALID.
 * info->height stays the swath's height; info->n_px its pixels. */
int aptgpu_process_image_project(const aptgpu_context *ctx, const float *signal, size_t n, int contrast, float percent,
                                 int rotate, const aptgpu_color_settings *color, int channels,
                                 const aptgpu_map_settings *map, const aptgpu_map_layers *layers,
                                 const double *sat_positions, const aptgpu_orbit_settings *orbit,
                                 const aptgpu_projection_settings *proj, int output, const aptgpu_png_settings *png,
                                 uint8_t **out, size_t *n_out, aptgpu_image_result *info, char *err, size_t err_cap);
/* Device-resident: aptgpu_plan_process_device_image (+ overlay with `layers`) followed by the reprojection of
 * recording i onto proj[i] into d_out[i] (out_cap[i] bytes, 4-byte aligned), on the recording's stream without a host
 * round trip.  Exactly one of sat_positions / n_positions and orbit is given (arrays of count).  d_png (with png_cap)
 * is nullable: then no PNG; aptgpu_png_bound(proj[i].width, proj[i].height, 4) always suffices.  Through
 * aptgpu_plan_image_results: an out_cap[i] that is too small (APTGPU_PROJECT_REASON_CAPACITY; never truncated), a
 * position count that differs from the height (APTGPU_MAP_REASON_COUNT), an SGP4 error (APTGPU_SAT_REASON_SGP4). */
int aptgpu_plan_process_device_image_project(aptgpu_plan *plan, int count, const float *const *d_rows,
                                             const size_t *rows_cap, int contrast, float percent, int rotate,
                                             const aptgpu_color_settings *color, int channels,
                                             const aptgpu_map_settings *map, const aptgpu_map_layers *layers,
                                             const double *const *sat_positions, const size_t *n_positions,
                                             const aptgpu_orbit_settings *const *orbit, uint8_t *const *d_images,
                                             const aptgpu_projection_settings *proj, uint8_t *const *d_out,
                                             const size_t *out_cap, const aptgpu_png_settings *png,
                                             uint8_t *const *d_png, const size_t *png_cap, char *err, size_t err_cap);

/* ---- composite: several passes on one map grid ----
 * A station records several passes a day; what follows their reprojection is one map of all of them.  Each of the
 * 1 <= count <= APTGPU_COMPOSITE_MAX_PASSES passes is an unrotated swath image of its own height, gray or RGBA, with
 * its own track and its own yaw / hscale / vscale; one aptgpu_projection_settings describes the shared grid, and its
 * channel, sampling, grid_deg and grid_color apply to every pass.  Per output pixel every pass, in list order, goes
 * through the reprojection above unchanged (the same kernel text, so a pass's sample c_p has aptgpu_project_image's
 * bits) and also keeps its corrected off-nadir distance x_p.  Over the passes that cover the pixel:
 *   APTGPU_COMPOSITE_FIRST    c_p of the first covering pass: the caller orders the passes by priority
 *   APTGPU_COMPOSITE_NADIR    c_p of the covering pass with the smallest |x_p|, the lower index on an exact tie: the
 *                             pass that saw the pixel with the least panoramic distortion
 *   APTGPU_COMPOSITE_FEATHER  per channel (alpha too), in f64 and in pass order, v = sum(w_p c_p) / sum(w_p) with
 *                             w_p = 456 - |x_p| (> 0 where a pass covers), the channel = floor(v + 0.5) clamped to u8
 * No covering pass gives (0, 0, 0, 0).  The graticule is blended last and once, as the reprojection does.  The
 * coverage plane, where asked for, holds the number of covering passes of every pixel (0..16), one byte each: the
 * mask that tells "black" from "not seen".
 * A pass whose own record carries a status fails the composite (a position count that differs from its height,
 * APTGPU_MAP_REASON_COUNT; an SGP4 error, APTGPU_SAT_REASON_SGP4): the composite's record gets
 * APTGPU_COMPOSITE_REASON_PASS, that pass's record keeps its own reason, and nothing is written.  An output capacity
 * below width * height * 4 is APTGPU_PROJECT_REASON_CAPACITY.  The images are unrotated by contract: no entry point
 * here takes a rotation. */
#define APTGPU_COMPOSITE_FIRST 0
#define APTGPU_COMPOSITE_NADIR 1
#define APTGPU_COMPOSITE_FEATHER 2
#define APTGPU_COMPOSITE_MAX_PASSES 16
#define APTGPU_COMPOSITE_REASON_PASS 12 /* aptgpu_image_result.reason of the composite's record: a pass failed */
typedef struct aptgpu_composite_settings {
    uint32_t struct_size; /* sizeof(aptgpu_composite_settings) */
    int32_t blend;        /* APTGPU_COMPOSITE_* */
    uint32_t reserved;    /* 0 */
} aptgpu_composite_settings;
/* Host only: aptgpu_projection_fit for the union of the swaths of n_tracks tracks (counts[t] pairs each).  Every
 * track's longitudes are unwrapped from the first track's first position, so passes on both sides of the antimeridian
 * share one axis.  One track gives aptgpu_projection_fit's grid. */
int aptgpu_projection_fit_many(const double *const *tracks, const size_t *counts, size_t n_tracks, double hscale,
                               int kind, double step_deg, uint32_t max_width, aptgpu_projection_settings *out,
                               char *err, size_t err_cap);
/* Composites host images: images[p] holds heights[p] rows of 2080 px of channels[p] (1 or 4) bytes, sat_positions[p]
 * its track (n_positions[p] = heights[p] pairs), map[p] its yaw / hscale / vscale (map and its entries nullable:
 * 0, 1, 1).  output as aptgpu_project_image: *out is the RGBA grid or its PNG file.  coverage is nullable; otherwise
 * *coverage receives proj->width * proj->height bytes.  Both are released with aptgpu_free.  count 0 or above 16, a
 * null entry, an unknown blend or a non-zero reserved is APTGPU_ERR_INVALID before the device is touched. */
int aptgpu_composite_images(const aptgpu_context *ctx, int count, const uint8_t *const *images,
                            const uint32_t *heights, const int *channels, const double *const *sat_positions,
                            const size_t *n_positions, const aptgpu_map_settings *const *map,
                            const aptgpu_projection_settings *proj, const aptgpu_composite_settings *composite,
                            int output, const aptgpu_png_settings *png, uint8_t **out, size_t *n_out,
                            uint8_t **coverage, char *err, size_t err_cap);
/* Device-resident: d_images[p] is what aptgpu_plan_process_device_image[_map] left for recording p of the last decode
 * call (unrotated, heights[p] rows of capacity; the height itself is the recording's record's).  Exactly one of
 * sat_positions / n_positions and orbit is given (arrays of count); with orbit a track is computed on the GPU and a
 * pass's geometry defaults to its draw_map.  Each pass's track stage runs on its recording's stream; the composite
 * launch runs on recording 0's behind one event per pass that ran elsewhere, without a host round trip.  d_out holds
 * out_cap bytes (4-byte aligned), d_coverage (nullable) width * height bytes, d_png (nullable, png_cap bytes;
 * aptgpu_png_bound(width, height, 4) always suffices) the PNG file of the grid.  After it,
 * aptgpu_plan_image_results with a count of count + 1 returns the passes' records followed by the composite's (status,
 * reason, height = the grid's, png_bytes). */
int aptgpu_plan_composite_device_images(aptgpu_plan *plan, int count, const uint8_t *const *d_images,
                                        const uint32_t *heights, const int *channels,
                                        const double *const *sat_positions, const size_t *n_positions,
                                        const aptgpu_orbit_settings *const *orbit,
                                        const aptgpu_map_settings *const *map, const aptgpu_projection_settings *proj,
                                        const aptgpu_composite_settings *composite, uint8_t *d_out, size_t out_cap,
                                        uint8_t *d_coverage, const aptgpu_png_settings *png, uint8_t *d_png,
                                        size_t png_cap, char *err, size_t err_cap);

/* ---- despeckle: a band-aware median of the rows, in front of process() ----
 * The reference's to-do list names it (docs/development.md:139 "Investigate about despeckle") and has no code for it,
 * so the definition is this library's; tests/np_despeckle_model.py states it in numpy.  Signal to signal: n floats in,
 * n floats out, opt-in; nothing else changes when it is not called.
 *  - h = n / 2080 whole rows are filtered; the samples past h * 2080 are copied bit for bit.  h == 0: the output is
 *    the input, replaced = 0, status OK, no limits are computed.
 *  - Every row is eight column bands, [0,39) [39,86) [86,995) [995,1040) and the same + 1040 (sync, space, video and
 *    telemetry of channels A and B).  The window of pixel (y, x) in band [b0, b1) is the (2r+1)^2 samples at rows
 *    clamp(y + dy, 0, h - 1) and columns clamp(x + dx, b0, b1 - 1): it never leaves the band, edges are replicated.
 *  - med = the window's element of rank (2r+1)^2 / 2 (0-based) in IEEE totalOrder on the bits (the key of
 *    APTGPU_CONTRAST_HISTOGRAM_FLOAT), with its own bits.  out = med if med is not NaN and !(fabsf(x - med) <= t),
 *    else x: a NaN x among finite neighbours is replaced, a sample in a mostly-NaN window is kept; with t = 0 this
 *    is the plain median except that +-0 are left alone.
 *  - threshold == 0: t = 0.  Otherwise (low, high) = aptgpu_percent(signal, 0.98) of the unfiltered signal, exactly
 *    what APTGPU_CONTRAST_PERCENT with 0.98 reports for it, and t = threshold * (high - low) in f32 (a NaN t makes
 *    every sample with a non-NaN med take med).  A limits failure (aptgpu_image_result reason 3) fails the host-array
 *    forms with aptgpu_percent's status and message; the plan form records it and writes the unfiltered rows.
 *  - replaced counts the samples for which the rule picked med (also where med's bits equal x's). */
typedef struct aptgpu_despeckle_settings {
    uint32_t struct_size; /* sizeof(aptgpu_despeckle_settings) */
    int32_t radius;       /* 1 (3 x 3) or 2 (5 x 5); anything else is APTGPU_ERR_INVALID */
    float threshold;      /* >= 0 and not NaN (else APTGPU_ERR_INVALID): a fraction of the 98 % range */
} aptgpu_despeckle_settings;
typedef struct aptgpu_despeckle_result {
    int32_t status;    /* APTGPU_OK or APTGPU_ERR_INTERNAL */
    int32_t reason;    /* 0; 3 the limits found no low bucket; 4 the decode before it failed (plan form) */
    uint32_t height;   /* whole rows filtered */
    uint32_t reserved;
    uint64_t replaced; /* samples that took their window's median */
    float low, high;   /* the 98 % limits (0 when threshold == 0 or height == 0) */
    float t;           /* threshold * (high - low) */
    uint32_t reserved2;
} aptgpu_despeckle_result;
/* settings nullable (= radius 1, threshold 0) in every entry point below.  *out malloc'd, n floats (aptgpu_free);
 * info nullable. */
int aptgpu_despeckle(const aptgpu_context *ctx, const float *signal, size_t n,
                     const aptgpu_despeckle_settings *settings, float **out, aptgpu_despeckle_result *info, char *err,
                     size_t err_cap);
/* The same on the CPU, in plain C++ (no GPU needed): what the kernel is tested against besides the numpy model. */
int aptgpu_despeckle_host(const float *signal, size_t n, const aptgpu_despeckle_settings *settings, float **out,
                          aptgpu_despeckle_result *info, char *err, size_t err_cap);
/* Device-resident, chained behind the last aptgpu_plan_decode_device call on each recording's stream without a host
 * round trip (the row count comes from the decode record on the device; with a rows_cap below the decoded height the
 * rows the decode wrote, as the image stage).  d_rows[i] is the rows buffer given to the decode call (same
 * rows_cap[i]); d_out[i] has the same capacity, rows_cap[i] * 2080 floats, and must not overlap any d_rows[j]
 * (APTGPU_ERR_INVALID).  d_out may then be passed as d_rows to any aptgpu_plan_process_device* call.  16-byte
 * aligned buffers take the vector path.  Timer names: image_percent (threshold > 0), image_despeckle. */
int aptgpu_plan_despeckle_device(aptgpu_plan *plan, int count, const float *const *d_rows, const size_t *rows_cap,
                                 const aptgpu_despeckle_settings *settings, float *const *d_out, char *err,
                                 size_t err_cap);
/* Waits for the despeckle stage of the last call and copies the records. */
int aptgpu_plan_despeckle_results(aptgpu_plan *plan, int count, aptgpu_despeckle_result *results);

/* ---- thermal calibration: brightness temperature of an infrared channel ----
 * The reference has no calibration, so the definition is this library's; tests/np_thermal_model.py states it in
 * numpy.  It follows the procedure of the NOAA KLM User's Guide §7.1.2.4 with the 8-bit APT telemetry scaled to
 * 10-bit counts.  Opt-in, a stage of its own behind the decode: rows in, a Kelvin plane (and optionally a u8 scale
 * image in the standard row layout) out; nothing else changes when it is not called.
 *  - h = n / 2080 whole rows.  aptgpu_read_telemetry's stage runs first and gives telemetry_row, the wedge values
 *    v[1..16] of the selected channel (settings.channel: 0 = A, 1 = B; its columns start at base = 1040 * channel)
 *    and its index for aptgpu_channel_name().  h < 200 is reason 2; a failed decode in front of it (plan form) 4.
 *  - The identity is settings.channel_id, or with -1 the telemetry's index.  3 ("4"), 4 ("5") and 5 ("3b") pick the
 *    coefficient set; anything else is reason 13 (APTGPU_THERMAL_REASON_CHANNEL), not a thermal channel.
 *  - Space view: for each of the 128 rows from telemetry_row the f32 mean of columns [base + 44, base + 82), summed
 *    sequentially and divided by 38.  The 128 means are ranked by IEEE totalOrder on their bits, ties by row; the 16
 *    lowest and the 16 highest are dropped (minute markers) and `space` is the f64 mean of the other 96, in row order.
 *  - Scalars, all f64, plain + - * / in this order, never contracted:
 *      y = {31, 63, 95, 127, 159, 191, 224, 255, 0}, x = v[1..9]; mx = sum(x) / 9, my = sum(y) / 9,
 *      sxy = sum((x - mx) * (y - my)), sxx = sum((x - mx) * (x - mx)), slope = sxy / sxx, icpt = my - slope * mx,
 *      count10(u) = 4 * (slope * u + icpt);
 *      C_i = count10(v[9 + i]), T_i = (prt[i][0] + prt[i][1] * C_i) + prt[i][2] * (C_i * C_i), i = 1..4,
 *      t_bb = (((T_1 + T_2) + T_3) + T_4) / 4, t_bb* = A + B * t_bb,
 *      n_bb = (c1 * ((nu * nu) * nu)) / (exp((c2 * nu) / t_bb*) - 1), c1 = 1.1910427e-5, c2 = 1.4387752,
 *      c_bb = count10(v[15]), c_space = count10(space).
 *    sxx == 0, a non-finite scalar or c_space == c_bb is reason 14 (APTGPU_THERMAL_REASON_DEGENERATE).
 *  - Per pixel x of the video columns [base + 86, base + 995), 909 a row, in f32 with every scalar rounded to f32
 *    (k1 = c1 * nu^3 and k2 = c2 * nu are rounded after the f64 product):
 *      C_e = 4 * (slope * x + icpt), N_lin = N_s + ((n_bb - N_s) * (c_space - C_e)) / (c_space - c_bb),
 *      N_e = N_lin + ((b0 + b1 * N_lin) + b2 * (N_lin * N_lin)), T = (k2 / log(1 + k1 / N_e) - A) / B,
 *      T = NaN unless N_e > 0 and N_e is finite.
 *  - The scale image (image_channels 1 or 4), in f32: s = (T - t_low) / (t_high - t_low),
 *    level = (uint8)(min(max(s, 0), 1) * 255 + 0.5), with APTGPU_THERMAL_COLD_WHITE 255 - level.  Gray: the level,
 *    0 where T is NaN.  RGBA: palette[level] (default R = G = B = level) with A = 255; (0, 0, 0, 0) where T is NaN.
 *    Every column outside the channel's video is 0 (A = 255).
 *  - A failed record (any reason) leaves the planes of its rows all NaN / level 0 (A = 0) in the plan form; the
 *    host-array forms return APTGPU_ERR_INTERNAL with the record filled and no planes.
 * The coefficients are the caller's.  The per-satellite values (the four PRT polynomials, and per channel the
 * centroid wave number nu, the effective-temperature line A, B, the space radiance N_s and the non-linearity
 * b0, b1, b2) are tabulated in the NOAA KLM User's Guide, Appendix D (one section per satellite); this library
 * ships no presets. */
#define APTGPU_THERMAL_COLD_WHITE 1u        /* settings.flags: cold is white (the usual infrared rendering) */
#define APTGPU_THERMAL_REASON_CHANNEL 13    /* aptgpu_thermal_result.reason */
#define APTGPU_THERMAL_REASON_DEGENERATE 14
#define APTGPU_THERMAL_PX 909               /* floats per row of the Kelvin plane */
typedef struct aptgpu_thermal_coeffs {
    uint32_t struct_size; /* sizeof(aptgpu_thermal_coeffs) */
    uint32_t reserved;
    double prt[4][3];     /* T_i = prt[i][0] + prt[i][1] * C + prt[i][2] * C^2 */
    double channel[3][7]; /* 3B, 4, 5 (in this order): nu, A, B, N_s, b0, b1, b2 */
} aptgpu_thermal_coeffs;  /* a non-finite value or B == 0: APTGPU_ERR_INVALID */
typedef struct aptgpu_thermal_settings {
    uint32_t struct_size;   /* sizeof(aptgpu_thermal_settings) */
    int32_t channel;        /* 0 = A, 1 = B */
    int32_t channel_id;     /* -1: from the telemetry; else an index of aptgpu_channel_name() */
    int32_t image_channels; /* 0: no scale image; 1 gray; 4 RGBA */
    uint32_t flags;         /* APTGPU_THERMAL_COLD_WHITE; any other bit is APTGPU_ERR_INVALID */
    float t_low, t_high;    /* Kelvin at levels 0 and 255; finite, t_high > t_low (else APTGPU_ERR_INVALID) */
    uint32_t reserved;
    const uint8_t *palette; /* nullable: 256 * 3 RGB bytes by level (image_channels 4 only, else APTGPU_ERR_INVALID) */
} aptgpu_thermal_settings;
typedef struct aptgpu_thermal_result {
    int32_t status;         /* APTGPU_OK or APTGPU_ERR_INTERNAL */
    int32_t reason;         /* 0; 2 too short for telemetry; 4 the decode before it failed; 13; 14 */
    uint32_t height;        /* whole rows */
    uint32_t telemetry_row;
    int32_t channel_id;     /* the identity used (-1: the telemetry gave none) */
    uint32_t reserved;
    uint64_t n_nan;         /* NaN pixels of the Kelvin plane */
    double slope, icpt, space, c_space, c_bb, t_bb, n_bb;
    float t_min, t_max;     /* over the finite pixels of the Kelvin plane; NaN when there is none */
} aptgpu_thermal_result;
/* coeffs and settings are required.  *kelvin: malloc'd, height * 909 floats; *image (required iff image_channels != 0):
 * malloc'd, height * 2080 * image_channels bytes (aptgpu_free both); info nullable. */
int aptgpu_calibrate_thermal(const aptgpu_context *ctx, const float *signal, size_t n,
                             const aptgpu_thermal_coeffs *coeffs, const aptgpu_thermal_settings *settings,
                             float **kelvin, uint8_t **image, aptgpu_thermal_result *info, char *err, size_t err_cap);
/* The same on the CPU, in plain C++ (no GPU needed): the same scalars bit for bit, the same f32 pixel arithmetic
 * except for the C library's logf. */
int aptgpu_calibrate_thermal_host(const float *signal, size_t n, const aptgpu_thermal_coeffs *coeffs,
                                  const aptgpu_thermal_settings *settings, float **kelvin, uint8_t **image,
                                  aptgpu_thermal_result *info, char *err, size_t err_cap);
/* Device-resident, chained behind the last aptgpu_plan_decode_device call on each recording's stream without a host
 * round trip (the row count comes from the decode record on the device; with a rows_cap below the decoded height the
 * rows the decode wrote).  d_rows[i] is the rows buffer given to the decode call (same rows_cap[i]); d_kelvin[i]
 * holds rows_cap[i] * 909 floats; d_images (required iff image_channels != 0) rows_cap[i] * 2080 * image_channels
 * bytes each, 4-byte aligned for RGBA, which the PNG, projection and composite calls on device images take as they
 * are.  Neither may overlap any d_rows[j] (APTGPU_ERR_INVALID).  Timer names: image_telemetry,
 * image_thermal_space, image_thermal_setup, image_thermal_map. */
int aptgpu_plan_calibrate_thermal_device(aptgpu_plan *plan, int count, const float *const *d_rows,
                                         const size_t *rows_cap, const aptgpu_thermal_coeffs *coeffs,
                                         const aptgpu_thermal_settings *settings, float *const *d_kelvin,
                                         uint8_t *const *d_images, char *err, size_t err_cap);
/* Waits for the thermal stage of the last call and copies the records. */
int aptgpu_plan_thermal_results(aptgpu_plan *plan, int count, aptgpu_thermal_result *results);

/* ---- geolocation of the swath: lat / lon, sun angle, sun-normalised rows ----
 * The overlay and the reprojection go from a place on the Earth to a pixel (latlon_to_rel_px, map.rs:71-100).  This
 * stage goes the other way, for the 909 video columns of a channel.  The reference has nothing like it, so the
 * definition is this library's; tests/np_geoloc_model.py states it in numpy.  Opt-in, a stage of its own behind the
 * decode; nothing else changes when it is not called.
 *  - h = n / 2080 rows; a track of h (lat, lon) pairs in radians, the caller's (sat_positions) or SGP4's on the GPU
 *    from an aptgpu_orbit_settings (exactly one of the two); aptgpu_map_settings for yaw, hscale, vscale (nullable:
 *    0, 1, 1).  start, ref_az, x_res, y_res, yaw are the overlay's scalars (map.rs:59-69) and xoff[r] the x of
 *    latlon_to_rel_px(track[r]) (map.rs:110-114), as the overlay and the reprojection use them, except xoff[0] = 0:
 *    track[0] is the start point, whose relative pixel is (0, 0) by definition, where the evaluated expression returns
 *    either 0 or up to acos(1 - 2^-53) / x_res = 3e-5 px depending on how one cosine rounds.
 *  - Sample points: video column k = 0 .. 908 of a row is image column base + 86 + k (base = 1040 * channel) and
 *    relative pixel x_rel = k - 453 (image column 539 of channel A is relative pixel 0).  The geometry is the same
 *    for both channels: the planes are h x 909 and carry no channel.
 *  - Forward point of (r, k), all f64, never contracted; (phi0, lam0) = track[0]:
 *      x = x_rel + xoff[r],  b = -x * x_res,  a = (r - yaw * x) * y_res,
 *      S = (cos phi0 cos lam0, cos phi0 sin lam0, sin phi0),  N = (-sin phi0 cos lam0, -sin phi0 sin lam0, cos phi0),
 *      E = (-sin lam0, cos lam0, 0),  T = cos(ref_az) N + sin(ref_az) E,  R = -sin(ref_az) N + cos(ref_az) E,
 *      P = (cos b cos a) S + (cos b sin a) T + (sin b) R,
 *      lat = atan2(Pz, hypot(Px, Py)),  lon = atan2(Py, Px)  (in (-pi, pi], never unwrapped),
 *      valid iff acos(cos a * cos b) < pi / 3  (beyond that distance latlon_to_rel_px clamps and has no inverse).
 *    An invalid pixel is NaN in both planes and unchanged in the rows.
 *  - Sun: row r is seen at t = start_ms + 500 * r (map.rs:45), start_ms = unix_ms (APTGPU_REF_TIME_START) or
 *    unix_ms - 500 * h (APTGPU_REF_TIME_END); with an orbit its reference time rules.  The Astronomical Almanac's
 *    low-precision series, f64, C fmod:
 *      n = t / 86400000 + 2440587.5 - 2451545.0,
 *      L = fmod(280.460 + 0.9856474 n, 360),  g = rad(fmod(357.528 + 0.9856003 n, 360)),
 *      lam = rad(L + 1.915 sin g + 0.020 sin 2g),  eps = rad(23.439 - 0.0000004 n),
 *      alpha = atan2(cos eps sin lam, cos lam),  delta = asin(sin eps sin lam),
 *      theta = rad(15 * fmod(18.697374558 + 24.06570982441908 n, 24)),
 *      U = (cos delta cos(alpha - theta), cos delta sin(alpha - theta), sin delta),
 *      cos_sun(r, k) = (float)((Px Ux + Py Uy) + Pz Uz).
 *  - Normalised rows: the channel's 909 columns in f32, never contracted:
 *      out = valid ? black + (x - black) / fmaxf(c, cmin) : x,  c = cos_sun,  cmin = (float)cos(max_zenith_deg / 180 * pi);
 *    every other column is copied unchanged, a NaN x stays NaN.
 *  - The record counts the invalid pixels (n_outside), the valid ones with c < cmin (n_capped) and gives the extremes
 *    of c over the valid ones, whatever outputs were asked for.
 *  - Record reasons (status APTGPU_ERR_INTERNAL): APTGPU_MAP_REASON_COUNT (7) the position count differs from the
 *    height; APTGPU_SAT_REASON_SGP4 (10); APTGPU_GEOLOC_REASON_HEIGHT (15) fewer than two rows, so no direction of
 *    flight; APTGPU_GEOLOC_REASON_DECODE (16) the decode in front failed (plan form).  The plan form then writes the
 *    planes of the rows as NaN and copies the rows unchanged; the host-array forms return APTGPU_ERR_INTERNAL with
 *    the record filled and no outputs. */
#define APTGPU_GEOLOC_PX 909             /* samples per row of the planes */
#define APTGPU_GEOLOC_REASON_HEIGHT 15   /* aptgpu_geoloc_result.reason */
#define APTGPU_GEOLOC_REASON_DECODE 16
typedef struct aptgpu_geoloc_settings {
    uint32_t struct_size;  /* sizeof(aptgpu_geoloc_settings) */
    uint32_t flags;        /* 0; any set bit is APTGPU_ERR_INVALID */
    int32_t channel;       /* 0 = A, 1 = B: the half of the row image the normalisation rewrites */
    int32_t time_kind;     /* APTGPU_REF_TIME_START / APTGPU_REF_TIME_END; used when no orbit is given */
    int64_t unix_ms;       /* the reference time, milliseconds since 1970-01-01T00:00:00Z; likewise */
    float black_level;     /* the zero level in row units; finite */
    float max_zenith_deg;  /* in (0, 90), else APTGPU_ERR_INVALID; the bindings default to 80 */
} aptgpu_geoloc_settings;
typedef struct aptgpu_geoloc_result {
    uint32_t struct_size;  /* the caller's sizeof(aptgpu_geoloc_result) */
    int32_t status;        /* APTGPU_OK or APTGPU_ERR_INTERNAL */
    int32_t reason;        /* 0, 7, 10, 15, 16 */
    uint32_t height;       /* whole rows */
    uint64_t n_outside;    /* invalid pixels of the h x 909 plane */
    uint64_t n_capped;     /* valid pixels whose cos_sun is below cmin */
    float cos_min, cos_max; /* over the valid pixels; NaN when there is none */
} aptgpu_geoloc_result;
/* settings is required.  Exactly one of sat_positions (n_positions pairs) and orbit.  Each output pointer is nullable
 * and what is null is not computed: *latlon, malloc'd, height * 909 (lat, lon) pairs of f64, interleaved; *cos_sun,
 * height * 909 floats; *rows_out, n floats, which needs the signal (APTGPU_ERR_INVALID without).  With signal NULL,
 * n / 2080 still gives the height.  aptgpu_free all three; info nullable (its struct_size set by the caller). */
int aptgpu_geolocate(const aptgpu_context *ctx, const float *signal, size_t n, const double *sat_positions,
                     size_t n_positions, const aptgpu_orbit_settings *orbit, const aptgpu_map_settings *map,
                     const aptgpu_geoloc_settings *settings, double **latlon, float **cos_sun, float **rows_out,
                     aptgpu_geoloc_result *info, char *err, size_t err_cap);
/* The same on the CPU, in plain C++ (no GPU needed): the same source text per pixel, the C library's f64 functions. */
int aptgpu_geolocate_host(const float *signal, size_t n, const double *sat_positions, size_t n_positions,
                          const aptgpu_orbit_settings *orbit, const aptgpu_map_settings *map,
                          const aptgpu_geoloc_settings *settings, double **latlon, float **cos_sun, float **rows_out,
                          aptgpu_geoloc_result *info, char *err, size_t err_cap);
/* The sun of the series above at one instant (CPU): out[0] = declination, out[1] = sub-solar longitude in (-pi, pi],
 * both in radians. */
int aptgpu_sun_position(int64_t unix_ms, double out[2]);
/* Device-resident, chained behind the last aptgpu_plan_decode_device call on each recording's stream without a host
 * round trip (the height comes from the decode record on the device; with a rows_cap below it, rows_cap rows).
 * Exactly one of sat_positions (with n_positions) and orbit, per recording as in the map entry points.  d_latlon[i]
 * holds rows_cap[i] * 909 * 2 doubles and must be 16-byte aligned; d_cos[i] rows_cap[i] * 909 floats, d_out[i]
 * rows_cap[i] * 2080 floats, both 4-byte aligned.  Each of the three arrays is nullable: what is null is not
 * computed.  d_out[i] == d_rows[i] normalises in place; any other overlap of an output with a rows buffer or with
 * another output is APTGPU_ERR_INVALID.  Timer names: image_geoloc_track, image_geoloc_rows, image_geoloc. */
int aptgpu_plan_geolocate_device(aptgpu_plan *plan, int count, const float *const *d_rows, const size_t *rows_cap,
                                 const double *const *sat_positions, const size_t *n_positions,
                                 const aptgpu_orbit_settings *const *orbit, const aptgpu_map_settings *map,
                                 const aptgpu_geoloc_settings *settings, double *const *d_latlon,
                                 float *const *d_cos, float *const *d_out, char *err, size_t err_cap);
/* Waits for the geolocation stage of the last call and copies the records (each results[i].struct_size set). */
int aptgpu_plan_geoloc_results(aptgpu_plan *plan, int count, aptgpu_geoloc_result *results);

/* ---- fitting the map overlay to the image: yaw, hscale, vscale and the time offset ----
 * Every stage that places the image on the Earth takes yaw, hscale, vscale and the pass's time on trust.  The
 * reference leaves them to the user's eye (docs/development.md: "Look for defaults for yaw and scales?"), so the
 * definition is this library's; tests/np_fit_model.py states it in numpy.  Opt-in, a stage of its own behind
 * process(); nothing else changes when it is not called.  All real arithmetic is f64 and never contracted; everything
 * summed is an integer, so no sum depends on its order.  The defaults of aptgpu_fit_default_settings have not been
 * tried on a real pass: the stage has been judged on synthetic scenes only.
 *  - Input: an unrotated 8-bit gray image of h rows of 2080 pixels (aptgpu_process_image with rotate = No and
 *    channels = 1); a channel; the layer set and a mask of its layers (bit k = layer k; 0 = countries and lakes: states
 *    are political lines and show in no image); a long track T of h + 2 M (lat, lon) pairs in radians, M =
 *    margin_rows: image row r under shift s in [-M, M] is seen from T[M + s + r].  The track is the caller's
 *    (n_positions must be h + 2 M, else reason 7) or SGP4's on the device from an aptgpu_orbit_settings, for
 *    t = start_ms + 500 (r - M), r = 0 .. h + 2 M - 1, start_ms row 0's time as in "the satellite track" (exactly one
 *    of the two).  Initial aptgpu_map_settings (nullable: 0, 1, 1).
 *  - Edge planes, exact integers: v[r][k] = image[r][1040 ch + 86 + k], k = 0 .. 908;
 *      G[r][k] = |v[r][min(k+1, 908)] - v[r][max(k-1, 0)]| + |v[min(r+1, h-1)][k] - v[max(r-1, 0)][k]|,
 *      E_R[r][k] = the sum of G over |dr| <= R, |dk| <= R, clipped to the plane (u32).
 *    Round p of `rounds` uses R_p = radius << (rounds - 1 - p); R_0 > 64 is APTGPU_ERR_INVALID.
 *  - Sample points (host; aptgpu_fit_sample_points returns the list): the masked layers in draw order, each part, each
 *    segment p0 -> p1 in (lon, lat) degrees: n = max(1, ceil(max(|dlon|, |dlat|) / spacing_deg)) points
 *    p0 + (p1 - p0) * ((double) i / (double) n), i = 0 .. n - 1; a one-vertex part gives that vertex; the last vertex
 *    of a longer part is not a point of its own.  More than 2^22 points: APTGPU_ERR_INVALID.
 *  - Per shift s: start = T[M + s], end = T[M + s + h - 1], ref_az = geo::azimuth(start, end), D = geo::distance(start,
 *    end) (the overlay's scalars, so the fitted numbers mean what aptgpu_map_settings means), S, T, R the frame of the
 *    geolocation stage above from (start, ref_az).  For a point at (lat, lon) = (lat_deg / 180 * pi, lon_deg / 180 *
 *    pi) with unit vector P = (cos lat cos lon, cos lat sin lon, sin lat) and U.V = (U0 V0 + U1 V1) + U2 V2:
 *      a = atan2(P.T, P.S),  b = asin(clamp(P.R, -1, 1)),  valid iff P.S > 0.5
 *    (latlon_to_rel_px's (a, b) inside its pi / 3 clamp, without its acos of a value near 1).  bx[r] is the b of
 *    T[M + s + r], bx[0] = 0.
 *  - Per candidate (s, yaw, hscale, vscale) and valid point: kx = hscale / 0.0005, ky = (double) h * vscale / D,
 *      x0 = -b kx,  y = a ky + yaw x0,  e = (uint) min(max(y, 0), h - 1),  x = x0 - (-bx[e] kx),
 *      col = floor(x + 0.5) + 453,  row = floor(y + 0.5);  inside iff 0 <= col < 909 and 0 <= row < h.
 *    score = the sum of E_R[row][col] over the inside points (u64), count their number; q = (double) score / (double)
 *    count when count >= min_points.  Otherwise, and when |s| > M, hscale <= 0 or vscale <= 0, the candidate is
 *    invalid: q = -1, score 0, count 0.
 *  - Round p evaluates the grid centre + i * step_p (one product, one sum), i in [-n, n] on each of the four axes, with
 *    shift_step_p = max(1, shift_step >> p) rows and step / 2^p for the other three; candidate index
 *    ((is Ny + iy) Nh + ih) Nv + iv, each from 0.  The winner has the greatest score / count, compared as exact
 *    rationals; on a tie the lowest index wins.  It is the next round's centre, kept in the record on the device: no
 *    launch waits on the host between rounds.
 *  - Record reasons: with status APTGPU_ERR_INTERNAL, APTGPU_MAP_REASON_COUNT (7), APTGPU_SAT_REASON_SGP4 (10),
 *    APTGPU_GEOLOC_REASON_HEIGHT (15: h < 16, refused before any launch) and APTGPU_FIT_REASON_NO_CANDIDATE (17: a
 *    round without a valid candidate); with status APTGPU_OK, APTGPU_FIT_REASON_FLAT (18): the winning score of a round
 *    is 0, as on a constant image, and the result is the initial settings with shift 0.  Later rounds do not run.
 *  - scores_out (nullable; malloc'd, aptgpu_free) receives rounds * n_candidates records {u64 score, u32 count, u32 0}
 *    in round, then index order; rounds that did not run are zero.
 * Kernel groups (tools/fit_timing.py; with settings->timing their event-pair times land in the record):
 * image_fit_edge, image_fit_angles, image_fit_score.  A plan-chained form, whose height is known only on the device,
 * does not exist. */
#define APTGPU_FIT_REASON_NO_CANDIDATE 17 /* aptgpu_fit_result.reason */
#define APTGPU_FIT_REASON_FLAT 18
#define APTGPU_FIT_MAX_ROUNDS 8
#define APTGPU_FIT_MAX_POINTS (1u << 22)
#define APTGPU_FIT_MAX_CANDIDATES (1u << 20)
typedef struct aptgpu_fit_settings {
    uint32_t struct_size;  /* sizeof(aptgpu_fit_settings) */
    uint32_t flags;        /* 0; any set bit is APTGPU_ERR_INVALID */
    int32_t channel;       /* 0 = A, 1 = B */
    uint32_t layer_mask;   /* bit k = layer k (APTGPU_MAP_*); 0 = countries and lakes */
    int32_t margin_rows;   /* M >= 0 */
    int32_t rounds;        /* 1 .. 8 */
    int32_t radius;        /* the last round's box radius, >= 0; radius << (rounds - 1) <= 64 */
    int32_t min_points;    /* >= 1 */
    int32_t shift_step, n_shift;   /* rows, >= 1; >= 0 */
    int32_t n_yaw, n_hscale, n_vscale; /* >= 0 */
    int32_t timing;        /* nonzero: time the kernel groups (aptgpu_fit_result.ms_*); GPU forms only */
    double yaw_step, hscale_step, vscale_step; /* >= 0 */
    double spacing_deg;    /* > 0 */
} aptgpu_fit_settings;
typedef struct aptgpu_fit_round {
    double c_yaw, c_hscale, c_vscale; /* the centre the round started from */
    double w_yaw, w_hscale, w_vscale; /* its winner */
    double q;                         /* the winner's (double) score / (double) count; -1 without a winner */
    int32_t c_shift, w_shift;         /* rows */
    uint32_t count, index;            /* the winner's inside points and candidate index */
    uint64_t score;
} aptgpu_fit_round;
typedef struct aptgpu_fit_result {
    uint32_t struct_size;  /* the caller's sizeof(aptgpu_fit_result) */
    int32_t status;        /* APTGPU_OK or APTGPU_ERR_INTERNAL */
    int32_t reason;        /* 0, 7, 10, 15, 17, 18 */
    uint32_t height;
    uint32_t n_rounds;     /* rounds that ran */
    uint32_t n_points;     /* sample points */
    uint32_t n_candidates; /* per round */
    int32_t shift_rows;
    int64_t time_offset_ms; /* 500 * shift_rows: add it to the pass's reference time */
    double yaw, hscale, vscale, q;
    uint32_t count, done;  /* done: device bookkeeping, nonzero once the rounds have ended */
    float ms_edge, ms_angles, ms_score, ms_pick; /* with settings->timing; else 0 */
    aptgpu_fit_round round[APTGPU_FIT_MAX_ROUNDS];
} aptgpu_fit_result;
/* The suggested defaults: margin_rows 120; shift_step 8, n_shift 15; yaw_step 0.02, n 3; hscale_step and vscale_step
 * 0.04, n 3; rounds 4; radius 2; spacing_deg 0.05; min_points 64; channel A; the default mask. */
void aptgpu_fit_default_settings(aptgpu_fit_settings *out);
/* image: height rows of 2080 bytes on the host.  settings and layers are required; exactly one of sat_positions and
 * orbit; map nullable; info nullable (its struct_size set by the caller); scores_out nullable.  A failed record returns
 * APTGPU_ERR_INTERNAL with *info filled. */
int aptgpu_fit_overlay(const aptgpu_context *ctx, const uint8_t *image, size_t height, const double *sat_positions,
                       size_t n_positions, const aptgpu_orbit_settings *orbit, const aptgpu_map_layers *layers,
                       const aptgpu_map_settings *map, const aptgpu_fit_settings *settings, aptgpu_fit_result *info,
                       void **scores_out, size_t *n_scores, char *err, size_t err_cap);
/* The same for an image already in the memory of ctx's device (nullable ctx: device 0), of a height the caller
 * states, on `stream` (a hipStream_t; NULL: the default stream).  The call returns once the record has been read. */
int aptgpu_fit_overlay_device(const aptgpu_context *ctx, const uint8_t *d_image, size_t height, void *stream,
                              const double *sat_positions, size_t n_positions, const aptgpu_orbit_settings *orbit,
                              const aptgpu_map_layers *layers, const aptgpu_map_settings *map,
                              const aptgpu_fit_settings *settings, aptgpu_fit_result *info, void **scores_out,
                              size_t *n_scores, char *err, size_t err_cap);
/* The same on the CPU, in plain C++ (no GPU needed): the same source text per point and candidate, the C library's
 * f64 functions. */
int aptgpu_fit_overlay_host(const uint8_t *image, size_t height, const double *sat_positions, size_t n_positions,
                            const aptgpu_orbit_settings *orbit, const aptgpu_map_layers *layers,
                            const aptgpu_map_settings *map, const aptgpu_fit_settings *settings,
                            aptgpu_fit_result *info, void **scores_out, size_t *n_scores, char *err, size_t err_cap);
/* The sample points alone (CPU): *xy malloc'd (aptgpu_free), *n_points (lon, lat) pairs in degrees.  layer_mask 0: the
 * default mask. */
int aptgpu_fit_sample_points(const aptgpu_map_layers *layers, uint32_t layer_mask, double spacing_deg, double **xy,
                             size_t *n_points, char *err, size_t err_cap);

/* ---- land / sea / lake mask of the swath, and map-coloured false colour ----
 * Whether a point of the Earth is land, sea or lake, from the polygons of the layer set (countries.shp and lakes.shp,
 * which the overlay only ever draws as outlines).  The reference has nothing like it, so the definition is this
 * library's; tests/np_landmask_model.py states it in numpy.  Opt-in, a stage of its own; nothing else changes when it
 * is not called.
 *  - Classes, one uint8 per point: APTGPU_LAND_SEA 0, APTGPU_LAND_LAND 1, APTGPU_LAND_LAKE 2, APTGPU_LAND_INVALID 255: a
 *    NaN lat or lon, which is what the geolocation stage returns beyond 60 degrees of arc.  A point is lake if `lake`,
 *    else land if `land`, else sea: land = the crossing count against all rings of APTGPU_MAP_COUNTRIES is odd, lake =
 *    the count against all rings of APTGPU_MAP_LAKES is odd.  Even-odd over the whole layer: holes and enclaves come
 *    out right, shapes that overlap in sloppy data come out as their parity.  An absent layer counts 0.
 *  - Edges: the consecutive vertex pairs of every part, and a closing edge from the last vertex to the first where the
 *    two differ.  Coordinates are the layer's own f64 degrees (lon = x, lat = y), untouched.  A non-finite vertex is
 *    APTGPU_ERR_INVALID ("land mask: a vertex of the layer set is not finite") when the table is built:
 *    aptgpu_map_layers_set and the shapefile reader take such vertices as they come.
 *  - Point: (lat, lon) in radians; py = lat * 57.29577951308232, px = lon * 57.29577951308232 (one f64 multiply each).
 *  - Crossing rule, a ray going east; every operation is an f64 operation rounded on its own, never contracted:
 *      straddle = (y1 > py) != (y2 > py)
 *      d        = (x2 - x1) * (py - y1) - (px - x1) * (y2 - y1)
 *      crossing = straddle && (y2 > y1 ? d > 0 : d < 0)
 *    No division, no libm call, no epsilon.  The count is an integer: it does not depend on the order or grouping of
 *    the edges, so any acceleration structure is exact.  A horizontal edge never straddles and a point on a vertex or on
 *    an edge falls on the side the half-open rule gives it.
 *  - Acceleration: n_bands latitude bands (default 720, in [1, 7200]),
 *      band(y) = clamp((int) floor((y + 90.0) * (n_bands / 180.0)), 0, n_bands - 1),
 *    an edge is listed in bands band(min(y1, y2)) .. band(max(y1, y2)), horizontal edges are dropped.  band() is
 *    monotone, so the band of py lists every edge that can straddle py, each once; a point counts the edges of its own
 *    band only.  The output does not depend on n_bands.
 *  - Swath form: the points are those of the geolocation stage above (same track or orbit, same map settings), row r,
 *    video column k at mask[r * 909 + k]; the lat / lon plane is never written.  Record reasons as there: 7, 10, 15, 16.
 *    The host-array forms return APTGPU_ERR_INTERNAL with the record filled and no mask; the plan form writes 255 over
 *    the rows and counts them invalid.
 *  - The record counts the four classes and gives the table's size: non-horizontal edges per layer and the band entries
 *    of both layers together. */
#define APTGPU_LAND_SEA 0
#define APTGPU_LAND_LAND 1
#define APTGPU_LAND_LAKE 2
#define APTGPU_LAND_INVALID 255
typedef struct aptgpu_land_mask_settings {
    uint32_t struct_size;  /* sizeof(aptgpu_land_mask_settings) */
    uint32_t flags;        /* 0; any set bit is APTGPU_ERR_INVALID */
    int32_t n_bands;       /* 1 .. 7200; the bindings default to 720 */
    int32_t reserved;      /* 0 */
} aptgpu_land_mask_settings;
typedef struct aptgpu_land_mask_result {
    uint32_t struct_size;  /* the caller's sizeof(aptgpu_land_mask_result) */
    int32_t status;        /* APTGPU_OK or APTGPU_ERR_INTERNAL */
    int32_t reason;        /* 0, 7, 10, 15, 16 */
    uint32_t height;       /* whole rows (0 in the plane forms) */
    uint64_t n_sea, n_land, n_lake, n_invalid;
    uint32_t n_edges[2];   /* non-horizontal edges of countries, lakes */
    uint64_t n_band_entries; /* records of the table, both layers */
} aptgpu_land_mask_result;
/* The swath form: height rows, exactly one of sat_positions (n_positions pairs) and orbit, map nullable (0, 1, 1),
 * layers required with countries or lakes present, settings nullable (720 bands).  *mask: malloc'd, height * 909
 * bytes (aptgpu_free); info nullable (its struct_size set by the caller).  Refused before a device is touched
 * (APTGPU_ERR_INVALID): a null or empty layer set, a struct_size that is too small, a flag, n_bands out of range. */
int aptgpu_land_mask(const aptgpu_context *ctx, size_t height, const double *sat_positions, size_t n_positions,
                     const aptgpu_orbit_settings *orbit, const aptgpu_map_settings *map,
                     const aptgpu_map_layers *layers, const aptgpu_land_mask_settings *settings, uint8_t **mask,
                     aptgpu_land_mask_result *info, char *err, size_t err_cap);
/* The same on the CPU, in plain C++ (no GPU needed). */
int aptgpu_land_mask_host(size_t height, const double *sat_positions, size_t n_positions,
                          const aptgpu_orbit_settings *orbit, const aptgpu_map_settings *map,
                          const aptgpu_map_layers *layers, const aptgpu_land_mask_settings *settings, uint8_t **mask,
                          aptgpu_land_mask_result *info, char *err, size_t err_cap);
/* The plane form: n (lat, lon) pairs of f64 in radians, interleaved, of any shape (the plane of aptgpu_geolocate, the
 * lat / lon of a map grid).  latlon null or not 8-byte aligned: APTGPU_ERR_INVALID.  *mask: n bytes. */
int aptgpu_land_mask_plane(const aptgpu_context *ctx, const double *latlon, size_t n, const aptgpu_map_layers *layers,
                           const aptgpu_land_mask_settings *settings, uint8_t **mask, aptgpu_land_mask_result *info,
                           char *err, size_t err_cap);
int aptgpu_land_mask_plane_host(const double *latlon, size_t n, const aptgpu_map_layers *layers,
                                const aptgpu_land_mask_settings *settings, uint8_t **mask,
                                aptgpu_land_mask_result *info, char *err, size_t err_cap);
/* Device-resident, chained behind the last aptgpu_plan_decode_device call on each recording's stream (the height comes
 * from the decode record on the device; with a rows_cap below it, rows_cap rows).  Tracks and orbits as
 * aptgpu_plan_geolocate_device.  d_mask[i] holds rows_cap[i] * 909 bytes and may not overlap a rows buffer or another
 * mask.  The table is built once per layer set and band count and uploaded once per slot.  Timer names:
 * image_geoloc_track, image_geoloc_rows, image_land_mask. */
int aptgpu_plan_land_mask_device(aptgpu_plan *plan, int count, const float *const *d_rows, const size_t *rows_cap,
                                 const double *const *sat_positions, const size_t *n_positions,
                                 const aptgpu_orbit_settings *const *orbit, const aptgpu_map_settings *map,
                                 const aptgpu_map_layers *layers, const aptgpu_land_mask_settings *settings,
                                 uint8_t *const *d_mask, char *err, size_t err_cap);
/* Waits for the land mask stage of the last call and copies the records (each results[i].struct_size set). */
int aptgpu_plan_land_mask_results(aptgpu_plan *plan, int count, aptgpu_land_mask_result *results);
/* Map-coloured false colour: image is the un-rotated gray image of aptgpu_process_image (height rows of 2080 bytes),
 * mask a swath mask of mask_height rows of 909 bytes (mask_height != height: APTGPU_ERR_INVALID), palettes three
 * 256 x 256 x 3 RGB images for sea, land and lake, each of palette_bytes[k] bytes (anything but 196608:
 * APTGPU_ERR_INVALID), tunes = {ch_a_tune_start, ch_a_tune_end, ch_b_tune_start, ch_b_tune_end}.  *rgba: malloc'd,
 * height * 2080 * 4 bytes.  Every pixel is (v, v, v, 255) except channel A's video columns x in [86, 995): there
 * c = mask[y * 909 + x - 86], and for c in {0, 1, 2} the pixel is palette_c[val_b][val_a] with alpha 255, (val_a, val_b)
 * from tune_input_values (processing.rs:125-140) of the pixel and of its channel-B partner 1040 columns on, as in
 * aptgpu_process_image's false colour; c == 255 stays gray.  Rotation is the caller's business, afterwards. */
int aptgpu_false_color_masked(const aptgpu_context *ctx, const uint8_t *image, size_t height, const uint8_t *mask,
                              size_t mask_height, const uint8_t *const *palettes, const size_t *palette_bytes,
                              const float tunes[4], uint8_t **rgba, char *err, size_t err_cap);
int aptgpu_false_color_masked_host(const uint8_t *image, size_t height, const uint8_t *mask, size_t mask_height,
                                   const uint8_t *const *palettes, const size_t *palette_bytes, const float tunes[4],
                                   uint8_t **rgba, char *err, size_t err_cap);

/* ====================================================================== */
/* 4b. FM demodulation of IQ recordings, in front of decode() */
/* ====================================================================== */
/* The reference reads audio only ("IQ files are not supported, these files should be FM demodulated into WAVs
 * first", docs/usage.md), so the definition is this library's; tests/np_fm_model.py states it in numpy f64.  Opt-in, a
 * stage of its own: IQ frames in, audio at fs / D out, which any decode entry point takes at that rate.
 *  - Input: N complex frames, interleaved I then Q.  APTGPU_IQ_U8: v - 127.5 (the rtl_sdr convention); APTGPU_IQ_S8;
 *    APTGPU_IQ_S16: little endian, `as f32`; APTGPU_IQ_F32: the bits.  Values are never scaled.
 *    APTGPU_FM_SWAP_IQ exchanges I and Q.
 *  - Taps: h = aptgpu_filter_design(Lowpass{cutout_pi_rad = 2 channel_cutout_hz / fs, channel_atten,
 *    delta_w_pi_rad = 2 channel_delta_hz / fs}), the quotients in f32 as Freq::hz takes them (2.f * f / (float) fs);
 *    T is its length.
 *  - Mix: pw = (uint32) llround(shift_hz / fs * 2^32) in two's complement; theta_i = 2 pi ((uint32) i * pw) / 2^32,
 *    the product in 32-bit unsigned arithmetic (exact for every i); u[i] = x[i] * e^{-j theta_i}.  The frequency
 *    actually used is (int32) pw * fs / 2^32 (aptgpu_fm_info.shift_hz_used).  pw == 0 skips the mix.  The phasor of
 *    frame i is that of the integer phase at i - i % 8, advanced i % 8 times by one f32 complex multiply with
 *    e^{-j theta_1}.
 *  - Filter and decimate, the valid part only: v[m] = sum_{k < T} h[k] * u[m D + T - 1 - k], m in [0, M),
 *    M = (N - T) / D + 1 for N >= T, else 0; summed from k = T - 1 down to 0.
 *  - Discriminate: a[m] = (fs_out / (2 pi deviation_hz)) * atan2(Im p, Re p), p = v[m + 1] * conj(v[m]),
 *    m in [0, M - 1): n_out = max(M - 1, 0) floats at fs_out = fs / D.  p == 0 gives 0.  A non-finite component of
 *    v[m] or v[m + 1] gives NaN: NaN and +-Inf frames reach exactly the outputs whose two windows contain them.
 *    n_out == 0 is APTGPU_OK with an empty result (the decode behind it says "too short" in its own words).
 *  - All device arithmetic is f32, contraction allowed; nothing is bit-pinned against the model.  With
 *    e = sqrt(2) * 2 (T + 8) * 2^-24 * sum|h| * max|x| an output is within
 *    g (e / |v[m]| + e / |v[m + 1]|) + 4 * 2^-24 * max(|a|, 1e-3 g), g = fs_out / (2 pi deviation_hz), of the model.
 *  - Refused on the host, before a device is touched, with APTGPU_ERR_INVALID and a text naming the field: a short
 *    struct_size; an unknown format or flag; sample_rate_hz == 0; decimation == 0 or > 4096; sample_rate_hz %
 *    decimation != 0 (the output rate is a whole number of Hz); a non-finite or non-positive channel_cutout_hz,
 *    channel_delta_hz or deviation_hz; a non-finite shift_hz or |shift_hz| > fs / 2; channel_atten not finite or not
 *    above 8 dB; channel_cutout_hz + channel_delta_hz / 2 > fs_out / 2 (the filter would alias); more than 4096 taps. */
#define APTGPU_IQ_U8 0
#define APTGPU_IQ_S8 1
#define APTGPU_IQ_S16 2
#define APTGPU_IQ_F32 3
#define APTGPU_FM_SWAP_IQ 1u
#define APTGPU_FM_MAX_BATCH 64 /* recordings of one aptgpu_fm_demodulate_device call */
typedef struct aptgpu_fm_settings {
    uint32_t struct_size;     /* sizeof(aptgpu_fm_settings) */
    int32_t format;           /* APTGPU_IQ_* */
    uint32_t sample_rate_hz;  /* fs, complex frames per second */
    uint32_t decimation;      /* D >= 1 */
    double shift_hz;          /* the signal's offset from the recording's centre */
    float channel_cutout_hz;  /* usually 18000 */
    float channel_atten;      /* dB, usually 40 */
    float channel_delta_hz;   /* usually 8000 */
    float deviation_hz;       /* usually 17000 (APT) */
    uint32_t flags;           /* APTGPU_FM_SWAP_IQ */
    uint32_t reserved;
} aptgpu_fm_settings;
/* The usual values above, format U8, D = 1, no shift; sample_rate_hz is left 0 for the caller. */
void aptgpu_fm_default_settings(aptgpu_fm_settings *settings);

typedef struct aptgpu_fm aptgpu_fm;
typedef struct aptgpu_fm_info {
    uint32_t struct_size; /* in: sizeof(aptgpu_fm_info) */
    uint32_t fs_out;      /* Hz */
    uint32_t n_taps;      /* T */
    uint32_t decimation;  /* D */
    uint32_t pw;          /* phase increment per frame, 2^32 = one turn */
    uint32_t reserved;
    double shift_hz_used;
    const float *taps;    /* h, n_taps floats, owned by the demodulator */
} aptgpu_fm_info;
/* Checks the settings, designs the taps and uploads them, once.  Runs on ctx->device and ctx->stream (NULL: the null
 * stream); ctx NULL = device 0. */
int aptgpu_fm_create(const aptgpu_context *ctx, const aptgpu_fm_settings *settings, aptgpu_fm **fm, char *err,
                     size_t err_cap);
void aptgpu_fm_destroy(aptgpu_fm *fm);
int aptgpu_fm_get_info(const aptgpu_fm *fm, aptgpu_fm_info *info);
size_t aptgpu_fm_out_len(const aptgpu_fm *fm, size_t n_frames);
/* The checks and the design alone (no GPU): info as above, *taps malloc'd (aptgpu_free), info->taps NULL. */
int aptgpu_fm_design(const aptgpu_fm_settings *settings, aptgpu_fm_info *info, float **taps, char *err, size_t err_cap);
/* Host arrays: iq holds n_frames * 2 components; *audio malloc'd (aptgpu_free), *n_out floats at *rate_hz. */
int aptgpu_fm_demodulate(const aptgpu_context *ctx, const aptgpu_fm_settings *settings, const void *iq, size_t n_frames,
                         float **audio, size_t *n_out, uint32_t *rate_hz, char *err, size_t err_cap);
/* The same on the CPU, in plain C++ (no GPU needed): the same f32 arithmetic except sincos and atan2 (and the
 * compiler's contraction). */
int aptgpu_fm_demodulate_host(const aptgpu_fm_settings *settings, const void *iq, size_t n_frames, float **audio,
                              size_t *n_out, uint32_t *rate_hz, char *err, size_t err_cap);
/* Device-resident: `count` (<= APTGPU_FM_MAX_BATCH) recordings in one kernel launch, asynchronous on the
 * demodulator's stream, with no host synchronisation and no allocation.  This is the way to put work in front of a
 * plan: a plan created on the same stream orders its decode after it.  d_iq[i]: n_frames[i] frames, aligned to one
 * component (1, 2 or 4 bytes); 16-byte alignment lets the loads be 16 bytes wide, with the same result bit for bit.
 * d_audio[i] receives aptgpu_fm_out_len(fm, n_frames[i]) floats and nothing behind them.  A null pointer (with
 * something to read or write), a misaligned one or audio_cap[i] below the output length is APTGPU_ERR_INVALID before
 * anything is enqueued.  A recording's result does not depend on its place in the batch. */
int aptgpu_fm_demodulate_device(aptgpu_fm *fm, int count, const void *const *d_iq, const size_t *n_frames,
                                float *const *d_audio, const size_t *audio_cap, char *err, size_t err_cap);
/* A two-channel WAV (16-bit integer or 32-bit float) as the IQ recording, through aptgpu_wav_parse: the rate and the
 * format come from the header and overrule the settings' fields.  Anything else is APTGPU_ERR_UNSUPPORTED. */
int aptgpu_fm_demodulate_wav(const aptgpu_context *ctx, const aptgpu_fm_settings *settings, const void *file_bytes,
                             size_t n, float **audio, size_t *n_out, uint32_t *rate_hz, char *err, size_t err_cap);

/* ====================================================================== */
/* 4b'. AFC: follow the carrier of an IQ recording, in front of §4b */
/* ====================================================================== */
/* §4b needs shift_hz exactly; a recording's carrier is off by the tuner's error (30-60 ppm at 137 MHz: 4-8 kHz) and by
 * a Doppler shift that changes through the pass (+-3.4 kHz).  This stage estimates the carrier block by block from the
 * raw frames and demodulates with an NCO that follows the estimates.  The reference has nothing comparable, so the
 * definition is this library's; tests/np_afc_model.py states it in numpy.  Opt-in: nothing of §4b changes.
 *
 * Settings (aptgpu_afc_settings) next to the aptgpu_fm_settings of §4b, with fs = sample_rate_hz:
 *   block_frames  B, a power of two in 64 ... 2^20 (default 4096)
 *   lag           L in 1 ... 64, or 0 = auto: floor(fs / (4 (max_offset_hz + deviation_hz))) clamped to 1 ... 64
 *   smooth_blocks W, odd, 1 ... 1023 (default 15)
 *   max_offset_hz finite, > 0 (default 15000): estimates further than this from shift_hz are not believed
 *   min_coherence in [0, 1) (default 0.05)
 * pw_base is §4b's pw of shift_hz.  A recording of n frames has nb = ceil(n / B) blocks, nb <= 2^20.
 *
 * Stage A, block sums.  Components are integers: u8 2 raw - 255 (twice §4b's value), s8 / s16 the value; SWAP_IQ is
 *   applied.  For block b, over its frames i in [b B, min((b + 1) B, n)):
 *     re[b] = sum I[i + L] I[i] + Q[i + L] Q[i]   over i with i + L < n (the terms reach into the next block)
 *     im[b] = sum Q[i + L] I[i] - I[i + L] Q[i]   over the same i
 *     en[b] = sum I[i]^2 + Q[i]^2                 over all frames of the block
 *   exact in int64 (a block of s16 at -32768 reaches 2^51, a window of 1023 such 2^61).  F32: the components are the
 *   floats; products and sums are f64, in any order.  The sums are returned as f64 triples {re, im, en} per block: for
 *   the integer formats that conversion is exact.
 * Stage B, the table.  All arithmetic is f64 without contraction; adds run in ascending block order from 0.
 *   1. The window of b is [max(b - W / 2, 0), min(b + W / 2, nb - 1)]; R and E are its sums of (re, im) and en.
 *   2. coherence[b] = sqrt(Rre^2 + Rim^2) / E, 0 where E == 0; returned as f32 (a NaN as 0x7FC00000).
 *   3. If a component of R or E is not finite the block is not good and has no estimate.  Otherwise
 *        q = (uint32) llrint(atan2(Rim, Rre) / (2 pi) * 2^32), d = (int32)(q - (uint32)(L * pw_base)),
 *        rel = llround((double) d / L), est[b] = pw_base + rel.
 *   4. b is good iff coherence[b] (the f64 value) >= min_coherence and |rel| * fs / 2^32 <= max_offset_hz.
 *   5. Hold: pw[b] = est[j], j the nearest good block at or before b; if there is none, the first good block after b;
 *      if no block is good, pw[b] = pw_base.
 *   6. phase0[0] = 0, phase0[b + 1] = phase0[b] + B * pw[b] in uint32.
 *   7. step[b] = (f32) cos t, (f32) -sin t in f64 with t = (int32) pw[b] * pi / 2^31: §4b's step of pw[b].
 *   Per block: the 16-byte aptgpu_afc_record {pw, phase0, step_re, step_im}, coherence (f32) and good (u8).
 * Stage C, tracked demodulation: §4b with one change.  The phase of frame i is phase0[b] + (uint32)(i - b B) * pw[b],
 *   b = i / B.  A run of 8 lies inside one block; its first phasor is that of the phase at i - i % 8 and its step is
 *   step[b].  The mix is always made (also where every pw is 0).  Filter, discriminate, the non-finite rules and §4b's
 *   bound are unchanged, with the model's phasor that of the table's phase.  A table whose every block has
 *   pw = pw_base != 0 and phase0 = (uint32)(b B pw_base) gives §4b's bits.
 * The frequency steps between blocks are a few Hz (Doppler moves by at most about 100 Hz / s): under 1e-3 of the
 * deviation, as DC that the AM demodulation behind it removes.  Not built: a chirp inside blocks, DC-spike removal, a
 * streaming or causal form (§4f's streams are untouched), any narrowing of the estimator's band: stage A sees the whole
 * recorded band, so a stronger signal elsewhere in it wins.
 *
 * Refused on the host, before a device is touched, with APTGPU_ERR_INVALID and a text naming the field: everything
 * §4b refuses; a short struct_size; block_frames not a power of two or outside 64 ... 2^20; lag above 64;
 * smooth_blocks even or outside 1 ... 1023; max_offset_hz not finite or not positive; min_coherence not in [0, 1);
 * n_frames with more than 2^20 blocks; n_blocks that is not ceil(n_frames / B) where a table is passed in. */
typedef struct aptgpu_afc_settings {
    uint32_t struct_size;   /* sizeof(aptgpu_afc_settings) */
    uint32_t block_frames;  /* B */
    uint32_t lag;           /* L; 0 = auto */
    uint32_t smooth_blocks; /* W */
    float max_offset_hz;
    float min_coherence;
} aptgpu_afc_settings;
void aptgpu_fm_afc_default_settings(aptgpu_afc_settings *settings);

typedef struct aptgpu_afc_record {
    uint32_t pw;     /* phase increment per frame of the block, 2^32 = one turn */
    uint32_t phase0; /* phase of the block's first frame */
    float step_re, step_im;
} aptgpu_afc_record;

typedef struct aptgpu_afc_info {
    uint32_t struct_size; /* in: sizeof(aptgpu_afc_info) */
    uint32_t block_frames, lag, smooth_blocks; /* lag: the one used */
    uint32_t pw_base;
    uint32_t sample_rate_hz;
    double max_offset_hz, min_coherence;
} aptgpu_afc_info;
/* The checks of both settings and what they come to (no GPU). */
int aptgpu_fm_afc_design(const aptgpu_fm_settings *fm_settings, const aptgpu_afc_settings *settings,
                         aptgpu_afc_info *info, char *err, size_t err_cap);

/* Stage A on host arrays: *sums malloc'd (aptgpu_free), 3 * *n_blocks doubles, {re, im, en} per block. */
int aptgpu_fm_afc_sums(const aptgpu_context *ctx, const aptgpu_fm_settings *fm_settings,
                       const aptgpu_afc_settings *settings, const void *iq, size_t n_frames, double **sums,
                       size_t *n_blocks, char *err, size_t err_cap);
int aptgpu_fm_afc_sums_host(const aptgpu_fm_settings *fm_settings, const aptgpu_afc_settings *settings, const void *iq,
                            size_t n_frames, double **sums, size_t *n_blocks, char *err, size_t err_cap);
/* Stage B on the caller's sums (3 * n_blocks doubles): *table, *coherence and *good malloc'd (aptgpu_free), n_blocks
 * entries each; coherence and good nullable. */
int aptgpu_fm_afc_estimate(const aptgpu_context *ctx, const aptgpu_fm_settings *fm_settings,
                           const aptgpu_afc_settings *settings, const double *sums, size_t n_blocks,
                           aptgpu_afc_record **table, float **coherence, uint8_t **good, char *err, size_t err_cap);
int aptgpu_fm_afc_estimate_host(const aptgpu_fm_settings *fm_settings, const aptgpu_afc_settings *settings,
                                const double *sums, size_t n_blocks, aptgpu_afc_record **table, float **coherence,
                                uint8_t **good, char *err, size_t err_cap);
/* Stage C with the caller's table of n_blocks = ceil(n_frames / B) records; the outputs as aptgpu_fm_demodulate's. */
int aptgpu_fm_demodulate_tracked(const aptgpu_context *ctx, const aptgpu_fm_settings *fm_settings,
                                 const aptgpu_afc_settings *settings, const void *iq, size_t n_frames,
                                 const aptgpu_afc_record *table, size_t n_blocks, float **audio, size_t *n_out,
                                 uint32_t *rate_hz, char *err, size_t err_cap);
int aptgpu_fm_demodulate_tracked_host(const aptgpu_fm_settings *fm_settings, const aptgpu_afc_settings *settings,
                                      const void *iq, size_t n_frames, const aptgpu_afc_record *table, size_t n_blocks,
                                      float **audio, size_t *n_out, uint32_t *rate_hz, char *err, size_t err_cap);
/* All three stages.  table, coherence, good and n_blocks are nullable: where given they receive stage B's outputs,
 * malloc'd (aptgpu_free). */
int aptgpu_fm_demodulate_afc(const aptgpu_context *ctx, const aptgpu_fm_settings *fm_settings,
                             const aptgpu_afc_settings *settings, const void *iq, size_t n_frames, float **audio,
                             size_t *n_out, uint32_t *rate_hz, aptgpu_afc_record **table, float **coherence,
                             uint8_t **good, size_t *n_blocks, char *err, size_t err_cap);
int aptgpu_fm_demodulate_afc_host(const aptgpu_fm_settings *fm_settings, const aptgpu_afc_settings *settings,
                                  const void *iq, size_t n_frames, float **audio, size_t *n_out, uint32_t *rate_hz,
                                  aptgpu_afc_record **table, float **coherence, uint8_t **good, size_t *n_blocks,
                                  char *err, size_t err_cap);
/* Device-resident, behind an aptgpu_fm (whose settings, device and stream it takes; the aptgpu_fm must be alive in
 * every aptgpu_fm_afc_demodulate_device call; aptgpu_fm_afc_destroy does not need it):
 * the work space for APTGPU_FM_MAX_BATCH recordings of up to max_frames frames is allocated here, once. */
typedef struct aptgpu_fm_afc aptgpu_fm_afc;
int aptgpu_fm_afc_create(aptgpu_fm *fm, const aptgpu_afc_settings *settings, size_t max_frames, aptgpu_fm_afc **afc,
                         char *err, size_t err_cap);
void aptgpu_fm_afc_destroy(aptgpu_fm_afc *afc);
/* `count` (<= APTGPU_FM_MAX_BATCH) recordings through the three stages: three kernel launches on the demodulator's
 * stream, no allocation and no host synchronisation.  d_iq, n_frames, d_audio, audio_cap as
 * aptgpu_fm_demodulate_device.  d_sums, d_table, d_coherence, d_good: nullable arrays of `count` nullable device
 * pointers; where one is given, recording i's stage-A sums (3 doubles per block, 8-byte aligned) or its table
 * (ceil(n_frames[i] / B) entries; d_table[i] 16-byte aligned, d_coherence[i] 4-byte) is left there, otherwise in the
 * work space.  n_frames[i] above max_frames is refused. */
int aptgpu_fm_afc_demodulate_device(aptgpu_fm_afc *afc, int count, const void *const *d_iq, const size_t *n_frames,
                                    float *const *d_audio, const size_t *audio_cap, double *const *d_sums,
                                    aptgpu_afc_record *const *d_table, float *const *d_coherence,
                                    uint8_t *const *d_good, char *err, size_t err_cap);

/* ====================================================================== */
/* 4c. flywheel sync: row starts tracked through noise and dropouts */
/* ====================================================================== */
/* find_sync (decode.rs:204-263) keeps the largest value of an unnormalised +-1 correlation inside 0.8 of a row: one
 * noise maximum moves a row by up to half a row, a dropout shuffles the lines, and under five frames the decode fails.
 * The reference lists the remedy among its open items ("Improve syncing ... more resilient to noise, maybe working
 * with the mean and variance", docs/development.md:148) and has no code for it, so the definition is this library's;
 * tests/np_track_model.py states it in numpy.  Opt-in, a stage of its own behind the front end: nothing else changes
 * when it is not called.
 *
 * All arithmetic is IEEE f32 in the order written; every product is rounded before it is added or subtracted (no
 * contraction); division and square root are the correctly rounded ones.
 *
 * Input   x[0..n): the low-passed envelope at the work rate (decode()'s "filter_result" step, a plan's `filtered`
 *         buffer).  pw = work_rate / 4160 must be an integer in 1..8; L = 2080 pw, G = 38 pw, M = n - G; g[j] is
 *         generate_sync_frame's template.  n < L + G is refused.
 * Score   for every i in [0, M):
 *             c  = 0, then +- x[i+j] for j ascending                 (the reference's chain)
 *             S1 = 0 (+ x[i+j]),  S2 = 0 (+ x[i+j]*x[i+j]),  j ascending
 *             m = S1 / f32(G);  V = S2 - S1*m
 *             num = c + S1 * f32(10.0/38.0)                          (the template minus its mean, -10/38)
 *             den = sqrt(V * f32(G * (1 - (10/38)^2)))               (constant evaluated in f64, rounded once)
 *             s[i] = num / den  if V > 1e-4f * S2 and num, den finite;  else 0
 *         the zero-mean normalised cross-correlation.  The relative floor makes silence, a constant, NaN / +-Inf
 *         windows and overflowing squares score 0 (no evidence) instead of noise; s is bit-identical under a
 *         power-of-two gain while no square overflows or underflows.
 * Track   settings max_jitter = w (work samples, 0..64, default 8; 4 w < L) and penalty = lambda (finite, >= 0,
 *         default 0.1).  In chunks of C = L - w positions, ascending (bp: the back-pointer kept per position):
 *             cur = 0 and bp = START if i < L, else -inf
 *             for d in 0, -1, +1, -2, +2, ..., -w, +w:   j = i - L - d
 *                 if j >= 0:  v = best[j] - (lambda * f32(|d|));  if v > cur: cur = v, bp = d    (strictly greater)
 *             best[i] = s[i] + cur
 *         End: the first maximum of best over [max(0, M - L), M).  Positions: follow bp back to START; they come out
 *         ascending, K of them.  Rows: every p_k with p_k + L <= n gives row[c] = x[p_k + pw c], c < 2080 (the
 *         sample's own bits).  Per position also s[p_k], the caller's lock indicator (near 1 on a clean frame, near
 *         0 in noise). */
typedef struct aptgpu_track_settings {
    uint32_t struct_size; /* sizeof(aptgpu_track_settings) */
    uint32_t max_jitter;  /* w: 0..64 work samples a row start may move against the previous one */
    float penalty;        /* lambda: finite, >= 0; what one sample of such a move costs, in units of s */
    uint32_t reserved;
} aptgpu_track_settings;
typedef struct aptgpu_track_result {
    uint32_t struct_size; /* sizeof(aptgpu_track_result): set by the caller of the host-array forms and of
                             aptgpu_plan_track_results (every record), written by the device otherwise */
    int32_t status;       /* APTGPU_OK or APTGPU_ERR_INTERNAL */
    int32_t reason;       /* 0; 1 the decode before it refused the recording (less than 10 rows: no filtered signal);
                             2 shorter than L + G; 3 more positions than the list holds; 4 ok, rows truncated to
                             rows_cap */
    uint32_t n_positions; /* K */
    uint32_t n_rows;      /* rows written: the positions with p + L <= n, never more than rows_cap */
    uint32_t end;         /* the path's last position */
    uint64_t n;           /* work samples of the recording */
    float total;          /* best[end]: the path's score sum minus its penalties */
    uint32_t reserved;
} aptgpu_track_result;
#define APTGPU_TRACK_MAX_JITTER 64
/* settings nullable (= w 8, lambda 0.1) in every entry point below; outputs malloc'd (aptgpu_free).  Every refusal —
 * a struct_size not set, w > 64, 4 w >= L, a negative or non-finite penalty, a work rate that is no multiple of 4160 Hz
 * or above 8 x 4160, n < L + G — is APTGPU_ERR_INVALID before a device is touched.
 *
 * aptgpu_track_sync: `count` (>= 1) host signals of n[i] work-rate samples through one launch per kernel.
 * positions[i] / scores[i]: results[i].n_positions entries; rows (nullable): rows[i] holds results[i].n_rows * 2080
 * floats.  results[i].struct_size must be set. */
int aptgpu_track_sync(const aptgpu_context *ctx, int count, const float *const *signals, const size_t *n,
                      uint32_t work_rate_hz, const aptgpu_track_settings *settings, uint64_t **positions,
                      float **scores, float **rows /* nullable */, aptgpu_track_result *results, char *err,
                      size_t err_cap);
/* The same for one signal on the CPU, in plain C++ (no GPU needed): the same bits.  score_out (nullable): all n - G
 * values of s. */
int aptgpu_track_sync_host(const float *signal, size_t n, uint32_t work_rate_hz, const aptgpu_track_settings *settings,
                           uint64_t **positions, float **scores, float **rows /* nullable */,
                           float **score_out /* nullable */, aptgpu_track_result *info, char *err, size_t err_cap);
/* s alone: scores[i] receives n[i] - G floats. */
int aptgpu_sync_score(const aptgpu_context *ctx, int count, const float *const *signals, const size_t *n,
                      uint32_t work_rate_hz, float **scores, char *err, size_t err_cap);
/* Device-resident: re-aligns the first `count` recordings of the plan's last decode call from their slots' filtered
 * buffers (in either layout the front end left) into d_rows[i] (rows_cap[i] rows of 2080 floats, which may be the
 * decode's own buffer), chained behind the decode on the call's stream: asynchronous, no host synchronisation, no
 * allocation after the first use on a slot.  The sample count comes from the decode record on the device.  Works on
 * sync = 0 and sync = 1 plans, and where the decode's own record says "less than 5 sync frames"; a recording the
 * decode refused as shorter than 10 rows is recorded with reason 1.  The decode's own records, positions and rows (in
 * another buffer) are left alone.  Timer names: track_score, track_dp, track_rows. */
int aptgpu_plan_track_device(aptgpu_plan *plan, int count, const aptgpu_track_settings *settings, float *const *d_rows,
                             const size_t *rows_cap, char *err, size_t err_cap);
/* Waits for the stage of the last call and copies the records (every results[i].struct_size set). */
int aptgpu_plan_track_results(aptgpu_plan *plan, int count, aptgpu_track_result *results);
/* Positions and their scores of recording i of the last aptgpu_plan_track_device call: min(cap, K) entries each
 * (pos, scores nullable), K in *n_positions. */
int aptgpu_plan_track_positions(aptgpu_plan *plan, int i, uint64_t *pos, float *scores, size_t cap,
                                size_t *n_positions);
/* Input signal -> tracked rows in one call: the front end of a sync = 0 plan (same settings, same refusals as
 * aptgpu_decode, "less than 10 rows" included), then the stage.  *rows_out: *n_out = rows * 2080 floats exactly as the
 * stage gathers them (no final filter pass: the sample's own bits); positions / scores (nullable): info->n_positions
 * entries.  info nullable. */
int aptgpu_decode_tracked(const aptgpu_context *ctx, const aptgpu_settings *settings, const float *signal, size_t n,
                          uint32_t input_rate_hz, const aptgpu_track_settings *track, float **rows_out, size_t *n_out,
                          uint64_t **positions /* nullable */, float **scores /* nullable */,
                          aptgpu_track_result *info /* nullable */, char *err, size_t err_cap);

/* ====================================================================== */
/* 4d. live decode: audio pushed in chunks, finished rows handed back */
/* ====================================================================== */
/* The reference lists "Live decoding, from a TCP stream or using librtlsdr or from audio" among its open items
 * (docs/development.md:151).  A stream takes the recording in pushes of any size and hands out, after every push, the
 * image rows that are FINAL: a row (a work-rate sample, a correlation, a peak) is final when it exists in strict
 * decode() of the complete recording with the same bits for EVERY continuation of what has been pushed, the empty one
 * included.  It is released in the first push after which that holds — never earlier, never later — so the rows of all
 * pushes and of aptgpu_stream_finish, concatenated, are bit-identical to decode() of the whole recording, and how many
 * come out of which push is a function of the chunk boundaries alone.
 *   work sample i   final once every input sample its resampler window reads has been pushed (l > 1), or i < n / m
 *                   (l == 1); finish adds the tail the reference computes with absent samples skipped (dsp.rs:257)
 *   position i      scanned once i + 38 pw < work_len (decode.rs:225)
 *   row of peak k   final once a later peak was pushed and p_k + samples_per_row < work_len; the last peak never gives a
 *                   row (decode.rs:125-131); sync == 0: row r once (r + 1) samples_per_row <= work_len
 * aptgpu_stream_finish then reports what decode() would: "Got less than 10 rows of samples, ..." or "Found less than 5
 * sync frames, ..." with APTGPU_ERR_INTERNAL.  The one difference from decode(): rows released before such an error
 * stay released (a failing finish itself releases none).
 * Strict arithmetic only: APTGPU_MODE_FAST, APTGPU_MODE_FP16_TAPS, the matrix-core switch, export_wav and
 * export_resample_filtered are APTGPU_ERR_UNSUPPORTED; no step callback is invoked.  work_rate must be a multiple of
 * 4160 Hz (the reference's message, APTGPU_ERR_INTERNAL) with sync == 0 as well.  All state lives on the device in a
 * record and three rings of fixed size (input, F, correlation); nothing grows with the recording. */
#define APTGPU_STREAM_F32 0 /* samples are f32, as wav::load_wav produces them */
#define APTGPU_STREAM_S16 1 /* mono int16 (the value `as f32`) */
typedef struct aptgpu_stream aptgpu_stream;
typedef struct aptgpu_stream_settings {
    uint32_t struct_size;   /* sizeof(aptgpu_stream_settings); 0 is refused */
    uint32_t input_rate_hz;
    int32_t sync;
    int32_t format;         /* APTGPU_STREAM_* */
    uint32_t max_push;      /* samples one launch sequence takes (longer pushes are split); 0 = 65536; at most 2^24 */
    uint32_t reserved;
} aptgpu_stream_settings;
typedef struct aptgpu_stream_info {
    uint32_t struct_size;   /* set by the caller */
    uint32_t work_rate;
    uint32_t pw;
    uint32_t samples_per_row;
    uint32_t l, m;
    uint32_t n_resample_taps, n_lowpass_taps;
    uint32_t max_push;
    uint32_t cap_in, cap_f, cap_corr; /* ring capacities in samples (powers of two; cap_corr 0 when sync == 0) */
    uint64_t device_bytes;  /* what the stream holds on the device (host handle: in host memory): the record, the rings,
                               the taps — fixed at creation — and the host-fed form's staging of 64 rows, which grows only
                               when one push can release more */
} aptgpu_stream_info;
typedef struct aptgpu_stream_result {
    uint32_t struct_size;   /* set by the caller */
    int32_t status;         /* APTGPU_OK or APTGPU_ERR_INTERNAL */
    int32_t reason;         /* 0; 1 "<10 rows"; 2 "<5 sync frames"; 5-7 an internal bound was exceeded (a defect: the
                               stream stays failed until reset) */
    uint32_t n_rows;        /* rows released by this push (or finish) */
    uint64_t rows_total;    /* rows released so far */
    uint64_t n_sync;        /* peaks found so far (0 when sync == 0) */
    uint64_t n_in;          /* samples pushed so far */
    uint64_t work_len;      /* final work-rate samples */
    uint64_t scan_pos;      /* correlation positions the picker has consumed (0 when sync == 0) */
} aptgpu_stream_result;
/* ctx nullable (device 0, strict, a stream of its own).  Every refusal happens before a device is touched. */
int aptgpu_stream_create(const aptgpu_context *ctx, const aptgpu_settings *settings,
                         const aptgpu_stream_settings *stream_settings, aptgpu_stream **out, char *err, size_t err_cap);
/* The same state machine in plain C++ on the CPU (no GPU needed): same handle type, same bits, same release schedule;
 * ctx (nullable) is read for its mode only.  The *_device entry points refuse such a handle. */
int aptgpu_stream_create_host(const aptgpu_context *ctx, const aptgpu_settings *settings,
                              const aptgpu_stream_settings *stream_settings, aptgpu_stream **out, char *err,
                              size_t err_cap);
void aptgpu_stream_destroy(aptgpu_stream *stream);
int aptgpu_stream_get_info(const aptgpu_stream *stream, aptgpu_stream_info *info);
/* Back to the state after creation (nothing is reallocated). */
int aptgpu_stream_reset(aptgpu_stream *stream, char *err, size_t err_cap);
/* Upper bound of the rows a push of n more samples — or, n == 0, a finish — can release now.  One event of the
 * reference's picker can push any number of peaks at once (decode.rs:244-246: a correlation that climbs for rows on end
 * is followed by as many copies as rows went by), so the bound does not follow from n alone: it is
 * work_len(samples so far + n) / samples_per_row + 1 minus the rows the host knows to be out (the host-fed calls and
 * aptgpu_stream_results learn that count; device-resident pushes that never ask see the bound grow by a row per row
 * pushed).  Two or three on a pass that keeps its sync.  0 for a null stream. */
size_t aptgpu_stream_rows_bound(const aptgpu_stream *stream, size_t n);
/* Host-fed: n samples (float or int16_t, as created) in; result->n_rows rows of 2080 floats and their work-rate
 * positions out (rows_cap rows of room in each; below aptgpu_stream_rows_bound(stream, n) is APTGPU_ERR_INVALID before
 * anything is consumed).  result->struct_size must be set.  One record is read back per call, whatever n is.  After a
 * finish only reset and destroy are accepted. */
int aptgpu_stream_push(aptgpu_stream *stream, const void *samples, size_t n, float *rows, uint64_t *positions,
                       size_t rows_cap, aptgpu_stream_result *result, char *err, size_t err_cap);
int aptgpu_stream_finish(aptgpu_stream *stream, float *rows, uint64_t *positions, size_t rows_cap,
                         aptgpu_stream_result *result, char *err, size_t err_cap);
/* Device-resident: samples, rows and positions are device pointers; asynchronous on the context's stream, no host
 * synchronisation, nothing read back.  A push longer than max_push becomes several launch sequences.  The end-of-signal
 * errors are reported by aptgpu_stream_results, which waits and returns the record of the last push. */
int aptgpu_stream_push_device(aptgpu_stream *stream, const void *d_samples, size_t n, float *d_rows,
                              uint64_t *d_positions, size_t rows_cap, char *err, size_t err_cap);
int aptgpu_stream_finish_device(aptgpu_stream *stream, float *d_rows, uint64_t *d_positions, size_t rows_cap, char *err,
                                size_t err_cap);
int aptgpu_stream_results(aptgpu_stream *stream, aptgpu_stream_result *result, char *err, size_t err_cap);

/* ====================================================================== */
/* 4e. live flywheel sync: tracked row starts for the live decoder */
/* ====================================================================== */
/* A tracked stream finds its rows with §4c's tracker in place of the reference's picker.  Opt-in: a stream that is not
 * created through the entry points below is §4d's, unchanged.  tests/np_live_track_model.py states the definition in
 * numpy.
 *
 * §22's finality ("the same for every continuation") does not exist for the tracker: the survivors of the dynamic
 * programme merge only after hundreds of rows.  A tracked stream therefore commits with a fixed decision lag.
 * Notation is §4c's: L = 2080 pw, G = 38 pw, w, lambda; s, best and bp are §4c's values of the whole recording bit for
 * bit.  They are causal: s[i], best[i] and bp[i] are final once i + G <= work_len (§4d's count of final F).
 * m = work_len - G, or 0 when work_len < G; K = lag_rows.
 *  1. Checkpoints are absolute.  Checkpoint e = 1, 2, ... is processed as soon as m >= e L, in order, however many a
 *     push crosses; nothing about the tracker happens between checkpoints.  Positions, scores, rows and the release
 *     schedule are functions of the samples and of which push first makes m >= e L.
 *  2. Commit behind the best survivor.  At checkpoint e let n = e L.  `end` is the first maximum of best over
 *     [n - L, n); the survivor is the chain from `end` through bp to a START node.  Committed, ascending, is every node
 *     v of it with  v + (K + 1) L <= n  and  v >= c + L - w,  c being the last committed position (the second
 *     condition is void before the first commit).
 *  3. Relock.  If a checkpoint commits at least one node and c is not a node of its survivor, n_relocks increases by
 *     one.  Steps between committed positions are in [L - w, L + w] except across a relock, where they are >= L - w.
 *  4. A committed position is released in the push that committed it: row[c] = F[v + pw c], c < 2080 (the sample's own
 *     bits, §4c's rule, not §4d's final filter pass), its lock indicator s[v].  v + L <= n - K L <= work_len: the row
 *     exists.
 *  5. finish() flushes the tail as §4d does (work_len is then the one-shot's n, M = n - G), processes the checkpoints
 *     with e L <= M, takes `end` as the first maximum of best over [max(0, M - L), M) and commits every node of its
 *     survivor under the second condition alone.  Those with v + L <= n are released; a last position without a full row
 *     counts in n_positions only.  n < L + G: "track: the signal is shorter than one row and one sync frame"
 *     (APTGPU_ERR_INTERNAL), nothing released.
 *  6. When lag_rows is at least the number of checkpoints of the recording nothing is released before finish(), and
 *     finish() releases exactly aptgpu_track_sync of the whole F: positions, scores and rows bit for bit.
 * The stream's record then reports n_sync = positions committed so far and scan_pos = m.  State on the device, all of
 * fixed size: §4d's record and input ring, an F ring and a score ring that reach back to the oldest position still
 * committable, 2 L sums, one back-pointer byte per position over the deepest back-track, the tracker's record. */
#define APTGPU_LIVE_TRACK_MAX_LAG 64
typedef struct aptgpu_live_track_settings {
    uint32_t struct_size; /* sizeof(aptgpu_live_track_settings) */
    uint32_t lag_rows;    /* K: 0..64 rows a position is held back (0 = greedy); default 8, four seconds */
    uint32_t max_jitter;  /* aptgpu_track_settings' w */
    float penalty;        /* ... and lambda */
} aptgpu_live_track_settings;
typedef struct aptgpu_stream_track_result {
    uint32_t struct_size;     /* set by the caller */
    uint32_t n_relocks;
    uint64_t n_positions;     /* committed so far */
    uint64_t m;               /* positions whose score and sums are final */
    uint64_t next_checkpoint; /* e of the next checkpoint */
    uint64_t last_position;   /* c; meaningful when has_position */
    int32_t has_position;
    uint32_t reserved;
    uint32_t cap_best;        /* capacities of the sums' ring (floats) and of the back-pointers' (bytes), powers of two; */
    uint32_t cap_bp;          /* the score ring has aptgpu_stream_info.cap_f entries */
} aptgpu_stream_track_result;
/* §4d's aptgpu_stream_create / _create_host with a tracker: stream_settings->sync is ignored.  track nullable (= lag 8,
 * w 8, lambda 0.1).  Refused besides what §4d refuses, before a device is touched: a struct_size not set, lag_rows > 64
 * and what §4c refuses of w, lambda and the work rate (APTGPU_ERR_INVALID).  The handle is accepted by every
 * aptgpu_stream_* entry point of §4d; aptgpu_stream_rows_bound follows from rule 2 (three rows per checkpoint the call
 * can reach, and the nodes a finish can commit). */
int aptgpu_stream_create_tracked(const aptgpu_context *ctx, const aptgpu_settings *settings,
                                 const aptgpu_stream_settings *stream_settings, const aptgpu_live_track_settings *track,
                                 aptgpu_stream **out, char *err, size_t err_cap);
int aptgpu_stream_create_tracked_host(const aptgpu_context *ctx, const aptgpu_settings *settings,
                                      const aptgpu_stream_settings *stream_settings,
                                      const aptgpu_live_track_settings *track, aptgpu_stream **out, char *err,
                                      size_t err_cap);
/* The lock indicators of the rows the last host-fed push or finish released: min(cap, n_rows) floats, n_rows in *n.
 * APTGPU_ERR_INVALID for a stream that is not tracked. */
int aptgpu_stream_track_scores(aptgpu_stream *stream, float *scores, size_t cap, size_t *n, char *err, size_t err_cap);
/* Device-resident form: where the *_device calls that follow write the lock indicators of their rows (rows_cap floats of
 * device memory, row for row beside d_rows).  NULL (the state after creation and after reset): the stream keeps them to
 * itself. */
int aptgpu_stream_track_scores_device(aptgpu_stream *stream, float *d_scores, char *err, size_t err_cap);
/* Waits like aptgpu_stream_results and returns the tracker's record. */
int aptgpu_stream_track_results(aptgpu_stream *stream, aptgpu_stream_track_result *result, char *err, size_t err_cap);

/* ====================================================================== */
/* 4b'. FM demodulation in streaming form, and live decode from IQ */
/* ====================================================================== */
/* An SDR delivers IQ frames, not audio.  An FM stream takes them in pushes of any size and returns the outputs of §4b
 * as they become final.  Let x be the frames pushed so far, n their count, x* any continuation of x:
 *   M(n) = (n - T) / D + 1 for n >= T, else 0;  out_len(n) = max(M(n) - 1, 0) (aptgpu_fm_out_len).
 *   a[m] is FINAL once n >= (m + 1) D + T: from then on it has the bits aptgpu_fm_demodulate(x*) gives it on the same
 *   side (kernel or twin).  A push that takes the count from n0 to n1 returns exactly a[out_len(n0) .. out_len(n1)),
 *   never earlier and never later: the release schedule is a function of the chunk sizes alone.  There is no finish:
 *   the definition keeps the valid part only, so nothing is held back at the end.
 * The frame counter is 64 bits; the phase uses its low 32 bits ((uint32) i * pw), the runs of 8 its low 3.  A stream
 * created with first_frame counts its first frame as absolute frame first_frame: that offsets the phase and the run
 * grid (a station that runs on passes 2^32 frames after half an hour at 2.4 MS/s); the decimation grid counts from the
 * first frame pushed.  reset returns to first_frame.
 * State: the raw frames from max(M(n) - 1, 0) D on, fewer than T + D of them, in the input format, in two device
 * buffers used in turn; the next push computes the v it shares with the previous one again, from the same frames in
 * the same order.  The host mirrors n and nothing else: a device-resident push synchronises nothing and allocates
 * nothing.  A push of more than max_push_frames is a sequence of launches back to back.
 * Refused with APTGPU_ERR_INVALID and a text naming the field, before anything is enqueued and with the stream left as
 * it was: everything §4b refuses; a short struct_size; max_push_frames == 0 or above 2^28; a null pointer or one not
 * aligned to a component (audio: to a float) with something to read or write; audio_cap below
 * aptgpu_fm_stream_out_len. */
typedef struct aptgpu_fm_stream aptgpu_fm_stream;
typedef struct aptgpu_fm_stream_settings {
    uint32_t struct_size;      /* sizeof(aptgpu_fm_stream_settings) */
    uint32_t max_push_frames;  /* frames one launch takes (longer pushes are split; the host-fed staging): 1 ... 2^28 */
    uint64_t first_frame;      /* absolute index of the first frame pushed */
    uint64_t reserved;
} aptgpu_fm_stream_settings;
typedef struct aptgpu_fm_stream_info {
    uint32_t struct_size;      /* set by the caller */
    uint32_t fs_out, n_taps, decimation, pw; /* as aptgpu_fm_info */
    uint32_t carry_frames;     /* frames held now: frames - max(M(frames) - 1, 0) D */
    double shift_hz_used;
    const float *taps;         /* h, owned by the stream */
    uint64_t frames;           /* pushed so far */
    uint64_t outputs;          /* returned so far: out_len(frames) */
    uint64_t first_frame;
    uint64_t device_bytes;     /* fixed at creation (host handle: host memory, which follows the pushes' sizes) */
    uint32_t max_push_frames;
    uint32_t reserved;
} aptgpu_fm_stream_info;
/* stream_settings nullable (max_push_frames 2^20, first_frame 0).  ctx as aptgpu_fm_create: its device and stream (NULL: the null stream). */
int aptgpu_fm_stream_create(const aptgpu_context *ctx, const aptgpu_fm_settings *settings,
                            const aptgpu_fm_stream_settings *stream_settings, aptgpu_fm_stream **out, char *err,
                            size_t err_cap);
/* The twin in plain C++ (no GPU needed): the same indexing; equals aptgpu_fm_demodulate_host of the whole recording
 * bit for bit.  aptgpu_fm_stream_push_device refuses such a handle. */
int aptgpu_fm_stream_create_host(const aptgpu_fm_settings *settings, const aptgpu_fm_stream_settings *stream_settings,
                                 aptgpu_fm_stream **out, char *err, size_t err_cap);
void aptgpu_fm_stream_destroy(aptgpu_fm_stream *s);
int aptgpu_fm_stream_reset(aptgpu_fm_stream *s, char *err, size_t err_cap);
int aptgpu_fm_stream_get_info(const aptgpu_fm_stream *s, aptgpu_fm_stream_info *info);
/* The outputs a push of n_frames more frames returns now. */
size_t aptgpu_fm_stream_out_len(const aptgpu_fm_stream *s, size_t n_frames);
/* Host-fed: iq and audio are host arrays; returns when the audio is there. */
int aptgpu_fm_stream_push(aptgpu_fm_stream *s, const void *iq, size_t n_frames, float *audio, size_t audio_cap,
                          size_t *n_out, char *err, size_t err_cap);
/* Device-resident: asynchronous on the context's stream; the chunk is read in place (16-byte alignment of its runs
 * lets the loads be 16 bytes wide, with the same bits) and must stay until the stream has passed the call.  *n_out is
 * known on return; nothing is written behind it. */
int aptgpu_fm_stream_push_device(aptgpu_fm_stream *s, const void *d_iq, size_t n_frames, float *d_audio,
                                 size_t audio_cap, size_t *n_out, char *err, size_t err_cap);

/* Live decode from IQ: one object owns an FM stream, an aptgpu_stream created for fs_out in f32 and a device audio
 * scratch, all on the context's HIP stream; frames go in, final rows come out, the audio never leaves the device.  A
 * push is aptgpu_fm_stream_push_device into the scratch followed by aptgpu_stream_push_device of what it returned, in
 * pieces of at most max_push_frames frames; rows, positions, the record, finish and its errors are the decode
 * stream's (§4d), fed the one-shot's audio. */
typedef struct aptgpu_iq_live aptgpu_iq_live;
typedef struct aptgpu_iq_live_settings {
    uint32_t struct_size;      /* sizeof(aptgpu_iq_live_settings) */
    int32_t sync;
    uint32_t max_push_frames;  /* the FM stream's; 0 = 2^20 */
    uint32_t max_push;         /* the decode stream's (audio samples); 0 = its default */
    uint64_t first_frame;
} aptgpu_iq_live_settings;
int aptgpu_iq_live_create(const aptgpu_context *ctx, const aptgpu_settings *decode_settings,
                          const aptgpu_fm_settings *fm_settings, const aptgpu_iq_live_settings *live_settings,
                          aptgpu_iq_live **out, char *err, size_t err_cap);
int aptgpu_iq_live_create_host(const aptgpu_context *ctx, const aptgpu_settings *decode_settings,
                               const aptgpu_fm_settings *fm_settings, const aptgpu_iq_live_settings *live_settings,
                               aptgpu_iq_live **out, char *err, size_t err_cap);
void aptgpu_iq_live_destroy(aptgpu_iq_live *s);
int aptgpu_iq_live_reset(aptgpu_iq_live *s, char *err, size_t err_cap);
/* either info may be NULL */
int aptgpu_iq_live_get_info(const aptgpu_iq_live *s, aptgpu_fm_stream_info *fm_info, aptgpu_stream_info *stream_info);
/* aptgpu_stream_rows_bound of the audio a push of n_frames more frames produces (n_frames == 0: a finish) */
size_t aptgpu_iq_live_rows_bound(const aptgpu_iq_live *s, size_t n_frames);
int aptgpu_iq_live_push(aptgpu_iq_live *s, const void *iq, size_t n_frames, float *rows, uint64_t *positions,
                        size_t rows_cap, aptgpu_stream_result *result, char *err, size_t err_cap);
int aptgpu_iq_live_finish(aptgpu_iq_live *s, float *rows, uint64_t *positions, size_t rows_cap,
                          aptgpu_stream_result *result, char *err, size_t err_cap);
int aptgpu_iq_live_push_device(aptgpu_iq_live *s, const void *d_iq, size_t n_frames, float *d_rows,
                               uint64_t *d_positions, size_t rows_cap, char *err, size_t err_cap);
int aptgpu_iq_live_finish_device(aptgpu_iq_live *s, float *d_rows, uint64_t *d_positions, size_t rows_cap, char *err,
                                 size_t err_cap);
int aptgpu_iq_live_results(aptgpu_iq_live *s, aptgpu_stream_result *result, char *err, size_t err_cap);
/* Live decode from IQ with §4e's tracker: aptgpu_iq_live_create / _host whose decode stream is a tracked one
 * (live_settings->sync is ignored; track nullable = the defaults; §4e's refusals besides §4b''s and §4d's, all before a
 * device is touched).  The FM stream runs in front on the same HIP stream and the audio never leaves the device.  Every
 * aptgpu_iq_live_* entry point accepts the handle; rows, positions, lock indicators and records are those of a tracked
 * stream fed aptgpu_fm_demodulate's audio of the same pushes.  The three calls below are §4e's aptgpu_stream_track_* on
 * the coupling's decode stream; APTGPU_ERR_INVALID for a coupling that is not tracked. */
int aptgpu_iq_live_create_tracked(const aptgpu_context *ctx, const aptgpu_settings *decode_settings,
                                  const aptgpu_fm_settings *fm_settings, const aptgpu_iq_live_settings *live_settings,
                                  const aptgpu_live_track_settings *track, aptgpu_iq_live **out, char *err,
                                  size_t err_cap);
int aptgpu_iq_live_create_tracked_host(const aptgpu_context *ctx, const aptgpu_settings *decode_settings,
                                       const aptgpu_fm_settings *fm_settings,
                                       const aptgpu_iq_live_settings *live_settings,
                                       const aptgpu_live_track_settings *track, aptgpu_iq_live **out, char *err,
                                       size_t err_cap);
int aptgpu_iq_live_track_scores(aptgpu_iq_live *s, float *scores, size_t cap, size_t *n, char *err, size_t err_cap);
int aptgpu_iq_live_track_scores_device(aptgpu_iq_live *s, float *d_scores, char *err, size_t err_cap);
int aptgpu_iq_live_track_results(aptgpu_iq_live *s, aptgpu_stream_track_result *result, char *err, size_t err_cap);

/* ====================================================================== */
/* 5. WAV ingest in front of decode()                 */
/* ====================================================================== */
/* noaa_apt::load / wav::load_wav (src/noaa_apt.rs:114-130, src/wav.rs:11-57): the container is */
/* walked on the host exactly as hound 3.5.1's WavReader does (Cargo.toml:29), the samples are   */
/* converted on the GPU: first channel only, integers `as f32`, never scaled (wav.rs:30-51).     */

#define APTGPU_WAV_U8 0    /* 8 bit unsigned (minus 128)              */
#define APTGPU_WAV_I16 1   /* 16 bit                                  */
#define APTGPU_WAV_I24 2   /* 24 bit packed                           */
#define APTGPU_WAV_I24_4 3 /* 24 bit in a 4-byte container            */
#define APTGPU_WAV_I32 4   /* 32 bit                                  */
#define APTGPU_WAV_F32 5   /* IEEE float                              */

/* hound::WavSpec (+ where the samples are) */
typedef struct aptgpu_wav_spec {
    uint16_t channels;
    uint16_t bits_per_sample;
    uint16_t bytes_per_sample; /* block_align / channels */
    uint16_t sample_format;    /* 0 = hound::SampleFormat::Int, 1 = Float */
    uint32_t sample_rate;
    int32_t codec;             /* APTGPU_WAV_* */
    uint64_t data_offset;      /* payload of the data chunk inside the file image */
    uint64_t data_len;         /* bytes */
    uint64_t n_samples;        /* all channels (WavReader::len) */
    uint64_t n_frames;         /* == length of the Signal load_wav returns */
} aptgpu_wav_spec;

/* hound::WavReader::new + spec() on an in-memory image of the file (host only, no GPU).
 * Errors as the reference maps them (src/err.rs:72-83): APTGPU_ERR_WAV_OPEN for malformed or
 * unsupported files, APTGPU_ERR_IO for a short file, APTGPU_ERR_INTERNAL for too-wide samples. */
int aptgpu_wav_parse(const void *file_bytes, size_t n, aptgpu_wav_spec *spec, char *err,
                     size_t err_cap);
/* wav::load_wav: file image -> (Signal, rate).  *signal_out malloc'd; spec nullable. */
int aptgpu_load_wav(const aptgpu_context *ctx, const void *file_bytes, size_t n, float **signal_out,
                    size_t *n_out, uint32_t *sample_rate_hz, aptgpu_wav_spec *spec, char *err,
                    size_t err_cap);
/* noaa_apt::load(input_filename): reads the file, then as above. */
int aptgpu_load_wav_file(const aptgpu_context *ctx, const char *path, float **signal_out,
                         size_t *n_out, uint32_t *sample_rate_hz, aptgpu_wav_spec *spec, char *err,
                         size_t err_cap);
/* load + decode in one call: the data chunk is uploaded as it is (2 bytes per sample for PCM16
 * instead of 4) and converted in HBM — inside the fused front end for mono PCM16.  Output and
 * callbacks as aptgpu_decode; *sample_rate_hz (nullable) receives the WAV's rate. */
int aptgpu_decode_wav(const aptgpu_context *ctx, const aptgpu_settings *settings,
                      const void *file_bytes, size_t n, int sync, float **rows_out, size_t *n_out,
                      aptgpu_stats *stats, uint32_t *sample_rate_hz, char *err, size_t err_cap);
/* Device-resident batch: d_data[i] points at recording i's data-chunk payload in HBM, specs[i]
 * describes it (sample_rate must equal the plan's input rate).  Otherwise as
 * aptgpu_plan_decode_device. */
int aptgpu_plan_decode_device_wav(aptgpu_plan *plan, int count, const void *const *d_data,
                                  const aptgpu_wav_spec *specs, float *const *d_rows,
                                  const size_t *rows_cap, char *err, size_t err_cap);

/* wav::write_wav (src/wav.rs:59-98) for the {1 channel, 16 bit, Int} spec the resample tool
 * uses (src/resample.rs:53-58): normalise by dsp::get_max, `as i16`; returns the file image
 * hound's writer produces (44-byte PCM header + samples), malloc'd. */
int aptgpu_write_wav_i16(const aptgpu_context *ctx, const float *signal, size_t n,
                         uint32_t sample_rate_hz, void **wav_out, size_t *n_out, char *err,
                         size_t err_cap);
/* resample::resample (src/resample.rs:17-71) between file images: load_wav ->
 * dsp::resample(atten, delta_w) -> write_wav, all on the device; status callbacks at 0.0 / 0.2 /
 * 0.8 / 1.0 with the reference's texts (output_name, nullable, only appears in the 0.8 text),
 * "input" step when ctx->step is set.  atten / delta_w_pi_rad are settings.wav_resample_atten /
 * wav_resample_delta_freq (src/config.rs:100-106). */
int aptgpu_resample_wav(const aptgpu_context *ctx, const void *file_bytes, size_t n,
                        uint32_t output_rate_hz, float atten, float delta_w_pi_rad,
                        const char *output_name, void **wav_out, size_t *n_out, char *err,
                        size_t err_cap);
/* The same with file IO on both sides, copying the modification time (misc.rs:181-205). */
int aptgpu_resample_wav_file(const aptgpu_context *ctx, const char *input_path,
                             const char *output_path, uint32_t output_rate_hz, float atten,
                             float delta_w_pi_rad, char *err, size_t err_cap);
/* Both with Context::resample's second flag (src/context.rs:214-218; main.rs:125-130 passes
 * settings.export_resample_filtered): nonzero = fast_resampling's other decimation phase
 * (src/dsp.rs:265-273) and, when ctx->step is set, the expanded signal in "resample_filtered".
 * With ctx->step set every entry point of this section delivers the steps of Context::resample in the
 * reference's order: "input", "resample_filter", "resample_filtered", "resample_decimated". */
int aptgpu_resample_wav_ex(const aptgpu_context *ctx, const void *file_bytes, size_t n,
                           uint32_t output_rate_hz, float atten, float delta_w_pi_rad,
                           int export_resample_filtered, const char *output_name, void **wav_out,
                           size_t *n_out, char *err, size_t err_cap);
int aptgpu_resample_wav_file_ex(const aptgpu_context *ctx, const char *input_path,
                                const char *output_path, uint32_t output_rate_hz, float atten,
                                float delta_w_pi_rad, int export_resample_filtered, char *err,
                                size_t err_cap);

/* ====================================================================== */
/* 6. misc                                                                 */
/* ====================================================================== */
const char *aptgpu_version(void);
/* Incremented whenever a struct of this header changes layout or a function its signature (0.2.0: 2). */
int aptgpu_abi_version(void);
#define APTGPU_ABI_VERSION 2
int aptgpu_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* APTGPU_H */
