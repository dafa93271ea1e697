// apt_kernels.hpp — launch wrappers of the gfx950 kernels (definitions in
// apt_kernels_generic.hip and apt_kernels_fused.hip).  All launches are
// asynchronous on the given stream and never synchronise with the host.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "apt_front_end.hpp"

namespace apt::gpu {

// Device-side result record == aptgpu_result (include/aptgpu.h).
struct Result {
    int32_t status;
    int32_t reason;
    uint32_t n_rows;
    uint32_t n_sync;
    uint64_t work_len;
    uint64_t n_out;
};

// Device-side record of the image stage == aptgpu_image_result (include/aptgpu.h).
struct ImageResult {
    int32_t status;   // 0 ok, 1 Internal
    int32_t reason;   // 1 zero-length signal, 2 too short for telemetry, 3 no low bucket, 4 decode failed
    uint32_t height;  // rows of 2080 px
    uint32_t telemetry_row;
    float low, high;
    float telemetry_quality;
    int32_t channel_a, channel_b;  // index into the reference's channel-name table, -1 = none
    uint32_t reserved;
    uint64_t n_px;
    float values_a[16], values_b[16];
};

// Per-group record the front ends hand to the picker: an interval [lo, hi] that holds the maximum of
// the sync correlation over the group's positions, NaNs ignored (position 0 clamped to >= 0: the picker
// starts from the peak (0, 0.), decode.rs:208).  lo == hi where the front end evaluated the very
// arithmetic the picker re-evaluates (fast mode, the unfused kernels); the strict front ends — the
// specialised kernels and, since round 4, k_fused_any — bound the reference's 38 pw-term chain from pulse
// sums (apt_kernels_fused_impl.hpp stage 4, apt_kernels_fused_any_impl.hpp stage 4).  k_sync_words prunes a group only when a later group's lo exceeds its hi, and settles every
// comparison the bounds leave open with the exact chain: the intervals only decide how much is
// re-evaluated, never the result.
// [-inf, +inf] marks a group that must reach the exact test whatever its neighbours hold: one with a NaN
// position (never exceeded — `corr > NaN` is false, decode.rs:250 — so a terminal of the picker whatever
// the finite values around it are), or one whose F window is not finite.
struct GroupMax {
    float hi;
    float lo;
};

// A/B switches of the launch wrappers (APTGPU_* environment variables of tools/ and tests/): read ONCE, when a plan
// is created (read_launch_switches), and carried by the plan to every launch — not per launch: getenv is not safe
// against a concurrent setenv of another thread, and a plan must not change kernels in mid-life.
struct LaunchSwitches {
    int words_form = 1;          // APTGPU_WORDS_FORM=0: k_sync_words / k_sync_slots in their earlier form (A/B)
    bool orbit_lds = true;       // APTGPU_ORBIT_LDS=0: the orbit kernel's tables in global memory
    int orbit_alg = 1;           // APTGPU_ORBIT_ALG=0: the breadth-first closure form
    float gm_slack_scale = 1.f;  // APTGPU_GM_SLACK_SCALE (tests): widens the strict front ends' bounds
};
LaunchSwitches read_launch_switches();

// ---- one decode_device call = one launch per stage over all its recordings -----------
// Per-recording arguments travel BY VALUE in the kernel-argument segment (no H2D copy, no pinned
// staging, nothing for the host to wait on); blockIdx.y (front end, k_sync_words, k_sync_slots, k_gather_rows) or
// blockIdx.x (k_sync_orbit) picks the recording.  The workspace of a recording is a slot of the
// plan; the slots' pointers sit in a device table written once at plan creation.
constexpr int kMaxCall = 32;  // recordings per launch; longer calls are split
struct RecArgs {
    const void *x;       // f32 Signal, or mono PCM16 payload (front end only)
    uint64_t n;          // input samples
    uint64_t w;          // work-rate samples (fast_resampling_len / decimation length)
    float *rows;         // output pixel rows
    uint32_t rows_cap;   // rows `rows` has room for
    uint32_t slot;       // index into the slot table
};
struct CallArgs {
    uint32_t count;
    uint32_t tiles_x;  // persistent front end only: tiles of the call's longest recording (else 0)
    RecArgs rec[kMaxCall];
};
struct SlotPtrs {
    float *f;               // filtered work-rate signal F (see f_stride)
    GroupMax *gm;           // per-group correlation maxima
    const float *corr;      // full correlation (unfused path / step export only), else nullptr
    uint64_t *words;        // 52-bit terminal words
    uint64_t *nanw;         // 52-bit words: positions whose correlation is NaN
    uint32_t *slot_nt, *slot_cnt, *flags, *orbit_ws, *peaks;
    Result *res;
    uint32_t peaks_cap;
    uint32_t f_stride;      // 0: F contiguous; else F in pixel-phase planes of f_stride floats (f_index)
};

// Where F[i] lies in a slot's filtered buffer.  The k_fused instantiations write F in pw pixel-phase planes —
// F[i] at f[(i % pw) * stride + i / pw] — so that a pixel row (every pw-th sample from a sync position) is one
// contiguous run of a plane; stride == 0 is the contiguous layout of k_fused_any and the unfused kernels.
__host__ __device__ inline uint64_t f_index(uint64_t i, uint32_t pw, uint32_t stride)
{
    return stride ? (i % pw) * stride + i / pw : i;
}
// plane length of a plan whose longest work signal has max_w samples: a multiple of 4 floats, one quad of padding
__host__ __device__ inline uint32_t f_plane_stride(uint64_t max_w, uint32_t pw)
{
    return static_cast<uint32_t>(((max_w + pw - 1) / pw + 4 + 3) & ~3ull);
}

// ---- generic kernels (any l, m, tap count) --------------------------------------
// fast_resampling, dsp.rs:186-289: out[k], k < w
void resample_generic(hipStream_t s, const float *x, uint64_t n, const float *coeff,
                      uint32_t ntaps, uint32_t l, uint32_t m, float *out, uint64_t w);
// fp16-tap variant (APTGPU_MODE_FP16_TAPS, BASELINE config 5): tolerance-based, not bit-exact
uint32_t f16taps_pairs_per_phase(uint32_t l, uint32_t ntaps);
float f16taps_pack(uint32_t l, const float *coeff, uint32_t ntaps, uint16_t *table);  // returns 2^-s
void resample_f16taps(hipStream_t s, const float *x, uint64_t n, const uint16_t *table, uint32_t ntaps,
                      uint32_t l, uint32_t m, float unscale, float *out, uint64_t w);
// filter() followed by decimate(m), dsp.rs:386-410 + 294-307: out[k] = filter(x)[k*m]
void fir_decimate(hipStream_t s, const float *x, uint64_t n, const float *coeff, uint32_t ntaps,
                  uint32_t m, float *out, uint64_t n_out);
// demodulate, dsp.rs:350-383
void demodulate(hipStream_t s, const float *x, uint64_t n, float cosphi2, float sinphi, float *out);
// the cross-correlation of find_sync, decode.rs:225-233 (pw = work_rate / 4160)
void correlate(hipStream_t s, const float *f, uint64_t n_corr, uint32_t pw, float *corr);
// terminal flags of the peak picker: bit i of `bits` set <=> no corr[j] > corr[i] for
// j in (i, i+md]; corr[0] is clamped to >= 0 (the initial (0, 0.) peak, decode.rs:208); NaNs
// read as -inf (never a record; orbit_walk handles a phase that starts on one).
// md must be a multiple of 64; needs 2*md*4 bytes of LDS.
void terminals(hipStream_t s, const float *corr, uint64_t n_corr, uint32_t md, uint64_t *bits);
// the orbit of the peak picker over the terminal bitmask (one wave): writes the peak list
// (find_sync's return value) and fills the result record.
void orbit_walk(hipStream_t s, const uint64_t *bits, const float *corr, uint64_t n_corr, uint64_t work_len,
                uint32_t spr, uint32_t md, uint32_t *peaks, uint32_t peaks_cap, Result *res);
// row gather (decode.rs:120-134) taking every pw-th sample; raw = plain copy (the
// "sync_result" step), !raw = through the final NoFilter stage (decode.rs:158-159)
void gather_rows(hipStream_t s, const float *f, const uint32_t *peaks, Result *res,
                 uint32_t spr, uint32_t pw, bool raw, float *rows, uint32_t rows_cap);
// the same for the recordings of one call: rows / rows_cap from the call, F / peaks / res from the slots
void gather_rows_call(hipStream_t s, const CallArgs &call, const SlotPtrs *d_slots, uint32_t spr, uint32_t pw,
                      uint32_t max_rows_cap);

// the no-sync branch's tail (decode.rs:135-159, final decimation by m2 through NoFilter) and the result records of the
// recordings of one call in one launch; `rows_cap` of the call's records counts floats
void nosync_rows_call(hipStream_t s, const CallArgs &call, const SlotPtrs *d_slots, uint32_t spr, uint32_t m2, uint64_t max_w);

// ---- fused specialised front end (apt_kernels_fused.hip) --------------------------
// host: stage-1 tap-pair table [WIN][PS][2] (see apt_kernels_fused.hip) and its size in floats
uint32_t fused_tap_table_floats(uint32_t l, uint32_t m, uint32_t t1, int ch);
void fused_branch_taps(uint32_t l, uint32_t m, const float *coeff, uint32_t t1, int ch, float *hs, uint32_t t1_layout = 0);
int fused_chunk_of(uint32_t m, bool fast);  // window samples per stage-1 chunk of the specialised kernel for (m, strict / fast)
// host: stage-3 tap pairs h2p[k] = (h2[k-1], h2[k]), k = 0 .. t2  (2*(t2+1) floats)
void fused_lowpass_pairs(const float *h2, uint32_t t2, float *h2p);
// fp16-tap stage 1 (APTGPU_MODE_FP16_TAPS): table size in dwords, host-side table builder (returns
// the power-of-two unscale factor)
uint32_t fused_f16_table_dwords(uint32_t l, uint32_t m, uint32_t t1);
float fused_f16_branch_taps(uint32_t l, uint32_t m, const float *coeff, uint32_t t1, uint32_t *table);
// strict front ends: |pulse-sum correlation - sequential chain| <= fused_gm_slack(pw) * sum|F| (see stage 4)
float fused_gm_slack(uint32_t pw, float scale = 1.f);
// Per-plan parameters of the specialised front end, resident in HBM (the kernel fetches each when
// the stage that needs it starts, instead of holding them in SGPRs from its first instruction on).
// (TableGeom, the run-time geometry of the TABLE / PHASE stage 1: apt_front_end.hpp)
struct FusedParams {
    const float *hs;        // stage-1 table: tap pairs (fused_branch_taps), or the fp16 table
    const float *h2;        // low-pass taps [T2]
    const float *h2p;       // low-pass tap pairs (fused_lowpass_pairs)
    const SlotPtrs *slots;  // the plan's slot table
    float cosphi2, sinphi;
    float inv_sinphi;       // strict: verified RN(1/sinphi) or 0 (apt_envelope.hpp); fast: RN(1/sinphi)
    float f16_unscale;      // 2^-s of the fp16 tap prescale (fp16-tap mode)
    int32_t want_gm;        // sync search wanted: emit the per-group bounds of the correlation maxima
    float gm_slack;         // strict modes: half-width of a group's bounds per unit of sum|F| (fused_gm_slack)
    const float *table;     // TABLE mode: phase-major tap table [l][tpp] (fused_any_table)
    TableGeom tab;
    // kModeMfma: the plain resampler taps and their count (the scalar path of tiles that hold a non-finite sample)
    const float *coeff;
    uint32_t t1;
    uint32_t t2;            // kModeStrictPad2: the low-pass filter's own tap count (h2 / h2p are padded to kPadT2Max)
};
// One launch over the recordings of `call` of the k_fused instantiation the plan chose (fe.variant, with its LDS size): x
// -> F (slot's filtered buffer) and, if prm->want_gm, the per-group maxima of the sync cross-correlation.  Returns false
// where there is no instantiation for the input type or an input is misaligned.
// Inputs are f32 Signals, or (pcm16) mono int16 samples at 4-byte (SPLIT: dword loads of sample pairs) / even addresses.
// variant_out: receives the row of apt_kernels_fused_variants.hpp whose kernel the call launched (a FusedVariant; -1 where
// none was) — introspection, aptgpu_plan_read_internal("fused_variant").
bool fused_front_end(hipStream_t s, const FrontEnd &fe, bool pcm16, const CallArgs &call, const FusedParams *d_prm,
                     uint64_t max_w, int *variant_out = nullptr);
// kModeMfma: the matrix-core instantiations' table — [3 pieces][K / 32][64 lanes][4 dwords] bf16 fragments of the banded
// Toeplitz matrix of the resampler (h = h0 + h1 + h2 exactly)
uint32_t fused_mfma_table_dwords(uint32_t l, uint32_t m);
void fused_mfma_table(uint32_t l, uint32_t m, const float *coeff, uint32_t t1, uint32_t *table);

// ---- fused front end for any rate / profile (apt_kernels_fused_any.hip) -------------
// run-time parameters, taps phase-major in LDS; same outputs as fused_front_end (which geometries, and the table:
// apt_kernels_fused_any_geom.hpp)
// One launch over the recordings of `call` (f32 Signals, or — pcm16 — mono int16 payloads at even addresses): F into
// the slots' filtered buffers and, if want_gm, the per-group maxima of the sync correlation into their gm buffers.
bool fused_any_front_end(hipStream_t s, uint32_t l, uint32_t m, uint32_t t1, uint32_t t2, uint32_t pw, bool pcm16,
                         const CallArgs &call, const SlotPtrs *d_slots, uint64_t max_w, const float *table,
                         const float *h2, const float *h2p /* fused_lowpass_pairs */, float cosphi2, float sinphi,
                         float inv_sinphi, bool want_gm, float gm_slack_scale = 1.f);

// ---- parallel peak picker (apt_kernels_sync.hip) ------------------------------------
// Each launch covers the recordings of one call (CallArgs by value, slot table in HBM).
uint32_t sync_group_size();    // correlation positions per group (52)
uint32_t sync_chunk_groups();  // groups per k_sync_words / k_sync_slots workgroup
uint32_t sync_slot_cap();      // node terminals kept per chunk
// corr -> per-group maxima (unfused path; the fused front ends write them themselves)
void group_max(hipStream_t s, const float *corr, uint64_t n_corr, GroupMax *gm);
// coarse/fine terminal detection -> terminal words + ordered node-terminal lists.  use_corr: read
// the slots' full correlation (unfused kernels); else the correlation of the candidate groups is
// re-evaluated from F — strictly (the reference's chain) or, `fast`, from pulse sums, exactly as the
// front end of that mode did.
void sync_nodes(hipStream_t s, const CallArgs &call, const SlotPtrs *d_slots, uint64_t max_w, uint32_t pw,
                uint32_t spr, uint32_t md, bool fast, bool use_corr, const LaunchSwitches &sw = LaunchSwitches{});
// orbit of the picker (direct / pointer doubling, or the sequential walk as fallback): peak
// list + result record of every recording
size_t sync_orbit_ws_words(uint64_t w, uint32_t spr);  // uint32 words of scratch it needs
void sync_orbit(hipStream_t s, const CallArgs &call, const SlotPtrs *d_slots, uint32_t spr, uint32_t md,
                uint32_t pw, bool force_walk /* the sequential walk instead of the parallel picker */,
                const LaunchSwitches &sw = LaunchSwitches{});

// ---- consumers of the pixel rows (apt_kernels_image.hip) ------
// All take the pixel count from `res` (device) when it is non-null, else `n`; `cap` bounds it
// and sizes the launch.  `ws` is image_ws_bytes(cap) bytes of scratch, 16-byte aligned.
size_t image_ws_bytes(uint64_t max_px);
struct ImageWsPointers {
    float *limits;     // [0] low, [1] high
    uint32_t *counts;  // 1000 histogram buckets
    float *mean_a, *mean_b, *variance, *corr, *quality;
};
ImageWsPointers image_ws_pointers(void *ws, uint64_t max_px);
// resets the record; image_minmax / image_percent / image_telemetry do it themselves, so this is
// only needed in front of a bare image_set_limits + image_map_u8
void image_begin(hipStream_t s, ImageResult *out);
// dsp::get_min / get_max, dsp.rs:20-54 -> limits
void image_minmax(hipStream_t s, const float *x, const Result *res, uint64_t n, uint64_t cap, void *ws,
                  ImageResult *out);
// misc::percent, misc.rs:119-175 -> limits
void image_percent(hipStream_t s, const float *x, const Result *res, uint64_t n, uint64_t cap, float percent,
                   void *ws, ImageResult *out);
// telemetry::read_telemetry, telemetry.rs:125-243 -> out->values_*, rows; limits if set_limits
void image_telemetry(hipStream_t s, const float *x, const Result *res, uint64_t n, uint64_t cap, void *ws,
                     ImageResult *out, bool set_limits);
void image_set_limits(hipStream_t s, void *ws, uint64_t cap, float low, float high);
// map_signal_u8, noaa_apt.rs:249-259 (+ processing::rotate, processing.rs:21-37)
void image_map_u8(hipStream_t s, const float *x, const Result *res, uint64_t n, uint64_t cap, void *ws,
                  bool rotate, uint8_t *out, ImageResult *info);

// ---- WAV ingest (apt_kernels_ingest.hip) --------------------------
// data chunk bytes -> f32 Signal, first channel only, unscaled (wav.rs:30-51); codec is
// apt::WavCodec as int
void wav_to_signal(hipStream_t s, const void *d_data, uint64_t n_frames, uint32_t channels,
                   uint32_t bytes_per_sample, int codec, float *d_signal);

// wav::write_wav, 16-bit branch (wav.rs:83-86): normalise by d_limits[1] (get_max) -> i16
void quantize_i16(hipStream_t s, const float *d_x, uint64_t n, const float *d_limits, int16_t *d_out);

// exhaustive device-side check that division by c through rc = RN(1/c) + one FMA correction is
// correctly rounded (apt_envelope.hpp); run once per (device, divisor) and process, on a stream of
// its own (the current device must be `device`)
bool verify_fast_divide(int device, float c, float rc);

// writes a result record from the host's knowledge (too-short recording, no-sync path)
void set_result(hipStream_t s, Result *res, Result value);

}  // namespace apt::gpu
