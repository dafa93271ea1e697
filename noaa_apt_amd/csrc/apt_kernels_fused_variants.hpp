// apt_kernels_fused_variants.hpp — every k_fused instantiation the library is built with, in ONE list, and which of
// them serves which plan.  Host-only and free of HIP: apt_kernels_fused_variant.hip is compiled once per row and input
// type from this list, the Makefile reads the names from it, apt_kernels_fused.hip builds its table of launch functions
// from it, select_front_end (apt_front_end.hpp) chooses a plan's rows with the selection functions below, and
// tests/test_fused_variants.py checks those functions without a GPU.
// A new geometry, profile or mode: add a row, and the condition that selects it.
#pragma once

#include <cstdint>

namespace apt::gpu {

// k_fused's MODE template argument
constexpr int kModeStrict = 0;
constexpr int kModeF16Taps = 1;
constexpr int kModeFast = 2;
// kModeMfma (round 6): APTGPU_MODE_FAST with the resampler on the matrix cores.  Stage 1 is the banded Toeplitz product
// R[16 branches][16 windows] = H[16][K] X[K][16] through v_mfma_f32_16x16x32_bf16, f32 accumulation, on bf16 PIECES of the
// f32 operands: taps h = h0 + h1 + h2 exactly (three 8-bit pieces, split on the host), samples x = x0 + x1 (+ a remainder
// below 2^-16 |x|: none for 16-bit samples), split while the tile goes to LDS; five products (h0 x0, h0 x1, h1 x0, h1 x1,
// h2 x0) carry every term above 2^-24 of the largest.  bf16 has f32's exponent range: no scaling.  The f32-input MFMA,
// which would be bit-identical to kModeFast, shares the VALU's datapath and measured 0.66x; an f16 form with a
// power-of-two scale per sub-tile measured at parity with the VALU kernel, this one 6 % behind it (fast
// mode is bound by the tile's HBM round trip, not by the FIRs).  The work-rate stages behind are kModeFast's.  Tap COUNT
// is a run-time quantity here (the table is zero-padded to the kernel's K): a tuned resample_atten / resample_delta_freq
// stays on a specialised kernel while its taps per branch fit — what this mode is kept for.
constexpr int kModeMfma = 3;
// kModeStrictPad (round 6): kModeStrict's arithmetic in a SPLIT kernel compiled for a tap-count BOUND: the chunk-major table
// is laid out for the bound and holds zeros behind the filter's last tap.  sum + 0 * x = sum exactly for finite x (the sum
// starts at +0 and never becomes -0), so the results are bit-identical to the reference's, which skips those taps; a
// tile whose results are not all finite — where 0 * inf would have put a NaN the reference does not have — is evaluated
// again sample by sample from HBM, in the reference's order.  default_settings.toml:108-140 is a user-editable file:
// a tuned resample_atten / resample_delta_freq changes the tap count, and until round 6 such a plan fell to k_fused_any.
constexpr int kModeStrictPad = 4;
// kModeStrictPad2 (round 6): kModeStrictPad whose LOW-PASS length is a bound too (T2 = kPadT2Max: h2 / h2p hold zeros behind
// the filter's last tap — the taps an output meets last, since stage 3 walks them in ascending order — and a tile whose F
// values are not all finite is filtered again from D in LDS with the run-time tap count).  demodulation_atten is as
// user-editable as the resampler's settings (default_settings.toml:116) and moves the Kaiser length of the low-pass
// (25 dB: 37 taps; 24: 35; 26: 39): until this mode such a plan fell to k_fused_any, 7 x the stock step at 48 kHz.
constexpr int kModeStrictPad2 = 5;
// low-pass taps the kModeStrictPad2 instantiations are compiled for (standard profile; four pre-halo threads hold up to 51)
constexpr int kPadT2Max = 45;
// tap counts the padded strict instantiations are compiled for, about an eighth above the stock profiles' counts
// (standard 48 / 96 kHz: 83 / 165 taps per branch, stock 74 / 148; slow 48 / 96 kHz: 241 / 481, stock 215 / 429; fast
// profile at 96 kHz: 56, stock 50)
constexpr int kPadT1Max48k = 1079, kPadT1Max96k = 2145;
constexpr int kPadT1Max48kSlow = 3133, kPadT1Max96kSlow = 6253, kPadT1Max96kFastp = 727;
// tap counts the MFMA instantiations are compiled for (window of a tile's last branch + taps per branch <= K = 128 / 256)
constexpr int kMfmaT1Max48k = 1053, kMfmaT1Max96k = 2119;

// The list.  One row per kernel family: name, then k_fused's template arguments L, M, T1, T2, PW, NTHR, MODE.
//   BOTH: instantiated for f32 and for 16-bit PCM input;  F32: for f32 input only.
//   M > 0: SPLIT stage 1 (48 / 96 kHz; T1 = the filter's tap count, or the bound a padded kernel is compiled for);
//   M == 0: TABLE;  M = -nq: PHASE with nq branches per thread (T1 = 1: taps streamed from the table, else 0).
// One row per line, name first: the Makefile takes the names (and which rows are SPLIT) from these lines.
#define APT_FUSED_VARIANTS(BOTH, F32)                                                                                  \
    /* the standard profile (37-tap low-pass, pixel width 3) at 48 kHz (13 / 50, 959 taps) and 96 kHz (13 / 100, 1915) */ \
    BOTH(48k, 13, 50, 959, 37, 3, 256, kModeStrict)                                                                    \
    BOTH(96k, 13, 100, 1915, 37, 3, 256, kModeStrict)                                                                  \
    BOTH(48k_fast, 13, 50, 959, 37, 3, 256, kModeFast)                                                                 \
    BOTH(96k_fast, 13, 100, 1915, 37, 3, 256, kModeFast)                                                               \
    /* fp16-tap stage 1 (its table: fused_f16_branch_taps), stock 48 kHz only */                                       \
    BOTH(48k_f16taps, 13, 50, 959, 37, 3, 256, kModeF16Taps)                                                           \
    /* APTGPU_MODE_FAST on the matrix cores (kModeMfma): 48 / 96 kHz, standard profile, any tap count up to kMfmaT1Max* */ \
    BOTH(48k_mfma, 13, 50, kMfmaT1Max48k, 37, 3, 256, kModeMfma)                                                       \
    BOTH(96k_mfma, 13, 100, kMfmaT1Max96k, 37, 3, 256, kModeMfma)                                                      \
    /* strict, any tap count up to kPadT1Max* (kModeStrictPad): the standard, slow and fast profiles */                \
    BOTH(48k_pad, 13, 50, kPadT1Max48k, 37, 3, 256, kModeStrictPad)                                                    \
    BOTH(96k_pad, 13, 100, kPadT1Max96k, 37, 3, 256, kModeStrictPad)                                                   \
    BOTH(48k_slow_pad, 13, 30, kPadT1Max48kSlow, 61, 5, 256, kModeStrictPad)                                           \
    BOTH(96k_slow_pad, 13, 60, kPadT1Max96kSlow, 61, 5, 256, kModeStrictPad)                                           \
    /* (odd m: f32 input only, as the exact-count kernel) */                                                           \
    F32(96k_fastp_pad, 13, 75, kPadT1Max96kFastp, 43, 4, 256, kModeStrictPad)                                          \
    /* ... and any low-pass length up to kPadT2Max as well (kModeStrictPad2): 48 / 96 kHz, standard profile */         \
    BOTH(48k_pad2, 13, 50, kPadT1Max48k, kPadT2Max, 3, 256, kModeStrictPad2)                                           \
    BOTH(96k_pad2, 13, 100, kPadT1Max96k, kPadT2Max, 3, 256, kModeStrictPad2)                                          \
    /* ... and the standard profile's PHASE kernels (every rate a sound card records at) with a low-pass of up to      \
       kPadT2Max taps: one, two and four branches per thread */                                                        \
    BOTH(phase_std_pad2, 13, -1, 0, kPadT2Max, 3, 256, kModeStrictPad2)                                                \
    BOTH(phase2_std_pad2, 13, -2, 0, kPadT2Max, 3, 256, kModeStrictPad2)                                               \
    BOTH(phase4_std_pad2, 13, -4, 0, kPadT2Max, 3, 256, kModeStrictPad2)                                               \
    /* 48 kHz at the slow profile (13 / 30, 2783 taps; 61-tap low-pass, pixel width 5): the same SPLIT form */         \
    BOTH(48k_slow, 13, 30, 2783, 61, 5, 256, kModeStrict)                                                              \
    BOTH(48k_slow_fast, 13, 30, 2783, 61, 5, 256, kModeFast)                                                           \
    /* 96 kHz at the slow profile (13 / 60, 5565 taps): strict only (100 KB of unrolled taps per instantiation; it      \
       serves fast mode too) */                                                                                        \
    BOTH(96k_slow, 13, 60, 5565, 61, 5, 256, kModeStrict)                                                              \
    /* 96 kHz at the fast profile (13 / 75, 639 taps; 43-tap low-pass, pixel width 4).  Odd m: 4-byte window reads, f32 \
       input only — PCM16 payloads are staged */                                                                       \
    F32(96k_fastp, 13, 75, 639, 43, 4, 256, kModeStrict)                                                               \
    /* table-driven stage 1 (the fallback) + standard-profile work-rate stages, 512-thread workgroups */               \
    BOTH(tab_std, 13, 0, 0, 37, 3, 512, kModeStrict)                                                                   \
    BOTH(tab_std_fast, 13, 0, 0, 37, 3, 512, kModeFast)                                                                \
    /* phase-resident taps (stage 1 of rates like 44 100 Hz) + standard-profile work-rate stages, 256-thread workgroups */ \
    BOTH(phase_std, 13, -1, 0, 37, 3, 256, kModeStrict)                                                                \
    BOTH(phase_std_fast, 13, -1, 0, 37, 3, 256, kModeFast)                                                             \
    /* ... 256-thread workgroups whose threads hold two / four branches (256 < l <= 512: 22 050 Hz; 512 < l <= 1024:    \
       11 025 Hz) */                                                                                                   \
    BOTH(phase2_std, 13, -2, 0, 37, 3, 256, kModeStrict)                                                               \
    BOTH(phase2_std_fast, 13, -2, 0, 37, 3, 256, kModeFast)                                                            \
    BOTH(phase4_std, 13, -4, 0, 37, 3, 256, kModeStrict)                                                               \
    BOTH(phase4_std_fast, 13, -4, 0, 37, 3, 256, kModeFast)                                                            \
    /* ... 512-thread (256 < l <= 512) and 1024-thread (512 < l <= 1024) workgroups, one branch per thread */          \
    BOTH(phase512_std, 13, -1, 0, 37, 3, 512, kModeStrict)                                                             \
    BOTH(phase512_std_fast, 13, -1, 0, 37, 3, 512, kModeFast)                                                          \
    BOTH(phase1024_std, 13, -1, 0, 37, 3, 1024, kModeStrict)                                                           \
    BOTH(phase1024_std_fast, 13, -1, 0, 37, 3, 1024, kModeFast)                                                        \
    /* phase-resident taps + the FAST PROFILE's work-rate stages (43-tap low-pass, pixel width 4): 48 kHz (l = 26),     \
       96 kHz (l = 13, m = 75) and the other rates whose l <= 256 at work rate 16 640 */                               \
    BOTH(phase_fastp, 13, -1, 0, 43, 4, 256, kModeStrict)                                                              \
    BOTH(phase_fastp_fast, 13, -1, 0, 43, 4, 256, kModeFast)                                                           \
    /* ... with four / eight / sixteen branches per thread (44 100 Hz: l = 832; 22 050 Hz: l = 1664; 11 025 Hz:         \
       l = 3328); strict only, they serve fast mode too */                                                             \
    BOTH(phase4_fastp, 13, -4, 0, 43, 4, 256, kModeStrict)                                                             \
    BOTH(phase8_fastp, 13, -8, 0, 43, 4, 256, kModeStrict)                                                             \
    BOTH(phase16_fastp, 13, -16, 0, 43, 4, 256, kModeStrict)                                                           \
    /* ... the SLOW PROFILE's work-rate stages (61-tap low-pass, pixel width 5), taps streamed from the table (197 per  \
       branch at 44 100 / 22 050 / 11 025 Hz: l = 208 / 416 / 832, m = 441); strict only, they serve fast mode too */  \
    BOTH(phase_slowp, 13, -1, 1, 61, 5, 256, kModeStrict)                                                              \
    BOTH(phase2_slowp, 13, -2, 1, 61, 5, 256, kModeStrict)                                                             \
    BOTH(phase4_slowp, 13, -4, 1, 61, 5, 256, kModeStrict)

#define APT_FUSED_ENUM(name, ...) kFused_##name,
enum FusedVariant : int { kFusedNone = -1, APT_FUSED_VARIANTS(APT_FUSED_ENUM, APT_FUSED_ENUM) kFusedVariantCount };
#undef APT_FUSED_ENUM

struct FusedVariantRow {
    const char *name;
    int l, m, t1, t2, pw, nthr, mode;
    bool i16;  // instantiated for 16-bit PCM input as well
};
#define APT_FUSED_ROW_BOTH(name, ...) {#name, __VA_ARGS__, true},
#define APT_FUSED_ROW_F32(name, ...) {#name, __VA_ARGS__, false},
constexpr FusedVariantRow kFusedVariants[kFusedVariantCount] = {APT_FUSED_VARIANTS(APT_FUSED_ROW_BOTH, APT_FUSED_ROW_F32)};
#undef APT_FUSED_ROW_BOTH
#undef APT_FUSED_ROW_F32

// ---- which variant serves a plan.  Pure functions: no stream, no environment.

// the SPLIT row of `mode` compiled for exactly this geometry (M > 0: the PHASE / TABLE rows serve any), or kFusedNone
constexpr FusedVariant fused_exact_variant(uint32_t l, uint32_t m, uint32_t t1, uint32_t t2, uint32_t pw, int mode)
{
    for (int v = 0; v < kFusedVariantCount; ++v) {
        const FusedVariantRow &r = kFusedVariants[v];
        if (r.m > 0 && r.mode == mode && static_cast<uint32_t>(r.l) == l && static_cast<uint32_t>(r.m) == m &&
            static_cast<uint32_t>(r.t1) == t1 && static_cast<uint32_t>(r.t2) == t2 && static_cast<uint32_t>(r.pw) == pw)
            return static_cast<FusedVariant>(v);
    }
    return kFusedNone;
}

// kModeStrictPad2: the low-pass bound of the instantiation that serves a low-pass of t2 taps other than the profile's
// (a tuned demodulation_atten), or 0 — the standard profile's work-rate stages at 48 / 96 kHz ...
constexpr uint32_t fused_pad_t2_bound(uint32_t l, uint32_t m, uint32_t t2, uint32_t pw)
{
    if (l != 13 || pw != 3 || (m != 50 && m != 100)) return 0;
    if ((t2 & 1u) == 0 || t2 == 37 || t2 > static_cast<uint32_t>(kPadT2Max)) return 0;
    return static_cast<uint32_t>(kPadT2Max);
}
// ... and on the PHASE kernels (a tuned demodulation_atten at a sound-card rate)
constexpr uint32_t fused_phase_pad_t2_bound(uint32_t t2, uint32_t pw)
{
    if (pw != 3 || (t2 & 1u) == 0 || t2 == 37 || t2 > static_cast<uint32_t>(kPadT2Max)) return 0;
    return static_cast<uint32_t>(kPadT2Max);
}
// kModeStrictPad: the tap-count bound of the padded strict kernel that serves (l, m, t1, t2, pw), or 0
constexpr uint32_t fused_pad_t1_bound(uint32_t l, uint32_t m, uint32_t t1, uint32_t t2, uint32_t pw)
{
    if (l != 13 || (t1 & 1u) == 0) return 0;  // (Kaiser lengths are odd: filters.rs:164-167)
    uint32_t bound = 0;
    if ((t2 == 37 || fused_pad_t2_bound(l, m, t2, pw) != 0) && pw == 3) bound = m == 50 ? kPadT1Max48k : m == 100 ? kPadT1Max96k : 0;  // standard profile
    else if (t2 == 61 && pw == 5) bound = m == 30 ? kPadT1Max48kSlow : m == 60 ? kPadT1Max96kSlow : 0;  // slow profile
    else if (t2 == 43 && pw == 4) bound = m == 75 ? kPadT1Max96kFastp : 0;                            // fast profile, 96 kHz
    return t1 <= bound ? bound : 0;
}
// kModeMfma: the geometries a matrix-core instantiation serves
constexpr bool fused_mfma_fits(uint32_t l, uint32_t m, uint32_t t1, uint32_t t2, uint32_t pw)
{
    if (l != 13 || t2 != 37 || pw != 3 || (t1 & 1u) == 0) return false;  // (Kaiser lengths are odd: filters.rs:164-167)
    if (m == 50) return t1 <= static_cast<uint32_t>(kMfmaT1Max48k);
    if (m == 100) return t1 <= static_cast<uint32_t>(kMfmaT1Max96k);
    return false;
}

// SPLIT stage 1: 48 / 96 kHz
constexpr FusedVariant fused_split_variant(uint32_t l, uint32_t m, uint32_t t1, uint32_t t2, uint32_t pw, int mode, bool pcm16)
{
    if (mode == kModeStrictPad) {
        if (fused_pad_t1_bound(l, m, t1, t2, pw) == 0) return kFusedNone;
        if (fused_pad_t2_bound(l, m, t2, pw) != 0)  // the low-pass length a bound too (kModeStrictPad2)
            return m == 50 ? kFused_48k_pad2 : kFused_96k_pad2;
        if (m == 50) return kFused_48k_pad;
        if (m == 100) return kFused_96k_pad;
        if (m == 30) return kFused_48k_slow_pad;
        if (m == 60) return kFused_96k_slow_pad;
        if (m == 75 && !pcm16) return kFused_96k_fastp_pad;
        return kFusedNone;
    }
    if (mode == kModeMfma) {
        if (!fused_mfma_fits(l, m, t1, t2, pw)) return kFusedNone;
        return m == 50 ? kFused_48k_mfma : kFused_96k_mfma;
    }
    const FusedVariant strict = fused_exact_variant(l, m, t1, t2, pw, kModeStrict);
    if (strict == kFused_48k)  // (fp16 taps: stock 48 kHz only)
        return mode == kModeF16Taps ? kFused_48k_f16taps : mode == kModeFast ? kFused_48k_fast : kFused_48k;
    if (strict == kFused_48k_slow && mode != kModeF16Taps) return mode == kModeFast ? kFused_48k_slow_fast : kFused_48k_slow;
    if (strict == kFused_96k_fastp && mode == kModeStrict && !pcm16) return kFused_96k_fastp;
    if (strict == kFused_96k_slow && mode == kModeStrict) return kFused_96k_slow;
    if (strict == kFused_96k && mode != kModeF16Taps) return mode == kModeFast ? kFused_96k_fast : kFused_96k;
    return kFusedNone;
}

// TABLE stage 1
constexpr FusedVariant fused_table_variant(int mode)
{
    return mode == kModeFast ? kFused_tab_std_fast : mode == kModeStrict ? kFused_tab_std : kFusedNone;
}

// PHASE stage 1: workgroups of nthr threads with nq branches each (TableGeom's; 0 counts as 1),
// taps streamed or resident, and the work-rate stages of the profile (t2, pw) names
constexpr FusedVariant fused_phase_variant(uint32_t nq, uint32_t nthr, bool stream, uint32_t t2, uint32_t pw, int mode)
{
    const bool wide = nthr == 512, huge = nthr == 1024;
    if (t2 == 61 && pw == 5) {  // the slow profile's work-rate stages, streamed taps (strict instantiations only: they serve fast mode too)
        if (wide || huge || !stream) return kFusedNone;
        return nq == 1 ? kFused_phase_slowp : nq == 2 ? kFused_phase2_slowp : nq == 4 ? kFused_phase4_slowp : kFusedNone;
    }
    if (t2 == 43 && pw == 4 && nq > 1) {  // the fast profile's, four / eight / sixteen branches per thread (strict instantiations only)
        if (wide || huge) return kFusedNone;
        return nq == 4 ? kFused_phase4_fastp : nq == 8 ? kFused_phase8_fastp : nq == 16 ? kFused_phase16_fastp : kFusedNone;
    }
    if (t2 == 43 && pw == 4) {  // the fast profile's work-rate stages
        if (wide || huge) return kFusedNone;
        return mode == kModeFast ? kFused_phase_fastp_fast : mode == kModeStrict ? kFused_phase_fastp : kFusedNone;
    }
    if (pw == 3 && t2 != 37) {  // a tuned low-pass: kModeStrictPad2 (strict arithmetic: it serves APTGPU_MODE_FAST too)
        if (wide || huge || fused_phase_pad_t2_bound(t2, pw) == 0) return kFusedNone;
        return (nq == 1 || nq == 0) ? kFused_phase_std_pad2 : nq == 2 ? kFused_phase2_std_pad2 : nq == 4 ? kFused_phase4_std_pad2 : kFusedNone;
    }
    if (mode != kModeFast && mode != kModeStrict) return kFusedNone;
    const bool fast = mode == kModeFast;
    if (nq == 2 || nq == 4) {
        if (wide || huge) return kFusedNone;
        if (nq == 4) return fast ? kFused_phase4_std_fast : kFused_phase4_std;
        return fast ? kFused_phase2_std_fast : kFused_phase2_std;
    }
    if (huge) return fast ? kFused_phase1024_std_fast : kFused_phase1024_std;
    if (wide) return fast ? kFused_phase512_std_fast : kFused_phase512_std;
    return fast ? kFused_phase_std_fast : kFused_phase_std;
}

}  // namespace apt::gpu
