// apt_kernels_fused_launch.hpp — launch interface between apt_kernels_fused.hip (host-side tables and
// dispatch) and apt_kernels_fused_variant.hip (compiled once per k_fused instantiation: the rows of
// apt_kernels_fused_variants.hpp, which also has k_fused's modes and the tap-count bounds).
#pragma once

#include "apt_kernels.hpp"
#include "apt_kernels_fused_variants.hpp"

namespace apt::gpu {

// (phase_halves — PHASE stage 1 with one branch per thread takes its tile through LDS in two halves: apt_front_end.hpp)
// FusedGeom's variant argument for a mode
constexpr int fused_geom_var(int mode)
{
    return mode == kModeF16Taps ? 1 : mode == kModeMfma ? 2 : (mode == kModeStrictPad || mode == kModeStrictPad2) ? 3 : 0;
}

// Window samples per stage-1 chunk (one scalar-load wait per chunk) of the specialised kernels; host (table builder)
// and device agree through this and the layout functions below.  (Rounds 1-3: two samples x all 13 branches per chunk
// at 48 kHz, three at 96 kHz, every thread a whole window — 51.5 KB of input tile per 256 / 128 threads.)
constexpr int fused_chunk(int m, int mode)
{
    return 4;  // kSplitChunk
}

// SPLIT stage 1.  An input tile of 256 windows is 51.5 KB of LDS at 48 kHz (three workgroups per CU) and would be 102 KB
// at 96 kHz.  A 256-thread workgroup instead runs stage 1 over TWO sub-tiles of 128 windows, one after the other through
// the same LDS; in each, thread (half h, window a) computes the branches [b0, b0 + nbr) of window a only — h = 0: the
// first (l + 1) / 2 branches, h = 1: the rest.  All 256 threads then share a 26 KB (48 kHz) / 52 KB (96 kHz) tile:
// six workgroups per CU at 48 kHz (the work-rate stages' 26.1 KB set the footprint; round 3: 28.5 KB, five), three at 96 kHz where the
// 128-thread workgroups of rounds 1-3 reached 1.5 waves per SIMD.  The stages behind it see 256 threads x l outputs.  A half's taps: its own chunk-major table over
// the window samples [w0, w0 + 4 nch) its branches use, w0 a multiple of 4 (16-byte LDS reads); a chunk is 4
// samples x 3 branch pairs (24 dwords) followed by the odd branch's 4 taps (half 0 only): 28 = 16 + 8 + 4 dwords.
constexpr int kSplitChunk = 4, kSplitChunkDwords = 28;
constexpr int fused_branch_first(int l, int m, int b) { return (b * m + l - 1) / l; }
constexpr int fused_branch_end(int l, int m, int t1, int b)  // one past the last window sample branch b has a tap for
{
    const int cb = fused_branch_first(l, m, b), pb = cb * l - b * m;
    return cb + (t1 - pb + l - 1) / l;
}
constexpr int fused_split_b0(int l, int h) { return h == 0 ? 0 : (l + 1) / 2; }
constexpr int fused_split_nbr(int l, int h) { return h == 0 ? (l + 1) / 2 : l / 2; }
constexpr int fused_split_w0(int l, int m, int h) { return fused_branch_first(l, m, fused_split_b0(l, h)) / 4 * 4; }
constexpr int fused_split_nch(int l, int m, int t1, int h)
{
    int end = 0;
    for (int b = fused_split_b0(l, h); b < fused_split_b0(l, h) + fused_split_nbr(l, h); ++b)
        end = fused_branch_end(l, m, t1, b) > end ? fused_branch_end(l, m, t1, b) : end;
    return (end - fused_split_w0(l, m, h) + kSplitChunk - 1) / kSplitChunk;
}
// floats in front of half h's table (one zero row behind each half)
constexpr int fused_split_table_offset(int l, int m, int t1, int h)
{
    return h == 0 ? 0 : (fused_split_nch(l, m, t1, 0) + 1) * kSplitChunkDwords;
}

// arguments of one launch: the recordings of one call (see CallArgs / SlotPtrs in apt_kernels.hpp)
struct FusedLaunch {
    hipStream_t s;
    const CallArgs *call;      // host copy; passed to the kernel by value
    const FusedParams *prm;    // device-resident parameters of the plan
    uint64_t max_w;            // longest recording of the call, work samples (sizes grid.x)
    size_t table_lds_floats;   // TABLE mode: floats of LDS the table and the input tile take
};

// the launch of variant V for input samples of type XT: defined by apt_kernels_fused_variant.hip built with
// -DAPT_FUSED_VARIANT=V -DAPT_FUSED_XT=XT, one object per (row, input type) of the list
template <FusedVariant V, typename XT>
void fused_launch(const FusedLaunch &a);
#define APT_FUSED_DECL_F32(name, ...) template <> void fused_launch<kFused_##name, float>(const FusedLaunch &a);
#define APT_FUSED_DECL_BOTH(name, ...) APT_FUSED_DECL_F32(name) template <> void fused_launch<kFused_##name, int16_t>(const FusedLaunch &a);
APT_FUSED_VARIANTS(APT_FUSED_DECL_BOTH, APT_FUSED_DECL_F32)
#undef APT_FUSED_DECL_BOTH
#undef APT_FUSED_DECL_F32
#ifdef APT_WITH_PROBES
// timing probes (make PROBES=1; APTGPU_PROBE_STOP=1..7; sources under tools/probes/): the fast 48 kHz f32
// kernel cut off after a stage (1..5)
void fused_launch_probe1(const FusedLaunch &a);
void fused_launch_probe2(const FusedLaunch &a);
void fused_launch_probe3(const FusedLaunch &a);
void fused_launch_probe4(const FusedLaunch &a);
void fused_launch_probe5(const FusedLaunch &a);
// ... and the strict kernel cut off after a stage (11..15)
void fused_launch_probe11(const FusedLaunch &a);
void fused_launch_probe12(const FusedLaunch &a);
void fused_launch_probe13(const FusedLaunch &a);
void fused_launch_probe14(const FusedLaunch &a);
void fused_launch_probe15(const FusedLaunch &a);
void fused_launch_probe16(const FusedLaunch &a);  // strict, complete, no HBM reads
void fused_launch_probe8(const FusedLaunch &a);   // fast, complete, no HBM reads
void fused_launch_probe9(const FusedLaunch &a);   // fast, persistent with register prefetch
void fused_launch_probe17(const FusedLaunch &a);  // strict, persistent with register prefetch
#endif

}  // namespace apt::gpu
