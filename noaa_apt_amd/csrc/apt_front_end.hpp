// apt_front_end.hpp — what a plan decides once, when it is created, on the host: the filters and factors of decode()
// (design_plan), the APTGPU_* switches that shape the plan (PlanSwitches, read by read_plan_switches and nowhere else),
// and which front-end kernel serves it (select_front_end -> FrontEnd, which the plan stores and every launch reads).
// Host-only and free of HIP: tests/test_front_end_choice.py builds it with the host compiler and checks the choice
// without a GPU.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/aptgpu.h"
#include "apt_host.hpp"
#include "apt_kernels_fused_any_geom.hpp"
#include "apt_kernels_fused_variants.hpp"

namespace apt {

// The host-side design of decode() for (settings, input rate): decode.rs:55-100, 158-159, 204-216.
struct PlanDesign {
    // first resample (decode.rs:65-77)
    uint32_t l = 1, m = 1;
    Signal taps_resample;
    // demodulation (decode.rs:89; dsp.rs:360-363)
    float cosphi2 = 0.f, sinphi = 0.f;
    // low-pass (decode.rs:95-102)
    Signal taps_lowpass;
    // sync (decode.rs:204-216)
    uint32_t spr = 0, md = 0, pw = 0, n_sync_taps = 0;
    bool work_is_multiple = false;
    // final resample to 4160 (decode.rs:158-159)
    uint32_t l2 = 1, m2 = 1;
};
// throws apt::Error with the reference's messages
PlanDesign design_plan(const aptgpu_settings &settings, uint32_t input_rate, bool sync);

}  // namespace apt

namespace apt::gpu {

// The switches that decide a plan's shape (A/B switches of tools/ and tests/), as the environment had them when the plan
// was created: read ONCE per plan, by read_plan_switches — getenv is not safe against a concurrent setenv, and a plan
// must not change kernels in mid-life.  A 0 / 1 switch holds the first character of its value, -1 when it is not set.
struct PlanSwitches {
    int force_walk = -1;        // APTGPU_FORCE_WALK=1: the picker's sequential fallback
    int streams = 0;            // APTGPU_STREAMS: calls in flight, clamped to 1 .. 16 (0: not set)
    int fused_any = -1;         // APTGPU_FUSED_ANY=1 (tests): the run-time kernel even where a specialised one exists
    int phase_first = -1;       // APTGPU_PHASE_FIRST=0 (tests): the table-driven stage 1 wherever it exists
    int fast_mfma = -1;         // APTGPU_FAST_MFMA=0 / 1: the matrix-core kernels never / wherever instantiated
    int fused_pad = -1;         // APTGPU_FUSED_PAD=0 / 1: the kernels compiled for tap-count bounds never / for stock counts too
    int quiet = -1;             // APTGPU_QUIET=1: no note about a plan without a specialised front end
    int general_envelope = -1;  // APTGPU_GENERAL_ENVELOPE=1 (tests): the envelope's general division
    int phase_balanced = -1;    // APTGPU_PHASE_BALANCED=0 / 1: TableGeom::sq one way for every nq
    int phase_tt = -1;          // APTGPU_PHASE_TT=0: PHASE taps in phase-major rows only
    int phase_wide = -1;        // APTGPU_PHASE_WIDE=1: the 512- / 1024-thread PHASE forms first
    long table_lds_kb = 0;      // APTGPU_TABLE_LDS_KB=16 .. 160: LDS the TABLE form may take (else 80 KB)
    int phase_identity = -1;    // APTGPU_PHASE_IDENTITY=1: PHASE slot = thread, as until round 4
};
PlanSwitches read_plan_switches();

// Run-time geometry of the table-driven stage 1 (k_fused in TABLE mode; fused_table_supported fills it)
struct TableGeom {
    uint32_t l, m;             // interpolation / decimation factors
    uint32_t jlim;             // taps the reference uses (2*off + 1)
    uint32_t tpp;              // row stride of the phase-major table (>= taps per phase, odd)
    uint32_t xt;               // input tile, floats (multiple of 4)
    uint32_t off_x;            // LDS offset of the input tile in floats (the table sits at 0)
    uint32_t step_q, step_r;   // (NTHR*m) / l and % l: x0 / phase update between a thread's outputs
    uint32_t jl_a, jl_b;       // jlim / l and % l: taps of phase p = jl_a + (p < jl_b)
    // PHASE mode: the thread -> branch-slot assignment (fused_phase_table): `nperm` lists of `nthr` uint32 entries at
    // float offset `perm_off` of the table buffer, list (tile % nperm) for a tile; an entry >= step_r marks an idle thread
    uint32_t nthr, perm_off, nperm;
    uint32_t nq;               // PHASE mode: branches per thread (1, 2, 4, 8, 16)
    // PHASE mode: the slot stride — a thread with list entry u < sq holds the slots u + q sq (q < nq) that are < step_r.
    // nq == 1: sq = step_r.  nq == 4 (standard and slow profile), 8: sq = nthr (round 6: every thread has work and only the LAST slots of some threads
    // do not exist — l = 832: four slots for threads 0-63, three for the others, 13 wave-branches per tile instead of the 16
    // of sq = step_r / nq = 208, whose fourth wave ran every branch for 16 lanes: 2-3 % on the front end, not the 5 % the
    // instruction count promised — these kernels wait more than they issue, profiles/r06_phase_balanced_ab.txt).  Else
    // sq = step_r / nq (no gain / a loss measured).  APTGPU_PHASE_BALANCED=0 / 1 forces one form for every nq.
    uint32_t sq;
    uint32_t stream;           // PHASE mode: taps streamed from the table (filters too long for the registers), rows padded to 16
    // PHASE mode, exact != 0 (the tile phases repeat with a period nperm = 1 << perm_shift <= 8): list (tile % nperm) is
    // built for that tile's phase, and everything a tile derives from its index by division is tabulated — per phase r the
    // first input sample's quotient x0r[r] and remainder rbr[r] (tile = nperm t + r: X0 = x0r[r] + t xd), per thread the
    // window start and polyphase branch of each of its nq slots, packed (c | p << 16) at float offset cp_off
    // ([nperm][nthr][nq] uint32).  exact == 0: one list serves every tile and the kernel divides.
    uint32_t exact, perm_shift, cp_off, xd;
    // ... and the taps once more in THREAD order at float offset tt_off: [nperm][nq][tpp / 4][nthr] quads — quad e of
    // the branch of thread t's slot q — so that a wave's tap load is 1 KB of consecutive memory (from the phase-major
    // table every lane reads a row of its own: 64 cache lines per load)
    uint32_t tt_off;
    int32_t x0r[8];
    uint32_t rbr[8];
};

// PHASE stage 1 with ONE branch per thread (l <= 256: 44 100 Hz, 48 kHz at the fast profile, 8 / 16 / 24 / 32 kHz ...): the
// paired input tile goes through LDS in two halves of eight windows each (round 6; kernel and phase_geom must agree, hence
// a macro).  Its 45-52 KB were what held these kernels at three workgroups per CU.
#ifndef APT_PHASE_HALVES
#define APT_PHASE_HALVES 1
#endif
// (not the standard profile's kernel in APTGPU_MODE_FAST: its 68-tap branch is then fetched twice, in segments, by a kernel
// that has half the arithmetic to hide it under — 0.80 -> 0.86 ms per 16 at 44 100 Hz, profiles/r06_phase_halves_ab.txt)
constexpr bool phase_halves(int nq, bool stream, int nthr, int t2, bool fast)
{
    return APT_PHASE_HALVES != 0 && nq == 1 && !stream && nthr == 256 && !(fast && t2 == 37);
}

// Table-driven stage 1 + the specialised work-rate stages (k_fused in TABLE mode): any (l, m, taps) whose
// phase-major table and input tile fit two 512-thread workgroups per CU (lds_kb: PlanSwitches::table_lds_kb), standard-profile
// work-rate stages (37-tap low-pass, pw = 3).  11 025 Hz (l = 832) is the rate this exists for.
bool fused_table_supported(uint32_t l, uint32_t m, uint32_t t1, uint32_t t2, uint32_t pw, long lds_kb, TableGeom *geom);

// Phase-resident stage 1 + the specialised work-rate stages (k_fused in PHASE mode): a thread holds nq slots u + q S'
// (S' = step_r / nq <= threads) of the step_r outputs after which the polyphase branches repeat, and computes the
// 16 / nq outputs of each that fall into the tile, with the taps of their common branch in registers (or, `stream`,
// fetched sixteen at a time).  256 threads with nq = 1, 2, 4 (l <= 256, 512, 1024) at the standard profile, nq = 1, 4, 8,
// 16 at the fast profile, nq = 1, 2, 4 with streamed taps at the slow profile; 512- / 1024-thread forms with nq = 1 as
// fallbacks.  Every rate a sound card records at is served this way (44 100 Hz: l = 208; 22 050: 416; 11 025: 832).
// TableGeom use: step_r = S, step_q = S*m/l, tpp = row stride of the table (multiple of 4; 16 when streamed), off_x = f2
// entries per region of the paired input tile, xt = floats of the whole tile; the rest: see the struct.
bool fused_phase_supported(uint32_t l, uint32_t m, uint32_t t1, uint32_t t2, uint32_t pw, const PlanSwitches &sw, TableGeom *geom);
// kModeStrictPad2 on the PHASE kernels: the low-pass bound of the instantiation that serves a low-pass of t2 taps other than
// the standard profile's 37 (a tuned demodulation_atten at a sound-card rate), or 0 (APTGPU_FUSED_PAD=0: as until round 6,
// k_fused_any)
uint32_t fused_phase_pad_t2(uint32_t t2, uint32_t pw, const PlanSwitches &sw);
uint32_t fused_phase_table_floats(const TableGeom &geom);
// host: [l][tpp] taps, rows 16-byte aligned, then the thread assignment lists (geom.perm_off); t2: the low-pass length the
// KERNEL is compiled for (kFusedVariants[v].t2), which fixes its tile
void fused_phase_table(const TableGeom &geom, uint32_t t2, uint32_t pw, const float *coeff, float *table, const PlanSwitches &sw);

// ---- the plan's front end, chosen once
enum class FrontEndKind {  // (the values stats.fused / aptgpu_plan_info.fused report)
    Unfused = 0,  // the generic kernels, one per stage
    Split = 1,    // k_fused, SPLIT stage 1: compile-time specialised (48 / 96 kHz)
    Any = 2,      // k_fused_any: everything a run-time parameter
    Table = 3,    // k_fused, table-driven stage 1 (run-time l / m / taps, specialised work-rate stages)
    Phase = 4,    // k_fused, phase-resident stage 1 (likewise)
};
struct FrontEnd {
    FrontEndKind kind = FrontEndKind::Unfused;
    int kmode = kModeStrict;                              // the mode asked of the kernel family (kModeStrictPad: either padded form)
    FusedVariant variant[2] = {kFusedNone, kFusedNone};   // the k_fused instantiation for f32 / 16-bit PCM input (none: staged as f32)
    uint32_t pad_t1 = 0;  // != 0: the strict kernel compiled for this tap-count bound serves the plan (kModeStrictPad)
    uint32_t pad_t2 = 0;  // != 0: ... and for this low-pass bound (kModeStrictPad2: h2 / h2p padded, FusedParams::t2)
    bool fast = false;    // APTGPU_MODE_FAST served by the front end (the picker then re-evaluates from pulse sums)
    bool f16 = false;     // APTGPU_MODE_FP16_TAPS served by the specialised kernel (fp16 stage 1)
    bool mfma = false;    // fast mode on the matrix cores (kModeMfma: tuned tap counts, or APTGPU_FAST_MFMA=1)
    TableGeom geom{};     // Table / Phase
    size_t lds_floats = 0;  // Table / Phase: dynamic LDS of the launch, by the instantiation's own T2
    // F in pixel-phase planes (apt::gpu::f_index)?  The k_fused instantiations write them; k_fused_any and the unfused
    // kernels write F contiguously.  The ONE place that says so.
    bool writes_planes() const { return kind == FrontEndKind::Split || kind == FrontEndKind::Table || kind == FrontEndKind::Phase; }
};
// Pure: no stream, no environment.  mode: APTGPU_MODE_*; throws Internal where host and kernel would disagree on a tile.
FrontEnd select_front_end(uint32_t l, uint32_t m, uint32_t t1, uint32_t t2, uint32_t pw, int mode, bool work_is_multiple,
                          bool export_filtered, const PlanSwitches &sw);

}  // namespace apt::gpu
