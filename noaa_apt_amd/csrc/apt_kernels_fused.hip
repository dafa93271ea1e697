// apt_kernels_fused.hip — the fused, specialised front end of decode() for gfx950.
//
//   x (input rate) --polyphase FIR--> R --AM envelope--> D --low-pass--> F --sync corr--> C
//
// One launch produces F (the filtered work-rate signal, the only intermediate that goes
// back to HBM) and GM (the maximum of the sync cross-correlation over groups of GS
// consecutive positions — all the peak picker needs; see apt_kernels_sync.hip).  R, D
// and C never leave the CU.  Reference: src/decode.rs:77-110, src/dsp.rs:186-289,
// 350-410, src/decode.rs:225-233.
//
// Behind stage 1 thread t of a 256-thread workgroup owns the 13 consecutive work-rate samples 13 t .. 13 t + 12 of a
// tile of 3328 (halo threads either side: the low-pass and the envelope look back, the correlation looks ahead); R, D, F
// and the pulse sums go through two LDS regions.  Stage 1 — the polyphase resampler — comes in three forms:
//   SPLIT (M > 0: 48 / 96 kHz)   taps wave-uniform: scalar loads into pinned SGPR tuples, every window sample read once
//                                from LDS and broadcast against a pair of taps feeding a pair of accumulators;
//   PHASE (M < 0: every other rate a sound card records at)   taps thread-resident, samples paired in LDS;
//   TABLE (M == 0: fallback)     taps and samples from LDS.
// Every product and sum is a separate multiplication / addition in the reference's order: bit-identical to the scalar
// Rust loop (no FMA; #pragma fp contract(off)).  This file: the host side — the SPLIT tap tables in the layouts the kernels
// read and the launch; which kernel serves which plan: apt_front_end.hpp (select_front_end) over the list and the
// selection functions of apt_kernels_fused_variants.hpp.
#include "apt_kernels_fused_launch.hpp"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <type_traits>
#include <vector>

#pragma clang fp contract(off)

namespace apt::gpu {

namespace {
// the launch functions of the list's rows, [variant][pcm16]; launches variant v, false where there is none
using LaunchFn = void (*)(const FusedLaunch &);
#define APT_FUSED_FN_BOTH(name, ...) {&fused_launch<kFused_##name, float>, &fused_launch<kFused_##name, int16_t>},
#define APT_FUSED_FN_F32(name, ...) {&fused_launch<kFused_##name, float>, nullptr},
constexpr LaunchFn kFusedLaunch[kFusedVariantCount][2] = {APT_FUSED_VARIANTS(APT_FUSED_FN_BOTH, APT_FUSED_FN_F32)};
#undef APT_FUSED_FN_BOTH
#undef APT_FUSED_FN_F32
bool launch_variant(FusedVariant v, bool pcm16, const FusedLaunch &a, int *variant_out)
{
    const LaunchFn fn = v == kFusedNone ? nullptr : kFusedLaunch[v][pcm16 ? 1 : 0];
    if (fn) fn(a);
    if (variant_out) *variant_out = fn ? static_cast<int>(v) : static_cast<int>(kFusedNone);
    return fn != nullptr;
}
}  // namespace

// floats in the stage-1 tap table: the SPLIT layout (apt_kernels_fused_launch.hpp), one chunk-major table per half
uint32_t fused_tap_table_floats(uint32_t l, uint32_t m, uint32_t t1, int ch)
{
    (void)ch;  // kSplitChunk
    // (t1: the tap count the kernel is compiled for — the filter's own, or kModeStrictPad's bound)
    const int li = static_cast<int>(l), mi = static_cast<int>(m), ti = static_cast<int>(t1);
    return static_cast<uint32_t>(fused_split_table_offset(li, mi, ti, 1) + (fused_split_nch(li, mi, ti, 1) + 1) * kSplitChunkDwords);
}

// host: per half h, chunk c holds for its window samples q = w0 + 4 c + e (e < 4) the pairs (tap of branch b0 + 2k at
// q, tap of branch b0 + 2k + 1 at q) at dwords 6 e + 2 k, k < 3, then (a half with an odd number of branches) the last
// branch's taps at q = w0 + 4 c .. + 3 at dwords 24 .. 27; 0 where a branch has no tap for q; one zero row behind
// each half.  Tap of branch b at window sample q: coeff[p_b + (q - c_b) l], c_b = ceil(b m / l), p_b = c_b l - b m
// (dsp.rs:252-263).
// t1_layout (0: t1): the tap count the kernel is compiled for when that is a bound (kModeStrictPad) — the table then has
// that kernel's chunks and zeros behind the filter's last tap.
void fused_branch_taps(uint32_t l, uint32_t m, const float *coeff, uint32_t t1, int ch, float *hs, uint32_t t1_layout)
{
    (void)ch;
    if (t1_layout == 0) t1_layout = t1;
    const uint32_t tp = (t1_layout + l - 1) / l;
    const uint32_t clast = ((l - 1) * m + l - 1) / l;
    const uint32_t win = clast + tp;
    auto tap = [&](uint32_t b, int64_t q) -> float {
        const uint32_t cb = (b * m + l - 1) / l;
        const uint32_t pb = cb * l - b * m;
        if (q < static_cast<int64_t>(cb) || q >= static_cast<int64_t>(win)) return 0.f;
        const uint64_t j = pb + static_cast<uint64_t>(q - cb) * l;
        return j < t1 ? coeff[j] : 0.f;
    };
    const int li = static_cast<int>(l), mi = static_cast<int>(m), ti = static_cast<int>(t1_layout);
    for (int h = 0; h < 2; ++h) {
        const int b0 = fused_split_b0(li, h), nbr = fused_split_nbr(li, h), w0 = fused_split_w0(li, mi, h);
        const int nch_h = fused_split_nch(li, mi, ti, h);
        float *base = hs + fused_split_table_offset(li, mi, ti, h);
        for (int c = 0; c <= nch_h; ++c) {
            float *row = base + static_cast<size_t>(c) * kSplitChunkDwords;
            for (int i = 0; i < kSplitChunkDwords; ++i) row[i] = 0.f;
            if (c == nch_h) break;
            for (int e = 0; e < kSplitChunk; ++e) {
                const int64_t q = w0 + static_cast<int64_t>(kSplitChunk) * c + e;
                for (int k = 0; k < nbr / 2; ++k) {
                    row[6 * e + 2 * k] = tap(static_cast<uint32_t>(b0 + 2 * k), q);
                    row[6 * e + 2 * k + 1] = tap(static_cast<uint32_t>(b0 + 2 * k + 1), q);
                }
                if (nbr & 1) row[24 + e] = tap(static_cast<uint32_t>(b0 + nbr - 1), q);
            }
        }
    }
}

int fused_chunk_of(uint32_t m, bool fast)
{
    return fused_chunk(static_cast<int>(m), fast ? kModeFast : kModeStrict);
}

// host: stage-3 table h2p[k] = (h2[k-1], h2[k]) for k = 0 .. t2 (0 outside the filter)
void fused_lowpass_pairs(const float *h2, uint32_t t2, float *h2p)
{
    for (uint32_t k = 0; k <= t2; ++k) {
        h2p[2 * k] = k >= 1 ? h2[k - 1] : 0.f;
        h2p[2 * k + 1] = k < t2 ? h2[k] : 0.f;
    }
}

uint32_t fused_f16_table_dwords(uint32_t l, uint32_t m, uint32_t t1)
{
    const uint32_t tp = (t1 + l - 1) / l;
    const uint32_t clast = ((l - 1) * m + l - 1) / l;
    return ((clast + tp + 1) / 2) * 16;
}

// host: [ceil(WIN/2)][16] half2 bit patterns — entry (qp, b) = taps of branch b at window samples
// (2qp, 2qp+1), prescaled by a power of two into the fp16 normal range; returns 2^-s
float fused_f16_branch_taps(uint32_t l, uint32_t m, const float *coeff, uint32_t t1, uint32_t *table)
{
    const uint32_t tp = (t1 + l - 1) / l;
    const uint32_t clast = ((l - 1) * m + l - 1) / l;
    const uint32_t win = clast + tp;
    auto tap = [&](uint32_t b, uint32_t q) -> float {
        const uint32_t cb = (b * m + l - 1) / l;
        const uint32_t pb = cb * l - b * m;
        if (q < cb || q >= win) return 0.f;
        const uint64_t j = pb + static_cast<uint64_t>(q - cb) * l;
        return j < t1 ? coeff[j] : 0.f;
    };
    float mx = 0.f;
    for (uint32_t j = 0; j < t1; ++j) mx = fmaxf(mx, fabsf(coeff[j]));
    int e = 0;
    if (mx > 0.f) (void)frexpf(mx, &e);
    const int sh = -e + 1;  // scaled maximum in [1, 2)
    const float scale = ldexpf(1.f, sh);
    auto bits = [](float v) -> uint32_t {
        const _Float16 h = static_cast<_Float16>(v);
        uint16_t u;
        __builtin_memcpy(&u, &h, 2);
        return u;
    };
    const uint32_t nqp = (win + 1) / 2;
    for (uint32_t qp = 0; qp < nqp; ++qp)
        for (uint32_t b = 0; b < 16; ++b)
            table[qp * 16 + b] = b < l ? (bits(tap(b, 2 * qp) * scale) | (bits(tap(b, 2 * qp + 1) * scale) << 16)) : 0u;
    return ldexpf(1.f, -sh);
}

// Bound on |a - c| / sum|F| for a = the pulse-sum evaluation and c = the reference's sequential chain of
// the 38*pw-term sync correlation: gamma(38 pw - 1) + gamma(pw + 18) with gamma(k) = k u / (1 - k u),
// u = 2^-24, plus 3 % for the rounding of the bound's own arithmetic (the sum of |F|, the product, the
// two additions that form lo and hi: < 40 u relative).  `scale` (APTGPU_GM_SLACK_SCALE, tests; read at plan creation —
// LaunchSwitches) widens it so that the picker's exact settlement of open comparisons is exercised on ordinary inputs.
float fused_gm_slack(uint32_t pw, float scale)
{
    return static_cast<float>(38u * pw - 1u + pw + 18u) * 1.03f * 0x1p-24f * 1.0001f * (scale >= 1.f ? scale : 1.f);
}

// ---- kModeMfma: the FIRs as banded Toeplitz products on the matrix cores (apt_kernels_fused_variants.hpp)
namespace {
uint32_t mfma_kpad(uint32_t l, uint32_t m)
{
    const uint32_t t1max = m == 50 ? kMfmaT1Max48k : kMfmaT1Max96k;
    const uint32_t win = ((l - 1) * m + l - 1) / l + (t1max + l - 1) / l;
    return (win + 31u) / 32u * 32u;
}
// a row-major [rows <= 16][K] matrix -> A fragments of v_mfma_f32_16x16x32_bf16, three bf16 pieces per entry:
// table[(piece * nks + s) * 64 + lane] = 8 halves = entries (row = lane & 15, k = 32 s + 8 (lane >> 4) + j), j < 8, of
// piece 0 = the upper half of v's f32 pattern, piece 1 = that of v - piece 0, piece 2 = v - piece 0 - piece 1: three 8-bit
// pieces of the 24-bit significand, v = p0 + p1 + p2 exactly (subnormal taps aside: their last piece is truncated)
template <typename At>
void mfma_fragments(At &&at, uint32_t nks, uint32_t *table)
{
    auto upper = [](float v) -> uint32_t {
        uint32_t u;
        __builtin_memcpy(&u, &v, 4);
        return u >> 16;
    };
    auto value = [](uint32_t h) -> float {
        const uint32_t u = h << 16;
        float v;
        __builtin_memcpy(&v, &u, 4);
        return v;
    };
    for (uint32_t s = 0; s < nks; ++s)
        for (uint32_t lane = 0; lane < 64; ++lane)
            for (uint32_t jp = 0; jp < 4; ++jp) {
                uint32_t w[3] = {0, 0, 0};
                for (uint32_t h = 0; h < 2; ++h) {
                    const float v = at(lane & 15u, 32u * s + 8u * (lane >> 4) + 2u * jp + h);
                    const uint32_t p0 = upper(v);
                    const float r1 = v - value(p0);
                    const uint32_t p1 = upper(r1);
                    const float r2 = r1 - value(p1);
                    const uint32_t p2 = upper(r2);
                    w[0] |= p0 << (16u * h);
                    w[1] |= p1 << (16u * h);
                    w[2] |= p2 << (16u * h);
                }
                for (uint32_t pc = 0; pc < 3; ++pc) table[((pc * nks + s) * 64u + lane) * 4u + jp] = w[pc];
            }
}
}  // namespace

uint32_t fused_mfma_table_dwords(uint32_t l, uint32_t m) { return 3u * (mfma_kpad(l, m) / 32u) * 64u * 4u; }

// host: H[b][q] = coeff[p_b + (q - c_b) l] (0 outside the branch's taps): branch b of a window against window sample q
// (dsp.rs:252-263; c_b = ceil(b m / l), p_b = c_b l - b m), rows 13 .. 15 zero
void fused_mfma_table(uint32_t l, uint32_t m, const float *coeff, uint32_t t1, uint32_t *table)
{
    auto at = [&](uint32_t b, uint32_t q) -> float {
        if (b >= l) return 0.f;
        const uint32_t cb = (b * m + l - 1) / l, pb = cb * l - b * m;
        if (q < cb) return 0.f;
        const uint64_t j = pb + static_cast<uint64_t>(q - cb) * l;
        return j < t1 ? coeff[j] : 0.f;
    };
    mfma_fragments(at, mfma_kpad(l, m) / 32u, table);  // (no prescale: bf16 pieces carry f32's exponent)
}

bool fused_front_end(hipStream_t s, const FrontEnd &fe, bool pcm16, const CallArgs &call, const FusedParams *d_prm,
                     uint64_t max_w, int *variant_out)
{
    if (variant_out) *variant_out = static_cast<int>(kFusedNone);
    if (call.count == 0 || call.count > static_cast<uint32_t>(kMaxCall)) return false;
    const bool split = fe.kind == FrontEndKind::Split;
    if (pcm16)  // (SPLIT: dword loads of sample pairs)
        for (uint32_t i = 0; i < call.count; ++i)
            if (reinterpret_cast<uintptr_t>(call.rec[i].x) & (split ? 3u : 1u)) return false;
    const FusedVariant v = fe.variant[pcm16 ? 1 : 0];
    const FusedLaunch a{s, &call, d_prm, max_w, fe.lds_floats};
#ifdef APT_WITH_PROBES
    // APTGPU_PROBE_STOP: the timing probes stand in for the stock 48 kHz f32 kernels (fast: 1..5, 8, 9; strict: 11..17)
    static const int probe = [] {
        const char *e = std::getenv("APTGPU_PROBE_STOP");
        return e ? std::atoi(e) : 0;
    }();
    if (v == kFused_48k_fast && !pcm16 && probe >= 1 && probe <= 9 && probe != 6 && probe != 7) {  // (6, 7: the 128 / 192-thread forms, gone with the unsplit stage 1)
        void (*const fn[9])(const FusedLaunch &) = {fused_launch_probe1, fused_launch_probe2, fused_launch_probe3,
                                                    fused_launch_probe4, fused_launch_probe5, nullptr,
                                                    nullptr, fused_launch_probe8, fused_launch_probe9};
        fn[probe - 1](a);
        return true;
    }
    if (v == kFused_48k && !pcm16 && probe >= 11 && probe <= 17) {
        void (*const fn[7])(const FusedLaunch &) = {fused_launch_probe11, fused_launch_probe12, fused_launch_probe13,
                                                    fused_launch_probe14, fused_launch_probe15, fused_launch_probe16, fused_launch_probe17};
        fn[probe - 11](a);
        return true;
    }
#endif
    return launch_variant(v, pcm16, a, variant_out);
}

}  // namespace apt::gpu
