// apt_kernels_fused_any_geom.hpp — the run-time front end's (k_fused_any) host side: which launch shape serves a
// geometry, its LDS layout, and the phase-major tap table.  Host-only and free of HIP, so that the plan's choice of front
// end (apt_front_end.hpp) and its CPU test build with the host compiler alone.
#pragma once

#include <cstddef>
#include <cstdint>

namespace apt::gpu {

struct AnyGeom {
    uint32_t l, m, jlim;   // resampler: factors, taps the reference uses (2*off + 1)
    uint32_t tpp;          // row stride of the phase-major table (>= taps per phase, odd)
    uint32_t t2;           // low-pass taps
    uint32_t g, pulse;     // sync frame length 38*pw and pulse width 2*pw
    uint32_t kt, pre, own; // tile geometry (work samples)
    uint32_t xt;           // input tile, floats (multiple of 4)
    uint32_t off_x, off_a, off_b;  // LDS offsets in floats (table at 0)
    uint32_t step_q, step_r;       // (NTHR*m) / l and % l: x0 / phase update between a thread's outputs
    uint32_t jl_a, jl_b;           // jlim / l and % l: taps of phase p = jl_a + (p < jl_b)
    uint32_t table_in_global;      // the polyphase table does not fit LDS beside the tile: stage 1 reads its rows from HBM / L2
    uint64_t sign[4];              // bit j set <=> sync template[j] = +1 (decode.rs:188-198)
    float gm_slack_scale;          // APTGPU_GM_SLACK_SCALE as the plan read it (LaunchSwitches), host side only
};

constexpr int kAnyGS = 52;  // correlation positions per group (apt_kernels_sync.hip)
constexpr size_t kAnyLdsLimit = 160 * 1024;

struct AnyCandidate {
    int nthr, kpt;
};
// most resident waves per CU first (LDS permitting), then the larger tile
// (round 6: {256, 4} — a tile of 1024 work samples — for input rates beyond seventeen times the work rate's 1 / l share:
// 250 kHz SDR recordings, whose 2048-sample tile needs more input than the LDS holds, ran the unfused kernels)
constexpr AnyCandidate kAnyCandidates[] = {{256, 8}, {1024, 8}, {1024, 4}, {256, 4}};

inline bool any_make_geom(uint32_t l, uint32_t m, uint32_t t1, uint32_t t2, uint32_t pw, int nthr, int kpt, bool table_in_global,
                          AnyGeom *out, size_t *lds_bytes)
{
    AnyGeom g{};
    g.l = l;
    g.m = m;
    g.jlim = 2 * ((t1 - 1) / 2) + 1;
    const uint32_t per_phase = (g.jlim + l - 1) / l;
    g.tpp = per_phase | 1u;  // odd stride: rows of consecutive phases start in different banks
    g.t2 = t2;
    g.g = 38 * pw;
    g.pulse = 2 * pw;
    g.kt = static_cast<uint32_t>(nthr * kpt);
    if (38 * pw > 256) return false;  // sign bitmap
    // 32-bit in-tile index math: (tile outputs + look-ahead) * m + l must stay below 2^31 (per launch shape since round 6:
    // the old blanket test for the largest tile sent every rate above 170 kHz that is coprime to the work rate to the
    // unfused kernels)
    if ((static_cast<uint64_t>(g.kt) + 4096u) * m + l > 0x7fffffffull) return false;
    g.pre = (t2 + 2 * static_cast<uint32_t>(kpt) + static_cast<uint32_t>(kpt) - 1) / static_cast<uint32_t>(kpt) *
            static_cast<uint32_t>(kpt);  // multiple of KPT (and of 4)
    if (g.kt < g.pre + g.g + kAnyGS) return false;
    g.own = (g.kt - g.pre - (g.g - 1)) / kAnyGS * kAnyGS;
    if (g.own == 0) return false;
    g.xt = (static_cast<uint32_t>((static_cast<uint64_t>(g.kt) * m + l - 1) / l) + per_phase + 8 + 3) & ~3u;
    if (g.xt < static_cast<uint32_t>(nthr)) g.xt = static_cast<uint32_t>(nthr);  // (stage 4 keeps one float per thread there)
    const uint32_t slack = 64;
    // (a table that does not fit LDS beside the tile — 44 100 Hz at the slow profile: 29 k taps, 116 KB — stays in
    // HBM / L2 and stage 1 reads its rows from there: every thread 856 bytes per output, but fused: R, D and C still
    // never leave the CU)
    g.table_in_global = table_in_global ? 1u : 0u;
    g.off_x = table_in_global ? 0u : ((l * g.tpp + 3u) & ~3u);
    const uint32_t ab_len = ((g.kt + slack) + (g.kt + slack) / static_cast<uint32_t>(kpt) + 8u) & ~3u;  // padded
    g.off_a = g.off_x + g.xt;
    g.off_b = g.off_a + ab_len;
    g.step_q = static_cast<uint32_t>((static_cast<uint64_t>(nthr) * m) / l);
    g.step_r = static_cast<uint32_t>((static_cast<uint64_t>(nthr) * m) % l);
    g.jl_a = g.jlim / l;
    g.jl_b = g.jlim % l;
    for (uint32_t j = 0; j < g.g; ++j) {
        const bool plus = j >= g.pulse && j < 15 * g.pulse && (((j - g.pulse) / g.pulse) & 1) == 1;
        if (plus) g.sign[j >> 6] |= 1ull << (j & 63);
    }
    const size_t floats = static_cast<size_t>(g.off_b) + ab_len;
    *lds_bytes = floats * sizeof(float);
    *out = g;
    return *lds_bytes <= kAnyLdsLimit;
}

// picks the launch shape: maximise resident waves per CU, then tile size
inline bool any_choose_with(uint32_t l, uint32_t m, uint32_t t1, uint32_t t2, uint32_t pw, bool in_global, AnyCandidate *best,
                            AnyGeom *geom, size_t *lds)
{
    int best_score = 0;
    uint32_t best_kt = 0;
    bool found = false;
    for (const AnyCandidate &c : kAnyCandidates) {
        AnyGeom g;
        size_t bytes;
        if (!any_make_geom(l, m, t1, t2, pw, c.nthr, c.kpt, in_global, &g, &bytes)) continue;
        int wgs = static_cast<int>(kAnyLdsLimit / bytes);
        int waves = wgs * (c.nthr / 64);
        if (waves > 32) waves = 32;  // 8 per SIMD is plenty
        // tile efficiency matters too: weight by the owned fraction
        const int score = waves * 1000 + static_cast<int>(1000.0 * g.own / g.kt);
        if (!found || score > best_score || (score == best_score && g.kt > best_kt)) {
            best_score = score;
            best_kt = g.kt;
            *best = c;
            *geom = g;
            *lds = bytes;
            found = true;
        }
    }
    return found;
}

// the table in LDS where a launch shape exists for that; else in HBM / L2
inline bool any_choose(uint32_t l, uint32_t m, uint32_t t1, uint32_t t2, uint32_t pw, AnyCandidate *best, AnyGeom *geom, size_t *lds)
{
    return any_choose_with(l, m, t1, t2, pw, false, best, geom, lds) || any_choose_with(l, m, t1, t2, pw, true, best, geom, lds);
}

// run-time parameters, taps phase-major in LDS; same outputs as the specialised front ends
inline bool fused_any_supported(uint32_t l, uint32_t m, uint32_t t1, uint32_t t2, uint32_t pw)
{
    if (l == 0 || m == 0 || t1 == 0 || t2 == 0 || pw == 0) return false;
    AnyCandidate c;
    AnyGeom g;
    size_t lds;
    return any_choose(l, m, t1, t2, pw, &c, &g, &lds);
}

inline uint32_t fused_any_table_floats(uint32_t l, uint32_t t1)
{
    const uint32_t jlim = 2 * ((t1 - 1) / 2) + 1;
    return l * (((jlim + l - 1) / l) | 1u);
}

// host: phase-major table [l][tpp], row p = coeff[p], coeff[p + l], ... (zero padded)
inline void fused_any_table(uint32_t l, const float *coeff, uint32_t t1, float *table)
{
    const uint32_t jlim = 2 * ((t1 - 1) / 2) + 1;
    const uint32_t tpp = ((jlim + l - 1) / l) | 1u;
    for (uint32_t p = 0; p < l; ++p)
        for (uint32_t i = 0; i < tpp; ++i) {
            const uint64_t j = p + static_cast<uint64_t>(i) * l;
            table[static_cast<size_t>(p) * tpp + i] = j < jlim ? coeff[j] : 0.f;
        }
}

}  // namespace apt::gpu
