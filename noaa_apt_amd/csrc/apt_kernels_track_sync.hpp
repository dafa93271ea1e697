// apt_kernels_track_sync.hpp — the flywheel sync stage behind the front end: a normalised sync score for every work
// sample and a dynamic programme that tracks the row starts through noise and dropouts (apt_kernels_track_sync.hip on
// the GPU, apt_track_sync.cpp on the CPU).  The reference only names the item
// (docs/development.md:148), so the definition is this library's: include/aptgpu.h states it in full and
// tests/np_track_model.py restates it in numpy.  The per-sample arithmetic below is ONE text for the kernels and the
// host twin; every operation is a separately rounded IEEE f32 one (both sides are built with contraction off).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define APT_TRK_HD __host__ __device__ inline
#else
#define APT_TRK_HD inline
#endif

namespace apt::track {

constexpr int kPx = 2080;
constexpr int kMaxJitter = 64;
constexpr int kMaxPw = 8;
constexpr int kStart = -128;  // back-pointer of a path's first position (one byte per position)

// the sign of the sync template at index j (generate_sync_frame, decode.rs:188-198; sync_template_plus of
// apt_sync_corr.hpp, restated here so that this header also serves a plain C++ translation unit)
APT_TRK_HD constexpr bool template_plus(int j, int pw)
{
    const int pulse = 2 * pw;
    if (j < pulse || j >= 15 * pulse) return false;
    return (((j - pulse) / pulse) & 1) == 1;
}

APT_TRK_HD uint32_t bits_of(float v)
{
    uint32_t b;
    __builtin_memcpy(&b, &v, sizeof b);
    return b;
}
APT_TRK_HD bool finite(float v) { return (bits_of(v) & 0x7F800000u) != 0x7F800000u; }

// the constants of the score: the template's mean is -10/38, the squared norm of (template - mean) is G (1 - (10/38)^2)
APT_TRK_HD float mean_weight() { return static_cast<float>(10.0 / 38.0); }
APT_TRK_HD float norm_of(uint32_t g) { return static_cast<float>(static_cast<double>(g) * (1.0 - (10.0 / 38.0) * (10.0 / 38.0))); }

// One sample of a position's three chains: c (the reference's +-1 correlation, sync_corr_strict's bits), S1 and S2.
APT_TRK_HD void score_step(float v, bool plus, float &c, float &s1, float &s2)
{
#pragma clang fp contract(off)
    c = plus ? c + v : c - v;
    s1 = s1 + v;
    const float q = v * v;
    s2 = s2 + q;
}
// ... with the square computed once for neighbouring positions that share the sample
APT_TRK_HD void score_step_sq(float v, float q, bool plus, float &c, float &s1, float &s2)
{
#pragma clang fp contract(off)
    c = plus ? c + v : c - v;
    s1 = s1 + v;
    s2 = s2 + q;
}

// The score of a position from its three sums: the zero-mean normalised cross-correlation, or 0 (no evidence) where
// the window's variance is below the relative floor — silence, a constant, NaN / Inf windows, overflowing squares.
APT_TRK_HD float score_finish(float c, float s1, float s2, float fg, float norm, float wmean)
{
#pragma clang fp contract(off)
    const float m = s1 / fg;
    const float p = s1 * m;
    const float var = s2 - p;
    const float t = s1 * wmean;
    const float num = c + t;
    const float floor_ = 1e-4f * s2;
    if (!(var > floor_)) return 0.f;
    const float r = var * norm;
    const float den = sqrtf(r);
    if (!finite(num) || !finite(den)) return 0.f;
    return num / den;
}

// The best predecessor of position i: prev(d) returns best[i - L - d] for a d whose index is >= 0.  Candidates in the
// order 0, -1, +1, ..., -w, +w; a later one wins only when strictly greater.
template <typename Prev>
APT_TRK_HD void best_predecessor(int32_t i, int32_t L, int w, float lam, Prev &&prev, float &cur_out, int &bp_out)
{
#pragma clang fp contract(off)
    float cur = i < L ? 0.f : -__builtin_inff();
    int bp = kStart;
    const int32_t j0 = i - L;
    if (j0 >= 0) {
        const float v = prev(0);  // lam * 0 = 0, best - 0 = best
        const float v0 = v - lam * 0.f;
        if (v0 > cur) {
            cur = v0;
            bp = 0;
        }
    }
    for (int k = 1; k <= w; ++k) {
        const float pen = lam * static_cast<float>(k);
        if (j0 + k >= 0) {  // d = -k
            const float v = prev(-k) - pen;
            if (v > cur) {
                cur = v;
                bp = -k;
            }
        }
        if (j0 - k >= 0) {  // d = +k
            const float v = prev(k) - pen;
            if (v > cur) {
                cur = v;
                bp = k;
            }
        }
    }
    cur_out = cur;
    bp_out = bp;
}

}  // namespace apt::track

#if defined(__HIPCC__)
// ---- the per-thread body of the score kernels (k_track_score, k_stream_track_score): ONE text for the order-sensitive
// sums.  `tile` (LDS, 16-byte aligned) holds the workgroup's kScoreTile positions' samples and their halo, sample e of
// the tile at tile[e]; thread tid computes the positions 4 tid .. 4 tid + 3 from 16-byte reads (lane t reads quad
// t + k: consecutive addresses).  The three chains of a position are sequential by definition; the twelve chains of a
// thread are independent.
namespace apt::track {

constexpr int kScoreThreads = 256;
constexpr int kScorePer = 4;                           // positions per thread
constexpr int kScoreTile = kScoreThreads * kScorePer;  // positions per workgroup
template <int PW>
struct ScoreTile {
    static constexpr int G = 38 * PW;
    static constexpr int Q = (G + kScorePer - 1 + 3) / 4;  // quads a thread reads: its G + 3 samples
    static constexpr int LEN = kScoreTile + 4 * Q;         // floats of the tile with its halo (Q quads from the last thread's first)
};

template <int PW>
__device__ __forceinline__ void score_four(const float *__restrict__ tile, int tid, float (&out)[kScorePer])
{
    constexpr int G = ScoreTile<PW>::G, Q = ScoreTile<PW>::Q;
    float c[kScorePer], s1[kScorePer], s2[kScorePer];
#pragma unroll
    for (int p = 0; p < kScorePer; ++p) c[p] = s1[p] = s2[p] = 0.f;
    const float4 *__restrict__ quads = reinterpret_cast<const float4 *>(tile) + tid;
    // One quad of the thread's run: sample j = j0 + e is sample j - p of position p's window.  j0 is a compile-time
    // constant wherever this is called (signs and window tests fold away).
    auto quad = [&](const float4 v4, const int j0) {
        const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = j0 + e;
            const float q = __fmul_rn(v[e], v[e]);
#pragma unroll
            for (int p = 0; p < kScorePer; ++p)
                if (j - p >= 0 && j - p < G) score_step_sq(v[e], q, template_plus(j - p, PW), c[p], s1[p], s2[p]);
        }
    };
    // Unrolled whole, the Q quads' LDS reads are all issued up front (241 VGPRs at pw = 3, the budget's 256 above).  The
    // template repeats every 4 pw samples = pw quads between its first pulse and its tail, and its tail is all minus:
    // where every one of the four windows is inside such a zone the loop over it stays a loop, with the signs of its
    // first turn.  Same additions in the same order: same bits.
    constexpr int K0 = (2 * PW + 3 + 3) / 4;                  // first quad with j - 3 >= 2 pw
    constexpr int P = (30 * PW - 4 * K0) / (4 * PW);          // whole periods from there that end by 30 pw
    constexpr int K1 = K0 + P * PW;
    constexpr int K2 = (30 * PW + 3 + 3) / 4;                 // first quad with j - 3 >= 30 pw
    constexpr int K3 = G / 4;                                 // quads that end inside the window of position 0
    static_assert(K1 <= K2 && K2 <= K3 && K3 <= Q, "zones of the score loop");
#pragma unroll
    for (int k = 0; k < K0; ++k) quad(quads[k], 4 * k);
#pragma unroll 1
    for (int it = 0; it < P; ++it) {
        const float4 *__restrict__ qp = quads + K0 + it * PW;
#pragma unroll
        for (int kk = 0; kk < PW; ++kk) quad(qp[kk], 4 * (K0 + kk));
    }
#pragma unroll
    for (int k = K1; k < K2; ++k) quad(quads[k], 4 * k);
#pragma unroll 1
    for (int k = K2; k < K3; ++k) quad(quads[k], 4 * K2);
#pragma unroll
    for (int k = K3; k < Q; ++k) quad(quads[k], 4 * k);
    const float fg = static_cast<float>(G), norm = norm_of(G), wmean = mean_weight();
#pragma unroll
    for (int p = 0; p < kScorePer; ++p) out[p] = score_finish(c[p], s1[p], s2[p], fg, norm, wmean);
}

}  // namespace apt::track
#endif

// ---- the host side (apt_track_sync.cpp; CPU only)
#include <vector>

#include "../../include/aptgpu.h"
#include "apt_host.hpp"

namespace apt::track {

struct Settings {
    int w;      // max_jitter
    float lam;  // penalty
};
struct Geometry {
    uint32_t pw, L, G;
    uint32_t M;        // positions scored: n - G
    uint32_t pos_cap;  // upper bound of the path's length
};
// NULL = the defaults (w = 8, lambda = 0.1).  A struct_size that is too small, w > 64, a negative or non-finite
// penalty: Error{Invalid}.
Settings check_settings(const aptgpu_track_settings *s);
// pw = work_rate / 4160 must be an integer in 1..8 and 4 w < L: Error{Invalid} otherwise
uint32_t pixel_width(uint32_t work_rate_hz, const Settings &s);
// the path can have at most this many positions over m scores (every step is at least L - w)
inline uint32_t positions_bound(uint64_t m, uint32_t L, int w) { return static_cast<uint32_t>(m / (L - static_cast<uint32_t>(w)) + 2); }
// n >= L + G and n < 2^31: Error{Invalid} otherwise
Geometry geometry_of(uint64_t n, uint32_t pw, const Settings &s);
// checks info->struct_size where info is given
void check_result_struct(const aptgpu_track_result *info);

// The definition in plain C++.  score: g.M floats.  positions / scores: the path, ascending; rows (nullable): 2080
// floats per position p with p + L <= n, appended.
void score_host(const float *x, const Geometry &g, float *score);
void track_host(const float *x, uint64_t n, const Geometry &g, const Settings &s, const float *score,
                std::vector<uint32_t> &positions, std::vector<float> &scores, std::vector<float> *rows,
                aptgpu_track_result *info);
const char *reason_text(int reason);

}  // namespace apt::track

#if defined(__HIPCC__)
#include "apt_kernels.hpp"

namespace apt::gpu {

// Device-side record == aptgpu_track_result (include/aptgpu.h).
struct TrackResult {
    uint32_t struct_size;
    int32_t status;        // 0 ok, 1 Internal
    int32_t reason;        // 0; 1 the decode before it refused the recording; 2 too short; 3 position list overflow; 4 rows truncated
    uint32_t n_positions;  // K
    uint32_t n_rows;       // rows written
    uint32_t end;          // the path's last position
    uint64_t n;            // work samples of the recording
    float total;           // best[end]
    uint32_t reserved;
};

constexpr int kTrackMaxCall = 32;  // recordings per launch
// One recording of a launch.  x is read through f_index(i, pw, f_stride); n comes from res->work_len on the device
// when res is given (the plan form: the decode record of the same slot), else from `n`.
struct TrackRec {
    const float *x;
    const Result *res;
    uint64_t n;          // samples (res == nullptr), else the capacity the buffers were sized for
    uint32_t f_stride;
    uint32_t pos_cap;    // entries of pos / pscore; tmp has as many
    float *score;        // [n - G] s
    int8_t *bp;          // [n - G] back-pointers
    uint32_t *pos;       // [pos_cap] positions, ascending
    uint32_t *tmp;       // [pos_cap] the back-track's scratch
    float *pscore;       // [pos_cap] s at the positions
    float *rows;         // nullable
    uint32_t rows_cap;
    TrackResult *rec;
};
struct TrackCall {
    uint32_t count;
    TrackRec rec[kTrackMaxCall];
};

// k_track_score: s for every position of every recording of the call (grid: tiles of the longest x recordings).
void track_score(hipStream_t s, const TrackCall &call, uint32_t pw, uint64_t max_n);
// k_track_dp: the dynamic programme, the back-track, the positions' scores and the record; one workgroup per recording.
void track_dp(hipStream_t s, const TrackCall &call, uint32_t pw, int w, float lam);
// k_track_rows: row[c] = x[p + pw c] for the positions the record counts as rows.
void track_rows(hipStream_t s, const TrackCall &call, uint32_t pw, uint32_t max_rows);

}  // namespace apt::gpu
#endif
