// apt_kernels_stream_track.hip — the gfx950 kernels of live flywheel sync (include/aptgpu.h §4e).  Per
// launch sequence, behind k_stream_front:
//   k_stream_track_score<PW>  s[i] for the newly final positions [m0, m1): k_track_score's shape — a tile of F with its
//                             G + 3 halo staged into LDS through the ring index, four positions per thread from 16-byte
//                             LDS reads — and k_track_score's per-thread body itself (score_four of
//                             apt_kernels_track_sync.hpp: one text), so §21's bits
//   k_stream_track_dp         one workgroup: best / bp from m0 to m1 in pieces of at most C = L - w positions with a
//                             barrier between them, stopping at every checkpoint on the way for the end search (a tree
//                             reduction over (value, index), the lowest index among equals), the back-track and the
//                             commit (one thread: checkpoint() of apt_kernels_stream_track.hpp); then the records
//   k_stream_track_rows       row[c] = F[v + pw c] for the positions the sequence released
// The best window stays in HBM / L2 within a launch as between launches (DESIGN.md §24 weighs this against k_track_dp's
// LDS ring).  Every ring index is `absolute index & (capacity - 1)`: no access leaves its buffer whatever the records
// hold.  Every loop is bounded by values the host derived; reaching a bound is status 1 with a reason.
#include "apt_kernels_stream_track.hpp"

#pragma clang fp contract(off)

namespace apt::gpu {

namespace st = apt::stream;
namespace tk = apt::stream_track;

namespace {

using apt::track::kScorePer;
using apt::track::kScoreThreads;
using apt::track::kScoreTile;
constexpr int kDpThreads = 1024;
constexpr int kMaxWalk = 2 * static_cast<int>(tk::kMaxLag) + 16;

template <int PW>
__global__ void __launch_bounds__(kScoreThreads)
k_stream_track_score(const float *__restrict__ ring_f, uint32_t fmask, float *__restrict__ ring_s, uint32_t smask,
                     const st::State *__restrict__ state, uint64_t m0, uint64_t m1, uint64_t w1)
{
    constexpr int LEN = apt::track::ScoreTile<PW>::LEN;
    __shared__ __attribute__((aligned(16))) float tile[LEN];

    if (state->status != 0) return;  // (a failed stream stays failed until reset)
    const uint64_t i0 = m0 + static_cast<uint64_t>(blockIdx.x) * kScoreTile;
    if (i0 >= m1) return;
    const int tid = static_cast<int>(threadIdx.x);
    // the tile through the ring index (the wrap included); beyond the final samples nothing a position below m1 reads
    for (int e = tid; e < LEN; e += kScoreThreads) {
        const uint64_t i = i0 + static_cast<uint32_t>(e);
        tile[e] = i < w1 ? ring_f[static_cast<uint32_t>(i) & fmask] : 0.f;
    }
    __syncthreads();

    float out[kScorePer];
    apt::track::score_four<PW>(tile, tid, out);  // (§21's body, one text: the sums are §21's bit for bit)
    __syncthreads();
#pragma unroll
    for (int p = 0; p < kScorePer; ++p) tile[kScorePer * tid + p] = out[p];
    __syncthreads();
    for (int e = tid; e < kScoreTile; e += kScoreThreads) {
        const uint64_t i = i0 + static_cast<uint32_t>(e);
        if (i < m1) ring_s[static_cast<uint32_t>(i) & smask] = tile[e];
    }
}

// The rings are read and written by the same workgroup across barriers: no __restrict__, no const on them.
__global__ void __launch_bounds__(kDpThreads)
k_stream_track_dp(const tk::Params T, st::State *state, tk::Record *record, const float *ring_s, float *ring_best,
                  int8_t *ring_bp, uint64_t *positions, float *scores, uint32_t rows_cap, uint64_t n_in, uint64_t m0, uint64_t m1,
                  uint64_t w1, uint32_t trips, int first, int finish)
{
    __shared__ float rv[kDpThreads];
    __shared__ uint64_t ri[kDpThreads];
    __shared__ uint64_t walk[kMaxWalk];
    const int tid = static_cast<int>(threadIdx.x);
    const bool leader = tid == 0;
    const uint32_t smask = T.cap_s - 1, bmask = T.cap_best - 1, pmask = T.cap_bp - 1;
    const uint64_t L = T.L, C = L - static_cast<uint64_t>(T.w);

    // (every thread reads the records as the launch before left them; the leader alone writes them, at the end)
    const int32_t status0 = state->status;
    uint64_t next = record->next_checkpoint;
    __shared__ st::State S;  // (the leader's working copies: in LDS, so that no lane pays scratch for them)
    __shared__ tk::Record R;
    if (leader) {
        S = *state;
        R = *record;
        st::release_begin(S, first != 0);
    }
    __syncthreads();

    // the first maximum of best over [lo, hi) (hi - lo <= L), then the leader's back-track and commit
    auto run_checkpoint = [&](uint64_t n, bool lagged, uint64_t lo, uint64_t hi) {
        float bv = -__builtin_inff();
        uint64_t bi = ~0ull;
        for (uint64_t i = lo + static_cast<uint32_t>(tid); i < hi; i += kDpThreads) {
            const float v = ring_best[static_cast<uint32_t>(i) & bmask];
            if (v > bv || bi == ~0ull) {
                bv = v;
                bi = i;
            }
        }
        rv[tid] = bv;
        ri[tid] = bi;
        __syncthreads();
        for (int step = kDpThreads / 2; step > 0; step >>= 1) {
            if (tid < step) {
                const float v2 = rv[tid + step];
                const uint64_t i2 = ri[tid + step];
                if (i2 != ~0ull && (ri[tid] == ~0ull || v2 > rv[tid] || (v2 == rv[tid] && i2 < ri[tid]))) {
                    rv[tid] = v2;
                    ri[tid] = i2;
                }
            }
            __syncthreads();
        }
        if (leader && S.status == 0) {
            const bool ok = tk::checkpoint(
                T, R, n, lagged, ri[0], walk, [&](uint64_t v) { return static_cast<int>(ring_bp[static_cast<uint32_t>(v) & pmask]); },
                [&](uint64_t v) {
                    if (S.status == 0 && v + L <= w1) tk::put_row(S, v, ring_s[static_cast<uint32_t>(v) & smask], positions, scores, rows_cap);
                });
            if (!ok) {
                S.status = 1;
                S.reason = tk::kReasonWalkCap;
            }
        }
        __syncthreads();  // rv / ri are free for the next checkpoint
    };

    if (status0 == 0) {
        uint64_t dp = m0;
        bool cap_hit = false;  // (trips is the same in every thread)
        for (;;) {
            if (trips-- == 0) {
                cap_hit = true;
                break;
            }
            const uint64_t cpn = next * L;
            const uint64_t target = cpn < m1 ? cpn : m1;
            while (dp < target) {  // (dp grows by C >= 1 or reaches the target: at most (target - dp) / C + 1 turns)
                const uint64_t pe = dp + C < target ? dp + C : target;
                for (uint64_t i = dp + static_cast<uint32_t>(tid); i < pe; i += kDpThreads) {
                    float b;
                    int back;
                    tk::dp_position(
                        T, i, ring_s[static_cast<uint32_t>(i) & smask], [&](uint64_t j) { return ring_best[static_cast<uint32_t>(j) & bmask]; },
                        b, back);
                    // (the piece writes [dp, pe) and reads [dp - L - w, pe - L + w], which ends below dp: 2 L positions)
                    ring_best[static_cast<uint32_t>(i) & bmask] = b;
                    ring_bp[static_cast<uint32_t>(i) & pmask] = static_cast<int8_t>(back);
                }
                __syncthreads();
                dp = pe;
            }
            if (cpn > m1) break;
            run_checkpoint(cpn, true, cpn - L, cpn);
            next += 1;
        }
        if (leader && cap_hit && S.status == 0) {
            S.status = 1;
            S.reason = tk::kReasonTripCap;
        }
        if (finish && !cap_hit) {
            if (w1 < L + T.G) {
                if (leader && S.status == 0) {
                    S.status = 1;
                    S.reason = tk::kReasonTooShort;
                }
            } else {
                run_checkpoint(m1, false, m1 > L ? m1 - L : 0, m1);
            }
        }
    }
    if (!leader) return;
    if (status0 == 0) {
        R.next_checkpoint = next;
        R.m = m1;
        S.n_sync = R.n_positions;
        S.scan_pos = m1;
    }
    S.n_in = n_in;
    S.work_len = w1;
    if (finish) S.finished = 1;
    *record = R;
    *state = S;
}

__global__ void __launch_bounds__(256)
k_stream_track_rows(const st::Params P, const st::State *__restrict__ state, const float *__restrict__ ring_f,
                    const uint64_t *__restrict__ positions, float *__restrict__ rows, uint32_t rows_cap)
{
    const uint32_t rel_n = state->rel_n, rel_base = state->rel_base;
    const uint32_t fmask = P.cap_f - 1;
    for (uint32_t j = blockIdx.y; j < rel_n; j += gridDim.y) {
        const uint32_t r = rel_base + j;
        if (r >= rows_cap) return;
        const uint64_t pos = positions[r];
        float *dst = rows + static_cast<uint64_t>(r) * st::kPx;
        for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < static_cast<uint32_t>(st::kPx); c += gridDim.x * blockDim.x)
            dst[c] = ring_f[static_cast<uint32_t>(pos + static_cast<uint64_t>(P.pw) * c) & fmask];
    }
}

template <int PW>
void launch_score(hipStream_t s, const st::Params &P, const tk::Params &T, const StreamBuffers &b, const StreamTrackBuffers &t,
                  uint64_t m0, uint64_t m1, uint64_t w1)
{
    const unsigned grid = static_cast<unsigned>((m1 - m0 + kScoreTile - 1) / kScoreTile);
    hipLaunchKernelGGL(k_stream_track_score<PW>, dim3(grid), dim3(kScoreThreads), 0, s, b.ring_f, P.cap_f - 1, t.ring_s, T.cap_s - 1, b.state,
                       m0, m1, w1);
}

}  // namespace

void stream_track_score(hipStream_t s, const st::Params &P, const tk::Params &T, const StreamBuffers &b, const StreamTrackBuffers &t,
                        uint64_t m0, uint64_t m1, uint64_t w1)
{
    if (m1 <= m0) return;
    switch (T.pw) {
    case 1: launch_score<1>(s, P, T, b, t, m0, m1, w1); break;
    case 2: launch_score<2>(s, P, T, b, t, m0, m1, w1); break;
    case 3: launch_score<3>(s, P, T, b, t, m0, m1, w1); break;
    case 4: launch_score<4>(s, P, T, b, t, m0, m1, w1); break;
    case 5: launch_score<5>(s, P, T, b, t, m0, m1, w1); break;
    case 6: launch_score<6>(s, P, T, b, t, m0, m1, w1); break;
    case 7: launch_score<7>(s, P, T, b, t, m0, m1, w1); break;
    case 8: launch_score<8>(s, P, T, b, t, m0, m1, w1); break;
    default: throw apt::Error{apt::ErrorKind::Internal, "stream: no score kernel for this pixel width"};
    }
}

void stream_track_dp(hipStream_t s, const st::Params &P, const tk::Params &T, const StreamBuffers &b, const StreamTrackBuffers &t,
                     uint64_t *positions, float *scores, uint32_t rows_cap, uint64_t n_in, uint64_t m0, uint64_t m1, uint64_t w1, bool first,
                     bool finish)
{
    if (T.walk_cap > static_cast<uint32_t>(kMaxWalk)) throw apt::Error{apt::ErrorKind::Internal, "stream: back-track bound above the kernel's list"};
    // the checkpoints in (m0, m1], and the turn that finds none left
    const uint64_t trips = (m1 - m0) / T.L + 2;
    hipLaunchKernelGGL(k_stream_track_dp, dim3(1), dim3(kDpThreads), 0, s, T, b.state, t.record, t.ring_s, t.ring_best, t.ring_bp, positions,
                       scores, rows_cap, n_in, m0, m1, w1, static_cast<uint32_t>(trips > 0xFFFFFFFFull ? 0xFFFFFFFFull : trips), first ? 1 : 0,
                       finish ? 1 : 0);
}

void stream_track_rows(hipStream_t s, const st::Params &P, const StreamBuffers &b, const uint64_t *positions, float *rows, uint32_t rows_cap,
                       uint32_t grid_rows)
{
    if (grid_rows == 0 || rows_cap == 0) return;
    if (grid_rows > 1024u) grid_rows = 1024u;
    hipLaunchKernelGGL(k_stream_track_rows, dim3(3, grid_rows), dim3(256), 0, s, P, b.state, b.ring_f, positions, rows, rows_cap);
}

}  // namespace apt::gpu
