// apt_kernels_track_sync.hip — the flywheel sync stage on gfx950 (apt_kernels_track_sync.hpp).
//
//   k_track_score<PW>  s[i] for every position: a tile of x plus a G-sample halo in LDS; a thread computes four
//                      consecutive positions, whose windows overlap in all but three samples, from 16-byte LDS reads
//                      (lane t reads quad t + k: consecutive addresses).  The three chains of a position are
//                      sequential by definition; the twelve chains of a thread are independent.
//   k_track_dp         one workgroup per recording: chunks of C = L - w positions with a barrier between them (every
//                      predecessor lies at least C back), the last 2 L values of `best` as a ring in LDS, one byte of
//                      back-pointer per position in HBM; then the end search, the back-track, the positions' scores
//                      and the record.
//   k_track_rows       row[c] = x[p + pw c], one workgroup per row.
// x is read through f_index: a contiguous signal, or the pixel-phase planes the k_fused instantiations write.
#include "apt_kernels_track_sync.hpp"

#include "apt_plan.hpp"

namespace apt::gpu {

namespace {

using apt::track::kPx;
using apt::track::kStart;

using apt::track::kScorePer;
using apt::track::kScoreThreads;
using apt::track::kScoreTile;
constexpr int kDpThreads = 1024;

// the recording's sample count as the kernels see it: 0 where there is nothing to track (*reason says why)
__device__ __forceinline__ uint64_t samples_of(const TrackRec &r, uint32_t L, uint32_t G, int *reason)
{
    uint64_t n = r.n;
    *reason = 0;
    if (r.res) {
        const int32_t status = r.res->status, why = r.res->reason;
        const uint64_t w = r.res->work_len;
        if (status != 0 && why != 2) {  // (2: "less than 5 sync frames" — the front end ran, F is there)
            *reason = 1;
            return 0;
        }
        n = w < n ? w : n;  // (never past what the buffers were sized for)
    }
    if (n < static_cast<uint64_t>(L) + G) {
        *reason = 2;
        return 0;
    }
    return n;
}

template <int PW>
__global__ void __launch_bounds__(kScoreThreads)
k_track_score(const TrackCall call)
{
    constexpr int G = apt::track::ScoreTile<PW>::G, LEN = apt::track::ScoreTile<PW>::LEN;
    __shared__ __attribute__((aligned(16))) float tile[LEN];

    const TrackRec r = call.rec[blockIdx.y];
    int reason;
    const uint64_t n = samples_of(r, static_cast<uint32_t>(kPx) * PW, G, &reason);
    if (n == 0) return;
    const uint32_t M = static_cast<uint32_t>(n) - G;
    const uint32_t i0 = blockIdx.x * static_cast<uint32_t>(kScoreTile);
    if (i0 >= M) return;
    const int tid = static_cast<int>(threadIdx.x);
    const float *__restrict__ x = r.x;

    if (r.f_stride == 0) {
        for (int e = tid; e < LEN; e += kScoreThreads) {
            const uint64_t i = static_cast<uint64_t>(i0) + static_cast<uint32_t>(e);
            tile[e] = i < n ? x[i] : 0.f;
        }
    } else {
        // planes: sample i lies at plane i % PW, index i / PW — a plane at a time, lanes on consecutive addresses
        const uint32_t a0 = i0 / PW;
        constexpr int PER = (LEN + PW - 1) / PW + 1;
        for (int idx = tid; idx < PW * PER; idx += kScoreThreads) {
            const uint32_t ph = static_cast<uint32_t>(idx / PER), k = static_cast<uint32_t>(idx % PER);
            const uint64_t i = static_cast<uint64_t>(a0 + k) * PW + ph;
            if (i >= i0 && i < static_cast<uint64_t>(i0) + LEN)
                tile[i - i0] = i < n ? x[static_cast<uint64_t>(ph) * r.f_stride + a0 + k] : 0.f;
        }
    }
    __syncthreads();

    float out[kScorePer];
    apt::track::score_four<PW>(tile, tid, out);  // (the zone loop: apt_kernels_track_sync.hpp)
    // through the tile, so that lanes store consecutive addresses
    __syncthreads();
#pragma unroll
    for (int p = 0; p < kScorePer; ++p) tile[kScorePer * tid + p] = out[p];
    __syncthreads();
    for (int e = tid; e < kScoreTile; e += kScoreThreads) {
        const uint32_t i = i0 + static_cast<uint32_t>(e);
        if (i < M) r.score[i] = tile[e];
    }
}

__global__ void __launch_bounds__(kDpThreads)
k_track_dp(const TrackCall call, uint32_t pw, int w, float lam)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const TrackRec r = call.rec[blockIdx.x];
    const int32_t L = static_cast<int32_t>(kPx * pw), G = static_cast<int32_t>(38u * pw);
    const int32_t R = 2 * L, C = L - w;
    float *ring = lds;                                              // [R] best[j] at j % R
    float *rv = lds + R;                                            // [kDpThreads] the end search
    int32_t *ri = reinterpret_cast<int32_t *>(rv + kDpThreads);     // [kDpThreads]
    int32_t *bc = ri + kDpThreads;                                  // [2] broadcast
    const int tid = static_cast<int>(threadIdx.x);

    int reason;
    const uint64_t n = samples_of(r, static_cast<uint32_t>(L), static_cast<uint32_t>(G), &reason);
    if (n == 0) {
        if (tid == 0) {
            TrackResult rec{};
            rec.struct_size = sizeof(TrackResult);
            rec.status = APTGPU_ERR_INTERNAL;
            rec.reason = reason;
            rec.n = r.res ? r.res->work_len : r.n;
            *r.rec = rec;
        }
        return;
    }
    const int32_t M = static_cast<int32_t>(n) - G;
    const float *__restrict__ score = r.score;
    int8_t *__restrict__ bp = r.bp;

    for (int32_t c0 = 0; c0 < M; c0 += C) {
        const int32_t c0r = c0 % R;
        const int32_t cend = c0 + C < M ? c0 + C : M;
        for (int32_t i = c0 + tid; i < cend; i += kDpThreads) {
            const float sv = score[i];
            int32_t ir = c0r + (i - c0);
            if (ir >= R) ir -= R;
            int32_t jr = ir - L;  // (i - L) % R
            if (jr < 0) jr += R;
            float cur;
            int b;
            apt::track::best_predecessor(
                i, L, w, lam,
                [&](int d) {
                    int32_t q = jr - d;
                    q = q < 0 ? q + R : (q >= R ? q - R : q);
                    return ring[q];
                },
                cur, b);
            // (the chunk writes slots [c0, c0 + C) and reads [c0 - L - w, c0): 2 L positions in all, distinct mod R)
            ring[ir] = __fadd_rn(sv, cur);
            bp[i] = static_cast<int8_t>(b);
        }
        __syncthreads();
    }

    // the first maximum of best over the last row of positions
    const int32_t lo = M - L > 0 ? M - L : 0;
    const int32_t lor = lo % R;
    float bv = -__builtin_inff();
    int32_t bi = 0x7FFFFFFF;
    for (int32_t i = lo + tid; i < M; i += kDpThreads) {
        int32_t q = lor + (i - lo);
        if (q >= R) q -= R;
        const float v = ring[q];
        if (v > bv) {
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
            const int32_t i2 = ri[tid + step];
            if (v2 > rv[tid] || (v2 == rv[tid] && i2 < ri[tid])) {
                rv[tid] = v2;
                ri[tid] = i2;
            }
        }
        __syncthreads();
    }

    // the back-track: one thread follows the bytes, the others then turn the list round
    if (tid == 0) {
        const int32_t end = ri[0];
        uint32_t k = 0, fit = 0;
        bool overflow = false;
        for (int32_t p = end;;) {
            if (k >= r.pos_cap) {
                overflow = true;
                break;
            }
            r.tmp[k++] = static_cast<uint32_t>(p);
            if (static_cast<uint64_t>(p) + static_cast<uint32_t>(L) <= n) fit += 1;
            const int d = bp[p];
            if (d == kStart) break;
            p = p - L - d;
        }
        TrackResult rec{};
        rec.struct_size = sizeof(TrackResult);
        rec.n = n;
        rec.end = static_cast<uint32_t>(end);
        rec.total = rv[0];
        if (overflow) {
            rec.status = APTGPU_ERR_INTERNAL;
            rec.reason = 3;
            k = 0;
        } else {
            rec.n_positions = k;
            rec.n_rows = fit;
            if (r.rows && fit > r.rows_cap) {
                rec.n_rows = r.rows_cap;
                rec.reason = 4;
            }
        }
        *r.rec = rec;
        bc[0] = static_cast<int32_t>(k);
    }
    __syncthreads();
    const uint32_t K = static_cast<uint32_t>(bc[0]);
    for (uint32_t k = static_cast<uint32_t>(tid); k < K; k += kDpThreads) {
        const uint32_t p = r.tmp[K - 1u - k];
        r.pos[k] = p;
        r.pscore[k] = score[p];
    }
}

__global__ void __launch_bounds__(256)
k_track_rows(const TrackCall call, uint32_t pw)
{
    const TrackRec r = call.rec[blockIdx.y];
    if (!r.rows) return;
    const uint32_t n_rows = r.rec->n_rows;  // (never more than rows_cap, nor than pos_cap)
    for (uint32_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const uint32_t p = r.pos[row];
        float *__restrict__ dst = r.rows + static_cast<uint64_t>(row) * kPx;
        if (r.f_stride) {
            const float *__restrict__ src = r.x + static_cast<uint64_t>(p % pw) * r.f_stride + p / pw;
            for (uint32_t c = threadIdx.x; c < static_cast<uint32_t>(kPx); c += blockDim.x) dst[c] = src[c];
        } else {
            const float *__restrict__ src = r.x + p;
            for (uint32_t c = threadIdx.x; c < static_cast<uint32_t>(kPx); c += blockDim.x)
                dst[c] = src[static_cast<uint64_t>(c) * pw];
        }
    }
}

template <int PW>
void launch_score(hipStream_t s, const TrackCall &call, uint64_t max_n)
{
    const uint64_t m = max_n - 38u * PW;
    const unsigned gx = static_cast<unsigned>((m + kScoreTile - 1) / kScoreTile);
    hipLaunchKernelGGL(k_track_score<PW>, dim3(gx ? gx : 1, call.count), dim3(kScoreThreads), 0, s, call);
}

}  // namespace

void track_score(hipStream_t s, const TrackCall &call, uint32_t pw, uint64_t max_n)
{
    if (call.count == 0 || max_n < 2118ull * pw) return;
    switch (pw) {
    case 1: launch_score<1>(s, call, max_n); break;
    case 2: launch_score<2>(s, call, max_n); break;
    case 3: launch_score<3>(s, call, max_n); break;
    case 4: launch_score<4>(s, call, max_n); break;
    case 5: launch_score<5>(s, call, max_n); break;
    case 6: launch_score<6>(s, call, max_n); break;
    case 7: launch_score<7>(s, call, max_n); break;
    case 8: launch_score<8>(s, call, max_n); break;
    default: throw apt::Error{apt::ErrorKind::Internal, "track: no score kernel for this pixel width"};
    }
}

void track_dp(hipStream_t s, const TrackCall &call, uint32_t pw, int w, float lam)
{
    if (call.count == 0) return;
    if (pw < 1 || pw > static_cast<uint32_t>(apt::track::kMaxPw))
        throw apt::Error{apt::ErrorKind::Internal, "track: no ring for this pixel width"};
    // the ring of 2 L floats, the end search's two arrays and the broadcast words: 58 KB at pw = 3, 141 KB at pw = 8
    const size_t lds = (static_cast<size_t>(2u * kPx) * pw + 2u * kDpThreads + 4u) * sizeof(float);
    if (lds > 64u * 1024u)
        apt::hip_check(hipFuncSetAttribute(reinterpret_cast<const void *>(k_track_dp),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)),
                       "hipFuncSetAttribute (k_track_dp LDS)");
    hipLaunchKernelGGL(k_track_dp, dim3(call.count), dim3(kDpThreads), lds, s, call, pw, w, lam);
}

void track_rows(hipStream_t s, const TrackCall &call, uint32_t pw, uint32_t max_rows)
{
    if (call.count == 0 || max_rows == 0) return;
    hipLaunchKernelGGL(k_track_rows, dim3(max_rows, call.count), dim3(256), 0, s, call, pw);
}

}  // namespace apt::gpu
