// apt_kernels_afc.hip — k_afc_sums and k_afc_table: stages A and B of the AFC in front of the FM demodulator
// (apt_kernels_afc.hpp has the arithmetic, include/aptgpu.h §4b' the definition, DESIGN.md §27 the layout).  Built
// without contraction: stage B's f64 expressions are rounded product by product.
//
// k_afc_sums  grid (blocks of the longest recording, recordings), 256 threads: one workgroup per block of B frames.  The
//   block is walked in chunks of 2048 frames.  A thread fetches the chunk's run of 8 at tid * 8 (16-byte loads where
//   the recording is 16-byte aligned, as k_fm's load), threads 0 ... 7 the 64 frames behind the chunk that the lag
//   reaches; the integer (F32: float) components go to LDS as 8-byte pairs at j + j / 32, which keeps the eight stores
//   of a thread on distinct banks.  Then thread t sums frames t, t + 256, ... of the chunk with their partners L
//   further on: consecutive lanes read consecutive pairs.  Every product pair is widened to 64 bits before it is
//   added.  (Forming the pairs of 8-bit components in int32 was tried: 6.68 ms against 6.34 and 6.38 ms for the u8
//   shape of profiles/r27_afc.txt, no gain; the kernel's time goes with its workgroup count)  Waves
//   reduce by shuffles, the workgroup through LDS, and thread 0 stores the three sums as doubles.  No atomics.
// k_afc_table one workgroup of 1024 threads per recording: the window sums and the estimate of every block
//   (estimate_block), the first good block (a min reduction), then in chunks of 1024 blocks the hold (an inclusive
//   max-scan of the good indices, carried from chunk to chunk) and phase0 (a uint32 sum-scan of B * pw).
#include "apt_kernels_afc.hpp"

#include "apt_kernels_fm_body.hpp"

namespace apt::gpu {

namespace {

using apt::afc::Design;
using apt::afc::Record;
using apt::afc::Sums;
using apt::fm::kRun;

constexpr uint32_t kSumThreads = 256, kChunk = kSumThreads * kRun, kWave = 64;
constexpr uint32_t kTableThreads = 1024;

__device__ __forceinline__ uint32_t pair_index(uint32_t j) { return j + (j >> 5); }

template <class T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        if constexpr (std::is_same_v<T, double>)
            v += __shfl_down(v, o, kWave);
        else
            v += static_cast<T>(__shfl_down(static_cast<long long>(v), o, kWave));
    }
    return v;
}

template <int FMT>
__global__ __launch_bounds__(kSumThreads) void k_afc_sums(const AfcBatch batch, const Design d, const uint32_t swap)
{
    using T = typename Sums<FMT>::T;
    using Pair = std::conditional_t<FMT == APTGPU_IQ_F32, float2, int2>;
    constexpr uint32_t kPairs = kChunk + apt::afc::kMaxLag;
    __shared__ Pair pairs[kPairs + (kPairs >> 5) + 1];
    __shared__ T part[3][kSumThreads / kWave];

    const AfcRecording rec = batch.r[blockIdx.y];
    const uint64_t n = rec.n_frames;
    const uint64_t lo = static_cast<uint64_t>(blockIdx.x) << d.log2_B;
    if (lo >= n) return;  // past this recording's blocks (uniform over the workgroup)
    const uint64_t hi = lo + d.B < n ? lo + d.B : n;
    const uint32_t tid = threadIdx.x, L = d.L;
    const fm_body::OneSegment src(rec.iq, n);

    auto stage_run = [&](uint64_t i0, uint32_t j0) {  // the run of 8 at absolute frame i0 -> pairs j0 ...
        uint32_t raw[2 * kRun];
        src.template load_run<FMT>(i0, raw);  // zeros behind the recording: never summed
#pragma unroll
        for (int k = 0; k < kRun; ++k) {
            const uint32_t a = raw[2 * k + (swap ? 1 : 0)], b = raw[2 * k + (swap ? 0 : 1)];
            Pair p;
            if constexpr (FMT == APTGPU_IQ_F32) {
                p = make_float2(__uint_as_float(a), __uint_as_float(b));
            } else {
                p = make_int2(apt::afc::int_component<FMT>(a), apt::afc::int_component<FMT>(b));
            }
            pairs[pair_index(j0 + static_cast<uint32_t>(k))] = p;
        }
    };

    Sums<FMT> s;
    for (uint64_t c0 = lo; c0 < hi; c0 += kChunk) {  // (c0 is a multiple of 8: B is)
        const uint64_t reach = hi + L;               // frames behind this are not read
        if (c0 + tid * kRun < reach) stage_run(c0 + tid * kRun, tid * kRun);
        if (tid < apt::afc::kMaxLag / kRun && c0 + kChunk + tid * kRun < reach)
            stage_run(c0 + kChunk + tid * kRun, kChunk + tid * kRun);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kRun; ++k) {
            const uint32_t j = tid + static_cast<uint32_t>(k) * kSumThreads;
            const uint64_t i = c0 + j;
            if (i < hi) {
                const Pair x0 = pairs[pair_index(j)];
                s.energy(static_cast<T>(x0.x), static_cast<T>(x0.y));
                if (i + L < n) {
                    const Pair x1 = pairs[pair_index(j + L)];
                    s.lagged(static_cast<T>(x0.x), static_cast<T>(x0.y), static_cast<T>(x1.x), static_cast<T>(x1.y));
                }
            }
        }
        __syncthreads();
    }

    const T re = wave_sum(s.re), im = wave_sum(s.im), en = wave_sum(s.en);
    if ((tid & (kWave - 1)) == 0) {
        part[0][tid / kWave] = re;
        part[1][tid / kWave] = im;
        part[2][tid / kWave] = en;
    }
    __syncthreads();
    if (tid == 0) {
        T sum[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            sum[q] = part[q][0];
#pragma unroll
            for (uint32_t w = 1; w < kSumThreads / kWave; ++w) sum[q] += part[q][w];
        }
        double *out = rec.sums + 3ull * blockIdx.x;
        out[0] = static_cast<double>(sum[0]);
        out[1] = static_cast<double>(sum[1]);
        out[2] = static_cast<double>(sum[2]);
    }
}

// inclusive scan of one value per thread over the workgroup (Hillis-Steele in two LDS rows); *total: the last one
template <class Op>
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t *buf, Op op, uint32_t *total)
{
    const uint32_t tid = threadIdx.x;
    uint32_t src = 0;
    buf[tid] = v;
    __syncthreads();
    for (uint32_t o = 1; o < kTableThreads; o <<= 1) {
        uint32_t x = buf[src * kTableThreads + tid];
        if (tid >= o) x = op(buf[src * kTableThreads + tid - o], x);
        src ^= 1u;
        buf[src * kTableThreads + tid] = x;
        __syncthreads();
    }
    const uint32_t r = buf[src * kTableThreads + tid];
    *total = buf[src * kTableThreads + kTableThreads - 1];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(kTableThreads) void k_afc_table(const AfcBatch batch, const Design d)
{
    __shared__ uint32_t buf[2 * kTableThreads];
    const AfcRecording rec = batch.r[blockIdx.x];
    const uint32_t nb = static_cast<uint32_t>(apt::afc::blocks_of(rec.n_frames, d.log2_B));  // <= 2^20
    if (nb == 0) return;
    const uint32_t tid = threadIdx.x;
    constexpr uint32_t kNone = 0xFFFFFFFFu;

    // the estimates (est in the record's pw for now) and the first good block
    uint32_t first = kNone;
    for (uint32_t b = tid; b < nb; b += kTableThreads) {
        const apt::afc::Estimate e = apt::afc::estimate_block(rec.sums, nb, b, d);
        rec.table[b].pw = e.est;
        rec.coherence[b] = apt::afc::coherence_out(e.coherence);
        rec.good[b] = e.good ? 1 : 0;
        if (e.good && first == kNone) first = b;
    }
    buf[tid] = first;
    __syncthreads();  // (also makes this workgroup's stores to the table visible to its threads)
    for (uint32_t o = kTableThreads / 2; o > 0; o >>= 1) {
        if (tid < o) buf[tid] = buf[tid] < buf[tid + o] ? buf[tid] : buf[tid + o];
        __syncthreads();
    }
    first = buf[0];
    __syncthreads();
    const uint32_t fallback = first != kNone ? rec.table[first].pw : d.pw_base;  // a good block's pw stays its estimate

    uint32_t held = 0, phase_carry = 0;  // held: 1 + the last good block of the chunks before this one, 0 = none
    for (uint32_t base = 0; base < nb; base += kTableThreads) {
        const uint32_t b = base + tid;
        const bool in = b < nb;
        uint32_t total;
        uint32_t j = block_scan(in && rec.good[b] ? b + 1u : 0u, buf, [](uint32_t x, uint32_t y) { return x > y ? x : y; },
                                &total);
        j = j > held ? j : held;
        held = total > held ? total : held;
        const uint32_t pw = !in ? 0u : j ? rec.table[j - 1u].pw : fallback;
        const uint32_t inc = d.B * pw;
        const uint32_t sum = block_scan(inc, buf, [](uint32_t x, uint32_t y) { return x + y; }, &total);
        // (every read of a pw above is behind block_scan's barriers, in front of the stores below)
        if (in) rec.table[b] = apt::afc::record_of(pw, phase_carry + sum - inc);
        phase_carry += total;
    }
}

using SumsKernel = void (*)(const AfcBatch, const Design, const uint32_t);
SumsKernel sums_kernel_of(int format)
{
    switch (format) {
    case APTGPU_IQ_U8: return k_afc_sums<APTGPU_IQ_U8>;
    case APTGPU_IQ_S8: return k_afc_sums<APTGPU_IQ_S8>;
    case APTGPU_IQ_S16: return k_afc_sums<APTGPU_IQ_S16>;
    default: return k_afc_sums<APTGPU_IQ_F32>;
    }
}

}  // namespace

void afc_sums(hipStream_t stream, int format, bool swap, const Design &d, const AfcBatch &batch, int count,
              uint32_t max_blocks)
{
    if (count <= 0 || max_blocks == 0) return;
    hipLaunchKernelGGL(sums_kernel_of(format), dim3(max_blocks, static_cast<uint32_t>(count)), dim3(kSumThreads), 0, stream,
                       batch, d, swap ? 1u : 0u);
}

void afc_table(hipStream_t stream, const Design &d, const AfcBatch &batch, int count)
{
    if (count <= 0) return;
    hipLaunchKernelGGL(k_afc_table, dim3(static_cast<uint32_t>(count)), dim3(kTableThreads), 0, stream, batch, d);
}

}  // namespace apt::gpu
