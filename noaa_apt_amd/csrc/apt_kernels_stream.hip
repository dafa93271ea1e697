// apt_kernels_stream.hip — the gfx950 kernels of live decode (include/aptgpu.h §4d).  Per push:
//   k_stream_front  the newly final work samples [w0, w1) in tiles of 256: input window from the ring into LDS, R over
//                   the tile and the T2 samples before it (recomputed, not carried), D, F -> the F ring
//   k_stream_corr   the strict correlation of the newly scannable positions -> the corr ring (as many workgroups as
//                   the positions need)
//   k_stream_sync   one workgroup: the picker as window-maximum jumps over the corr ring (picker_run of
//                   apt_kernels_stream.hpp), then the rows that became final
//   k_stream_rows   gathers those rows from the F ring
// Order comes from the stream alone: no workgroup waits for another, nothing is read back between the kernels.
// Every ring index is `absolute index & (capacity - 1)`, so no access leaves its buffer whatever the state holds.
#include "apt_kernels_stream.hpp"

#include "apt_envelope.hpp"
#include "apt_sync_corr.hpp"

#pragma clang fp contract(off)

namespace apt::gpu {

namespace st = apt::stream;

namespace {

constexpr int kSyncThreads = 1024;

__device__ __forceinline__ float ring_in_at(const void *__restrict__ ring, bool s16, uint64_t i, uint32_t mask)
{
    const uint32_t q = static_cast<uint32_t>(i) & mask;
    return s16 ? static_cast<float>(static_cast<const int16_t *>(ring)[q]) : static_cast<const float *>(ring)[q];
}

// LDS: win[win_cap] | R[kTile + t2 + 1] | D[kTile + t2 + 1]
__global__ void __launch_bounds__(st::kTile)
k_stream_front(const st::Params P, const void *__restrict__ ring_in, const float *__restrict__ table,
               const float *__restrict__ h2, float *__restrict__ ring_f, st::State *__restrict__ state, uint64_t w0,
               uint64_t w1, uint64_t n_avail)
{
    extern __shared__ float lds[];
    float *win = lds;
    float *R = lds + P.win_cap;
    float *D = R + (st::kTile + P.t2 + 1);

    const uint64_t k0 = w0 + static_cast<uint64_t>(blockIdx.x) * st::kTile;
    if (k0 >= w1) return;
    const uint64_t k1 = k0 + st::kTile < w1 ? k0 + st::kTile : w1;
    const uint64_t ka = k0 > P.t2 ? k0 - P.t2 : 0;
    const uint32_t n_r = static_cast<uint32_t>(k1 - ka);  // <= kTile + t2

    uint64_t lo, hi;
    st::input_window(P, ka, k1, n_avail, lo, hi);
    if (hi - lo > P.win_cap) {  // (the host sized win_cap as the bound of this difference)
        if (threadIdx.x == 0) {
            state->status = 1;
            state->reason = st::kReasonWindow;
        }
        return;
    }
    const uint32_t n_win = static_cast<uint32_t>(hi - lo);
    // the window, converted to f32 on the way in (s16 as the PCM16 front ends do)
    for (uint32_t i = threadIdx.x; i < n_win; i += st::kTile) win[i] = ring_in_at(ring_in, P.s16 != 0, lo + i, P.cap_in - 1);
    __syncthreads();

    for (uint32_t r = threadIdx.x; r < n_r; r += st::kTile) {
        R[r] = st::resample_at(
            P, ka + r, hi, [&](uint64_t i) { return win[static_cast<uint32_t>(i - lo)]; },
            [&](uint32_t ph, uint32_t i) { return table[static_cast<size_t>(ph) * P.tpp + i]; });
    }
    __syncthreads();
    for (uint32_t r = threadIdx.x; r < n_r; r += st::kTile) {
        // D[0] = 0; D[ka] of a later tile is never read (F[i] reads D[i - T2 + 1 .. i])
        float d = 0.f;
        if (r > 0) d = envelope_general(envelope_radicand(R[r - 1], R[r], P.cosphi2), P.sinphi);
        D[r] = d;
    }
    __syncthreads();
    const uint64_t i = k0 + threadIdx.x;
    if (i < k1) {
        const float f = st::lowpass_at(
            i, P.t2, [&](uint64_t q) { return D[static_cast<uint32_t>(q - ka)]; }, [&](uint32_t j) { return h2[j]; });
        ring_f[static_cast<uint32_t>(i) & (P.cap_f - 1)] = f;
    }
}

// corr[i] for i in [c0, c1): the reference's chain over the F ring
__global__ void __launch_bounds__(256)
k_stream_corr(const st::Params P, const float *__restrict__ ring_f, float *__restrict__ ring_c, uint64_t c0, uint64_t c1)
{
    const uint64_t i = c0 + static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (i >= c1) return;
    const uint32_t fmask = P.cap_f - 1;
    ring_c[static_cast<uint32_t>(i) & (P.cap_c - 1)] =
        sync_corr_strict_rolled(P.pw, [&](uint32_t j) { return ring_f[static_cast<uint32_t>(i + j) & fmask]; });
}

// the workgroup's maximum of corr[a .. e]: NaNs ignored, the lowest index among equals; the same value in every thread
__device__ st::Best block_best(const float *__restrict__ ring_c, uint32_t mask, uint64_t a, uint64_t e, st::Best *red)
{
    st::Best b{st::kNone, 0.f};
    for (uint64_t i = a + threadIdx.x; i <= e; i += kSyncThreads) {
        const float v = ring_c[static_cast<uint32_t>(i) & mask];
        if (!st::is_nan(v)) b = st::best_of(b, st::Best{i, v});
    }
    for (int d = 32; d >= 1; d >>= 1) {
        st::Best o;
        o.idx = __shfl_down(b.idx, d, 64);
        o.val = __shfl_down(b.val, d, 64);
        b = st::best_of(b, o);
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = b;
    __syncthreads();
    st::Best all{st::kNone, 0.f};
    for (int w = 0; w < kSyncThreads / 64; ++w) all = st::best_of(all, red[w]);
    __syncthreads();  // red is free for the next reduction
    return all;
}

__global__ void __launch_bounds__(kSyncThreads)
k_stream_sync(const st::Params P, st::State *__restrict__ state, const float *__restrict__ ring_c,
              uint64_t *__restrict__ positions, uint32_t rows_cap, uint64_t n_in, uint64_t w1, int first, int finish)
{
    __shared__ st::Best red[kSyncThreads / 64];
    const bool leader = threadIdx.x == 0;
    // (the state as the kernel before left it: every thread reads the same record)
    st::Pick pk = st::pick_load(*state);
    const uint64_t corr_done = state->corr_done;
    __syncthreads();  // nobody still reads the record when the leader writes it
    if (leader) st::release_begin(*state, first != 0);
    bool ok = true;
    uint64_t s_end = corr_done;
    if (P.sync && pk.status == 0) {
        s_end = w1 > P.g ? w1 - P.g : 0;
        if (s_end < corr_done) s_end = corr_done;
        const uint32_t cmask = P.cap_c - 1;  // (k_stream_corr filled [corr_done, s_end) before this launch)
        ok = st::picker_run(
            P, pk, s_end, [&](uint64_t a, uint64_t e) { return block_best(ring_c, cmask, a, e, red); },
            [&](uint64_t i) { return ring_c[static_cast<uint32_t>(i) & cmask]; },
            [&](uint64_t p_old, uint64_t istar, uint64_t copies) {
                if (leader) st::pend_event(P, *state, p_old, istar, copies, w1, finish != 0, positions, rows_cap);
            });
    }
    if (!leader) return;
    if (!ok) {
        pk.status = 1;
        pk.reason = st::kReasonTripCap;
    }
    st::pick_store(pk, *state);
    state->corr_done = s_end;
    state->n_in = n_in;
    state->work_len = w1;
    st::release_rows(P, *state, finish != 0, positions, rows_cap);
}

// grid.y workgroup rows walk the rows the record counts for this launch (however many: one event of the picker can
// release any number of copies); grid.x * 256 threads cover a row's 2080 pixels
__global__ void __launch_bounds__(256)
k_stream_rows(const st::Params P, const st::State *__restrict__ state, const float *__restrict__ ring_f,
              const uint64_t *__restrict__ positions, float *__restrict__ rows, uint32_t rows_cap)
{
    const uint32_t rel_n = state->rel_n, rel_base = state->rel_base;
    const uint64_t rel_first = state->rel_first;
    const uint32_t fmask = P.cap_f - 1;
    for (uint32_t j = blockIdx.y; j < rel_n; j += gridDim.y) {
        const uint32_t r = rel_base + j;
        if (r >= rows_cap) return;
        const uint64_t pos = positions[r];
        const bool first_row = rel_first + j == 0;
        float *dst = rows + static_cast<uint64_t>(r) * st::kPx;
        for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < static_cast<uint32_t>(st::kPx); c += gridDim.x * blockDim.x) {
            const float f = ring_f[static_cast<uint32_t>(pos + static_cast<uint64_t>(P.pw) * c) & fmask];
            dst[c] = st::row_pixel(f, first_row && c == 0);
        }
    }
}

}  // namespace

size_t stream_front_lds_bytes(const st::Params &P)
{
    return (static_cast<size_t>(P.win_cap) + 2u * (st::kTile + P.t2 + 1)) * sizeof(float);
}

void stream_front(hipStream_t s, const st::Params &P, const StreamBuffers &b, uint64_t w0, uint64_t w1, uint64_t n_avail)
{
    if (w1 <= w0) return;
    const unsigned grid = static_cast<unsigned>((w1 - w0 + st::kTile - 1) / st::kTile);
    hipLaunchKernelGGL(k_stream_front, dim3(grid), dim3(st::kTile), stream_front_lds_bytes(P), s, P, b.ring_in, b.table, b.h2,
                       b.ring_f, b.state, w0, w1, n_avail);
}

void stream_corr(hipStream_t s, const st::Params &P, const StreamBuffers &b, uint64_t w0, uint64_t w1)
{
    if (!P.sync) return;
    const uint64_t c0 = w0 > P.g ? w0 - P.g : 0, c1 = w1 > P.g ? w1 - P.g : 0;
    if (c1 <= c0) return;
    hipLaunchKernelGGL(k_stream_corr, dim3(static_cast<unsigned>((c1 - c0 + 255) / 256)), dim3(256), 0, s, P, b.ring_f, b.ring_c, c0, c1);
}

void stream_sync(hipStream_t s, const st::Params &P, const StreamBuffers &b, uint64_t *positions, uint32_t rows_cap,
                 uint64_t n_in, uint64_t w1, bool first, bool finish)
{
    hipLaunchKernelGGL(k_stream_sync, dim3(1), dim3(kSyncThreads), 0, s, P, b.state, b.ring_c, positions, rows_cap, n_in, w1,
                       first ? 1 : 0, finish ? 1 : 0);
}

void stream_rows(hipStream_t s, const st::Params &P, const StreamBuffers &b, const uint64_t *positions, float *rows,
                 uint32_t rows_cap, uint32_t grid_rows)
{
    if (grid_rows == 0 || rows_cap == 0) return;
    if (grid_rows > 1024u) grid_rows = 1024u;
    hipLaunchKernelGGL(k_stream_rows, dim3(3, grid_rows), dim3(256), 0, s, P, b.state, b.ring_f, positions, rows, rows_cap);
}

}  // namespace apt::gpu
