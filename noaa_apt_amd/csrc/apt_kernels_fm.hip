// apt_kernels_fm.hip — k_fm: convert, mix, filter, decimate and discriminate an IQ recording in one kernel
// (apt_kernels_fm.hpp has the arithmetic, DESIGN.md §20 the layout and its bank arithmetic).
//
// A workgroup of up to 256 threads owns nv consecutive v[m] of one recording (nv - 1 outputs; neighbouring tiles share one
// v, which both compute in the same order) and the frames [m0 D, m0 D + (nv - 1) D + T) under them.
//  load   A thread takes runs of 8 frames that start at multiples of 8 of the absolute frame index: one, two or four
//         16-byte loads where the recording's pointer is 16-byte aligned and the run lies inside the recording, else
//         component loads of the same bits.  The run is converted, mixed (first phasor from the integer phase, seven
//         complex multiplies) and stored once: frame s + l goes to row l % D, column l / D of the tile (float2).
//  filter Thread c sums hr[j] * tile[j % D][c + j / D] for j = 0 .. T - 1: for a tap, consecutive lanes read
//         consecutive float2, for any D.  The tap and its place in the tile (a table made with the plan) are
//         wave-uniform and fetched eight at a time, so eight LDS reads are in flight per column.  VPT columns one
//         workgroup apart per thread share them.
//  disc   v goes to the front of the tile; thread c writes a[m0 + c] from v[c] and v[c + 1].
#include "apt_kernels_fm.hpp"

#include "apt_plan.hpp"

namespace apt::gpu {

namespace {

using apt::fm::Cx;
using apt::fm::kRun;

// the 8 frames of the run at i0 (a multiple of 8) as raw component bits: I of frame k in raw[2 k], Q in raw[2 k + 1]
template <int FMT>
__device__ __forceinline__ void load_run(const uint8_t *__restrict__ iq, uint64_t i0, uint64_t n_frames, bool aligned16,
                                         uint32_t (&raw)[2 * kRun])
{
    constexpr uint32_t cb = FMT == APTGPU_IQ_S16 ? 2u : FMT == APTGPU_IQ_F32 ? 4u : 1u;
    const uint8_t *p = iq + i0 * (2u * cb);
    if (aligned16 && i0 + kRun <= n_frames) {
        constexpr int kWide = static_cast<int>(2u * cb * kRun / 16u);  // 1, 2 or 4 loads of 16 bytes
        uint32_t w[4 * kWide];
#pragma unroll
        for (int k = 0; k < kWide; ++k) {
            const uint4 q = reinterpret_cast<const uint4 *>(p)[k];
            w[4 * k] = q.x;
            w[4 * k + 1] = q.y;
            w[4 * k + 2] = q.z;
            w[4 * k + 3] = q.w;
        }
#pragma unroll
        for (int k = 0; k < 2 * kRun; ++k) {
            if constexpr (cb == 1u)
                raw[k] = (w[k / 4] >> (8 * (k % 4))) & 0xFFu;
            else if constexpr (cb == 2u)
                raw[k] = (w[k / 2] >> (16 * (k % 2))) & 0xFFFFu;
            else
                raw[k] = w[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < 2 * kRun; ++k) {
            uint32_t v = 0;
            if (i0 + static_cast<uint64_t>(k / 2) < n_frames) {
                if constexpr (cb == 1u)
                    v = p[k];
                else if constexpr (cb == 2u)
                    v = reinterpret_cast<const uint16_t *>(p)[k];
                else
                    v = reinterpret_cast<const uint32_t *>(p)[k];
            }
            raw[k] = v;
        }
    }
}

template <int FMT, bool MIX, int VPT>
__global__ __launch_bounds__(256) void k_fm(const FmBatch batch, const FmParams P)
{
    extern __shared__ float2 tile[];
    const FmRecording rec = batch.r[blockIdx.y];
    const uint32_t T = P.T, D = P.D, R = P.R;
    const uint64_t n_frames = rec.n_frames;
    if (n_frames < T) return;
    const uint64_t n_v = (n_frames - T) / D + 1;  // M
    const uint64_t m0 = static_cast<uint64_t>(blockIdx.x) * (P.nv - 1);
    if (m0 + 1 >= n_v) return;  // no output left (uniform over the workgroup)
    const uint32_t nv = static_cast<uint32_t>(n_v - m0 < P.nv ? n_v - m0 : P.nv);  // >= 2
    const uint64_t s = m0 * D;                                                     // the tile's first frame
    const uint32_t frames = (nv - 1) * D + T;                                      // s + frames <= n_frames
    const uint32_t tid = threadIdx.x, threads = blockDim.x;

    // ---- load: runs of 8 by absolute index
    {
        const uint64_t g0 = s / kRun;
        const uint32_t runs = static_cast<uint32_t>((s + frames - 1) / kRun - g0) + 1;
        const bool aligned16 = (reinterpret_cast<uintptr_t>(rec.iq) & 15u) == 0;
        const bool swap = P.swap != 0;
        for (uint32_t g = tid; g < runs; g += threads) {
            const uint64_t i0 = (g0 + g) * kRun;
            uint32_t raw[2 * kRun];
            load_run<FMT>(rec.iq, i0, n_frames, aligned16, raw);
            Cx ph{1.f, 0.f};
            if constexpr (MIX) ph = apt::fm::phasor_of_phase(static_cast<uint32_t>(i0) * P.pw);
            // local index of the run's first frame (negative: frames in front of the tile, dropped)
            const int64_t l0 = static_cast<int64_t>(i0) - static_cast<int64_t>(s);
            uint32_t row = 0, col = 0;
            if (l0 > 0) {
                col = static_cast<uint32_t>(l0) / D;
                row = static_cast<uint32_t>(l0) - col * D;
            }
#pragma unroll
            for (int k = 0; k < kRun; ++k) {
                const float ci = apt::fm::component<FMT>(raw[2 * k]), cq = apt::fm::component<FMT>(raw[2 * k + 1]);
                Cx x{swap ? cq : ci, swap ? ci : cq};
                if constexpr (MIX) {
                    x = apt::fm::cmul(x, ph);
                    ph = apt::fm::cmul(ph, Cx{P.step_re, P.step_im});
                }
                const int64_t l = l0 + k;
                if (l >= 0 && l < static_cast<int64_t>(frames)) {
                    tile[apt::fm::tile_index(row, col, R)] = make_float2(x.re, x.im);
                    if (++row == D) {
                        row = 0;
                        ++col;
                    }
                }
            }
        }
    }
    __syncthreads();

    // ---- filter: thread c, columns c + r * blockDim.x
    uint32_t c[VPT];
    float re[VPT], im[VPT];
#pragma unroll
    for (int r = 0; r < VPT; ++r) {
        const uint32_t cc = tid + static_cast<uint32_t>(r) * threads;
        c[r] = cc < nv ? cc : nv - 1;  // (lanes past the tile's v repeat its last one; their sums are dropped)
        re[r] = 0.f;
        im[r] = 0.f;
    }
    {
        const float *__restrict__ hr = P.taps_rev;
        const uint32_t *__restrict__ off = P.offsets;
        auto tap = [&](float h, uint32_t o) {
#pragma unroll
            for (int r = 0; r < VPT; ++r) {
                const float2 u = tile[o + c[r]];
                re[r] += h * u.x;
                im[r] += h * u.y;
            }
        };
        uint32_t j = 0;
        for (; j + 8 <= T; j += 8) {
            float h[8];
            uint32_t o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                h[k] = hr[j + k];
                o[k] = off[j + k];
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) tap(h[k], o[k]);
        }
        for (; j < T; ++j) tap(hr[j], off[j]);
    }
    __syncthreads();

    // ---- discriminate
#pragma unroll
    for (int r = 0; r < VPT; ++r) {
        const uint32_t cc = tid + static_cast<uint32_t>(r) * threads;
        if (cc < nv) tile[cc] = make_float2(re[r], im[r]);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < VPT; ++r) {
        const uint32_t cc = tid + static_cast<uint32_t>(r) * threads;
        if (cc + 1 < nv) {
            const float2 v0 = tile[cc], v1 = tile[cc + 1];
            rec.audio[m0 + cc] = apt::fm::discriminate(Cx{v0.x, v0.y}, Cx{v1.x, v1.y}, P.gain);
        }
    }
}

using Kernel = void (*)(const FmBatch, const FmParams);

template <int FMT, bool MIX>
Kernel kernel_of_vpt(uint32_t vpt)
{
    return vpt == 4 ? k_fm<FMT, MIX, 4> : vpt == 2 ? k_fm<FMT, MIX, 2> : k_fm<FMT, MIX, 1>;
}
template <int FMT>
Kernel kernel_of_mix(bool mix, uint32_t vpt)
{
    return mix ? kernel_of_vpt<FMT, true>(vpt) : kernel_of_vpt<FMT, false>(vpt);
}
Kernel kernel_of(int format, bool mix, uint32_t vpt)
{
    switch (format) {
    case APTGPU_IQ_U8: return kernel_of_mix<APTGPU_IQ_U8>(mix, vpt);
    case APTGPU_IQ_S8: return kernel_of_mix<APTGPU_IQ_S8>(mix, vpt);
    case APTGPU_IQ_S16: return kernel_of_mix<APTGPU_IQ_S16>(mix, vpt);
    default: return kernel_of_mix<APTGPU_IQ_F32>(mix, vpt);
    }
}

}  // namespace

void fm_prepare(int format, bool mix, const apt::fm::Tile &tile)
{
    if (tile.lds_bytes <= 64u * 1024u) return;
    apt::hip_check(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel_of(format, mix, tile.vpt)),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(tile.lds_bytes)),
                   "hipFuncSetAttribute (k_fm LDS)");
}

void fm_demodulate(hipStream_t stream, int format, bool mix, const apt::fm::Tile &tile, const FmBatch &batch, int count,
                   uint32_t max_tiles, const FmParams &p)
{
    if (count <= 0 || max_tiles == 0) return;
    const Kernel k = kernel_of(format, mix, tile.vpt);
    hipLaunchKernelGGL(k, dim3(max_tiles, static_cast<uint32_t>(count)), dim3(tile.threads), tile.lds_bytes, stream, batch, p);
}

}  // namespace apt::gpu
