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
// The three stages are fm_tile() of apt_kernels_fm_body.hpp, which k_fm_stream shares; k_fm reads one recording.
#include "apt_kernels_fm.hpp"

#include "apt_kernels_fm_body.hpp"
#include "apt_plan.hpp"

namespace apt::gpu {

namespace {

template <int FMT, bool MIX, int VPT>
__global__ __launch_bounds__(256) void k_fm(const FmBatch batch, const FmParams P)
{
    extern __shared__ float2 tile[];
    const FmRecording rec = batch.r[blockIdx.y];
    fm_body::fm_tile<FMT, MIX, VPT>(fm_body::OneSegment(rec.iq, rec.n_frames), rec.audio, P, tile, blockIdx.x);
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
