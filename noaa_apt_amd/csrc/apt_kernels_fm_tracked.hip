// apt_kernels_fm_tracked.hip — k_fm_tracked: stage C of the AFC (include/aptgpu.h §4b').  It is k_fm's
// tile (fm_tile of apt_kernels_fm_body.hpp: the same load, filter and discriminate, built the same way) with the phasors
// of every run of 8 taken from the recording's table instead of one increment: a 16-byte record per block of B frames.
// The mix is always made.
#include "apt_kernels_afc.hpp"

#include "apt_kernels_fm_body.hpp"
#include "apt_plan.hpp"

namespace apt::gpu {

namespace {

template <int FMT, int VPT>
__global__ __launch_bounds__(256) void k_fm_tracked(const FmBatch batch, const AfcTables tables, const FmParams P)
{
    extern __shared__ float2 tile[];
    const FmRecording rec = batch.r[blockIdx.y];
    fm_body::fm_tile<FMT, true, VPT>(fm_body::OneSegment(rec.iq, rec.n_frames), rec.audio, P, tile, blockIdx.x,
                                     fm_body::TablePhase{tables.table[blockIdx.y], tables.log2_B});
}

using Kernel = void (*)(const FmBatch, const AfcTables, const FmParams);

template <int FMT>
Kernel kernel_of_vpt(uint32_t vpt)
{
    return vpt == 4 ? k_fm_tracked<FMT, 4> : vpt == 2 ? k_fm_tracked<FMT, 2> : k_fm_tracked<FMT, 1>;
}
Kernel kernel_of(int format, uint32_t vpt)
{
    switch (format) {
    case APTGPU_IQ_U8: return kernel_of_vpt<APTGPU_IQ_U8>(vpt);
    case APTGPU_IQ_S8: return kernel_of_vpt<APTGPU_IQ_S8>(vpt);
    case APTGPU_IQ_S16: return kernel_of_vpt<APTGPU_IQ_S16>(vpt);
    default: return kernel_of_vpt<APTGPU_IQ_F32>(vpt);
    }
}

}  // namespace

void fm_tracked_prepare(int format, const apt::fm::Tile &tile)
{
    if (tile.lds_bytes <= 64u * 1024u) return;
    apt::hip_check(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel_of(format, tile.vpt)),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(tile.lds_bytes)),
                   "hipFuncSetAttribute (k_fm_tracked LDS)");
}

void fm_demodulate_tracked(hipStream_t stream, int format, const apt::fm::Tile &tile, const FmBatch &batch,
                           const AfcTables &tables, int count, uint32_t max_tiles, const FmParams &p)
{
    if (count <= 0 || max_tiles == 0) return;
    hipLaunchKernelGGL(kernel_of(format, tile.vpt), dim3(max_tiles, static_cast<uint32_t>(count)), dim3(tile.threads),
                       tile.lds_bytes, stream, batch, tables, p);
}

}  // namespace apt::gpu
