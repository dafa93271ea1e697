// apt_kernels_fm_stream.hip — k_fm_stream: k_fm's tile (apt_kernels_fm_body.hpp) over the virtual recording
// carry ++ chunk of one push (apt_kernels_fm_stream.hpp).  The chunk is read where the caller left it;
// only the load stage knows that there are two segments.
#include "apt_kernels_fm_stream.hpp"

#include "apt_kernels_fm_body.hpp"
#include "apt_plan.hpp"

namespace apt::gpu {

namespace {

template <int FMT, bool MIX, int VPT>
__global__ __launch_bounds__(256) void k_fm_stream(const FmStreamPush push, const FmParams P)
{
    extern __shared__ float2 tile[];
    const fm_body::TwoSegment src{push.carry, push.chunk, push.first, push.n_total, push.n_carry};
    fm_body::fm_tile<FMT, MIX, VPT>(src, push.audio, P, tile, blockIdx.x);
}

using Kernel = void (*)(const FmStreamPush, const FmParams);

template <int FMT, bool MIX>
Kernel kernel_of_vpt(uint32_t vpt)
{
    return vpt == 4 ? k_fm_stream<FMT, MIX, 4> : vpt == 2 ? k_fm_stream<FMT, MIX, 2> : k_fm_stream<FMT, MIX, 1>;
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

void fm_stream_prepare(int format, bool mix, const apt::fm::Tile &tile)
{
    if (tile.lds_bytes <= 64u * 1024u) return;
    apt::hip_check(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel_of(format, mix, tile.vpt)),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(tile.lds_bytes)),
                   "hipFuncSetAttribute (k_fm_stream LDS)");
}

void fm_stream_launch(hipStream_t stream, int format, bool mix, const apt::fm::Tile &tile, const FmStreamPush &push,
                      uint32_t tiles, const FmParams &p)
{
    if (tiles == 0) return;
    const Kernel k = kernel_of(format, mix, tile.vpt);
    hipLaunchKernelGGL(k, dim3(tiles), dim3(tile.threads), tile.lds_bytes, stream, push, p);
}

}  // namespace apt::gpu
