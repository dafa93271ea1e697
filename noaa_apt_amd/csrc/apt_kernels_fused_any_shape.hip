// apt_kernels_fused_any_shape.hip — ONE launch shape of k_fused_any per compilation: APT_ANY_NTHR threads with APT_ANY_PER
// outputs each.  The Makefile compiles this file once per shape (fused_any_<NTHR>x<PER>.o): 256x8 and 1024x8,
// 1024x4, and 256x4 (tiles of 1024 work samples: input rates whose 2048-sample tile does not fit the LDS).
#if !defined(APT_ANY_NTHR) || !defined(APT_ANY_PER)
#error "compile with -DAPT_ANY_NTHR=<threads> -DAPT_ANY_PER=<outputs per thread>"
#endif
#include "apt_kernels_fused_any_impl.hpp"

namespace apt::gpu {

template <>
void fused_any_launch<APT_ANY_NTHR, APT_ANY_PER>(APT_ANY_SHAPE_ARGS)
{
    launch_any_shape<APT_ANY_NTHR, APT_ANY_PER>(s, call, d_slots, max_w, pcm16, table, h2, h2p, cosphi2, sinphi, inv_sinphi, want_gm, g, lds, prof);
}

}  // namespace apt::gpu
