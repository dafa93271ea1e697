// apt_kernels_fused_variant.hip — ONE instantiation of k_fused (apt_kernels_fused_impl.hpp) per compilation: the row
// APT_FUSED_VARIANT of apt_kernels_fused_variants.hpp for input samples of type APT_FUSED_XT.  The Makefile compiles this
// file once per row and input type (-DAPT_FUSED_VARIANT=kFused_<name> -DAPT_FUSED_XT=float|int16_t), one object each.
#if !defined(APT_FUSED_VARIANT) || !defined(APT_FUSED_XT)
#error "compile with -DAPT_FUSED_VARIANT=kFused_<row name> -DAPT_FUSED_XT=<float|int16_t>"
#endif
#include "apt_kernels_fused_impl.hpp"

namespace apt::gpu {

template <>
void fused_launch<APT_FUSED_VARIANT, APT_FUSED_XT>(const FusedLaunch &a)
{
    constexpr FusedVariantRow r = kFusedVariants[APT_FUSED_VARIANT];
    static_assert(r.i16 || std::is_same_v<APT_FUSED_XT, float>, "this row is instantiated for f32 input only");
    launch_fused_args<r.l, r.m, r.t1, r.t2, r.pw, r.nthr, r.mode, APT_FUSED_XT>(a);
}

}  // namespace apt::gpu
