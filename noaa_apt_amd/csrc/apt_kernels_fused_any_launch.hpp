// apt_kernels_fused_any_launch.hpp — interface between the dispatcher (apt_kernels_fused_any.hip) and
// apt_kernels_fused_any_shape.hip, compiled once per launch shape.
#pragma once

#include "apt_kernels.hpp"
#include "apt_kernels_fused_any_geom.hpp"

namespace apt::gpu {

#define APT_ANY_SHAPE_ARGS                                                                                          \
    hipStream_t s, const CallArgs &call, const SlotPtrs *d_slots, uint64_t max_w, bool pcm16, const float *table,   \
        const float *h2, const float *h2p, float cosphi2, float sinphi, float inv_sinphi, bool want_gm,             \
        const AnyGeom &g, size_t lds, int prof
// NTHR threads with PER outputs each: the Makefile builds 256x8, 1024x8, 1024x4 and 256x4
template <int NTHR, int PER>
void fused_any_launch(APT_ANY_SHAPE_ARGS);
template <> void fused_any_launch<256, 8>(APT_ANY_SHAPE_ARGS);
template <> void fused_any_launch<1024, 8>(APT_ANY_SHAPE_ARGS);
template <> void fused_any_launch<1024, 4>(APT_ANY_SHAPE_ARGS);
template <> void fused_any_launch<256, 4>(APT_ANY_SHAPE_ARGS);

}  // namespace apt::gpu
