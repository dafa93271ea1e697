// apt_color_tune.hpp — the false colour tune of processing.rs:126-140, written once for every kernel that colours a
// pixel (apt_kernels_color.hip, apt_kernels_landmask.hip), for the plain C++ twin of the latter and for the entry points
// that fold the settings (apt_capi_image.hip, apt_capi_landmask.hip).  Host and device.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define APT_TUNE_HD __host__ __device__ inline
#else
#define APT_TUNE_HD inline
#endif

namespace apt::gpu {

// The false colour tune of one channel (processing.rs:126-140) with the settings folded in on the
// host: s' = start * 0.3f, e' = end * 0.3f, k = (1 + e') - s', o = s' * 255; out = in * k - o.
struct ColorTune {
    float k_a, o_a, k_b, o_b;
};

// the per-call part, f32 as the reference rounds it
inline ColorTune color_tune_of(float a_start, float a_end, float b_start, float b_end)
{
    const float factor = 0.3f;
    const float s_a = a_start * factor, e_a = a_end * factor;
    const float s_b = b_start * factor, e_b = b_end * factor;
    ColorTune t;
    t.k_a = 1.f + e_a - s_a;
    t.o_a = s_a * 255.f;
    t.k_b = 1.f + e_b - s_b;
    t.o_b = s_b * 255.f;
    return t;
}

// tune_input_values (processing.rs:126-140): `(in * k - o).clamp(0., 255.) as u32`; clamp keeps a
// NaN and `as u32` makes it 0
APT_TUNE_HD uint32_t tune(uint32_t in, float k, float o)
{
    const float t = static_cast<float>(in) * k - o;
    if (t != t) return 0u;
    const float c = t < 0.f ? 0.f : (t > 255.f ? 255.f : t);
    return static_cast<uint32_t>(c);
}

}  // namespace apt::gpu
