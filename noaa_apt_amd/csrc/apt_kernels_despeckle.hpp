// apt_kernels_despeckle.hpp — the despeckle stage in front of process(): a band-aware median of the decoded f32 rows
// (apt_kernels_despeckle.hip on the GPU, apt_despeckle.cpp on the CPU).  The reference only names the
// item (docs/development.md:139), so this is the definition; tests/np_despeckle_model.py states it in numpy.
//
//  Shape      h = n / 2080 whole rows; samples past h * 2080 are copied bit for bit.  h == 0: out = in, replaced = 0,
//             status OK, no limits are computed.
//  Bands      each row is eight column bands, [0,39) [39,86) [86,995) [995,1040) and the same + 1040 (sync, space,
//             video, telemetry of channels A and B, decode.rs:16-35).  A window never leaves its band.
//  Window     radius r in {1, 2}: the (2r+1)^2 samples at rows clamp(y + dy, 0, h - 1) and columns
//             clamp(x + dx, b0, b1 - 1) of the pixel's band [b0, b1); clamping replicates the edge sample.
//  Median     samples are ordered by IEEE totalOrder on their bits (key = bits ^ (sign ? ~0 : 0x80000000) as u32, as
//             §16); med is the element of rank (2r+1)^2 / 2 (0-based), returned with its own bits.
//  Decision   out = med if med is not NaN and !(fabsf(x - med) <= t), else x.  One f32 subtraction and one comparison.
//             A NaN x among finite neighbours is replaced, a sample in a mostly-NaN window is kept; t = 0 is the plain
//             median except that +-0 are left alone.
//  Threshold  threshold == 0: t = 0, no limits pass.  Otherwise (low, high) = misc::percent(signal, 0.98) of the
//             unfiltered signal (what APTGPU_CONTRAST_PERCENT reports for it) and t = threshold * (high - low) in f32.
//             A NaN t makes every sample with a non-NaN med take med.
//  Count      replaced = the samples for which the rule picked med (also where med's bits equal x's).
#pragma once

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define APT_DSP_HD __host__ __device__ inline
#else
#define APT_DSP_HD inline
#endif

namespace apt::despeckle {

constexpr int kPx = 2080;
constexpr int kHalfPx = 1040;

// IEEE totalOrder as an unsigned compare, and back
APT_DSP_HD uint32_t key_of_bits(uint32_t b) { return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
APT_DSP_HD uint32_t bits_of_key(uint32_t k) { return k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu); }

// the band [*b0, *b1) of column x < 2080
APT_DSP_HD void band_of(int x, int *b0, int *b1)
{
    const int off = x >= kHalfPx ? kHalfPx : 0;
    const int xm = x - off;
    *b0 = off + (xm < 39 ? 0 : xm < 86 ? 39 : xm < 995 ? 86 : 995);
    *b1 = off + (xm < 39 ? 39 : xm < 86 ? 86 : xm < 995 ? 995 : kHalfPx);
}

APT_DSP_HD uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
APT_DSP_HD uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
// (the three-operand forms are what the compiler turns into v_min3_u32 / v_max3_u32 / v_med3_u32)
APT_DSP_HD uint32_t umin3(uint32_t a, uint32_t b, uint32_t c) { return umin(umin(a, b), c); }
APT_DSP_HD uint32_t umax3(uint32_t a, uint32_t b, uint32_t c) { return umax(umax(a, b), c); }
APT_DSP_HD uint32_t umed3(uint32_t a, uint32_t b, uint32_t c) { return umax(umin(a, b), umin(umax(a, b), c)); }

// Median of 9 from three columns sorted ascending (c[0] <= c[1] <= c[2]): the largest of the lows, the median of the
// mids and the smallest of the highs bracket it.
APT_DSP_HD uint32_t median9_sorted_columns(const uint32_t (&a)[3], const uint32_t (&b)[3], const uint32_t (&c)[3])
{
    return umed3(umax3(a[0], b[0], c[0]), umed3(a[1], b[1], c[1]), umin3(a[2], b[2], c[2]));
}

// Median of 25 by forgetful selection: of any 14 keys neither the smallest nor the largest can have rank 12 among the
// 25, so both are dropped and the next key joins; 11 rounds leave three keys around their median.  Every index is a
// compile-time constant (registers, no scratch); the array is used up.
namespace detail {
APT_DSP_HD void cx(uint32_t &lo, uint32_t &hi)
{
    const uint32_t a = lo, b = hi;
    lo = umin(a, b);
    hi = umax(a, b);
}
// moves the smallest of v[0..S) to v[0] and the largest to v[S-1]
template <int S>
APT_DSP_HD void ends(uint32_t (&v)[25])
{
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < S / 2; ++i) cx(v[i], v[S - 1 - i]);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 1; i <= (S - 1) / 2; ++i) cx(v[0], v[i]);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = S / 2; i < S - 1; ++i) cx(v[i], v[S - 1]);
}
template <int S>
APT_DSP_HD uint32_t forget(uint32_t (&v)[25])
{
    if constexpr (S == 3) {
        return umed3(v[0], v[1], v[2]);
    } else {
        ends<S>(v);
        v[0] = v[14 + (14 - S)];  // the next key takes the minimum's place; v[S-1], the maximum, falls off the end
        return forget<S - 1>(v);
    }
}
}  // namespace detail
APT_DSP_HD uint32_t median25(uint32_t (&v)[25]) { return detail::forget<14>(v); }

}  // namespace apt::despeckle

// ---- the host side (apt_despeckle.cpp; CPU only)
#include "../../include/aptgpu.h"
#include "apt_host.hpp"

namespace apt::despeckle {

struct Settings {
    int radius;
    float threshold;
};
// NULL = the defaults (radius 1, threshold 0).  A struct_size that is too small, a radius other than 1 or 2, a
// negative or NaN threshold: Error{Invalid}.
Settings check_settings(const aptgpu_despeckle_settings *s);
// the message of a record whose status is not OK, by its reason (those of aptgpu_image_result)
const char *reason_text(int reason);
// misc::percent (misc.rs:119-175) as the image stage's kernels compute it; false: no low bucket (reason 3).  n > 0.
bool percent_host(const float *x, size_t n, float percent, float *low, float *high);
// The definition in plain C++: out receives n floats, *info the record.  A limits failure throws Error{Internal}
// after filling info->status / reason.
void run_host(const float *x, size_t n, const Settings &s, float *out, aptgpu_despeckle_result *info);

}  // namespace apt::despeckle

#if defined(__HIPCC__)
#include "apt_kernels.hpp"

namespace apt::gpu {

// Device-side record == aptgpu_despeckle_result (include/aptgpu.h).
struct DespeckleResult {
    int32_t status;   // 0 ok, 1 Internal
    int32_t reason;   // 0, or the limits' reason (3 no low bucket), 4 the decode before it failed
    uint32_t height;  // whole rows filtered
    uint32_t reserved;
    uint64_t replaced;
    float low, high, t;
    uint32_t reserved2;
};

// Scratch of the stage per recording: the record, and the ImageResult the limits pass reports into.
size_t despeckle_ws_bytes();
DespeckleResult *despeckle_ws_record(void *ws);
ImageResult *despeckle_ws_limits_info(void *ws);

// One k_despeckle<radius> launch on s (behind a memset of the record).  x, n, cap, res: as for image_map_u8 (the
// sample count comes from the decode record on the device when res is set); out has x's capacity and must not overlap
// it.  threshold > 0: limits[0..1] and lim_info are what image_percent(.., 0.98f, ..) left on the same stream; a limits
// failure is recorded (status, reason) and x is copied unfiltered.  threshold == 0: both are ignored (nullable).
void despeckle(hipStream_t s, const float *x, const Result *res, uint64_t n, uint64_t cap, int radius, float threshold,
               const float *limits, const ImageResult *lim_info, float *out, DespeckleResult *rec);

}  // namespace apt::gpu
#endif
