// apt_kernels_eqfloat.hpp — histogram equalisation of process()'s image on the f32 signal, before the pixel
// values become integers (apt_kernels_eqfloat.hip; the reference's docs/development.md:105-106).
//
// APTGPU_CONTRAST_HISTOGRAM_FLOAT: per half (columns [0, 1040) and [1040, 2080) of the n / 2080 whole rows,
// N = 1040 * height samples), order the samples by IEEE totalOrder on their bits (key = bits ^ (sign ? ~0 :
// 0x80000000)), cum(p) = samples of the half with key <= key(p), out(p) = (255f32 * (cum as f32 / N as f32)) as u8:
// imageext.rs:33,38 with one bin per representable value.
//
// level(c) = (255f32 * (c as f32 / N as f32)) as u8 is non-decreasing, so out(p) = #{v in 1..255 : key(p) >= T_v}
// with T_v the c_v-th smallest key, c_v the smallest c with level(c) >= v: 255 exact order statistics per half,
// found by a three-level radix multi-select (11 + 11 + 10 bits) over integer counters.
#pragma once

#include "apt_kernels.hpp"

namespace apt::gpu {

// Scratch of the mode, per recording: the counters of the three levels (2 halves x (2048 + 255*2048 + 255*1024)
// u32), then the select records and the 2 x 255 thresholds.  image_equalize_float zeroes the counters itself.
size_t eqfloat_ws_bytes();
// The thresholds T_1..T_255 of half A, then of half B, as sorted u32 keys (after image_equalize_float).
const uint32_t *eqfloat_ws_thresholds(const void *eq_ws);

// The thresholds of both halves of x's whole rows: memset, then count / select for each of the three levels, all on
// s.  n, cap, res: as for image_map_u8 (the pixel count comes from the decode record on the device when res is set).
void image_equalize_float(hipStream_t s, const float *x, const Result *res, uint64_t n, uint64_t cap, void *eq_ws);

// The output pass: every pixel's level by a binary search in its half's thresholds, the optional 180-degree
// rotation folded in as a gather, `channels` bytes per pixel (1 = gray, 4 = RGBA with R = G = B, A = 255).  Fills
// info's limits (from image_ws: MinMax's, as Histogram reports them), height and n_px like image_color.  out:
// 4-byte aligned for channels 1, 16-byte aligned for channels 4.
void image_color_float(hipStream_t s, const float *x, const Result *res, uint64_t n, uint64_t cap, void *image_ws,
                       const void *eq_ws, int channels, bool rotate, uint8_t *out, ImageResult *info);

}  // namespace apt::gpu
