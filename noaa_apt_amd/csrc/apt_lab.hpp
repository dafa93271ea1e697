// apt_lab.hpp — CIE Lab of the `lab` crate 0.11.0 (Cargo.lock:991) for the equalisation of a false-colour
// image (imageext.rs:50-64,66-95,124-143): Lab::from_rgb on the host, Lab::to_rgb split into f32 arithmetic
// that host and device share and a threshold quantiser that stands in for its powf.
//
// The constants and formulas restate the crate's published source; the crate itself could not be built
// next to this code, so the restatement is pinned by tests/np_lab_model.py, not by the crate.
// Every operation is rounded on its own (contract off) and every constant is an f32 literal or an f32
// expression evaluated in f32, as the crate writes them.
#pragma once

#include <cstddef>
#include <cstdint>
#include <memory>

#if defined(__HIP__)
#define APT_LAB_HD __host__ __device__
#else
#define APT_LAB_HD
#endif

namespace apt::lab {

constexpr int kPaletteEntries = 65536;         // palette colour (a, b) at b*256 + a, as the packed palette
constexpr int kEntries = kPaletteEntries + 256;  // then the grays (v, v, v) at 65536 + v
constexpr int kBins = 101;                     // `l as usize` in 0..=100 (histogram_lab)
constexpr int kLevels = 255;                   // quantiser thresholds t[1..255]

constexpr float kKappa = 24389.f / 27.f;
constexpr float kEpsilon = 216.f / 24389.f;
constexpr float kCbrtEpsilon = 6.f / 29.f;
constexpr float kWhiteX = 0.9504492182750991f;
constexpr float kWhiteZ = 1.0889166484304715f;
constexpr float kS0 = 0.003130668442500564f;

// What the device needs of one palette, uploaded in one copy: (a, b) and the L bin of every entry, and the
// quantiser (palette-independent).  thr[k - 1] = t[k], the smallest non-negative f32 c with q(c) >= k.
struct Tables {
    float ab[kEntries][2];
    float thr[256];  // thr[255] unused
    uint8_t bin[kEntries];
};

// Lab::to_rgb up to xyz_to_rgb_map's argument: the linear r, g, b.  Only f32 + - * /.
APT_LAB_HD inline void to_linear(float l, float a, float b, float rgb[3])
{
#pragma clang fp contract(off)
    const float fy = (l + 16.f) / 116.f;
    const float fx = a / 500.f + fy;
    const float fz = fy - b / 200.f;
    const float xr = fx > kCbrtEpsilon ? (fx * fx) * fx : (fx * 116.f - 16.f) / kKappa;
    const float yr = l > kEpsilon * kKappa ? (fy * fy) * fy : l / kKappa;
    const float zr = fz > kCbrtEpsilon ? (fz * fz) * fz : (fz * 116.f - 16.f) / kKappa;
    const float x = xr * kWhiteX, y = yr, z = zr * kWhiteZ;
    rgb[0] = (x * 3.2404541621141054f - y * 1.5371385127977166f) - z * 0.4985314095560162f;
    rgb[1] = (x * -0.9692660305051868f + y * 1.8760108454466942f) + z * 0.04155601753034984f;
    rgb[2] = (x * 0.05564343095911469f - y * 0.20402591351675387f) + z * 1.0572251882231791f;
}

// q(c) = #{k : c >= t[k]}: the thresholds ascend, so that count is the length of the prefix with
// thr <= c.  Negative and NaN give 0, c >= t[255] gives 255, as the crate's clamp does.
APT_LAB_HD inline uint32_t quantise(float c, const float *thr)
{
    uint32_t lo = 0, hi = kLevels;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (c >= thr[mid]) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Lab::to_rgb with the quantiser: R | G << 8 | B << 16 | 0xff << 24
APT_LAB_HD inline uint32_t to_rgba(float l, float a, float b, const float *thr)
{
    float c[3];
    to_linear(l, a, b, c);
    return quantise(c[0], thr) | (quantise(c[1], thr) << 8) | (quantise(c[2], thr) << 16) | 0xff000000u;
}

// ---- host side (apt_lab.cpp)
// Lab::from_rgb, with the C library's powf at run time
void from_rgb(const uint8_t rgb[3], float lab[3]);
// `l as usize` (saturating: negative and NaN give 0), kept <= 100
uint8_t bin_of(float l);
// the crate's xyz_to_rgb_map + round + clamp, computed directly (powf): the quantiser's definition
uint32_t quantise_direct(float c);
// the 255 thresholds (computed once per process)
const float *thresholds();
// the tables of one 256*256*3 RGB palette (pixel (a, b) at (b*256 + a)*3); the last palette's tables are
// kept, so a palette that stays the same is computed once
std::shared_ptr<const Tables> tables_for(const uint8_t *palette_rgb);

}  // namespace apt::lab
