// apt_lab.cpp — the host side of apt_lab.hpp: Lab::from_rgb of every palette colour and gray, the quantiser's
// thresholds, and the two CPU entry points aptgpu_lab_from_rgb / aptgpu_lab_to_rgb.
//
// Built like apt_host.cpp (-ffp-contract=off): every f32 operation rounds on its own, and the powers are
// the C library's powf, called at run time (Rust's f32::powf calls the same function on Linux).
#include "apt_lab.hpp"

#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/aptgpu.h"

namespace apt::lab {

namespace {

// rgb_to_xyz_map: one sRGB channel value to linear
float linear(uint8_t v)
{
    const float c = static_cast<float>(v);
    if (c > 10.f) return powf((c + 0.055f * 255.f) / (1.055f * 255.f), 2.4f);
    return c / (12.92f * 255.f);
}

// xyz_to_lab_map
float lab_f(float t)
{
    if (t > kEpsilon) return powf(t, 1.f / 3.f);
    return (kKappa * t + 16.f) / 116.f;
}

float from_bits(uint32_t u)
{
    float f;
    std::memcpy(&f, &u, sizeof f);
    return f;
}

}  // namespace

void from_rgb(const uint8_t rgb[3], float lab[3])
{
    const float r = linear(rgb[0]), g = linear(rgb[1]), b = linear(rgb[2]);
    const float x = (r * 0.4124564390896921f + g * 0.357576077643909f) + b * 0.18043748326639894f;
    const float y = (r * 0.21267285140562248f + g * 0.715152155287818f) + b * 0.07217499330655958f;
    const float z = (r * 0.019333895582329317f + g * 0.119192025881303f) + b * 0.9503040785363677f;
    const float fx = lab_f(x / kWhiteX), fy = lab_f(y), fz = lab_f(z / kWhiteZ);
    lab[0] = 116.f * fy - 16.f;
    lab[1] = 500.f * (fx - fy);
    lab[2] = 200.f * (fy - fz);
}

uint8_t bin_of(float l)
{
    if (!(l > 0.f)) return 0;  // negative, zero and NaN
    // l never reaches 101 (white is 100 exactly); the reference would panic past 100, the tables stay in bounds
    return l >= 100.f ? 100 : static_cast<uint8_t>(l);
}

uint32_t quantise_direct(float c)
{
    const float v = c > kS0 ? 1.055f * powf(c, 1.f / 2.4f) - 0.055f : c * 12.92f;
    const float r = roundf(v * 255.f);  // half away from zero, as Rust's round
    if (!(r > 0.f)) return 0;           // (NaN too)
    return r >= 255.f ? 255u : static_cast<uint32_t>(r);
}

const float *thresholds()
{
    static const std::vector<float> thr = [] {
        std::vector<float> t(256, INFINITY);
        // t[k]: bisection over the bit patterns of the non-negative floats, whose order is the numbers' order;
        // q(1.0) = 255 bounds every search
        const uint32_t one = 0x3f800000u;
        for (uint32_t k = 1; k <= static_cast<uint32_t>(kLevels); ++k) {
            uint32_t lo = 0, hi = one;  // q(from_bits(hi)) >= k holds throughout
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (quantise_direct(from_bits(mid)) >= k) hi = mid;
                else lo = mid + 1;
            }
            t[k - 1] = from_bits(lo);
        }
        return t;
    }();
    return thr.data();
}

std::shared_ptr<const Tables> tables_for(const uint8_t *palette_rgb)
{
    constexpr size_t kBytes = 256 * 256 * 3;
    static std::mutex mu;
    static std::vector<uint8_t> last;
    static std::shared_ptr<const Tables> cached;
    std::lock_guard<std::mutex> lock(mu);
    if (cached && std::memcmp(last.data(), palette_rgb, kBytes) == 0) return cached;
    auto t = std::make_shared<Tables>();
    for (int i = 0; i < kEntries; ++i) {
        uint8_t rgb[3];
        if (i < kPaletteEntries) {
            std::memcpy(rgb, palette_rgb + 3 * static_cast<size_t>(i), 3);
        } else {
            rgb[0] = rgb[1] = rgb[2] = static_cast<uint8_t>(i - kPaletteEntries);
        }
        float lab[3];
        from_rgb(rgb, lab);
        t->ab[i][0] = lab[1];
        t->ab[i][1] = lab[2];
        t->bin[i] = bin_of(lab[0]);
    }
    std::memcpy(t->thr, thresholds(), sizeof t->thr);
    last.assign(palette_rgb, palette_rgb + kBytes);
    cached = t;
    return cached;
}

}  // namespace apt::lab

extern "C" {

int aptgpu_lab_from_rgb(const uint8_t *rgb, size_t n, float *lab)
{
    if (n && (!rgb || !lab)) return APTGPU_ERR_INVALID;
    for (size_t i = 0; i < n; ++i) apt::lab::from_rgb(rgb + 3 * i, lab + 3 * i);
    return APTGPU_OK;
}

int aptgpu_lab_to_rgb(const float *lab, size_t n, uint8_t *rgb)
{
    if (n && (!lab || !rgb)) return APTGPU_ERR_INVALID;
    const float *thr = apt::lab::thresholds();
    for (size_t i = 0; i < n; ++i) {
        const uint32_t p = apt::lab::to_rgba(lab[3 * i], lab[3 * i + 1], lab[3 * i + 2], thr);
        rgb[3 * i] = static_cast<uint8_t>(p);
        rgb[3 * i + 1] = static_cast<uint8_t>(p >> 8);
        rgb[3 * i + 2] = static_cast<uint8_t>(p >> 16);
    }
    return APTGPU_OK;
}

}  // extern "C"
