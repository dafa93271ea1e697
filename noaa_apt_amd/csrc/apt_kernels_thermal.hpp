// apt_kernels_thermal.hpp — the thermal calibration stage behind the decode: brightness temperature of an infrared
// channel from the telemetry the image stage already reads (apt_kernels_thermal.hip on the GPU, apt_thermal.cpp on the
// CPU).  The reference has no calibration, so this is the definition (include/aptgpu.h states it in
// full; tests/np_thermal_model.py in numpy).  The scalar chain and the per-pixel arithmetic are written once, here,
// for both sides.
//
//  Telemetry  read_telemetry as the image stage runs it: telemetry_row, v[1..16] of the selected channel, its index.
//  Identity   settings.channel_id, or with -1 the telemetry's index; 5 "3b", 3 "4", 4 "5" pick coefficient set 0 / 1 / 2.
//  Space      128 rows from telemetry_row: f32 mean of columns [base + 44, base + 82), sequential; ranked by
//             totalOrder key, ties by row; ranks [16, 112) kept; their f64 mean in row order.
//  Scalars    f64, plain + - * / in the stated order (scalars_of), no contraction.
//  Pixel      f32 with every scalar rounded to f32 (kelvin_of); NaN unless N_e > 0 and finite.
//  Level      f32 (level_of); NaN -> level 0 (alpha 0).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#include "apt_kernels_despeckle.hpp"  // key_of_bits / bits_of_key, APT_DSP_HD

namespace apt::thermal {

constexpr int kPx = 2080;
constexpr int kHalfPx = 1040;
constexpr int kSpace0 = 44, kSpaceN = 38;    // the space view's columns [base + 44, base + 82)
constexpr int kVideo0 = 86, kVideoN = 909;   // the video columns [base + 86, base + 995)
constexpr int kSpaceRows = 128, kTrim = 16;  // ranks [kTrim, kSpaceRows - kTrim) are kept
constexpr int kReasonShort = 2, kReasonDecode = 4, kReasonChannel = 13, kReasonDegenerate = 14;
constexpr double kC1 = 1.1910427e-5, kC2 = 1.4387752;

// coefficient set of an identity (index of aptgpu_channel_name), -1: not a thermal channel
APT_DSP_HD int set_of_identity(int id) { return id == 5 ? 0 : id == 3 ? 1 : id == 4 ? 2 : -1; }

APT_DSP_HD bool finite64(double v) { return v - v == 0.0; }

struct Scalars {
    double slope, icpt, space, c_space, c_bb, t_bb, n_bb;
    bool ok;  // false: degenerate (reason 14)
};

// The scalar chain.  v: wedges 1..16 of the channel (v[0] = wedge 1); prt: [4][3]; ch: nu, A, B, N_s, b0, b1, b2.
APT_DSP_HD Scalars scalars_of(const float *v, double space, const double (*prt)[3], const double *ch)
{
    const double y[9] = {31., 63., 95., 127., 159., 191., 224., 255., 0.};
    double sx = 0., sy = 0.;
    for (int k = 0; k < 9; ++k) {
        sx = sx + static_cast<double>(v[k]);
        sy = sy + y[k];
    }
    const double mx = sx / 9., my = sy / 9.;
    double sxy = 0., sxx = 0.;
    for (int k = 0; k < 9; ++k) {
        const double dx = static_cast<double>(v[k]) - mx;
        sxy = sxy + dx * (y[k] - my);
        sxx = sxx + dx * dx;
    }
    Scalars s{};
    s.slope = sxy / sxx;
    s.icpt = my - s.slope * mx;
    s.space = space;
    double t_sum = 0.;
    for (int i = 0; i < 4; ++i) {
        const double c = 4. * (s.slope * static_cast<double>(v[9 + i]) + s.icpt);
        const double t = (prt[i][0] + prt[i][1] * c) + prt[i][2] * (c * c);
        t_sum = i == 0 ? t : t_sum + t;
    }
    s.t_bb = t_sum / 4.;
    const double nu = ch[0];
    const double t_eff = ch[1] + ch[2] * s.t_bb;
    s.n_bb = (kC1 * ((nu * nu) * nu)) / (exp((kC2 * nu) / t_eff) - 1.);
    s.c_bb = 4. * (s.slope * static_cast<double>(v[14]) + s.icpt);
    s.c_space = 4. * (s.slope * space + s.icpt);
    s.ok = sxx != 0. && finite64(s.slope) && finite64(s.icpt) && finite64(s.space) && finite64(s.t_bb) &&
           finite64(s.n_bb) && finite64(s.c_bb) && finite64(s.c_space) && s.c_space != s.c_bb;
    return s;
}

// what the pixel arithmetic reads: the scalars and the channel's coefficients, rounded to f32
struct PixelParams {
    float slope, icpt, n_s, n_bb, c_space, c_bb, b0, b1, b2, k1, k2, a, b;
    int32_t ok;  // 0: the record failed, every pixel is NaN
    uint32_t reserved[2];
};

APT_DSP_HD PixelParams pixel_params(const Scalars &s, const double *ch)
{
    PixelParams p{};
    p.slope = static_cast<float>(s.slope);
    p.icpt = static_cast<float>(s.icpt);
    p.n_s = static_cast<float>(ch[3]);
    p.n_bb = static_cast<float>(s.n_bb);
    p.c_space = static_cast<float>(s.c_space);
    p.c_bb = static_cast<float>(s.c_bb);
    p.b0 = static_cast<float>(ch[4]);
    p.b1 = static_cast<float>(ch[5]);
    p.b2 = static_cast<float>(ch[6]);
    p.k1 = static_cast<float>(kC1 * ((ch[0] * ch[0]) * ch[0]));
    p.k2 = static_cast<float>(kC2 * ch[0]);
    p.a = static_cast<float>(ch[1]);
    p.b = static_cast<float>(ch[2]);
    p.ok = s.ok ? 1 : 0;
    return p;
}

APT_DSP_HD float quiet_nan() { return __builtin_nanf(""); }

// brightness temperature of one sample
APT_DSP_HD float kelvin_of(float x, const PixelParams &p)
{
    const float ce = 4.f * (p.slope * x + p.icpt);
    const float n_lin = p.n_s + ((p.n_bb - p.n_s) * (p.c_space - ce)) / (p.c_space - p.c_bb);
    const float n_e = n_lin + ((p.b0 + p.b1 * n_lin) + p.b2 * (n_lin * n_lin));
    if (!(n_e > 0.f) || !(n_e - n_e == 0.f)) return quiet_nan();
    return (p.k2 / logf(1.f + p.k1 / n_e) - p.a) / p.b;
}

// level of the scale image of a non-NaN temperature
APT_DSP_HD uint32_t level_of(float t, float t_low, float t_high, bool cold_white)
{
    float s = (t - t_low) / (t_high - t_low);
    s = s < 0.f ? 0.f : s;
    s = s > 1.f ? 1.f : s;
    const uint32_t level = static_cast<uint32_t>(s * 255.f + 0.5f);
    return cold_white ? 255u - level : level;
}

}  // namespace apt::thermal

// ---- the host side (apt_thermal.cpp; CPU only)
namespace apt::thermal {

struct Settings {
    int channel;         // 0 A, 1 B
    int channel_id;      // -1: from the telemetry
    int image_channels;  // 0, 1, 4
    bool cold_white;
    float t_low, t_high;
    const uint8_t *palette;  // nullable, 256 * 3
};
// Both required.  A struct_size that is too small, a non-finite coefficient, B == 0, a channel other than 0 / 1,
// image_channels other than 0 / 1 / 4, an unknown flag, non-finite limits, t_high <= t_low, a palette without
// image_channels 4: Error{Invalid}.
Settings check_settings(const aptgpu_thermal_coeffs *c, const aptgpu_thermal_settings *s);
// the message of a record whose status is not OK, by its reason
const char *reason_text(int reason);
// read_telemetry (telemetry.rs:125-243) as the image stage's kernels compute it: false below 200 rows.
struct Telemetry {
    uint32_t row;
    float values_a[16], values_b[16];
    int channel_a, channel_b;
};
bool telemetry_host(const float *x, size_t rows, Telemetry *out);
// The definition in plain C++.  kelvin receives h * 909 floats, image (image_channels != 0) h * 2080 * image_channels
// bytes, *info the record.  A failed record throws Error{Internal} after filling *info.
void run_host(const float *x, size_t n, const aptgpu_thermal_coeffs &c, const Settings &s, float *kelvin,
              uint8_t *image, aptgpu_thermal_result *info);

}  // namespace apt::thermal

#if defined(__HIPCC__)
namespace apt::gpu {

// Device-side record: aptgpu_thermal_result up to n_nan / t_min / t_max, which the map kernel's waves gather in
// kThermalParts partial records, 64 bytes apart: a wave adds its NaN count and lowers / raises the extremes (as
// totalOrder keys, 0xFFFFFFFF / 0 = none yet) in part[wave % kThermalParts] with integer atomics.  (All waves on one
// record cost 45 of the kernel's 55 us at 1198 rows: ~5000 atomics on three addresses, one after the other.)
// thermal_record_to_public folds the parts once the record is on the host.
constexpr int kThermalParts = 64;
struct ThermalPart {
    unsigned long long n_nan;
    uint32_t t_min_key, t_max_key;
    uint32_t pad[12];
};
struct ThermalRecord {
    int32_t status, reason;
    uint32_t height, telemetry_row;
    int32_t channel_id;
    uint32_t reserved;
    unsigned long long n_nan;  // (0 on the device)
    double slope, icpt, space, c_space, c_bb, t_bb, n_bb;
    uint32_t t_min_key, t_max_key;  // (none on the device)
    uint32_t pad[8];
    ThermalPart part[kThermalParts];
};
void thermal_record_to_public(const ThermalRecord &r, aptgpu_thermal_result *out);

// the coefficients, and the scale image's table, as kernel arguments
struct ThermalCoeffs {
    double prt[4][3];
    double channel[3][7];
};
struct ThermalTable {
    uint32_t has_palette;
    uint8_t rgb[768];
};

// Scratch of the stage per recording: the record, the pixel parameters, the telemetry record, the 128 row means.
size_t thermal_ws_bytes();
ThermalRecord *thermal_ws_record(void *ws);
ImageResult *thermal_ws_telemetry(void *ws);

// The three launches on s, behind image_telemetry(s, x, res, n, cap, image_ws, thermal_ws_telemetry(ws), false) on the
// same stream.  x, n, cap, res: as for image_map_u8 (the sample count comes from the decode record on the device when
// res is set).  kelvin holds cap / 2080 * 909 floats; image (nullable with image_channels == 0) cap * image_channels
// bytes, 4-byte aligned for RGBA.  `timed` brackets each launch with its timer name.
struct ThermalLaunch {
    const float *x;
    const Result *res;
    uint64_t n, cap;
    int channel, channel_id, image_channels;
    bool cold_white;
    float t_low, t_high;
    float *kelvin;
    uint8_t *image;
};
void thermal_space(hipStream_t s, const ThermalLaunch &l, void *ws);
void thermal_setup(hipStream_t s, const ThermalLaunch &l, const ThermalCoeffs &c, void *ws);
void thermal_map(hipStream_t s, const ThermalLaunch &l, const ThermalTable &table, void *ws);

}  // namespace apt::gpu
#endif
