// apt_thermal.cpp — the thermal calibration stage on the CPU: the checks every entry point shares, and the definition
// of apt_kernels_thermal.hpp in plain C++ (aptgpu_calibrate_thermal_host), which the kernels are tested against and
// which a stand-alone program can call without a GPU.
#include "apt_kernels_thermal.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace apt::thermal {

namespace {
uint32_t bits_of(float v)
{
    uint32_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}
float float_of(uint32_t b)
{
    float v;
    std::memcpy(&v, &b, sizeof v);
    return v;
}

// telemetry.rs:134-141: wedges 1-9, 7 variable wedges (0), wedges 1-9; 8 rows each
float telemetry_sample(int j)
{
    const int w = j >> 3;
    const int k = w < 9 ? w : (w < 16 ? -1 : w - 16);
    if (k < 0 || k == 8) return 0.f;
    if (k == 7) return 255.f;
    if (k == 6) return 224.f;
    return 31.f + 32.f * static_cast<float>(k);
}
}  // namespace

Settings check_settings(const aptgpu_thermal_coeffs *c, const aptgpu_thermal_settings *s)
{
    if (!c || !s) throw Error{ErrorKind::Invalid, "thermal: coefficients and settings are required"};
    if (c->struct_size < sizeof(aptgpu_thermal_coeffs))
        throw Error{ErrorKind::Invalid, "aptgpu_thermal_coeffs: struct_size not set"};
    if (s->struct_size < sizeof(aptgpu_thermal_settings))
        throw Error{ErrorKind::Invalid, "aptgpu_thermal_settings: struct_size not set"};
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(c->prt[i][k])) throw Error{ErrorKind::Invalid, "thermal: a PRT coefficient is not finite"};
    for (int i = 0; i < 3; ++i) {
        for (int k = 0; k < 7; ++k)
            if (!std::isfinite(c->channel[i][k]))
                throw Error{ErrorKind::Invalid, "thermal: a channel coefficient is not finite"};
        if (c->channel[i][2] == 0.) throw Error{ErrorKind::Invalid, "thermal: B must not be 0"};
    }
    if (s->channel != 0 && s->channel != 1) throw Error{ErrorKind::Invalid, "thermal: channel must be 0 (A) or 1 (B)"};
    if (s->image_channels != 0 && s->image_channels != 1 && s->image_channels != 4)
        throw Error{ErrorKind::Invalid, "thermal: image_channels must be 0, 1 or 4"};
    if (s->flags & ~APTGPU_THERMAL_COLD_WHITE) throw Error{ErrorKind::Invalid, "thermal: unknown flag"};
    if (!std::isfinite(s->t_low) || !std::isfinite(s->t_high) || !(s->t_high > s->t_low))
        throw Error{ErrorKind::Invalid, "thermal: t_low and t_high must be finite with t_high > t_low"};
    if (s->palette && s->image_channels != 4)
        throw Error{ErrorKind::Invalid, "thermal: a palette needs image_channels 4"};
    return Settings{s->channel, s->channel_id, s->image_channels, (s->flags & APTGPU_THERMAL_COLD_WHITE) != 0,
                    s->t_low, s->t_high, s->palette};
}

const char *reason_text(int reason)
{
    switch (reason) {
    case kReasonShort: return "Recording too short for telemetry decoding";
    case kReasonDecode: return "thermal: the decode before it failed";
    case kReasonChannel: return "thermal: not a thermal channel (APTGPU_THERMAL_REASON_CHANNEL)";
    case kReasonDegenerate:
        return "thermal: degenerate calibration, a zero or non-finite scalar (APTGPU_THERMAL_REASON_DEGENERATE)";
    default: return "thermal stage failed";
    }
}

bool telemetry_host(const float *x, size_t rows, Telemetry *out)
{
    constexpr size_t kLen = 200;
    if (rows < kLen) return false;
    // per-row band statistics, telemetry.rs:154-177 (sequential sums)
    std::vector<float> mean_a(rows), mean_b(rows), sd(rows);
    for (size_t r = 0; r < rows; ++r) {
        const float *a = x + r * kPx + 994;
        const float *b = x + r * kPx + 2034;
        float sa = 0.f, sb = 0.f;
        for (int i = 0; i < 44; ++i) sa += a[i];
        for (int i = 0; i < 44; ++i) sb += b[i];
        const float ma = sa / 44.f, mb = sb / 44.f;
        float va = 0.f, vb = 0.f;
        for (int i = 0; i < 44; ++i) {
            const float d = a[i] - ma;
            va += d * d;
        }
        for (int i = 0; i < 44; ++i) {
            const float d = b[i] - mb;
            vb += d * d;
        }
        mean_a[r] = ma;
        mean_b[r] = mb;
        sd[r] = std::sqrt((va + vb) / 88.f);
    }
    // first strict maximum of the quality above 0, telemetry.rs:196,210-231
    const size_t nc = rows - kLen;
    size_t row = 0;
    float best = 0.f;
    for (size_t i = 0; i < nc; ++i) {
        float sum = 0.f, s = 0.f;
        for (size_t j = 0; j < kLen; ++j) {
            const float t = telemetry_sample(static_cast<int>(j));
            sum += t * mean_a[i + j];
            sum += t * mean_b[i + j];
        }
        for (size_t j = 0; j < kLen; ++j) s += sd[i + j];
        const float q = sum / s;
        if (q > best) {
            best = q;
            row = i;
        }
    }
    out->row = static_cast<uint32_t>(row);
    // Telemetry::from_bands, telemetry.rs:30-72
    float wa[25], wb[25];
    for (int w = 0; w < 25; ++w) {
        float sa = 0.f, sb = 0.f;
        for (int r = 0; r < 8; ++r) {
            sa += mean_a[row + static_cast<size_t>(w * 8 + r)];
            sb += mean_b[row + static_cast<size_t>(w * 8 + r)];
        }
        wa[w] = sa / 8.f;
        wb[w] = sb / 8.f;
    }
    for (int wedge = 1; wedge <= 16; ++wedge) {
        out->values_a[wedge - 1] = wedge <= 9 ? (wa[wedge - 1] + wa[wedge + 15]) / 2.f : wa[wedge - 1];
        out->values_b[wedge - 1] = wedge <= 9 ? (wb[wedge - 1] + wb[wedge + 15]) / 2.f : wb[wedge - 1];
    }
    // the channel names, telemetry.rs:93-121
    for (int ch = 0; ch < 2; ++ch) {
        const float value = ch == 0 ? out->values_a[15] : out->values_b[15];
        int name = 0;
        float best_d = 0.f;
        bool nan = false;
        for (int i = 0; i < 9; ++i) {
            const float d = std::fabs((out->values_a[i] + out->values_b[i]) / 2.f - value);
            if (d != d) nan = true;
            if (i == 0 || d < best_d) {
                name = i;
                best_d = d;
            }
        }
        (ch == 0 ? out->channel_a : out->channel_b) = nan ? -1 : name;
    }
    return true;
}

void run_host(const float *x, size_t n, const aptgpu_thermal_coeffs &c, const Settings &s, float *kelvin,
              uint8_t *image, aptgpu_thermal_result *info)
{
    aptgpu_thermal_result rec{};
    const size_t h = n / kPx;
    rec.height = static_cast<uint32_t>(h);
    rec.channel_id = s.channel_id;
    rec.t_min = rec.t_max = quiet_nan();
    auto fail = [&](int reason) {
        rec.status = APTGPU_ERR_INTERNAL;
        rec.reason = reason;
        if (info) *info = rec;
        throw Error{ErrorKind::Internal, reason_text(reason)};
    };
    Telemetry tel{};
    if (!telemetry_host(x, h, &tel)) fail(kReasonShort);
    rec.telemetry_row = tel.row;
    if (s.channel_id == -1) rec.channel_id = s.channel == 0 ? tel.channel_a : tel.channel_b;
    const int set = set_of_identity(rec.channel_id);
    if (set < 0) fail(kReasonChannel);
    const int base = kHalfPx * s.channel;
    const float *v = s.channel == 0 ? tel.values_a : tel.values_b;

    // the space view: 128 row means, ranked, the middle 96 averaged in row order
    float means[kSpaceRows];
    uint32_t keys[kSpaceRows];
    for (int r = 0; r < kSpaceRows; ++r) {
        const float *p = x + (static_cast<size_t>(tel.row) + static_cast<size_t>(r)) * kPx + base + kSpace0;
        float sum = 0.f;
        for (int i = 0; i < kSpaceN; ++i) sum += p[i];
        means[r] = sum / static_cast<float>(kSpaceN);
        keys[r] = despeckle::key_of_bits(bits_of(means[r]));
    }
    double sum = 0.;
    for (int r = 0; r < kSpaceRows; ++r) {
        int rank = 0;
        for (int j = 0; j < kSpaceRows; ++j) rank += (keys[j] < keys[r] || (keys[j] == keys[r] && j < r)) ? 1 : 0;
        if (rank >= kTrim && rank < kSpaceRows - kTrim) sum = sum + static_cast<double>(means[r]);
    }
    const double space = sum / static_cast<double>(kSpaceRows - 2 * kTrim);

    const Scalars sc = scalars_of(v, space, c.prt, c.channel[set]);
    rec.slope = sc.slope;
    rec.icpt = sc.icpt;
    rec.space = sc.space;
    rec.c_space = sc.c_space;
    rec.c_bb = sc.c_bb;
    rec.t_bb = sc.t_bb;
    rec.n_bb = sc.n_bb;
    if (!sc.ok) fail(kReasonDegenerate);
    const PixelParams pp = pixel_params(sc, c.channel[set]);

    const int ic = s.image_channels;
    if (ic) {
        std::memset(image, 0, h * kPx * static_cast<size_t>(ic));
        if (ic == 4)
            for (size_t i = 0; i < h * kPx; ++i) image[4 * i + 3] = 255;
    }
    uint32_t min_key = 0xFFFFFFFFu, max_key = 0u;
    for (size_t y = 0; y < h; ++y) {
        const float *row = x + y * kPx + base + kVideo0;
        for (int i = 0; i < kVideoN; ++i) {
            const float t = kelvin_of(row[i], pp);
            kelvin[y * kVideoN + static_cast<size_t>(i)] = t;
            const bool nan = t != t;
            if (nan) {
                rec.n_nan += 1;
            } else if (t - t == 0.f) {
                const uint32_t k = despeckle::key_of_bits(bits_of(t));
                min_key = std::min(min_key, k);
                max_key = std::max(max_key, k);
            }
            if (!ic) continue;
            const uint32_t level = nan ? 0u : level_of(t, s.t_low, s.t_high, s.cold_white);
            uint8_t *px = image + (y * kPx + static_cast<size_t>(base + kVideo0 + i)) * static_cast<size_t>(ic);
            if (ic == 1) {
                px[0] = static_cast<uint8_t>(level);
            } else {
                px[0] = s.palette ? s.palette[3 * level] : static_cast<uint8_t>(level);
                px[1] = s.palette ? s.palette[3 * level + 1] : static_cast<uint8_t>(level);
                px[2] = s.palette ? s.palette[3 * level + 2] : static_cast<uint8_t>(level);
                px[3] = nan ? 0 : 255;
                if (nan) px[0] = px[1] = px[2] = 0;
            }
        }
    }
    if (min_key <= max_key) {
        rec.t_min = float_of(despeckle::bits_of_key(min_key));
        rec.t_max = float_of(despeckle::bits_of_key(max_key));
    }
    if (info) *info = rec;
}

}  // namespace apt::thermal
