// apt_despeckle.cpp — the despeckle stage on the CPU: the settings checks every entry point shares, and the
// definition of apt_kernels_despeckle.hpp in plain C++ (aptgpu_despeckle_host), which the kernel is tested against.
#include "apt_kernels_despeckle.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace apt::despeckle {

namespace {
const char *kZeroMin = "Can't get minimum of a zero length vector";
const char *kNoLowBucket = "percent: no bucket reaches the low threshold (the reference panics here)";
const char *kDecodeFailed = "despeckle: the decode before it failed";

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
}  // namespace

Settings check_settings(const aptgpu_despeckle_settings *s)
{
    if (!s) return Settings{1, 0.f};
    if (s->struct_size < sizeof(aptgpu_despeckle_settings))
        throw Error{ErrorKind::Invalid, "aptgpu_despeckle_settings: struct_size not set"};
    if (s->radius != 1 && s->radius != 2) throw Error{ErrorKind::Invalid, "despeckle: radius must be 1 or 2"};
    if (!(s->threshold >= 0.f)) throw Error{ErrorKind::Invalid, "despeckle: threshold must be >= 0 and not NaN"};
    return Settings{s->radius, s->threshold};
}

const char *reason_text(int reason)
{
    switch (reason) {
    case 1: return kZeroMin;
    case 3: return kNoLowBucket;
    case 4: return kDecodeFailed;
    default: return "despeckle stage failed";
    }
}

bool percent_host(const float *x, size_t n, float percent, float *low, float *high)
{
    // dsp::get_min / get_max (dsp.rs:20-54): strict comparisons from best = x[0]
    float mn = x[0], mx = x[0];
    for (size_t i = 0; i < n; ++i) {
        if (x[i] < mn) mn = x[i];
        if (x[i] > mx) mx = x[i];
    }
    const float remainder = (1.f - percent) / 2.f;  // misc.rs:126
    const float total_range = mx - mn;              // misc.rs:137
    std::vector<uint32_t> buckets(1000, 0u);
    for (size_t i = 0; i < n; ++i) {
        // get_bucket (misc.rs:140-144): `as usize` saturates, NaN and negatives -> 0; then .min(999)
        const float t = std::trunc((x[i] - mn) / total_range * 1000.f);
        size_t b = 0;
        if (t > 0.f) b = t >= 999.f ? 999 : static_cast<size_t>(t);
        buckets[b] += 1;
    }
    uint32_t accum = 0;
    int low_bucket = -1, high_bucket = -1;
    for (int b = 0; b < 1000; ++b) {  // misc.rs:152-163
        accum += buckets[static_cast<size_t>(b)];
        const float frac = static_cast<float>(accum) / static_cast<float>(n);
        if (low_bucket < 0 && frac > remainder)
            low_bucket = b;
        else if (high_bucket < 0 && frac > 1.f - remainder)
            high_bucket = b;
    }
    if (high_bucket < 0) high_bucket = 999;  // misc.rs:165-169
    if (low_bucket < 0) return false;        // misc.rs:172 unwraps a None
    *low = static_cast<float>(low_bucket) / 1000.f * total_range + mn;
    *high = static_cast<float>(high_bucket) / 1000.f * total_range + mn;
    return true;
}

void run_host(const float *x, size_t n, const Settings &s, float *out, aptgpu_despeckle_result *info)
{
    aptgpu_despeckle_result rec{};
    const size_t h = n / kPx;
    rec.height = static_cast<uint32_t>(h);
    if (n) std::memcpy(out, x, n * sizeof(float));  // the tail, and everything the rule keeps
    float t = 0.f;
    if (h > 0 && s.threshold != 0.f) {
        if (!percent_host(x, n, 0.98f, &rec.low, &rec.high)) {
            rec.status = APTGPU_ERR_INTERNAL;
            rec.reason = 3;
            rec.low = rec.high = 0.f;
            if (info) *info = rec;
            throw Error{ErrorKind::Internal, reason_text(3)};
        }
        t = s.threshold * (rec.high - rec.low);
    }
    rec.t = t;
    const int r = s.radius, side = 2 * r + 1, count = side * side;
    uint32_t win[25];
    for (size_t y = 0; y < h; ++y) {
        const float *rows[5];
        for (int dy = -r; dy <= r; ++dy) {
            const ptrdiff_t yy = std::clamp<ptrdiff_t>(static_cast<ptrdiff_t>(y) + dy, 0, static_cast<ptrdiff_t>(h) - 1);
            rows[dy + r] = x + static_cast<size_t>(yy) * kPx;
        }
        for (int col = 0; col < kPx; ++col) {
            int b0, b1;
            band_of(col, &b0, &b1);
            int k = 0;
            for (int j = 0; j < side; ++j)
                for (int dx = -r; dx <= r; ++dx) win[k++] = key_of_bits(bits_of(rows[j][std::clamp(col + dx, b0, b1 - 1)]));
            std::nth_element(win, win + count / 2, win + count);
            const float med = float_of(bits_of_key(win[count / 2]));
            const float v = rows[r][col];
            if (med == med && !(std::fabs(v - med) <= t)) {
                out[y * kPx + static_cast<size_t>(col)] = med;
                rec.replaced += 1;
            }
        }
    }
    if (info) *info = rec;
}

}  // namespace apt::despeckle
