// apt_track_sync.cpp — the flywheel sync stage on the CPU: the settings checks and refusals every entry point shares
// (all of them before a device is touched), and the definition of apt_kernels_track_sync.hpp in plain C++
// (aptgpu_track_sync_host), which the kernels are tested against besides the numpy model.
#include "apt_kernels_track_sync.hpp"

#include <algorithm>
#include <cmath>

namespace apt::track {

Settings check_settings(const aptgpu_track_settings *s)
{
    if (!s) return Settings{8, 0.1f};
    if (s->struct_size < sizeof(aptgpu_track_settings))
        throw Error{ErrorKind::Invalid, "aptgpu_track_settings: struct_size not set"};
    if (s->max_jitter > static_cast<uint32_t>(kMaxJitter))
        throw Error{ErrorKind::Invalid, "track: max_jitter must be 0..64"};
    if (!(s->penalty >= 0.f) || !finite(s->penalty))
        throw Error{ErrorKind::Invalid, "track: penalty must be finite and >= 0"};
    return Settings{static_cast<int>(s->max_jitter), s->penalty};
}

uint32_t pixel_width(uint32_t work_rate_hz, const Settings &s)
{
    if (work_rate_hz == 0 || work_rate_hz % 4160u != 0)
        throw Error{ErrorKind::Invalid, "track: work_rate must be a multiple of 4160 Hz"};
    const uint32_t pw = work_rate_hz / 4160u;
    if (pw > static_cast<uint32_t>(kMaxPw))
        throw Error{ErrorKind::Invalid, "track: work_rate / 4160 must be 1..8"};
    if (4u * static_cast<uint32_t>(s.w) >= static_cast<uint32_t>(kPx) * pw)
        throw Error{ErrorKind::Invalid, "track: max_jitter must be below a quarter of a row"};
    return pw;
}

Geometry geometry_of(uint64_t n, uint32_t pw, const Settings &s)
{
    Geometry g{};
    g.pw = pw;
    g.L = static_cast<uint32_t>(kPx) * pw;
    g.G = 38u * pw;
    if (n < static_cast<uint64_t>(g.L) + g.G)
        throw Error{ErrorKind::Invalid, "track: the signal is shorter than one row and one sync frame"};
    if (n >= (1ull << 31)) throw Error{ErrorKind::Invalid, "track: the signal is too long (2^31 work samples)"};
    g.M = static_cast<uint32_t>(n - g.G);
    g.pos_cap = positions_bound(g.M, g.L, s.w);
    return g;
}

void check_result_struct(const aptgpu_track_result *info)
{
    if (info && info->struct_size < sizeof(aptgpu_track_result))
        throw Error{ErrorKind::Invalid, "aptgpu_track_result: struct_size not set"};
}

const char *reason_text(int reason)
{
    switch (reason) {
    case 1: return "track: the decode before it refused the recording (less than 10 rows of samples)";
    case 2: return "track: the signal is shorter than one row and one sync frame";
    case 3: return "track: more positions than the list holds";
    default: return "track stage failed";
    }
}

void score_host(const float *x, const Geometry &g, float *score)
{
    const float fg = static_cast<float>(g.G), norm = norm_of(g.G), wmean = mean_weight();
    std::vector<uint8_t> plus(g.G);
    for (uint32_t j = 0; j < g.G; ++j) plus[j] = template_plus(static_cast<int>(j), static_cast<int>(g.pw)) ? 1 : 0;
    for (uint32_t i = 0; i < g.M; ++i) {
        float c = 0.f, s1 = 0.f, s2 = 0.f;
        const float *p = x + i;
        for (uint32_t j = 0; j < g.G; ++j) score_step(p[j], plus[j] != 0, c, s1, s2);
        score[i] = score_finish(c, s1, s2, fg, norm, wmean);
    }
}

void track_host(const float *x, uint64_t n, const Geometry &g, const Settings &s, const float *score,
                std::vector<uint32_t> &positions, std::vector<float> &scores, std::vector<float> *rows,
                aptgpu_track_result *info)
{
    const int32_t L = static_cast<int32_t>(g.L), M = static_cast<int32_t>(g.M);
    std::vector<float> best(g.M);
    std::vector<int8_t> bp(g.M);
    // (a chunk of L - w positions reads nothing it writes: the plain ascending loop computes the same values)
    for (int32_t i = 0; i < M; ++i) {
        float cur;
        int b;
        best_predecessor(i, L, s.w, s.lam, [&](int d) { return best[static_cast<size_t>(i - L - d)]; }, cur, b);
        best[static_cast<size_t>(i)] = score[i] + cur;
        bp[static_cast<size_t>(i)] = static_cast<int8_t>(b);
    }
    int32_t end = std::max<int32_t>(0, M - L);
    for (int32_t i = end + 1; i < M; ++i)
        if (best[static_cast<size_t>(i)] > best[static_cast<size_t>(end)]) end = i;  // the first maximum
    positions.clear();
    for (int32_t p = end;;) {
        positions.push_back(static_cast<uint32_t>(p));
        const int d = bp[static_cast<size_t>(p)];
        if (d == kStart) break;
        p = p - L - d;
    }
    std::reverse(positions.begin(), positions.end());
    scores.resize(positions.size());
    uint32_t n_rows = 0;
    for (size_t k = 0; k < positions.size(); ++k) {
        scores[k] = score[positions[k]];
        if (static_cast<uint64_t>(positions[k]) + g.L <= n) n_rows += 1;
    }
    if (rows) {
        rows->resize(static_cast<size_t>(n_rows) * kPx);
        for (uint32_t r = 0; r < n_rows; ++r)
            for (int c = 0; c < kPx; ++c)
                (*rows)[static_cast<size_t>(r) * kPx + static_cast<size_t>(c)] = x[positions[r] + g.pw * static_cast<uint32_t>(c)];
    }
    if (info) {
        const uint32_t size = info->struct_size;
        *info = aptgpu_track_result{};
        info->struct_size = size;
        info->n_positions = static_cast<uint32_t>(positions.size());
        info->n_rows = n_rows;
        info->end = static_cast<uint32_t>(end);
        info->n = n;
        info->total = best[static_cast<size_t>(end)];
    }
}

}  // namespace apt::track
