// track_host_main.cpp — a stand-alone program around the CPU side of the flywheel sync stage (apt_track_sync.cpp: the
// settings checks, the refusals, score_host and track_host), for sanitizer builds.  No GPU, no library, no Python:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include tools/sanitize/track_host_main.cpp noaa_apt_amd/csrc/apt_track_sync.cpp -o track_host_main
//   ./track_host_main
//
// Every pixel width 1..8 at n in {L + G, L + G + 1, 3 L + G + 17} and w in {0, 1, 8, 64}, the input, the scores and
// every output allocated at exactly their sizes (an access past either end is the sanitizer's to report); silence (the
// tie rules: the path is 17, 17 + L, 17 + 2 L), noise with a NaN and an Inf, planted frames that must be found, the
// path's invariants, and every refusal.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "../../noaa_apt_amd/csrc/apt_kernels_track_sync.hpp"

namespace {

int failures = 0;
void expect(bool ok, const char *what)
{
    if (!ok) {
        std::fprintf(stderr, "FAILED: %s\n", what);
        ++failures;
    }
}

aptgpu_track_settings settings(uint32_t w, float lam)
{
    aptgpu_track_settings s{};
    s.struct_size = sizeof s;
    s.max_jitter = w;
    s.penalty = lam;
    return s;
}

struct Run {
    std::vector<float> score, scores, rows;
    std::vector<uint32_t> positions;
    aptgpu_track_result info{};
};

Run run(const std::vector<float> &x, uint32_t pw, uint32_t w, float lam)
{
    const aptgpu_track_settings cs = settings(w, lam);
    const apt::track::Settings st = apt::track::check_settings(&cs);
    expect(apt::track::pixel_width(4160u * pw, st) == pw, "pixel_width");
    const apt::track::Geometry g = apt::track::geometry_of(x.size(), pw, st);
    Run r;
    r.info.struct_size = sizeof r.info;
    r.score.resize(g.M);
    apt::track::score_host(x.data(), g, r.score.data());
    apt::track::track_host(x.data(), x.size(), g, st, r.score.data(), r.positions, r.scores, &r.rows, &r.info);
    // the invariants
    const uint32_t L = g.L;
    expect(!r.positions.empty() && r.positions.front() < L, "first position < L");
    expect(r.positions.back() < g.M && r.positions.back() + L >= g.M, "last position >= M - L");
    expect(r.positions.size() <= g.pos_cap, "positions_bound");
    for (size_t k = 1; k < r.positions.size(); ++k) {
        const uint32_t d = r.positions[k] - r.positions[k - 1];
        expect(d >= L - w && d <= L + w, "step within L +- w");
    }
    expect(r.info.n_positions == r.positions.size() && r.rows.size() == static_cast<size_t>(r.info.n_rows) * 2080u, "record");
    return r;
}

uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

template <typename Fn>
bool refused(Fn &&fn, const char *text)
{
    try {
        fn();
    } catch (const apt::Error &e) {
        return e.kind == apt::ErrorKind::Invalid && e.message.find(text) != std::string::npos;
    }
    return false;
}

}  // namespace

int main()
{
    const uint32_t jitters[] = {0, 1, 8, 64};
    for (uint32_t pw = 1; pw <= 8; ++pw) {
        const uint32_t L = 2080u * pw, G = 38u * pw;
        const size_t sizes[] = {L + G, L + G + 1, 3u * L + G + 17u};
        for (size_t n : sizes)
            for (uint32_t w : jitters) {
                const float lam = w == 8 || w == 1 ? 0.1f : 0.f;
                // silence: every tie rule
                const Run z = run(std::vector<float>(n, 0.f), pw, w, lam);
                if (n == sizes[2])
                    expect(z.positions.size() == 3 && z.positions[0] == 17 && z.positions[1] == 17 + L && z.positions[2] == 17 + 2 * L,
                           "silence: 17, 17 + L, 17 + 2 L");
                for (float v : z.score) expect(v == 0.f, "silence scores 0");
                // noise with planted frames, a NaN and an Inf
                std::vector<float> x(n);
                uint32_t seed = 12345u + pw * 977u + static_cast<uint32_t>(n);
                for (float &v : x) v = 4000.f + static_cast<float>(lcg(seed) >> 20) - 2048.f;
                const uint32_t first = 37u * pw + 5u;
                for (size_t p = first; p + G <= n; p += L)
                    for (uint32_t j = 0; j < G; ++j) x[p + j] += apt::track::template_plus(static_cast<int>(j), static_cast<int>(pw)) ? 9000.f : -3000.f;
                const Run clean = run(x, pw, w, lam);
                expect(clean.positions.front() == first, "the planted frames are found");
                expect(clean.scores.front() > 0.9f, "a planted frame scores near 1");
                x[n / 3] = std::numeric_limits<float>::quiet_NaN();
                x[n / 2 + 7] = std::numeric_limits<float>::infinity();
                const Run bad = run(x, pw, w, lam);
                for (float v : bad.score) expect(v == v && std::fabs(v) < 1.0001f, "scores stay finite and within +-1");
                expect(bad.score[n / 3 < bad.score.size() ? n / 3 : bad.score.size() - 1] == 0.f, "a NaN window scores 0");
            }
    }
    // the refusals
    {
        const apt::track::Settings d = apt::track::check_settings(nullptr);
        expect(d.w == 8 && d.lam == 0.1f, "defaults");
        auto bad = [&](auto change, const char *text) {
            aptgpu_track_settings s = settings(8, 0.1f);
            change(s);
            return refused([&] { (void)apt::track::check_settings(&s); }, text);
        };
        expect(bad([](auto &s) { s.struct_size = 8; }, "struct_size"), "struct_size");
        expect(bad([](auto &s) { s.max_jitter = 65; }, "max_jitter"), "w > 64");
        expect(bad([](auto &s) { s.penalty = -0.1f; }, "penalty"), "negative penalty");
        expect(bad([](auto &s) { s.penalty = std::nanf(""); }, "penalty"), "NaN penalty");
        expect(bad([](auto &s) { s.penalty = std::numeric_limits<float>::infinity(); }, "penalty"), "infinite penalty");
        expect(refused([&] { (void)apt::track::pixel_width(12481, d); }, "multiple of 4160"), "pw not an integer");
        expect(refused([&] { (void)apt::track::pixel_width(0, d); }, "multiple of 4160"), "rate 0");
        expect(refused([&] { (void)apt::track::pixel_width(4160 * 9, d); }, "1..8"), "pw above 8");
        expect(refused([&] { (void)apt::track::pixel_width(4160, apt::track::Settings{520, 0.f}); }, "quarter of a row"), "4 w >= L");
        expect(refused([&] { (void)apt::track::geometry_of(3 * 2118 - 1, 3, d); }, "shorter than one row"), "short n");
        expect(refused([&] { (void)apt::track::geometry_of(1ull << 31, 3, d); }, "too long"), "long n");
        aptgpu_track_result r{};
        r.struct_size = 8;
        expect(refused([&] { apt::track::check_result_struct(&r); }, "aptgpu_track_result"), "result struct_size");
    }
    std::printf(failures ? "track_host_main: %d check(s) failed\n" : "track_host_main: ok\n", failures);
    return failures ? 1 : 0;
}
