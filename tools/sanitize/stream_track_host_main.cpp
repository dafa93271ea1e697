// stream_track_host_main.cpp — a stand-alone program around the CPU side of live flywheel sync (apt_stream_track.cpp:
// the design, the refusals and the twin's tracker over its rings), for sanitizer builds.  No GPU, no library, no Python:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tools/sanitize/stream_track_host_main.cpp noaa_apt_amd/csrc/apt_stream_track.cpp noaa_apt_amd/csrc/apt_stream.cpp \
//       noaa_apt_amd/csrc/apt_track_sync.cpp noaa_apt_amd/csrc/apt_front_end.cpp noaa_apt_amd/csrc/apt_host.cpp \
//       -o stream_track_host_main
//   ./stream_track_host_main
//
// A synthetic recording (an AM carrier with a sync-like burst per row over noise, optionally a NaN and an Inf, a dropout
// of two seconds) of 14.4 rows at 11 025 Hz and 48 kHz, f32 and s16, lag_rows 0 / 1 / 8 / 64, through the twin in
// awkward chunkings — one chunk, 1-sample pushes across a checkpoint, sizes 0 / 1 / primes, half seconds, a max_push of
// a quarter row (pushes are split, the rings wrap) — with the sample, row, position and score buffers allocated at
// exactly their sizes (the rows at exactly rows_bound: an access past either end is the sanitizer's to report).  Every
// push goes through HostLive::push, the interface and the splitting into segments of max_push that the C API uses;
// pushes of 0 samples and one of more than max_push are among the chunkings.  Every chunking must give the first one's positions, scores and rows bit for bit; lag_rows = 64 must give the one-shot
// tracker's (track_host on the twin's own F is not available here: the positions' steps are checked instead); the twin
// itself refuses a read of a ring index that is not live.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../noaa_apt_amd/csrc/apt_kernels_stream_track.hpp"

namespace {

namespace st = apt::stream;
namespace tk = apt::stream_track;

int failures = 0;
void expect(bool ok, const std::string &what)
{
    if (!ok) {
        std::fprintf(stderr, "FAILED: %s\n", what.c_str());
        ++failures;
    }
}

aptgpu_settings standard()
{
    aptgpu_settings s{};
    s.work_rate = 12480;
    s.resample_atten = 30.f;
    s.resample_delta_freq = 1000.f;
    s.resample_cutout = 4800.f;
    s.demodulation_atten = 25.f;
    return s;
}

aptgpu_stream_settings stream_settings(uint32_t rate, int format, uint32_t max_push)
{
    aptgpu_stream_settings ss{};
    ss.struct_size = sizeof ss;
    ss.input_rate_hz = rate;
    ss.sync = 1;  // (not read by a tracked stream)
    ss.format = format;
    ss.max_push = max_push;
    return ss;
}

aptgpu_live_track_settings track_settings(uint32_t lag, uint32_t w = 8, float lam = 0.1f)
{
    aptgpu_live_track_settings t{};
    t.struct_size = sizeof t;
    t.lag_rows = lag;
    t.max_jitter = w;
    t.penalty = lam;
    return t;
}

std::vector<float> recording(uint32_t rate, double seconds, bool nonfinite)
{
    const size_t n = static_cast<size_t>(rate * seconds);
    std::vector<float> x(n);
    uint32_t lcg = 12345u;
    for (size_t i = 0; i < n; ++i) {
        const double t = static_cast<double>(i) / rate;
        const double row_t = std::fmod(t + 0.13, 0.5);
        const double env = row_t < 0.0067 ? (std::fmod(row_t * 1040.0, 1.0) < 0.5 ? 0.1 : 1.0) : 0.3 + 0.5 * row_t;
        lcg = lcg * 1664525u + 1013904223u;
        const double noise = (static_cast<double>(lcg >> 8) / (1 << 24) - 0.5) * 9000.0;
        const bool dropout = t > 3.1 && t < 5.1;
        x[i] = dropout ? 0.f : static_cast<float>(std::rint(12000.0 * env * std::cos(2.0 * 3.14159265358979 * 2400.0 * t) + noise));
    }
    if (nonfinite) {
        x[n / 2] = std::numeric_limits<float>::quiet_NaN();
        x[2 * n / 3] = std::numeric_limits<float>::infinity();
    }
    return x;
}

struct Output {
    std::vector<float> rows, scores;
    std::vector<uint64_t> pos;
    std::vector<uint32_t> per_call;
    st::State last{};
    tk::Record rec{};
};

Output run(const tk::Design &d, const std::vector<float> &x, const std::vector<size_t> &sizes)
{
    tk::HostTrackStream twin(d);
    st::HostLive &hs = twin;  // (what the C API holds)
    const st::Params &P = d.stream.P;
    Output out;
    size_t at = 0, k = 0;
    auto call = [&](size_t n, bool finish) {
        const uint32_t cap = hs.rows_bound(n);
        expect(cap == tk::rows_bound(d.T, hs.track_record()->m, tk::positions_final(d.T, st::work_count(P, hs.state().n_in + n, true))),
               "rows_bound is the tracker's");
        std::vector<float> rows(static_cast<size_t>(cap) * st::kPx), scores(cap);
        std::vector<uint64_t> pos(cap);
        std::vector<float> f(x.begin() + at, x.begin() + at + n);
        std::vector<int16_t> s(n);
        for (size_t i = 0; i < n; ++i) s[i] = static_cast<int16_t>(std::isfinite(f[i]) ? f[i] : 0.f);
        const char *src = P.s16 ? reinterpret_cast<const char *>(s.data()) : reinterpret_cast<const char *>(f.data());
        hs.push(n ? src : nullptr, n, true, finish, rows.data(), pos.data(), scores.data(), cap);
        at += n;
        const st::State &r = hs.state();
        expect(r.status == 0, "no internal bound reached (reason " + std::to_string(r.reason) + ")");
        expect(r.n_rows <= cap, "rows within the bound");
        out.rows.insert(out.rows.end(), rows.begin(), rows.begin() + static_cast<size_t>(r.n_rows) * st::kPx);
        out.pos.insert(out.pos.end(), pos.begin(), pos.begin() + r.n_rows);
        out.scores.insert(out.scores.end(), scores.begin(), scores.begin() + r.n_rows);
        out.per_call.push_back(r.n_rows);
    };
    while (at < x.size()) {
        size_t n = k < sizes.size() ? sizes[k] : x.size() - at;
        if (n > x.size() - at) n = x.size() - at;
        ++k;
        call(n, false);
    }
    call(0, true);
    out.last = hs.state();
    out.rec = *hs.track_record();
    return out;
}

bool same_bits(const std::vector<float> &a, const std::vector<float> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
}

void chunkings(uint32_t rate, int format, uint32_t lag, bool nonfinite)
{
    const aptgpu_settings s = standard();
    const std::string tag = std::to_string(rate) + (format ? " s16" : " f32") + " lag " + std::to_string(lag) + (nonfinite ? " nonfinite" : "");
    const std::vector<float> x = recording(rate, 7.2, nonfinite && format == 0);
    aptgpu_stream_settings ss = stream_settings(rate, format, 0);
    const aptgpu_live_track_settings ts = track_settings(lag);
    const tk::Design d = tk::design_tracked(&s, &ss, &ts, APTGPU_MODE_STRICT, false);
    const Output one = run(d, x, {x.size()});
    const uint64_t L = d.T.L;
    expect(one.last.n_in == x.size() && one.last.work_len == st::work_count(d.stream.P, x.size(), true), tag + ": counts");
    expect(one.rec.n_positions >= 13 && one.last.rows_total * st::kPx == one.rows.size() && one.last.rows_total + 1 >= one.rec.n_positions,
           tag + ": positions and rows");
    expect(one.rec.m == one.last.work_len - d.T.G && one.rec.next_checkpoint == one.rec.m / L + 1, tag + ": the record");
    for (size_t k = 1; k < one.pos.size(); ++k) expect(one.pos[k] + d.T.w >= one.pos[k - 1] + L, tag + ": steps are at least L - w");
    if (lag == 64) {
        expect(one.per_call.size() == 2 && one.per_call[0] == 0 && one.rec.n_relocks == 0, tag + ": nothing before finish");
        for (size_t k = 1; k < one.pos.size(); ++k) expect(one.pos[k] <= one.pos[k - 1] + L + d.T.w, tag + ": one path, steps at most L + w");
    }

    // 1-sample pushes across checkpoint 4 (m = 4 L), large chunks elsewhere
    const size_t at_cp = static_cast<size_t>((4 * L + d.T.G) * d.stream.P.m / d.stream.P.l);
    std::vector<size_t> single{at_cp - 700};
    single.insert(single.end(), 1500, 1);
    std::vector<size_t> odd;
    const size_t pattern[] = {0, 1, 7, 0, 1009, 1, 4099, 2, 0, 263};
    for (int rep = 0; rep < 600; ++rep) odd.push_back(pattern[rep % 10]);
    const std::vector<std::vector<size_t>> lists = {single, odd, std::vector<size_t>(200, rate / 2), std::vector<size_t>(200, 4096)};
    for (size_t q = 0; q < lists.size(); ++q) {
        const Output o = run(d, x, lists[q]);
        expect(same_bits(o.rows, one.rows) && same_bits(o.scores, one.scores) && o.pos == one.pos && o.rec.n_relocks == one.rec.n_relocks,
               tag + ": chunking " + std::to_string(q));
    }
    // a small max_push (pushes are split; the input ring wraps many times, the others as often as their reach allows)
    ss.max_push = static_cast<uint32_t>(L * d.stream.P.m / d.stream.P.l / 4);
    const tk::Design small = tk::design_tracked(&s, &ss, &ts, APTGPU_MODE_STRICT, false);
    expect(x.size() >= 3 * static_cast<size_t>(small.stream.P.cap_in) && one.last.work_len >= 3ull * small.T.cap_best, tag + ": the rings wrap");
    if (lag <= 1) expect(one.last.work_len >= 2ull * small.stream.P.cap_f && one.last.work_len >= 2ull * small.T.cap_bp, tag + ": F and bp wrap");
    const Output o = run(small, x, {x.size() / 3, 5, x.size() / 2});
    expect(same_bits(o.rows, one.rows) && same_bits(o.scores, one.scores) && o.pos == one.pos, tag + ": quarter-row max_push");
    // n above max_push (x.size() / 3 and x.size() / 2 are many segments each), n == 0 in the middle, and a push that is
    // exactly max_push + 1 samples: one full segment and one of a single sample
    expect(x.size() / 3 > 4 * static_cast<size_t>(ss.max_push), tag + ": pushes above max_push");
    const Output e = run(small, x, {0, static_cast<size_t>(ss.max_push) + 1, 0, 0, x.size() / 2, 0});
    expect(same_bits(e.rows, one.rows) && same_bits(e.scores, one.scores) && e.pos == one.pos, tag + ": max_push + 1 and empty pushes");
}

void refusals()
{
    const aptgpu_settings s = standard();
    const aptgpu_stream_settings ok = stream_settings(11025, 0, 0);
    auto refused = [&](aptgpu_settings st_, aptgpu_stream_settings ss, aptgpu_live_track_settings ts, apt::ErrorKind kind, const char *what) {
        try {
            (void)tk::design_tracked(&st_, &ss, &ts, APTGPU_MODE_STRICT, false);
            expect(false, std::string("not refused: ") + what);
        } catch (const apt::Error &e) {
            expect(e.kind == kind, std::string("error class: ") + what + " (" + e.message + ")");
        }
    };
    aptgpu_live_track_settings t = track_settings(65);
    refused(s, ok, t, apt::ErrorKind::Invalid, "lag_rows 65");
    t = track_settings(8);
    t.struct_size = 8;
    refused(s, ok, t, apt::ErrorKind::Invalid, "track struct_size");
    refused(s, ok, track_settings(8, 65), apt::ErrorKind::Invalid, "w 65");
    refused(s, ok, track_settings(8, 8, -1.f), apt::ErrorKind::Invalid, "negative penalty");
    aptgpu_stream_settings a = ok;
    a.struct_size = 0;
    refused(s, a, track_settings(8), apt::ErrorKind::Invalid, "stream struct_size 0");
    aptgpu_settings big = s;
    big.work_rate = 9 * 4160;
    refused(big, ok, track_settings(8), apt::ErrorKind::Invalid, "a work rate above 8 x 4160 Hz");

    // shorter than a row and a sync frame: finish reports the one-shot's refusal
    const std::vector<float> x = recording(11025, 0.4, false);
    const aptgpu_live_track_settings ts = track_settings(8);
    tk::HostTrackStream hs(tk::design_tracked(&s, &ok, &ts, APTGPU_MODE_STRICT, false));
    std::vector<float> rows(64 * st::kPx), scores(64);
    std::vector<uint64_t> pos(64);
    hs.push(x.data(), x.size(), true, false, rows.data(), pos.data(), scores.data(), 64);
    hs.push(nullptr, 0, true, true, rows.data(), pos.data(), scores.data(), 64);
    expect(hs.state().status == 1 && hs.state().reason == tk::kReasonTooShort && hs.state().n_rows == 0, "too short");
}

}  // namespace

int main()
{
    try {
        for (uint32_t lag : {0u, 1u, 8u, 64u}) {
            chunkings(11025, 0, lag, false);
            chunkings(11025, 1, lag, false);
        }
        chunkings(11025, 0, 8, true);
        chunkings(48000, 0, 1, false);
        chunkings(48000, 0, 8, true);
        refusals();
    } catch (const apt::Error &e) {
        std::fprintf(stderr, "FAILED: unexpected error: %s\n", e.message.c_str());
        return 1;
    }
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("stream_track_host_main: all checks passed\n");
    return 0;
}
