// stream_host_main.cpp — a stand-alone program around the CPU side of live decode (apt_stream.cpp: the design, the
// refusals and the twin's state machine over its rings), for sanitizer builds.  No GPU, no library, no Python:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tools/sanitize/stream_host_main.cpp noaa_apt_amd/csrc/apt_stream.cpp noaa_apt_amd/csrc/apt_front_end.cpp \
//       noaa_apt_amd/csrc/apt_host.cpp -o stream_host_main
//   ./stream_host_main
//
// A synthetic recording (an AM carrier with a sync-like burst per row, then a NaN and an Inf) of 12.4 rows at 11 025 Hz,
// 48 kHz, 24 960 Hz and 12 480 Hz, f32 and s16, sync and no sync, through the twin in awkward chunkings — one chunk,
// 1-sample pushes across a row boundary, sizes 0 / 1 / primes, pushes longer than a small max_push, a max_push of a
// quarter row (every ring wraps), a fading carrier whose picker pushes two dozen peaks in one event, 25 rows in one
// launch sequence — with the sample, row and position buffers allocated at exactly their sizes (the rows at exactly
// rows_bound: an access past either end is the sanitizer's to report).  Every push goes through HostLive::push, the
// interface and the splitting into segments of max_push that the C API uses; pushes of 0 samples and one of more than
// max_push are among the chunkings.  Every chunking must give the first one's rows bit for bit; the twin itself refuses
// a read of a ring index that is not live.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../noaa_apt_amd/csrc/apt_kernels_stream.hpp"

namespace {

namespace st = apt::stream;

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

aptgpu_stream_settings stream_settings(uint32_t rate, bool sync, int format, uint32_t max_push)
{
    aptgpu_stream_settings ss{};
    ss.struct_size = sizeof ss;
    ss.input_rate_hz = rate;
    ss.sync = sync ? 1 : 0;
    ss.format = format;
    ss.max_push = max_push;
    return ss;
}

std::vector<float> recording(uint32_t rate, double seconds, bool nonfinite)
{
    const size_t n = static_cast<size_t>(rate * seconds);
    std::vector<float> x(n);
    uint32_t lcg = 12345u;
    for (size_t i = 0; i < n; ++i) {
        const double t = static_cast<double>(i) / rate;
        const double row_t = std::fmod(t, 0.5);
        // seven pulses of 1040 Hz at the start of every row, a ramp behind them
        const double env = row_t < 0.0067 ? (std::fmod(row_t * 1040.0, 1.0) < 0.5 ? 0.1 : 1.0) : 0.3 + 0.5 * row_t;
        lcg = lcg * 1664525u + 1013904223u;
        const double noise = (static_cast<double>(lcg >> 8) / (1 << 24) - 0.5) * 600.0;
        x[i] = static_cast<float>(std::rint(12000.0 * env * std::cos(2.0 * 3.14159265358979 * 2400.0 * t) + noise));
    }
    if (nonfinite) {
        x[n / 2] = std::numeric_limits<float>::quiet_NaN();
        x[2 * n / 3] = std::numeric_limits<float>::infinity();
    }
    return x;
}

struct Output {
    std::vector<float> rows;
    std::vector<uint64_t> pos;
    st::State last{};
    std::string error;
};

// pushes x in chunks of the given sizes (the last one takes the rest), then finishes
Output run(const st::Design &d, const std::vector<float> &x, const std::vector<size_t> &sizes)
{
    st::HostStream twin(d);
    st::HostLive &hs = twin;  // (what the C API holds)
    const st::Params &P = d.P;
    Output out;
    size_t at = 0, k = 0;
    auto call = [&](size_t n, bool finish) {
        // exact-size buffers: the samples of this push, the rows and positions its bound allows
        const uint32_t cap = hs.rows_bound(n);
        expect(cap == st::rows_bound(P, hs.state().n_in + n, hs.state().rows_total), "rows_bound is the picker's");
        std::vector<float> rows(static_cast<size_t>(cap) * st::kPx);
        std::vector<uint64_t> pos(cap);
        std::vector<float> f(x.begin() + at, x.begin() + at + n);
        std::vector<int16_t> s(n);
        for (size_t i = 0; i < n; ++i) s[i] = static_cast<int16_t>(std::isfinite(f[i]) ? f[i] : 0.f);
        const char *src = P.s16 ? reinterpret_cast<const char *>(s.data()) : reinterpret_cast<const char *>(f.data());
        hs.push(n ? src : nullptr, n, true, finish, rows.data(), pos.data(), nullptr, cap);
        at += n;
        const st::State &r = hs.state();
        expect(r.n_rows <= cap, "rows within the bound");
        out.rows.insert(out.rows.end(), rows.begin(), rows.begin() + static_cast<size_t>(r.n_rows) * st::kPx);
        out.pos.insert(out.pos.end(), pos.begin(), pos.begin() + r.n_rows);
    };
    while (at < x.size()) {
        size_t n = k < sizes.size() ? sizes[k] : x.size() - at;
        if (n > x.size() - at) n = x.size() - at;
        ++k;
        call(n, false);
    }
    call(0, true);
    out.last = hs.state();
    if (out.last.status != 0) out.error = st::reason_text(out.last.reason);
    return out;
}

bool same_bits(const std::vector<float> &a, const std::vector<float> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
}

void chunkings(uint32_t rate, bool sync, int format, bool nonfinite)
{
    const aptgpu_settings s = standard();
    const std::string tag = std::to_string(rate) + (sync ? " sync" : " nosync") + (format ? " s16" : " f32") + (nonfinite ? " nonfinite" : "");
    const std::vector<float> x = recording(rate, 6.2, nonfinite && format == 0);
    aptgpu_stream_settings ss = stream_settings(rate, sync, format, 0);
    const st::Design d = st::design_stream(&s, &ss, APTGPU_MODE_STRICT, false);
    const Output one = run(d, x, {x.size()});
    expect(one.error.empty(), tag + ": decodes");
    expect(one.last.n_in == x.size() && one.last.work_len == st::work_count(d.P, x.size(), true), tag + ": counts");
    expect(one.last.rows_total * st::kPx == one.rows.size() && one.last.rows_total >= 9, tag + ": rows");
    if (!one.rows.empty()) expect(one.rows[0] == 0.f, tag + ": the very first pixel");
    for (size_t k = 1; k < one.pos.size(); ++k) expect(one.pos[k] >= one.pos[k - 1], tag + ": positions ascend");

    // 1-sample pushes across a row boundary, large chunks elsewhere
    std::vector<size_t> single{static_cast<size_t>(rate) * 2 - 700};
    single.insert(single.end(), 1500, 1);
    // zeros, ones and primes
    std::vector<size_t> odd;
    const size_t pattern[] = {0, 1, 7, 0, 1009, 1, 4099, 2, 0, 263};
    for (int rep = 0; rep < 400; ++rep) odd.push_back(pattern[rep % 10]);
    const std::vector<std::vector<size_t>> lists = {single, odd, std::vector<size_t>(200, rate / 2), std::vector<size_t>(200, 4096)};
    for (size_t q = 0; q < lists.size(); ++q) {
        const Output o = run(d, x, lists[q]);
        expect(same_bits(o.rows, one.rows) && o.pos == one.pos && o.error == one.error, tag + ": chunking " + std::to_string(q));
    }
    // a small max_push (pushes are split; every ring wraps several times)
    const uint32_t quarter_row = static_cast<uint32_t>(static_cast<uint64_t>(d.P.spr) * d.P.m / d.P.l / 4);
    ss.max_push = quarter_row;
    const st::Design small = st::design_stream(&s, &ss, APTGPU_MODE_STRICT, false);
    expect(x.size() >= 3 * static_cast<size_t>(small.P.cap_in) && one.last.work_len >= 3ull * small.P.cap_f, tag + ": the rings wrap");
    const Output o = run(small, x, {x.size() / 3, 5, x.size() / 2});
    expect(same_bits(o.rows, one.rows) && o.pos == one.pos, tag + ": quarter-row max_push");
    // n above max_push (x.size() / 3 and x.size() / 2 are many segments each), n == 0 in the middle, and a push that is
    // exactly max_push + 1 samples: one full segment and one of a single sample
    expect(x.size() / 3 > 4 * static_cast<size_t>(quarter_row), tag + ": pushes above max_push");
    const Output e = run(small, x, {0, static_cast<size_t>(quarter_row) + 1, 0, 0, x.size() / 2, 0});
    expect(same_bits(e.rows, one.rows) && e.pos == one.pos, tag + ": max_push + 1 and empty pushes");
}

// A carrier that fades for 14 s and then stays level: the picker replaces one peak for 28 rows and then pushes all the
// missing peaks in one event; and a pass of 25 rows in one launch sequence (max_push above the recording).
void many_rows_at_once()
{
    const aptgpu_settings s = standard();
    const uint32_t rate = 12480;
    std::vector<float> x(static_cast<size_t>(rate) * 24);
    for (size_t i = 0; i < x.size(); ++i) {
        const double t = static_cast<double>(i) / rate;
        x[i] = static_cast<float>(std::rint(20000.0 * (1.0 - 0.9 * std::fmin(t / 14.0, 1.0)) * std::cos(2.0 * 3.14159265358979 * 2400.0 * t)));
    }
    aptgpu_stream_settings ss = stream_settings(rate, true, 0, 0);
    const st::Design d = st::design_stream(&s, &ss, APTGPU_MODE_STRICT, false);
    const Output one = run(d, x, {x.size()});
    expect(one.error.empty() && one.last.rows_total >= 40, "fading carrier: decodes, " + std::to_string(one.last.rows_total) + " rows");
    size_t longest = 0, run_len = 0;
    for (size_t k = 0; k < one.pos.size(); ++k) {
        run_len = (k && one.pos[k] == one.pos[k - 1]) ? run_len + 1 : 1;
        longest = std::max(longest, run_len);
    }
    expect(longest >= 16, "fading carrier: many copies of one position (" + std::to_string(longest) + ")");
    const Output half = run(d, x, std::vector<size_t>(100, rate / 2));
    expect(same_bits(half.rows, one.rows) && half.pos == one.pos, "fading carrier: half-second pushes");

    const std::vector<float> pass = recording(11025, 12.6, false);
    ss = stream_settings(11025, true, 0, 1u << 18);
    const st::Design big = st::design_stream(&s, &ss, APTGPU_MODE_STRICT, false);
    ss.max_push = 0;
    const st::Design def = st::design_stream(&s, &ss, APTGPU_MODE_STRICT, false);
    const Output a = run(big, pass, {pass.size()}), b = run(def, pass, std::vector<size_t>(100, 4096));
    expect(a.error.empty() && a.last.rows_total >= 22, "25 rows in one launch sequence");
    expect(same_bits(a.rows, b.rows) && a.pos == b.pos, "25 rows in one launch sequence: the rows of small pushes");
}

void refusals()
{
    const aptgpu_settings s = standard();
    auto refused = [&](aptgpu_settings st_, aptgpu_stream_settings ss, int mode, bool mfma, apt::ErrorKind kind, const char *what) {
        try {
            (void)st::design_stream(&st_, &ss, mode, mfma);
            expect(false, std::string("not refused: ") + what);
        } catch (const apt::Error &e) {
            expect(e.kind == kind, std::string("error class: ") + what + " (" + e.message + ")");
        }
    };
    aptgpu_stream_settings ok = stream_settings(11025, true, 0, 0);
    aptgpu_stream_settings a = ok;
    a.struct_size = 0;
    refused(s, a, 0, false, apt::ErrorKind::Invalid, "struct_size 0");
    a = ok;
    a.format = 2;
    refused(s, a, 0, false, apt::ErrorKind::Invalid, "format");
    a = ok;
    a.input_rate_hz = 0;
    refused(s, a, 0, false, apt::ErrorKind::Invalid, "rate 0");
    a = ok;
    a.input_rate_hz = 4294967291u;
    refused(s, a, 0, false, apt::ErrorKind::RateOverflow, "rate overflow");
    aptgpu_settings t = s;
    t.work_rate = 12481;
    refused(t, ok, 0, false, apt::ErrorKind::Internal, "work_rate");
    refused(s, ok, APTGPU_MODE_FAST, false, apt::ErrorKind::Unsupported, "fast mode");
    refused(s, ok, APTGPU_MODE_FP16_TAPS, false, apt::ErrorKind::Unsupported, "fp16 taps");
    refused(s, ok, 0, true, apt::ErrorKind::Unsupported, "matrix cores");
    t = s;
    t.export_wav = 1;
    refused(t, ok, 0, false, apt::ErrorKind::Unsupported, "export_wav");

    // a recording of less than ten rows: rows come out, then finish reports the reference's error
    const std::vector<float> x = recording(11025, 4.9, false);
    const Output o = run(st::design_stream(&s, &ok, 0, false), x, std::vector<size_t>(100, 3000));
    expect(o.last.status == 1 && o.last.reason == st::kReasonTooShort && !o.rows.empty(), "too short: error after rows");
}

}  // namespace

int main()
{
    try {
        for (uint32_t rate : {11025u, 48000u, 24960u, 12480u})
            for (int sync = 0; sync < 2; ++sync)
                for (int format = 0; format < 2; ++format) chunkings(rate, sync != 0, format, false);
        chunkings(11025, true, 0, true);
        chunkings(48000, true, 0, true);
        many_rows_at_once();
        refusals();
    } catch (const apt::Error &e) {
        std::fprintf(stderr, "FAILED: unexpected error: %s\n", e.message.c_str());
        return 1;
    }
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("stream_host_main: all checks passed\n");
    return 0;
}
