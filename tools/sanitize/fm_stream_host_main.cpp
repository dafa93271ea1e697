// fm_stream_host_main.cpp — a stand-alone program around the CPU side of the streaming FM demodulator
// (apt_fm_stream.cpp: the checks and the twin, over apt_fm.cpp), for sanitizer builds.  No GPU, no library, no Python:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include tools/sanitize/fm_stream_host_main.cpp noaa_apt_amd/csrc/apt_fm_stream.cpp \
//       noaa_apt_amd/csrc/apt_fm.cpp noaa_apt_amd/csrc/apt_host.cpp -o fm_stream_host_main
//   ./fm_stream_host_main
//
// Every format with and without a shift, first_frame 0 and one that is no multiple of 8: the recording goes through
// one-frame pushes, seeded random pushes (zeros included) and pushes longer than max_push_frames.  Every chunk and every
// push's output is a heap block of exactly its size (an access past either end is the sanitizer's to report), the
// concatenated outputs must equal run_host of the whole recording bit for bit (first_frame 0) or the based one-shot,
// and the counts must follow out_len.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../noaa_apt_amd/csrc/apt_kernels_fm_stream.hpp"

namespace {

int failures = 0;
void expect(bool ok, const char *what)
{
    if (!ok) {
        std::fprintf(stderr, "FAILED: %s\n", what);
        ++failures;
    }
}

aptgpu_fm_settings settings(int format, uint32_t d, double shift)
{
    aptgpu_fm_settings s{};
    s.struct_size = sizeof s;
    s.format = format;
    s.sample_rate_hz = 48000u * d;
    s.decimation = d;
    s.shift_hz = shift;
    s.channel_cutout_hz = 18000.f;
    s.channel_atten = 40.f;
    s.channel_delta_hz = 8000.f;
    s.deviation_hz = 17000.f;
    return s;
}

uint32_t lcg(uint32_t &state) { return state = state * 1664525u + 1013904223u; }

// n frames of pseudo-random components (finite in every format)
std::vector<uint8_t> frames(int format, size_t n, uint32_t seed)
{
    const size_t cb = apt::fm::component_bytes(format);
    std::vector<uint8_t> bytes(n * 2 * cb);
    for (size_t i = 0; i < 2 * n; ++i) {
        const uint32_t r = lcg(seed) >> 8;
        uint8_t *p = bytes.data() + i * cb;
        if (format == APTGPU_IQ_F32) {
            const float q = static_cast<float>(r % 2001u) / 1000.f - 1.f;
            std::memcpy(p, &q, 4);
        } else {
            std::memcpy(p, &r, cb);
        }
    }
    return bytes;
}

// pushes `iq` in `sizes` through exact-size blocks; returns the concatenated outputs
std::vector<float> walk(apt::fm::HostFmStream &s, const std::vector<uint8_t> &iq, const std::vector<size_t> &sizes, size_t fb)
{
    const apt::fm::Design &d = s.design().fm;
    std::vector<float> all;
    size_t p = 0;
    for (size_t k : sizes) {
        const size_t expect_out = static_cast<size_t>(apt::fm::stream_out_len(d, s.frames() + k) - apt::fm::stream_out_len(d, s.frames()));
        uint8_t *chunk = static_cast<uint8_t *>(std::malloc(k * fb ? k * fb : 1));
        float *out = static_cast<float *>(std::malloc(expect_out ? expect_out * sizeof(float) : 1));
        if (k) std::memcpy(chunk, iq.data() + p * fb, k * fb);
        const size_t got = s.push(k ? chunk : nullptr, k, expect_out ? out : nullptr);
        expect(got == expect_out, "a push returns out_len(n1) - out_len(n0) outputs");
        all.insert(all.end(), out, out + got);
        std::free(chunk);
        std::free(out);
        p += k;
        expect(s.frames() == p && s.outputs() == apt::fm::stream_out_len(d, p), "frames and outputs");
        expect(s.carry_frames() == p - apt::fm::stream_out_len(d, p) * d.D && s.carry_frames() < d.T + d.D, "carry_frames");
    }
    return all;
}

bool same_bits(const std::vector<float> &a, const std::vector<float> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
}

bool refused(const aptgpu_fm_settings &fm, aptgpu_fm_stream_settings ss, const char *field)
{
    try {
        (void)apt::fm::design_stream(&fm, &ss);
    } catch (const apt::Error &e) {
        return e.kind == apt::ErrorKind::Invalid && e.message.find(field) != std::string::npos;
    }
    return false;
}

}  // namespace

int main()
{
    const uint32_t decimations[] = {1, 5, 8};
    const uint64_t firsts[] = {0, (1ull << 32) - 8 * 61 - 3};
    for (int format = APTGPU_IQ_U8; format <= APTGPU_IQ_F32; ++format)
        for (uint32_t dec : decimations)
            for (int mixed = 0; mixed < 2; ++mixed)
                for (uint64_t first : firsts) {
                    const aptgpu_fm_settings fm = settings(format, dec, mixed ? -0.13 * 48000. * dec : 0.);
                    aptgpu_fm_stream_settings ss{};
                    ss.struct_size = sizeof ss;
                    ss.max_push_frames = 97;
                    ss.first_frame = first;
                    const apt::fm::StreamDesign design = apt::fm::design_stream(&fm, &ss);
                    const size_t t = design.fm.T, n = t + 40 * dec + 13, fb = 2 * apt::fm::component_bytes(format);
                    const std::vector<uint8_t> iq = frames(format, n, 7u + static_cast<uint32_t>(format) * 31u + dec);
                    std::vector<float> want(apt::fm::out_len(design.fm, n));
                    apt::fm::run_host_based(design.fm, first, iq.data(), n, want.data());
                    if (first == 0) {
                        std::vector<float> plain(want.size());
                        apt::fm::run_host(design.fm, iq.data(), n, plain.data());
                        expect(same_bits(plain, want), "run_host_based(0) is run_host");
                    }
                    apt::fm::HostFmStream s(design);
                    expect(same_bits(walk(s, iq, std::vector<size_t>(n, 1), fb), want), "one-frame pushes");
                    s.reset();
                    std::vector<size_t> sizes;
                    uint32_t seed = 99u + dec;
                    for (size_t left = n; left;) {
                        size_t k = (lcg(seed) >> 10) % (3 * t + 1);
                        if ((lcg(seed) >> 12) % 5 == 0) k = 0;
                        k = k < left ? k : left;
                        sizes.push_back(k);
                        left -= k;
                    }
                    expect(same_bits(walk(s, iq, sizes, fb), want), "random pushes");
                    s.reset();
                    expect(same_bits(walk(s, iq, {n / 2, n - n / 2}, fb), want), "pushes longer than max_push_frames");
                }
    // the refusals of the stream's own settings and of a push's pointers
    {
        const aptgpu_fm_settings fm = settings(APTGPU_IQ_S16, 5, 0.);
        aptgpu_fm_stream_settings ss{};
        ss.struct_size = sizeof ss;
        ss.max_push_frames = 1000;
        aptgpu_fm_stream_settings bad = ss;
        bad.struct_size = 8;
        expect(refused(fm, bad, "struct_size"), "struct_size");
        bad = ss;
        bad.max_push_frames = 0;
        expect(refused(fm, bad, "max_push_frames"), "max_push_frames == 0");
        aptgpu_fm_settings bad_fm = fm;
        bad_fm.decimation = 0;
        expect(refused(bad_fm, ss, "decimation"), "what design_of refuses");
        const apt::fm::StreamDesign design = apt::fm::design_stream(&fm, &ss);
        alignas(16) static unsigned char block[64];
        auto push_refused = [&](const void *iq, size_t k, const void *audio, size_t cap, const char *text) {
            try {
                apt::fm::check_push(design, design.fm.T, iq, k, audio, cap, "iq", "audio");
            } catch (const apt::Error &e) {
                return e.kind == apt::ErrorKind::Invalid && e.message.find(text) != std::string::npos;
            }
            return false;
        };
        expect(push_refused(nullptr, 10, block, 2, "iq is null"), "null iq");
        expect(push_refused(block, 10, nullptr, 2, "audio is null"), "null audio");
        expect(push_refused(block + 1, 10, block, 2, "iq is not aligned"), "misaligned iq");
        expect(push_refused(block, 10, block + 2, 2, "audio is not aligned"), "misaligned audio");
        expect(push_refused(block, 10, block, 1, "audio_cap"), "audio_cap");
        expect(!push_refused(block, 10, block, 2, ""), "a fitting push is accepted");
        expect(!push_refused(nullptr, 0, nullptr, 0, ""), "an empty push needs no pointers");
    }
    std::printf(failures ? "fm_stream_host_main: %d check(s) failed\n" : "fm_stream_host_main: ok\n", failures);
    return failures ? 1 : 0;
}
