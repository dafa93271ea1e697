// fm_host_main.cpp — a stand-alone program around the CPU side of the FM demodulator (apt_fm.cpp: the settings checks,
// the design and run_host), for sanitizer builds.  No GPU, no library, no Python:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include tools/sanitize/fm_host_main.cpp noaa_apt_amd/csrc/apt_fm.cpp noaa_apt_amd/csrc/apt_host.cpp \
//       -o fm_host_main
//   ./fm_host_main
//
// Every format, with and without a shift and SWAP_IQ, at N in {0, T - 1, T, T + D - 1, T + D, T + D + 1, a few hundred
// outputs}, the input and the output allocated at exactly their sizes (an access past either end is the sanitizer's to
// report), every refusal, and a tone whose demodulated value is known.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../noaa_apt_amd/csrc/apt_kernels_fm.hpp"

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

// a tone f0 above the shift, in the format's components, exactly n frames
std::vector<uint8_t> tone(int format, size_t n, double fs, double hz)
{
    const size_t cb = apt::fm::component_bytes(format);
    std::vector<uint8_t> bytes(n * 2 * cb);
    for (size_t i = 0; i < 2 * n; ++i) {
        const double ph = 2. * 3.14159265358979323846 * hz * static_cast<double>(i / 2) / fs;
        const double v = (i % 2) ? std::sin(ph) : std::cos(ph);
        uint8_t *p = bytes.data() + i * cb;
        if (format == APTGPU_IQ_U8) {
            p[0] = static_cast<uint8_t>(std::lround(127.5 + 100. * v));
        } else if (format == APTGPU_IQ_S8) {
            const int8_t q = static_cast<int8_t>(std::lround(100. * v));
            std::memcpy(p, &q, 1);
        } else if (format == APTGPU_IQ_S16) {
            const int16_t q = static_cast<int16_t>(std::lround(20000. * v));
            std::memcpy(p, &q, 2);
        } else {
            const float q = static_cast<float>(v);
            std::memcpy(p, &q, 4);
        }
    }
    return bytes;
}

bool refused(aptgpu_fm_settings s, const char *field)
{
    try {
        (void)apt::fm::design_of(&s);
    } catch (const apt::Error &e) {
        return e.kind == apt::ErrorKind::Invalid && e.message.find(field) != std::string::npos;
    }
    return false;
}

}  // namespace

int main()
{
    const uint32_t decimations[] = {1, 5, 8};
    for (int format = APTGPU_IQ_U8; format <= APTGPU_IQ_F32; ++format)
        for (uint32_t d : decimations)
            for (int variant = 0; variant < 3; ++variant) {
                aptgpu_fm_settings s = settings(format, d, variant ? -0.13 * 48000. * d : 0.);
                if (variant == 2) s.flags = APTGPU_FM_SWAP_IQ;
                const apt::fm::Design design = apt::fm::design_of(&s);
                const size_t t = design.T;
                const size_t sizes[] = {0, t - 1, t, t + d - 1, t + d, t + d + 1, t + 300 * d + 3};
                for (size_t n : sizes) {
                    const double f0 = 3000.;
                    const std::vector<uint8_t> iq = tone(format, n, 48000. * d, (variant == 2 ? -1. : 1.) * (design.shift_used + f0));
                    const size_t n_out = apt::fm::out_len(design, n);
                    expect(n_out == (n >= t + d ? (n - t) / d : 0), "out_len");
                    std::vector<float> audio(n_out);
                    apt::fm::run_host(design, iq.data(), n, audio.data());
                    if (variant == 2) continue;  // (a mirrored tone stored Q first is another tone: the accesses count)
                    for (float a : audio)
                        if (!(std::fabs(a - static_cast<float>(f0 / 17000.)) < (format <= APTGPU_IQ_S8 ? 2e-2f : 1e-3f))) {
                            expect(false, "a tone demodulates to f0 / deviation");
                            break;
                        }
                }
            }
    // non-finite frames reach the outputs whose windows hold them and no others
    {
        aptgpu_fm_settings s = settings(APTGPU_IQ_F32, 1, 0.);
        const apt::fm::Design design = apt::fm::design_of(&s);
        std::vector<uint8_t> iq = tone(APTGPU_IQ_F32, 200, 48000., 2000.);
        const float nan = std::numeric_limits<float>::quiet_NaN();
        std::memcpy(iq.data() + 8 * 100, &nan, 4);
        std::vector<float> audio(apt::fm::out_len(design, 200));
        apt::fm::run_host(design, iq.data(), 200, audio.data());
        for (size_t m = 0; m < audio.size(); ++m)
            expect((audio[m] != audio[m]) == (m + design.T >= 100 && m <= 100), "NaN window");
    }
    // the refusals
    {
        aptgpu_fm_settings s = settings(APTGPU_IQ_U8, 5, 0.);
        auto with = [&](auto change) {
            aptgpu_fm_settings c = s;
            change(c);
            return c;
        };
        expect(refused(with([](auto &c) { c.struct_size = 8; }), "struct_size"), "struct_size");
        expect(refused(with([](auto &c) { c.format = 7; }), "format"), "format");
        expect(refused(with([](auto &c) { c.flags = 4; }), "flags"), "flags");
        expect(refused(with([](auto &c) { c.sample_rate_hz = 240001; }), "sample_rate_hz"), "fs % D");
        expect(refused(with([](auto &c) { c.decimation = 0; }), "decimation"), "D == 0");
        expect(refused(with([](auto &c) { c.decimation = 4097; c.sample_rate_hz = 4097u * 48000u; }), "decimation"), "D > 4096");
        expect(refused(with([](auto &c) { c.shift_hz = 120001.; }), "shift_hz"), "shift");
        expect(refused(with([](auto &c) { c.shift_hz = std::nan(""); }), "shift_hz"), "shift NaN");
        expect(refused(with([](auto &c) { c.channel_cutout_hz = -1.f; }), "channel_cutout_hz"), "cutout");
        expect(refused(with([](auto &c) { c.channel_delta_hz = 0.f; }), "channel_delta_hz"), "delta");
        expect(refused(with([](auto &c) { c.deviation_hz = std::numeric_limits<float>::infinity(); }), "deviation_hz"), "deviation");
        expect(refused(with([](auto &c) { c.channel_atten = 3.f; }), "channel_atten"), "atten");
        expect(refused(with([](auto &c) { c.channel_cutout_hz = 22000.f; }), "channel_cutout_hz + channel_delta_hz / 2"), "alias");
        expect(refused(with([](auto &c) { c.channel_delta_hz = 100.f; }), "4096 taps"), "taps");
        expect(refused(with([](auto &c) { c.channel_delta_hz = 1e-37f; }), "4096 taps"), "taps, tiny delta");
        expect(!refused(s, ""), "the usual settings are accepted");
    }
    std::printf(failures ? "fm_host_main: %d check(s) failed\n" : "fm_host_main: ok\n", failures);
    return failures ? 1 : 0;
}
