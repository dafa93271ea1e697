// afc_host_main.cpp — a stand-alone program around the CPU side of the AFC (apt_afc.cpp: the settings checks, the
// design, the block sums, the table and the tracked demodulator through apt_fm.cpp), for sanitizer builds.  No GPU, no
// library, no Python:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include tools/sanitize/afc_host_main.cpp noaa_apt_amd/csrc/apt_afc.cpp noaa_apt_amd/csrc/apt_fm.cpp \
//       noaa_apt_amd/csrc/apt_host.cpp -o afc_host_main
//   ./afc_host_main
//
// Every format, B in {64, 4096}, L in {1, 7, 64}, at N in {0, 1, L, L + 1, B - 1, B, B + 1, 3 B + 3, T + a few hundred
// outputs}, every buffer allocated at exactly its size (an access past either end is the sanitizer's to report): the
// sums of the most negative s16 (2^43 per block of 4096: signed overflow is the sanitizer's to report), a tone whose
// carrier the table must find, windows wider than the recording, a NaN frame, and every refusal.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../noaa_apt_amd/csrc/apt_kernels_afc.hpp"

namespace {

int failures = 0;
void expect(bool ok, const char *what)
{
    if (!ok) {
        std::fprintf(stderr, "FAILED: %s\n", what);
        ++failures;
    }
}

aptgpu_fm_settings fm_settings(int format, uint32_t d, double shift)
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

aptgpu_afc_settings afc_settings(uint32_t b, uint32_t lag, uint32_t w)
{
    aptgpu_afc_settings s;
    apt::afc::default_settings(&s);
    s.block_frames = b;
    s.lag = lag;
    s.smooth_blocks = w;
    return s;
}

// a tone at hz, in the format's components, exactly n frames
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

struct Run {
    std::vector<double> sums;
    std::vector<apt::afc::Record> table;
    std::vector<float> coherence, audio;
    std::vector<uint8_t> good;
};
Run run_all(const aptgpu_fm_settings &fs, const aptgpu_afc_settings &as, const std::vector<uint8_t> &iq, size_t n)
{
    const apt::fm::Design fd = apt::fm::design_of(&fs);
    const apt::afc::Design ad = apt::afc::design_of(fd, fs.deviation_hz, &as);
    const uint64_t nb = apt::afc::checked_blocks(ad, n);
    Run r;
    r.sums.resize(3 * nb);
    r.table.resize(nb);
    r.coherence.resize(nb);
    r.good.resize(nb);
    r.audio.resize(apt::fm::out_len(fd, n));
    apt::afc::sums_host(fd, ad, iq.data(), n, r.sums.data());
    apt::afc::table_host(ad, r.sums.data(), nb, r.table.data(), r.coherence.data(), r.good.data());
    apt::afc::tracked_host(fd, ad, iq.data(), n, r.table.data(), r.audio.data());
    return r;
}

bool refused(const aptgpu_afc_settings &as, const char *field)
{
    const aptgpu_fm_settings fs = fm_settings(APTGPU_IQ_U8, 5, 0.);
    try {
        const apt::fm::Design fd = apt::fm::design_of(&fs);
        (void)apt::afc::design_of(fd, fs.deviation_hz, &as);
    } catch (const apt::Error &e) {
        return e.kind == apt::ErrorKind::Invalid && e.message.find(field) != std::string::npos;
    }
    return false;
}

}  // namespace

int main()
{
    const uint32_t blocks[] = {64, 4096}, lags[] = {1, 7, 64};
    for (int format = APTGPU_IQ_U8; format <= APTGPU_IQ_F32; ++format)
        for (uint32_t b : blocks)
            for (uint32_t lag : lags)
                for (int swap = 0; swap < 2; ++swap) {
                    aptgpu_fm_settings fs = fm_settings(format, 5, 2000.);
                    if (swap) fs.flags = APTGPU_FM_SWAP_IQ;
                    const size_t t = apt::fm::design_of(&fs).T;
                    const size_t sizes[] = {0, 1, lag, lag + 1u, b - 1u, b, b + 1u, 3u * b + 3u, t + 300u * 5u + 3u};
                    for (size_t n : sizes) {
                        // the carrier 5 kHz above the shift (stored Q first: the mirrored tone)
                        const std::vector<uint8_t> iq = tone(format, n, 240000., swap ? -7000. : 7000.);
                        const Run r = run_all(fs, afc_settings(b, lag, 15), iq, n);
                        if (n < 3u * b || lag == 64) continue;  // (L = 64 at 240 kS/s: +-1875 Hz, the tone aliases)
                        for (size_t k = 0; k < r.table.size(); ++k) {
                            const double hz = static_cast<double>(static_cast<int32_t>(r.table[k].pw)) * 240000. / 4294967296.;
                            if (!(r.good[k] && std::fabs(hz - 7000.) < 20. && r.coherence[k] > 0.9f)) {
                                expect(false, "the table finds a tone's carrier");
                                break;
                            }
                        }
                    }
                }
    // the most negative s16: 2 * 32768^2 per frame, 2^43 per block; a window of 1023 blocks wider than the recording
    {
        const aptgpu_fm_settings fs = fm_settings(APTGPU_IQ_S16, 5, 0.);
        const size_t n = 3 * 4096;
        std::vector<uint8_t> iq(n * 4);
        const int16_t v = -32768;
        for (size_t i = 0; i < 2 * n; ++i) std::memcpy(iq.data() + 2 * i, &v, 2);
        const Run r = run_all(fs, afc_settings(4096, 1, 1023), iq, n);
        expect(r.sums[2] == 8796093022208. && r.sums[0] == 8796093022208. && r.sums[1] == 0., "2^43 per block");
        expect(r.sums[6] == 4095. * 2147483648., "the last block has one term less");
        expect(r.good[0] && r.table[1].pw == 0 && r.coherence[1] > 0.99f, "a constant is a carrier at 0 Hz");
    }
    // a NaN frame: its window has no estimate and holds its neighbour's
    {
        const aptgpu_fm_settings fs = fm_settings(APTGPU_IQ_F32, 5, 0.);
        const size_t n = 8 * 4096;
        std::vector<uint8_t> iq = tone(APTGPU_IQ_F32, n, 240000., 4000.);
        const float nan = std::numeric_limits<float>::quiet_NaN();
        std::memcpy(iq.data() + 8 * (4 * 4096 + 5), &nan, 4);
        const Run r = run_all(fs, afc_settings(4096, 1, 3), iq, n);
        expect(!r.good[3] && !r.good[4] && !r.good[5] && r.good[2] && r.good[6], "NaN window");
        expect(r.table[4].pw == r.table[2].pw && r.coherence[4] != r.coherence[4], "NaN block holds");
    }
    // the refusals
    {
        auto with = [&](auto change) {
            aptgpu_afc_settings c = afc_settings(4096, 0, 15);
            change(c);
            return c;
        };
        expect(refused(with([](auto &c) { c.struct_size = 8; }), "struct_size"), "struct_size");
        expect(refused(with([](auto &c) { c.block_frames = 32; }), "block_frames"), "B < 64");
        expect(refused(with([](auto &c) { c.block_frames = 96; }), "block_frames"), "B not a power of two");
        expect(refused(with([](auto &c) { c.block_frames = 1u << 21; }), "block_frames"), "B > 2^20");
        expect(refused(with([](auto &c) { c.lag = 65; }), "lag"), "L > 64");
        expect(refused(with([](auto &c) { c.smooth_blocks = 0; }), "smooth_blocks"), "W == 0");
        expect(refused(with([](auto &c) { c.smooth_blocks = 16; }), "smooth_blocks"), "W even");
        expect(refused(with([](auto &c) { c.smooth_blocks = 1025; }), "smooth_blocks"), "W > 1023");
        expect(refused(with([](auto &c) { c.max_offset_hz = 0.f; }), "max_offset_hz"), "max_offset 0");
        expect(refused(with([](auto &c) { c.max_offset_hz = std::nanf(""); }), "max_offset_hz"), "max_offset NaN");
        expect(refused(with([](auto &c) { c.min_coherence = 1.f; }), "min_coherence"), "min_coherence 1");
        expect(refused(with([](auto &c) { c.min_coherence = -0.1f; }), "min_coherence"), "min_coherence < 0");
        expect(refused(with([](auto &c) { c.min_coherence = std::nanf(""); }), "min_coherence"), "min_coherence NaN");
        expect(!refused(afc_settings(4096, 0, 15), ""), "the defaults are accepted");
        try {
            const aptgpu_fm_settings fs = fm_settings(APTGPU_IQ_U8, 5, 0.);
            const aptgpu_afc_settings as = afc_settings(64, 1, 1);
            const apt::fm::Design fd = apt::fm::design_of(&fs);
            (void)apt::afc::checked_blocks(apt::afc::design_of(fd, fs.deviation_hz, &as), (64ull << 20) + 1u);
            expect(false, "more than 2^20 blocks");
        } catch (const apt::Error &) {
        }
    }
    std::printf(failures ? "afc_host_main: %d check(s) failed\n" : "afc_host_main: ok\n", failures);
    return failures ? 1 : 0;
}
