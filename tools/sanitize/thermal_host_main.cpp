// thermal_host_main.cpp — a stand-alone program around the CPU side of the thermal calibration stage
// (apt_thermal.cpp: the settings checks and run_host), for sanitizer builds.  No GPU, no library, no Python:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include tools/sanitize/thermal_host_main.cpp noaa_apt_amd/csrc/apt_thermal.cpp -o thermal_host_main
//   ./thermal_host_main
//
// It builds row images as the tests do (a count scale, a black body, a space view, a ramp in the video), runs every
// channel, identity, image form and failure, the shortest accepted height and one with a frame in the middle, and
// checks only what must hold whatever the numbers are; a sanitizer report is the failure it is for.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../noaa_apt_amd/csrc/apt_kernels_thermal.hpp"

namespace {

std::vector<float> scene(size_t h, size_t frame_row, int identity_wedge)
{
    const double wedges[16] = {31, 63, 95, 127, 159, 191, 224, 255, 0, 104, 105, 106, 105.5, 120, 100, 0};
    std::vector<float> x(h * 2080);
    uint32_t lcg = 12345u;
    for (size_t r = 0; r < h; ++r)
        for (int ch = 0; ch < 2; ++ch) {
            float *row = x.data() + r * 2080 + 1040 * ch;
            const size_t w = ((r + 128 * 8 - frame_row) / 8) % 16;
            const double wedge = w == 15 ? wedges[identity_wedge] : wedges[w];
            for (int c = 0; c < 1040; ++c) {
                lcg = lcg * 1664525u + 1013904223u;
                const double noise = (static_cast<double>(lcg >> 8) / 16777216.0 - 0.5);
                double count = 11.0;
                if (c >= 39 && c < 86) count = 248.0;
                if (c >= 86 && c < 995) count = 40.0 + 212.0 * ((c - 86 + 3 * r) % 909) / 908.0 + noise;
                if (c >= 995) count = wedge + 0.5 * noise;
                row[c] = static_cast<float>(37.5 * count + 1200.0);
            }
        }
    return x;
}

int failures = 0;
void expect(bool ok, const char *what)
{
    if (!ok) {
        std::fprintf(stderr, "FAILED: %s\n", what);
        ++failures;
    }
}

}  // namespace

int main()
{
    aptgpu_thermal_coeffs co{};
    co.struct_size = sizeof co;
    for (int i = 0; i < 4; ++i) {
        co.prt[i][0] = 276.6;
        co.prt[i][1] = 0.0511;
        co.prt[i][2] = 1.4e-6;
    }
    const double sets[3][7] = {{2670.0, 1.70, 0.9975, 0.0, 0.0, 0.0, 0.0},
                               {928.0, 0.55, 0.9985, -5.5, 5.8, -0.11, 0.00052},
                               {834.0, 0.40, 0.9990, -3.5, 2.7, -0.05, 0.00024}};
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 7; ++k) co.channel[i][k] = sets[i][k];
    std::vector<uint8_t> palette(768);
    for (size_t i = 0; i < palette.size(); ++i) palette[i] = static_cast<uint8_t>(i * 7);

    const size_t shapes[3][2] = {{200, 0}, {263, 37}, {199, 0}};
    for (const auto &shape : shapes) {
        const size_t h = shape[0];
        for (int channel = 0; channel < 2; ++channel)
            for (int id = -1; id <= 5; ++id)
                for (int ic : {0, 1, 4}) {
                    const std::vector<float> x = scene(h, shape[1], 3);
                    aptgpu_thermal_settings st{};
                    st.struct_size = sizeof st;
                    st.channel = channel;
                    st.channel_id = id;
                    st.image_channels = ic;
                    st.flags = (id & 1) ? APTGPU_THERMAL_COLD_WHITE : 0u;
                    st.t_low = 180.f;
                    st.t_high = 320.f;
                    st.palette = ic == 4 && channel == 1 ? palette.data() : nullptr;
                    // exactly the planes' sizes: an access past either end is the sanitizer's to report
                    std::vector<float> kelvin(h * 909);
                    std::vector<uint8_t> image(h * 2080 * static_cast<size_t>(ic));
                    aptgpu_thermal_result info{};
                    bool threw = false;
                    try {
                        const apt::thermal::Settings s = apt::thermal::check_settings(&co, &st);
                        apt::thermal::run_host(x.data(), x.size(), co, s, kelvin.data(), ic ? image.data() : nullptr, &info);
                    } catch (const apt::Error &) {
                        threw = true;
                    }
                    const bool thermal_id = id == -1 || id >= 3;
                    if (h < 200)
                        expect(threw && info.reason == 2, "199 rows: reason 2");
                    else if (!thermal_id)
                        expect(threw && info.reason == 13, "not a thermal channel: reason 13");
                    else
                        expect(!threw && info.status == 0 && info.height == h && info.telemetry_row == shape[1] &&
                                   info.t_min <= info.t_max && info.n_nan < h * 909,
                               "a calibrated plane");
                }
    }
    // a NaN thermometer wedge: degenerate
    {
        std::vector<float> x = scene(200, 0, 3);
        x[83 * 2080 + 1000] = std::numeric_limits<float>::quiet_NaN();
        aptgpu_thermal_settings st{};
        st.struct_size = sizeof st;
        st.channel_id = 3;
        st.t_low = 180.f;
        st.t_high = 320.f;
        std::vector<float> kelvin(200 * 909);
        aptgpu_thermal_result info{};
        bool threw = false;
        try {
            apt::thermal::run_host(x.data(), x.size(), co, apt::thermal::check_settings(&co, &st), kelvin.data(), nullptr, &info);
        } catch (const apt::Error &) {
            threw = true;
        }
        expect(threw && info.reason == 14, "NaN wedge: reason 14");
    }
    std::printf(failures ? "thermal_host_main: %d check(s) failed\n" : "thermal_host_main: ok\n", failures);
    return failures ? 1 : 0;
}
