// fit_host_main.cpp — a stand-alone program around the CPU side of the overlay fit (apt_fit.cpp: the settings checks,
// the sampler and run_host), for sanitizer builds.  No GPU, no library, no Python:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include tools/sanitize/fit_host_main.cpp noaa_apt_amd/csrc/apt_fit.cpp noaa_apt_amd/csrc/apt_geoloc.cpp \
//       noaa_apt_amd/csrc/apt_map.cpp -o fit_host_main
//   ./fit_host_main
//
// The image, the track and the trace are allocated at exactly their sizes, so an access one element past any of them is
// a report.  A synthetic layer set (a graticule around the track, with a one-vertex part and a short segment) over
// a noise image, heights 16 and 70, both channels, margins 0 and 5, a box radius that exceeds
// the image, the flat image, the failing records and the refusals; it checks only what must hold whatever the numbers
// are.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../noaa_apt_amd/csrc/apt_kernels_fit.hpp"

namespace {

namespace fit = apt::fit;

int failures = 0;
void expect(bool ok, const char *what, size_t h)
{
    if (ok) return;
    std::fprintf(stderr, "FAILED: %s (h = %zu)\n", what, h);
    ++failures;
}

// a great circle from (lat0, lon0) heading az, one row every 0.5 s at 850 km
std::vector<double> track_of(size_t rows, double lat0, double lon0, double az)
{
    const double omega = std::sqrt(398600.4418 / std::pow(6371.0 + 850.0, 3));
    std::vector<double> t(2 * rows);
    for (size_t i = 0; i < rows; ++i) {
        const double d = omega * 0.5 * static_cast<double>(i);
        const double lat = std::asin(std::sin(lat0) * std::cos(d) + std::cos(lat0) * std::sin(d) * std::cos(az));
        const double lon = lon0 + std::atan2(std::sin(az) * std::sin(d) * std::cos(lat0), std::cos(d) - std::sin(lat0) * std::sin(lat));
        t[2 * i] = lat;
        t[2 * i + 1] = lon;
    }
    return t;
}

// meridians and parallels every 0.4 degrees around (lat, lon) in degrees, a one-vertex part and a short segment
apt::map::Layers graticule(double lat, double lon)
{
    apt::map::Layer l;
    auto part = [&](std::initializer_list<double> xy) {
        l.xy.insert(l.xy.end(), xy);
        l.parts.push_back(static_cast<uint32_t>(l.xy.size() / 2));
    };
    for (int i = -12; i <= 12; ++i) {
        part({lon + 0.4 * i, lat - 6., lon + 0.4 * i, lat, lon + 0.4 * i, lat + 6.});
        part({lon - 6., lat + 0.4 * i, lon + 6., lat + 0.4 * i});
    }
    part({lon, lat});
    part({lon + 0.01, lat + 0.01, lon + 0.02, lat + 0.01});
    apt::map::Layers layers;
    layers.set(apt::map::Layers::kCountries, l);
    return layers;
}

aptgpu_fit_settings settings_of(int channel, int margin, int rounds, int radius)
{
    aptgpu_fit_settings s{};
    s.struct_size = sizeof s;
    s.channel = channel;
    s.margin_rows = margin;
    s.rounds = rounds;
    s.radius = radius;
    s.min_points = 8;
    s.shift_step = 2;
    s.n_shift = 2;
    s.n_yaw = s.n_hscale = s.n_vscale = 1;
    s.yaw_step = 0.02;
    s.hscale_step = s.vscale_step = 0.04;
    s.spacing_deg = 0.05;
    return s;
}

void run(size_t h, int channel, int margin, int rounds, int radius, bool flat)
{
    const aptgpu_fit_settings cs = settings_of(channel, margin, rounds, radius);
    const fit::Settings st = fit::check_settings(&cs);
    const size_t rows = h + 2 * static_cast<size_t>(margin);
    const std::vector<double> track = track_of(rows, -0.7, -1.1, 0.15);
    const apt::map::Layers layers = graticule(-0.7 * 180. / fit::kPi, -1.1 * 180. / fit::kPi);
    const std::vector<double> points = fit::sample_points(layers, st.mask, st.spacing);
    expect(points.size() / 2 > 1000, "sample points", h);
    std::unique_ptr<uint8_t[]> image(new uint8_t[h * 2080]);
    for (size_t i = 0; i < h * 2080; ++i) image[i] = flat ? 90 : static_cast<uint8_t>(90 + (i * 7919u) % 50u);
    const size_t n = static_cast<size_t>(st.rounds) * st.grid.total();
    std::unique_ptr<fit::Sum[]> scores(new fit::Sum[n]);
    aptgpu_fit_result info{};
    info.struct_size = sizeof info;
    aptgpu_map_settings ms{sizeof(aptgpu_map_settings), 0, 0.01, 1.02, 0.98};
    fit::run_host(image.get(), h, track.data(), rows, points, apt::geoloc::check_geom(&ms), st, scores.get(), &info);
    expect(info.status == 0 && info.height == h && info.done == 1, "record", h);
    expect(info.n_points == points.size() / 2 && info.n_candidates == st.grid.total(), "counts", h);
    if (flat) {
        expect(info.reason == fit::kReasonFlat && info.n_rounds == 1 && info.yaw == 0.01 && info.shift_rows == 0, "flat", h);
    } else {
        expect(info.reason == 0 && info.n_rounds == static_cast<uint32_t>(rounds), "rounds", h);
        expect(std::abs(info.shift_rows) <= margin && info.time_offset_ms == 500 * info.shift_rows, "shift", h);
        expect(info.count >= st.min_points && info.q > 0., "winner", h);
    }
    for (size_t i = 0; i < n; ++i)
        expect(scores[i].zero == 0 && (scores[i].count >= st.min_points || (scores[i].count == 0 && scores[i].score == 0)),
               "trace", h);
}

template <typename Fn>
bool throws(Fn &&fn)
{
    try {
        fn();
    } catch (const apt::Error &) {
        return true;
    }
    return false;
}

}  // namespace

int main()
{
    run(16, 0, 0, 1, 0, false);
    run(16, 1, 5, 2, 32, false);  // the box is wider than the image is high
    run(70, 1, 5, 3, 2, false);
    run(70, 0, 5, 2, 1, true);

    // the failing records and the refusals
    const aptgpu_fit_settings cs = settings_of(0, 5, 2, 1);
    const fit::Settings st = fit::check_settings(&cs);
    const std::vector<double> track = track_of(40, 0.2, 0.3, 0.1);
    std::vector<uint8_t> image(30 * 2080, 7);
    aptgpu_fit_result info{};
    info.struct_size = sizeof info;
    expect(throws([&] { fit::run_host(image.data(), 30, track.data(), 39, {}, apt::geoloc::Geom{}, st, nullptr, &info); }) &&
               info.reason == apt::geoloc::kReasonCount, "count", 30);
    expect(throws([&] { fit::run_host(image.data(), 30, track.data(), 40, {}, apt::geoloc::Geom{}, st, nullptr, &info); }) &&
               info.reason == fit::kReasonNoCandidate && info.n_rounds == 1, "no points", 30);
    expect(throws([&] { fit::check_call(nullptr, nullptr, 30, st); }), "neither", 30);
    expect(throws([&] { fit::check_call(&info, nullptr, 15, st); }), "h = 15", 15);
    aptgpu_fit_settings bad = cs;
    bad.struct_size = 8;
    expect(throws([&] { fit::check_settings(&bad); }), "struct_size", 0);
    bad = cs;
    bad.radius = 33;
    expect(throws([&] { fit::check_settings(&bad); }), "radius", 0);
    bad = cs;
    bad.n_shift = bad.n_yaw = bad.n_hscale = bad.n_vscale = 16;
    expect(throws([&] { fit::check_settings(&bad); }), "candidates", 0);
    expect(throws([&] { fit::sample_points(graticule(0., 0.), 2u, 1e-6); }), "point cap", 0);
    // a short record of an older caller
    aptgpu_fit_result small{};
    small.struct_size = 16;
    small.n_rounds = 77;
    const std::vector<double> t16 = track_of(16, -0.7, -1.1, 0.15);
    const aptgpu_fit_settings c0 = settings_of(0, 0, 1, 0);
    fit::run_host(std::vector<uint8_t>(16 * 2080, 9).data(), 16, t16.data(), 16,
                  fit::sample_points(graticule(-0.7 * 180. / fit::kPi, -1.1 * 180. / fit::kPi), 2u, 0.05), apt::geoloc::Geom{},
                  fit::check_settings(&c0), nullptr, &small);
    expect(small.height == 16 && small.n_rounds == 77, "short record", 16);
    if (failures) return 1;
    std::puts("fit_host_main: ok");
    return 0;
}
