// geoloc_host_main.cpp — a stand-alone program around the CPU side of the geolocation stage (apt_geoloc.cpp: the
// settings checks, the sun and run_host), for sanitizer builds.  No GPU, no library, no Python:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include tools/sanitize/geoloc_host_main.cpp noaa_apt_amd/csrc/apt_geoloc.cpp noaa_apt_amd/csrc/apt_map.cpp \
//       -o geoloc_host_main
//   ./geoloc_host_main
//
// Every plane is allocated at exactly its size, so a write one element past it is a report.  Heights 2, 5 and 263,
// every output mask, out of place and in place, both channels, the failing records; it checks only what must hold
// whatever the numbers are.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../noaa_apt_amd/csrc/apt_kernels_geoloc.hpp"

namespace {

namespace geo = apt::geoloc;

int failures = 0;
void expect(bool ok, const char *what, size_t h, unsigned mask)
{
    if (ok) return;
    std::fprintf(stderr, "FAILED: %s (h = %zu, mask = %u)\n", what, h, mask);
    ++failures;
}

// a great circle from (lat0, lon0) heading az, one row every 0.5 s at 850 km
std::vector<double> track_of(size_t h, double lat0, double lon0, double az)
{
    const double omega = std::sqrt(398600.4418 / std::pow(6371.0 + 850.0, 3));
    std::vector<double> t(2 * h);
    for (size_t i = 0; i < h; ++i) {
        const double d = omega * 0.5 * static_cast<double>(i);
        const double lat = std::asin(std::sin(lat0) * std::cos(d) + std::cos(lat0) * std::sin(d) * std::cos(az));
        const double lon = lon0 + std::atan2(std::sin(az) * std::sin(d) * std::cos(lat0), std::cos(d) - std::sin(lat0) * std::sin(lat));
        t[2 * i] = lat;
        t[2 * i + 1] = lon;
    }
    return t;
}

aptgpu_geoloc_settings settings_of(int channel, int kind)
{
    aptgpu_geoloc_settings s{};
    s.struct_size = sizeof s;
    s.channel = channel;
    s.time_kind = kind;
    s.unix_ms = 1730635200000LL;
    s.black_level = 1500.f;
    s.max_zenith_deg = 80.f;
    return s;
}

void run(size_t h, unsigned mask, bool in_place, int channel)
{
    const size_t n = h * 2080 + 3;  // (a few floats behind the last whole row: copied, never normalised)
    const size_t px = h * 909;
    std::unique_ptr<float[]> x(new float[n]);
    for (size_t i = 0; i < n; ++i) x[i] = 1200.f + static_cast<float>((i * 7919u) % 9000u);
    const std::vector<double> track = track_of(h, 0.9, -1.2, 3.3);
    std::unique_ptr<double[]> latlon((mask & geo::kOutLatLon) ? new double[2 * px] : nullptr);
    std::unique_ptr<float[]> cos_sun((mask & geo::kOutCos) ? new float[px] : nullptr);
    std::unique_ptr<float[]> rows((mask & geo::kOutRows) && !in_place ? new float[n] : nullptr);
    float *rows_p = (mask & geo::kOutRows) ? (in_place ? x.get() : rows.get()) : nullptr;
    aptgpu_map_settings ms{sizeof(aptgpu_map_settings), 0, 0.02, 0.95, 1.05};
    const aptgpu_geoloc_settings cs = settings_of(channel, h % 2 ? APTGPU_REF_TIME_END : APTGPU_REF_TIME_START);
    aptgpu_geoloc_result info{};
    info.struct_size = sizeof info;
    geo::run_host(x.get(), n, track.data(), h, geo::check_geom(&ms), geo::check_settings(&cs), latlon.get(), cos_sun.get(),
                  rows_p, &info);
    expect(info.status == 0 && info.height == h, "record", h, mask);
    expect(info.n_outside == 0 && info.cos_min <= info.cos_max, "counters", h, mask);
    if (cos_sun)
        for (size_t i = 0; i < px; ++i) expect(cos_sun[i] >= -1.f && cos_sun[i] <= 1.f, "cos_sun in [-1, 1]", h, mask);
    if (latlon)
        for (size_t i = 0; i < px; ++i)
            expect(std::fabs(latlon[2 * i]) <= geo::kPi / 2 && std::fabs(latlon[2 * i + 1]) <= geo::kPi, "lat / lon range", h, mask);
    if (rows_p && !in_place) {
        const int base = 1040 * channel + 86;
        for (size_t r = 0; r < h; ++r)
            for (int c = 0; c < 2080; ++c)
                if (c < base || c >= base + 909) expect(rows_p[r * 2080 + c] == x[r * 2080 + c], "outside the video", h, mask);
        for (size_t i = h * 2080; i < n; ++i) expect(rows_p[i] == x[i], "tail", h, mask);
    }
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
    for (size_t h : {size_t(2), size_t(5), size_t(263)})
        for (unsigned mask = 0; mask < 8; ++mask)
            for (int in_place = 0; in_place < 2; ++in_place)
                run(h, mask, in_place != 0, static_cast<int>((h + mask) % 2));

    // the failing records: nothing may be written
    const std::vector<double> track = track_of(5, 0.2, 0.3, 0.1);
    const aptgpu_geoloc_settings cs = settings_of(0, APTGPU_REF_TIME_START);
    const geo::Settings st = geo::check_settings(&cs);
    aptgpu_geoloc_result info{};
    info.struct_size = sizeof info;
    expect(throws([&] { geo::run_host(nullptr, 2080, track.data(), 1, geo::Geom{}, st, nullptr, nullptr, nullptr, &info); }) &&
               info.reason == geo::kReasonHeight, "h = 1", 1, 0);
    expect(throws([&] { geo::run_host(nullptr, 5 * 2080, track.data(), 4, geo::Geom{}, st, nullptr, nullptr, nullptr, &info); }) &&
               info.reason == geo::kReasonCount, "count", 5, 0);
    expect(throws([&] { geo::run_host(nullptr, 0, nullptr, 0, geo::Geom{}, st, nullptr, nullptr, nullptr, nullptr); }), "h = 0", 0, 0);
    aptgpu_geoloc_settings bad = cs;
    bad.max_zenith_deg = 90.f;
    expect(throws([&] { geo::check_settings(&bad); }), "max_zenith_deg", 0, 0);
    bad = cs;
    bad.struct_size = 8;
    expect(throws([&] { geo::check_settings(&bad); }), "struct_size", 0, 0);
    expect(throws([&] { geo::check_call(nullptr, nullptr, false, false, 2); }), "neither", 0, 0);
    double sun[2];
    geo::sun_position(946728000000LL, sun);
    expect(std::fabs(sun[0] * 180. / geo::kPi + 23.0334) < 1e-3 && std::fabs(sun[1] * 180. / geo::kPi - 0.8252) < 1e-3, "sun", 0, 0);
    // a short record of an older caller
    aptgpu_geoloc_result small{};
    small.struct_size = 16;
    small.n_outside = 77;
    geo::run_host(nullptr, 2 * 2080, track.data(), 2, geo::Geom{}, st, nullptr, nullptr, nullptr, &small);
    expect(small.height == 2 && small.n_outside == 77, "short record", 2, 0);
    if (failures) return 1;
    std::puts("geoloc_host_main: ok");
    return 0;
}
