// landmask_host_main.cpp — a stand-alone program around the CPU side of the land / sea / lake mask (apt_landmask.cpp: the
// settings' checks, the table build, both sources and the colouriser), for sanitizer builds.  No GPU, no library, no
// Python:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include tools/sanitize/landmask_host_main.cpp noaa_apt_amd/csrc/apt_landmask.cpp \
//       noaa_apt_amd/csrc/apt_geoloc.cpp noaa_apt_amd/csrc/apt_map.cpp -o landmask_host_main
//   ./landmask_host_main
//
// Every buffer is allocated at exactly its size, so a read or write one element past it is a report.  Synthetic layers
// (a ring with a hole, an unclosed part, a one-vertex part, a horizontal edge, a lake), band counts 1, 7, 720 and 7200,
// planes with NaN and infinite points, heights 2, 5 and 263, the failing records and the refusals; it checks only what
// must hold whatever the numbers are: every band count gives the same mask, the counts add up, the swath form equals
// the plane form of the geolocation twin's points.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <vector>

#include "../../noaa_apt_amd/csrc/apt_kernels_landmask.hpp"

namespace {

namespace geo = apt::geoloc;
namespace lm = apt::landmask;

int failures = 0;
void expect(bool ok, const char *what, size_t a = 0, size_t b = 0)
{
    if (ok) return;
    std::fprintf(stderr, "FAILED: %s (%zu, %zu)\n", what, a, b);
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

void add_part(apt::map::Layer &l, std::initializer_list<double> xy)
{
    l.xy.insert(l.xy.end(), xy);
    l.parts.push_back(static_cast<uint32_t>(l.points()));
}

// layers around (lat 51.6, lon -68.8) degrees, where track_of(h, 0.9, -1.2, 3.3) starts
apt::map::Layers layers_of()
{
    apt::map::Layer co, la;
    add_part(co, {-75, 40, -60, 40, -60, 56, -75, 56, -75, 40});          // a box ...
    add_part(co, {-72, 44, -64, 44, -64, 53, -72, 53, -72, 44});          // ... with a hole
    add_part(co, {-70, 46, -66, 46, -66, 50, -70, 50});                   // an island in the hole, unclosed
    add_part(co, {-50, 30});                                              // one vertex: no edge
    add_part(co, {-90, 89.9, 0, 90, 90, 90, 180, 89.9, 0, 85, -90, 89.9}); // up to the pole
    add_part(la, {-69, 47, -67, 47, -67, 49, -69, 49, -69, 47});
    add_part(la, {-180, -10, -170, -10, -170, 10, -180, 10});             // abuts the antimeridian
    apt::map::Layers layers;
    layers.set(apt::map::Layers::kCountries, std::move(co));
    layers.set(apt::map::Layers::kLakes, std::move(la));
    return layers;
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

void check_counts(const aptgpu_land_mask_result &r, const uint8_t *mask, size_t n, const char *what)
{
    uint64_t c[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < n; ++i) {
        expect(mask[i] <= 2 || mask[i] == 255, "class value", i, mask[i]);
        c[mask[i] == 255 ? 3 : mask[i] & 3] += 1;
    }
    expect(r.n_sea == c[0] && r.n_land == c[1] && r.n_lake == c[2] && r.n_invalid == c[3], what, n);
}

void run_swath(const apt::map::Layers &layers, size_t h)
{
    const size_t px = h * 909;
    const std::vector<double> track = track_of(h, 0.9, -1.2, 3.3);
    aptgpu_map_settings ms{sizeof(aptgpu_map_settings), 0, 0.02, 0.95, 1.05};
    const geo::Geom g = geo::check_geom(&ms);
    // the twin's own points, for the plane form
    std::unique_ptr<double[]> latlon(new double[2 * px]);
    aptgpu_geoloc_result gi{};
    gi.struct_size = sizeof gi;
    geo::run_host(nullptr, h * 2080, track.data(), h, g, geo::Settings{0, false, 0, 0.f, 0.f}, latlon.get(), nullptr, nullptr, &gi);
    std::unique_ptr<uint8_t[]> first;
    for (int nb : {1, 7, 720, 7200}) {
        const lm::Table t = lm::build_table(layers, nb);
        expect(t.off.size() == 2 * static_cast<size_t>(nb) + 1 && t.off.back() == t.edges.size(), "table shape", nb);
        std::unique_ptr<uint8_t[]> swath(new uint8_t[px]), plane(new uint8_t[px]);
        aptgpu_land_mask_result a{}, b = lm::first_record(t, 0);
        a.struct_size = sizeof a;
        lm::run_swath_host(t, h, track.data(), h, g, swath.get(), &a);
        lm::run_plane_host(t, latlon.get(), px, plane.get(), &b);
        expect(a.status == 0 && a.height == h, "record", h, nb);
        check_counts(a, swath.get(), px, "swath counts");
        check_counts(b, plane.get(), px, "plane counts");
        for (size_t i = 0; i < px; ++i) expect(swath[i] == plane[i], "swath == plane", i, nb);
        if (first)
            for (size_t i = 0; i < px; ++i) expect(swath[i] == first[i], "band count changes nothing", i, nb);
        else
            first = std::move(swath);
    }
    if (h >= 263) {
        bool seen[3] = {false, false, false};
        for (size_t i = 0; i < px; ++i)
            if (first[i] <= 2) seen[first[i]] = true;
        expect(seen[0] && seen[1] && seen[2], "all three classes", h);
    }
}

void run_plane_edges(const apt::map::Layers &layers)
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double rad = 1. / lm::kDeg;
    // points on vertices, on a horizontal edge's latitude, at the pole, on the antimeridian, non-finite
    const std::vector<double> pts = {44 * rad, -72 * rad, 40 * rad, -70 * rad, 90 * rad, 0, -90 * rad, 0, 0, 180 * rad, 0, -180 * rad,
                                     nan, 0, 0, nan, inf, 0, -inf, 0, 0, inf, 0, -inf, 48 * rad, -68 * rad, 45 * rad, -65 * rad,
                                     41 * rad, -61 * rad};
    const size_t n = pts.size() / 2;
    std::unique_ptr<double[]> ll(new double[2 * n]);
    for (size_t i = 0; i < 2 * n; ++i) ll[i] = pts[i];
    std::unique_ptr<uint8_t[]> first;
    for (int nb : {1, 7, 720, 7200}) {
        const lm::Table t = lm::build_table(layers, nb);
        std::unique_ptr<uint8_t[]> mask(new uint8_t[n]);
        aptgpu_land_mask_result r = lm::first_record(t, 0);
        lm::run_plane_host(t, ll.get(), n, mask.get(), &r);
        check_counts(r, mask.get(), n, "edge points");
        expect(mask[6] == 255 && mask[7] == 255 && r.n_invalid == 2, "NaN is invalid", nb);
        expect(mask[12] == lm::kLake && mask[13] == lm::kSea && mask[14] == lm::kLand, "lake, hole, land", nb);
        if (first)
            for (size_t i = 0; i < n; ++i) expect(mask[i] == first[i], "band count changes nothing (edge points)", i, nb);
        else
            first = std::move(mask);
    }
    const lm::Table t = lm::build_table(layers, 720);
    aptgpu_land_mask_result r = lm::first_record(t, 0);
    lm::run_plane_host(t, nullptr, 0, nullptr, &r);  // an empty plane reads and writes nothing
    expect(r.n_sea + r.n_land + r.n_lake + r.n_invalid == 0, "empty plane");
}

void run_color(size_t h)
{
    const size_t px = h * 2080, mpx = h * 909;
    std::unique_ptr<uint8_t[]> image(new uint8_t[px]), mask(new uint8_t[mpx]), out(new uint8_t[4 * px]);
    std::unique_ptr<uint8_t[]> pal[3];
    const uint8_t *pals[3];
    for (int c = 0; c < 3; ++c) {
        pal[c].reset(new uint8_t[lm::kPaletteBytes]);
        for (int i = 0; i < lm::kPaletteBytes; ++i) pal[c][i] = static_cast<uint8_t>((i * 31 + c * 97) & 255);
        pals[c] = pal[c].get();
    }
    const uint8_t classes[4] = {0, 1, 2, 255};
    for (size_t i = 0; i < px; ++i) image[i] = static_cast<uint8_t>((i * 7919u) & 255u);
    for (size_t i = 0; i < mpx; ++i) mask[i] = classes[(i * 13u) & 3u];
    const float tunes[4] = {0.1f, -0.2f, 0.3f, 0.15f};
    lm::false_color_masked_host(image.get(), h, mask.get(), pals, tunes, out.get());
    for (size_t y = 0; y < h; ++y)
        for (size_t x = 0; x < 2080; ++x) {
            const size_t i = y * 2080 + x;
            const bool gray = x < 86 || x >= 995 || mask[y * 909 + (x < 86 ? 0 : x - 86 < 909 ? x - 86 : 0)] == 255;
            expect(out[4 * i + 3] == 255, "alpha", y, x);
            if (gray) expect(out[4 * i] == image[i] && out[4 * i + 1] == image[i] && out[4 * i + 2] == image[i], "gray", y, x);
        }
}

}  // namespace

int main()
{
    const apt::map::Layers layers = layers_of();
    for (size_t h : {size_t(2), size_t(5), size_t(263)}) run_swath(layers, h);
    run_plane_edges(layers);
    for (size_t h : {size_t(1), size_t(2), size_t(120)}) run_color(h);

    // the failing records: nothing may be written
    const lm::Table t = lm::build_table(layers, 720);
    const std::vector<double> track = track_of(5, 0.2, 0.3, 0.1);
    aptgpu_land_mask_result info{};
    info.struct_size = sizeof info;
    expect(throws([&] { lm::run_swath_host(t, 1, track.data(), 1, geo::Geom{}, nullptr, &info); }) &&
               info.reason == geo::kReasonHeight && info.height == 1, "h = 1");
    expect(throws([&] { lm::run_swath_host(t, 5, track.data(), 4, geo::Geom{}, nullptr, &info); }) &&
               info.reason == geo::kReasonCount, "count");
    // the refusals
    aptgpu_land_mask_settings s{sizeof(aptgpu_land_mask_settings), 0, 720, 0};
    expect(lm::check_settings(&s) == 720 && lm::check_settings(nullptr) == lm::kDefaultBands, "settings");
    for (int nb : {0, -1, 7201}) {
        aptgpu_land_mask_settings bad = s;
        bad.n_bands = nb;
        expect(throws([&] { lm::check_settings(&bad); }), "n_bands");
    }
    aptgpu_land_mask_settings bad = s;
    bad.struct_size = 8;
    expect(throws([&] { lm::check_settings(&bad); }), "struct_size");
    bad = s;
    bad.flags = 2;
    expect(throws([&] { lm::check_settings(&bad); }), "flags");
    expect(throws([&] { lm::build_table(apt::map::Layers{}, 720); }), "empty layer set");
    apt::map::Layers nf;
    apt::map::Layer l;
    add_part(l, {0, 0, 1, std::numeric_limits<double>::quiet_NaN(), 1, 1});
    nf.set(apt::map::Layers::kLakes, std::move(l));
    expect(throws([&] { lm::build_table(nf, 720); }), "non-finite vertex");
    // a short record of an older caller
    aptgpu_land_mask_result small{};
    small.struct_size = 16;
    small.n_sea = 77;
    std::unique_ptr<uint8_t[]> mask(new uint8_t[2 * 909]);
    const std::vector<double> track2 = track_of(2, 0.9, -1.2, 3.3);
    lm::run_swath_host(t, 2, track2.data(), 2, geo::Geom{}, mask.get(), &small);
    expect(small.height == 2 && small.n_sea == 77, "short record");
    if (failures) return 1;
    std::puts("landmask_host_main: ok");
    return 0;
}
