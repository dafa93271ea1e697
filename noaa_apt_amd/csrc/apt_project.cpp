// apt_project.cpp — host side of the reprojection (apt_project.hpp): the checks of aptgpu_projection_settings, the
// per-call values, the graticule's rows and columns and aptgpu_projection_fit, all with the C library's f64 libm
// (tests/np_project_model.py restates them with Python's math, the same library).
#include "apt_project.hpp"

#include <cmath>
#include <string>

#include "apt_host.hpp"

namespace apt::project {

namespace {

constexpr double kPi = 3.14159265358979323846;

[[noreturn]] void invalid(const std::string &msg)
{
    throw Error{ErrorKind::Invalid, "aptgpu_projection_settings: " + msg};
}

double rad(double deg) { return deg / 180. * kPi; }  // map.rs:144

}  // namespace

Grid checked(const aptgpu_projection_settings *p)
{
    if (!p || p->struct_size < sizeof(aptgpu_projection_settings)) invalid("struct_size not set");
    if (p->kind != APTGPU_PROJECTION_EQUIRECTANGULAR && p->kind != APTGPU_PROJECTION_MERCATOR) invalid("unknown kind");
    if (p->channel != APTGPU_PROJECTION_CHANNEL_A && p->channel != APTGPU_PROJECTION_CHANNEL_B)
        invalid("unknown channel");
    if (p->sampling != APTGPU_SAMPLING_NEAREST && p->sampling != APTGPU_SAMPLING_BILINEAR) invalid("unknown sampling");
    if (p->width < 1 || p->height < 1) invalid("width and height must be at least 1");
    if (static_cast<uint64_t>(p->width) * p->height > kMaxPixels)
        invalid("width * height exceeds APTGPU_PROJECTION_MAX_PIXELS (2^26)");
    if (!std::isfinite(p->step) || !(p->step > 0.)) invalid("step must be finite and > 0");
    if (!(std::fabs(p->lat_north) <= 90.)) invalid("lat_north must be within [-90, 90]");
    if (!std::isfinite(p->lon_west)) invalid("lon_west must be finite");
    if (p->kind == APTGPU_PROJECTION_EQUIRECTANGULAR &&
        !(std::fabs(p->lat_north - static_cast<double>(p->height - 1) * p->step) <= 90.))
        invalid("the last row's latitude must be within [-90, 90]");
    if (!std::isfinite(p->grid_deg) || p->grid_deg < 0.) invalid("grid_deg must be finite and >= 0");
    if (p->grid_deg > 0. && p->grid_deg < p->step) invalid("grid_deg must be 0 or at least step");
    if (p->reserved) invalid("reserved must be 0");
    Grid g{};
    g.kind = p->kind;
    g.channel = p->channel;
    g.sampling = p->sampling;
    g.graticule = p->grid_deg > 0. ? 1 : 0;
    g.width = p->width;
    g.height = p->height;
    g.lat_north = p->lat_north;
    g.lon_west = p->lon_west;
    g.step = p->step;
    g.y_north = std::asinh(std::tan(rad(p->lat_north)));
    g.step_rad = rad(p->step);
    g.grid_color = uint32_t(p->grid_color[0]) | (uint32_t(p->grid_color[1]) << 8) | (uint32_t(p->grid_color[2]) << 16) |
                   (uint32_t(p->grid_color[3]) << 24);
    return g;
}

std::vector<uint8_t> graticule(const Grid &g, double grid_deg)
{
    std::vector<uint8_t> flags;
    if (!(grid_deg > 0.)) return flags;
    flags.assign(static_cast<size_t>(g.width) + g.height, 0);
    // columns: the meridians m * grid_deg inside [lon_west, lon_west + (width - 1) * step], one more on each side
    const double lon_east = g.lon_west + static_cast<double>(g.width - 1) * g.step;
    const double m0 = std::floor(g.lon_west / grid_deg) - 1., m1 = std::ceil(lon_east / grid_deg) + 1.;
    for (double m = m0; m <= m1; m += 1.) {
        const double col = std::floor((m * grid_deg - g.lon_west) / g.step + 0.5);
        if (col >= 0. && col < static_cast<double>(g.width)) flags[static_cast<size_t>(col)] = 1;
    }
    // rows: the parallels m * grid_deg short of the poles
    const double n1 = std::floor(90. / grid_deg);
    for (double m = -n1; m <= n1; m += 1.) {
        const double lat = m * grid_deg;
        if (!(std::fabs(lat) < 90.)) continue;
        const double row = g.kind == APTGPU_PROJECTION_MERCATOR
                               ? std::floor((g.y_north - std::asinh(std::tan(rad(lat)))) / g.step_rad + 0.5)
                               : std::floor((g.lat_north - lat) / g.step + 0.5);
        if (row >= 0. && row < static_cast<double>(g.height)) flags[g.width + static_cast<size_t>(row)] = 1;
    }
    return flags;
}

void fit(const double *track, size_t count, double hscale, int kind, double step_deg, uint32_t max_width,
         aptgpu_projection_settings *out)
{
    fit_many(&track, &count, 1, hscale, kind, step_deg, max_width, out);
}

void fit_many(const double *const *tracks, const size_t *counts, size_t n_tracks, double hscale, int kind,
              double step_deg, uint32_t max_width, aptgpu_projection_settings *out)
{
    auto bad = [](const char *msg) { throw Error{ErrorKind::Invalid, std::string("aptgpu_projection_fit: ") + msg}; };
    if (kind != APTGPU_PROJECTION_EQUIRECTANGULAR && kind != APTGPU_PROJECTION_MERCATOR) bad("unknown kind");
    if (n_tracks == 0) bad("no track");
    for (size_t t = 0; t < n_tracks; ++t)
        if (counts[t] == 0) bad("the track is empty");
    const double *track = tracks[0];
    if (!std::isfinite(hscale) || !(hscale > 0.)) bad("hscale must be finite and > 0");
    const bool by_step = step_deg > 0.;
    if (by_step ? !std::isfinite(step_deg) : max_width < 2) bad("give a step > 0 or a maximum width of at least 2");
    double lat_min = track[0], lat_max = track[0], lon = track[1], lon_min = lon, lon_max = lon;
    double abs_max = std::fabs(track[0]);
    for (size_t t = 0; t < n_tracks; ++t) {
        track = tracks[t];
        for (size_t r = 0; r < counts[t]; ++r) {
            const double lat = track[2 * r];
            if (!std::isfinite(lat) || !std::isfinite(track[2 * r + 1])) bad("the track holds a non-finite position");
            if (r || t) {
                // a later track starts from the first track's first longitude: one unwrapped axis for all of them
                const double from = r ? track[2 * r - 1] : tracks[0][1];
                if (!r) lon = from;
                double d = std::fmod(track[2 * r + 1] - from, 2. * kPi);
                if (d > kPi) d -= 2. * kPi;
                if (d < -kPi) d += 2. * kPi;
                lon += d;
            }
            lat_min = std::fmin(lat_min, lat);
            lat_max = std::fmax(lat_max, lat);
            lon_min = std::fmin(lon_min, lon);
            lon_max = std::fmax(lon_max, lon);
            abs_max = std::fmax(abs_max, std::fabs(lat));
        }
    }
    const double half = 456. * 0.0005 / hscale;  // the swath's half angle (map.rs:64, the band of map.rs:116-121)
    const double lat_cap = (kind == APTGPU_PROJECTION_MERCATOR ? 85. : 90.) / 180. * kPi;
    lat_min = std::fmax(lat_min - half, -lat_cap);
    lat_max = std::fmin(lat_max + half, lat_cap);
    if (lat_min > lat_max) lat_min = lat_max;  // (a track beyond the Mercator cap: one row at the cap)
    const double c = std::cos(abs_max);
    const double grow = c > 0. ? half / c : 2. * kPi;
    lon_min -= grow;
    lon_max += grow;
    if (!(lon_max - lon_min <= 2. * kPi)) {
        const double mid = 0.5 * (lon_min + lon_max);
        lon_min = mid - kPi;
        lon_max = mid + kPi;
    }
    const double span = (lon_max - lon_min) * 180. / kPi;
    const double step = by_step ? step_deg : span / static_cast<double>(max_width - 1);
    if (!(step > 0.)) bad("the fitted step is not positive");
    const double cap_deg = kind == APTGPU_PROJECTION_MERCATOR ? 85. : 90.;  // (the conversion back may round past it)
    const double north = std::fmin(lat_max * 180. / kPi, cap_deg), south = std::fmax(lat_min * 180. / kPi, -cap_deg);
    const double width = std::floor(span / step + 0.5) + 1.;
    // equirectangular: the last row never lies south of `south` (so never past the pole)
    const double rows =
        kind == APTGPU_PROJECTION_MERCATOR
            ? std::floor((std::asinh(std::tan(rad(north))) - std::asinh(std::tan(rad(south)))) / rad(step) + 0.5) + 1.
            : std::floor((north - south) / step) + 1.;
    if (!(width * rows <= static_cast<double>(kMaxPixels))) bad("the fitted grid exceeds APTGPU_PROJECTION_MAX_PIXELS (2^26)");
    *out = aptgpu_projection_settings{};
    out->struct_size = sizeof(aptgpu_projection_settings);
    out->kind = kind;
    out->width = static_cast<uint32_t>(width);
    out->height = static_cast<uint32_t>(rows);
    out->lat_north = north;
    out->lon_west = lon_min * 180. / kPi;
    out->step = step;
    out->channel = APTGPU_PROJECTION_CHANNEL_A;
    out->sampling = APTGPU_SAMPLING_NEAREST;
    out->grid_deg = 0.;
}

}  // namespace apt::project
