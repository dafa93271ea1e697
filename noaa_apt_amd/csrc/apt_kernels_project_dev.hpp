// apt_kernels_project_dev.hpp — device functions shared by the reprojection (apt_kernels_project.hip) and the composite
// (apt_kernels_composite.hip): the tile, the source fetch, the bilinear channel and steps 2-4 of DESIGN.md §15 for one
// output pixel of one pass.  Both translation units evaluate one source text, so a pass seen through the composite has
// k_project's bits by construction.  Include only from a .hip file, under `#pragma clang fp contract(off)`.
#pragma once

#include "apt_kernels_map_dev.hpp"
#include "apt_project.hpp"

#pragma clang fp contract(off)

namespace apt::project {

namespace {

constexpr int kTileW = 64, kTileH = 4;
constexpr int kThreads = kTileW * kTileH;
constexpr int kPx = 2080;

// one source pixel as RGBA; neighbour indices are clamped to the band's pixels, x in [-455, 455], y in [0, h - 1]
__device__ inline uint32_t fetch(const uint8_t *src, int channels, int base, int h, int x, int y)
{
    x = x < -455 ? -455 : (x > 455 ? 455 : x);
    y = y < 0 ? 0 : (y > h - 1 ? h - 1 : y);
    const size_t at = static_cast<size_t>(y) * kPx + static_cast<size_t>(x + base);
    if (channels == 4) return reinterpret_cast<const uint32_t *>(src)[at];
    const uint32_t g = src[at];
    return g | (g << 8) | (g << 16) | 0xff000000u;
}

// (p00 (1 - fx) + p10 fx) (1 - fy) + (p01 (1 - fx) + p11 fx) fy of one channel, then (u8) floor(v + 0.5)
__device__ inline uint32_t lerp_u8(uint32_t p00, uint32_t p10, uint32_t p01, uint32_t p11, int shift, double fx, double fy)
{
    const double a = static_cast<double>((p00 >> shift) & 255u), b = static_cast<double>((p10 >> shift) & 255u);
    const double c = static_cast<double>((p01 >> shift) & 255u), d = static_cast<double>((p11 >> shift) & 255u);
    const double v = (a * (1. - fx) + b * fx) * (1. - fy) + (c * (1. - fx) + d * fx) * fy;
    const double r = floor(v + 0.5);
    return (r >= 255. ? 255u : (r > 0. ? static_cast<uint32_t>(r) : 0u)) << shift;
}

// sin, cos, tan of output row i's latitude (depends on neither the column nor the pass)
__device__ inline void row_terms(const Grid &g, uint32_t row, double out[3])
{
    const double i = static_cast<double>(row);
    const double lat = g.kind == APTGPU_PROJECTION_MERCATOR ? atan(sinh(g.y_north - i * g.step_rad))
                                                            : (g.lat_north - i * g.step) / 180. * apt::map::kPi;
    out[0] = sin(lat);
    out[1] = cos(lat);
    out[2] = tan(lat);
}

// sin(dl), cos(dl), cos(dl2) of output column j's longitude against one track's start
__device__ inline void col_terms(const Grid &g, uint32_t col, double start_lon, double out[3])
{
    const double j = static_cast<double>(col);
    const double lon = (g.lon_west + j * g.step) / 180. * apt::map::kPi;
    const double dl = lon - start_lon, dl2 = start_lon - lon;
    out[0] = sin(dl);
    out[1] = cos(dl);
    out[2] = cos(dl2);
}

// Steps 2-4 for one output pixel of one pass, from the staged terms: the corrected x, the validity rule and the
// sample.  Returns whether the pass covers the pixel; px is written only then.
__device__ inline bool sample_pass(const Grid &g, const apt::map::Scalars &sc, const double start[2], const double row[3],
                                   const double col[3], const double *xoff, uint32_t h, const uint8_t *src,
                                   int src_channels, double &x, uint32_t &px)
{
    double y, dist;
    apt::map::rel_px_from(sc, start[0], start[1], row[0], row[1], row[2], col[0], col[1], col[2], x, y, dist);
    bool valid = h != 0 && isfinite(x) && isfinite(y);
    if (valid) {
        x -= xoff[apt::map::est_row(y, h)];
        valid = isfinite(x) && x > -456. && x < 456. && y > 0. && y < static_cast<double>(h) && dist < apt::map::kPi / 3.;
    }
    if (!valid) return false;
    const int base = g.channel == APTGPU_PROJECTION_CHANNEL_B ? 1579 : 539, hi = static_cast<int>(h);
    if (g.sampling == APTGPU_SAMPLING_BILINEAR) {
        const double x0 = floor(x), y0 = floor(y);
        const double fx = x - x0, fy = y - y0;
        const int xi = static_cast<int>(x0), yi = static_cast<int>(y0);
        const uint32_t p00 = fetch(src, src_channels, base, hi, xi, yi);
        const uint32_t p10 = fetch(src, src_channels, base, hi, xi + 1, yi);
        const uint32_t p01 = fetch(src, src_channels, base, hi, xi, yi + 1);
        const uint32_t p11 = fetch(src, src_channels, base, hi, xi + 1, yi + 1);
        px = lerp_u8(p00, p10, p01, p11, 0, fx, fy) | lerp_u8(p00, p10, p01, p11, 8, fx, fy) |
             lerp_u8(p00, p10, p01, p11, 16, fx, fy) | lerp_u8(p00, p10, p01, p11, 24, fx, fy);
    } else {
        px = fetch(src, src_channels, base, hi, static_cast<int>(floor(x + 0.5)), static_cast<int>(floor(y + 0.5)));
    }
    return true;
}

}  // namespace

}  // namespace apt::project
