// apt_kernels_landmask.hpp — the land / sea / lake mask of the swath and the map-coloured false colour
// (apt_kernels_landmask.hip on the GPU, apt_landmask.cpp on the CPU).  The reference has no such stage, so
// this is the definition (include/aptgpu.h states it in full; tests/np_landmask_model.py in numpy).  The per-point and
// per-pixel arithmetic is written once, here, for both sides.
//
//  Point   (lat, lon) in radians as the geolocation stage returns them; py = lat * kDeg, px = lon * kDeg.
//  Edge    consecutive vertices of a part of countries.shp / lakes.shp, f64 degrees, plus the closing edge of an
//          unclosed part; horizontal edges are left out (they never straddle a point).
//  Rule    straddle = (y1 > py) != (y2 > py);  d = (x2 - x1) * (py - y1) - (px - x1) * (y2 - y1);
//          crossing = straddle && (y2 > y1 ? d > 0 : d < 0).  Every operation rounds on its own; the count is an integer.
//  Class   lake if the count against the lakes is odd, else land if the count against the countries is odd, else sea;
//          255 where lat or lon is NaN.
//  Bands   nb latitude bands; an edge is listed in every band between those of its two ends.  band() is monotone, so
//          the band of a point lists every edge that can straddle it, each once: a point is tested against its own band.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "apt_color_tune.hpp"  // ColorTune, tune(): the text process()'s false colour uses
#include "apt_kernels_geoloc.hpp"

namespace apt::landmask {

constexpr double kDeg = 57.29577951308232;
constexpr uint8_t kSea = 0, kLand = 1, kLake = 2, kInvalid = 255;
constexpr int kDefaultBands = 720, kMaxBands = 7200;
constexpr int kPaletteBytes = 256 * 256 * 3;

struct alignas(32) Edge {
    double x1, y1, x2, y2;
};
static_assert(sizeof(Edge) == 32, "one record is 32 bytes");

APT_DSP_HD bool crossing(const Edge &e, double px, double py)
{
    const bool straddle = (e.y1 > py) != (e.y2 > py);
    const double d = (e.x2 - e.x1) * (py - e.y1) - (px - e.x1) * (e.y2 - e.y1);
    // (&&: on the GPU the compiler skips d where no lane of the wave straddles, which is most records of a band)
    return straddle && (e.y2 > e.y1 ? d > 0. : d < 0.);
}

// clamp((int) floor((y + 90) * (nb / 180)), 0, nb - 1); `scale` is nb / 180.0.  The clamp is taken before the
// conversion, so an infinite y has a band too.  (y is never NaN here.)
APT_DSP_HD int band_of(double y, int nb, double scale)
{
    const double b = floor((y + 90.0) * scale);
    return b < 0. ? 0 : b > static_cast<double>(nb - 1) ? nb - 1 : static_cast<int>(b);
}

APT_DSP_HD uint8_t class_of(bool land, bool lake) { return lake ? kLake : land ? kLand : kSea; }

using Tune = apt::gpu::ColorTune;
// the settings folded as for process(): tunes = {a start, a end, b start, b end}
inline Tune tune_of(const float tunes[4]) { return apt::gpu::color_tune_of(tunes[0], tunes[1], tunes[2], tunes[3]); }

// One pixel of the map-coloured image, packed R | G << 8 | B << 16 | A << 24.  x: image column; g_a the gray value
// there, g_b the one 1040 columns on (read only inside channel A's video); c: the mask's class there.  pal: the three
// palettes as 65536 packed words each (sea, land, lake).
APT_DSP_HD uint32_t masked_pixel(uint32_t x, uint32_t g_a, uint32_t g_b, uint32_t c, const Tune &t, const uint32_t *pal)
{
    const uint32_t gray = (g_a * 0x010101u) | 0xff000000u;
    if (x < static_cast<uint32_t>(apt::geoloc::kVideo0) || x >= static_cast<uint32_t>(apt::geoloc::kVideo0 + apt::geoloc::kVideoN) || c > 2u)
        return gray;
    return pal[c * 65536u + apt::gpu::tune(g_b, t.k_b, t.o_b) * 256u + apt::gpu::tune(g_a, t.k_a, t.o_a)];
}

}  // namespace apt::landmask

// ---- the host side (apt_landmask.cpp; CPU only)
namespace apt::landmask {

// The acceleration table of one layer set: for layer L (0 countries, 1 lakes) and band b the records
// edges[off[L * nb + b] .. off[L * nb + b + 1]).
struct Table {
    int nb = 0;
    uint64_t gen = 0;          // the layer set's generation it was built from
    uint32_t n_edges[2] = {};  // non-horizontal edges per layer
    std::vector<uint32_t> off; // 2 * nb + 1
    std::vector<Edge> edges;
};
// Null settings: 720 bands.  A struct_size that is too small, a flag, n_bands outside [1, 7200]: Error{Invalid}.
int check_settings(const aptgpu_land_mask_settings *s);
// A layer set with neither countries nor lakes, a non-finite vertex, 2^32 band entries or more: Error{Invalid}.
Table build_table(const apt::map::Layers &layers, int nb);
void put_result(aptgpu_land_mask_result *out, aptgpu_land_mask_result r);
aptgpu_land_mask_result first_record(const Table &t, uint32_t height);
uint8_t classify(const Table &t, double lat, double lon);
// The definition in plain C++.  latlon: n (lat, lon) pairs; mask: n bytes; the four counts into *rec.
void run_plane_host(const Table &t, const double *latlon, size_t n, uint8_t *mask, aptgpu_land_mask_result *rec);
// The swath form: the geolocation stage's host twin for the points, then the plane form.  mask: h * 909 bytes.  A
// failed record throws Error{Internal} after filling *info; nothing is written then.
void run_swath_host(const Table &t, size_t h, const double *track, size_t count, const apt::geoloc::Geom &g,
                    uint8_t *mask, aptgpu_land_mask_result *info);
// image: h rows of 2080 gray bytes; mask: h * 909; palettes: three times 256 * 256 * 3 RGB bytes; out: h * 2080 * 4
void false_color_masked_host(const uint8_t *image, size_t h, const uint8_t *mask, const uint8_t *const *palettes,
                             const float tunes[4], uint8_t *out);
void pack_palettes(const uint8_t *const *palettes, uint32_t *packed);  // 3 * 65536 words

}  // namespace apt::landmask

#if defined(__HIPCC__)
#include "apt_plan.hpp"

namespace apt::gpu {

// Device-side record: the head of aptgpu_land_mask_result, and the four counts, which the waves gather in kLandParts
// partial records, 64 bytes apart (a wave uses part[wave % kLandParts]).
constexpr int kLandParts = 64;
struct LandPart {
    unsigned long long n[4];  // sea, land, lake, invalid
    uint32_t pad[8];
};
struct LandRecord {
    int32_t status, reason;
    uint32_t height, reserved;
    uint32_t pad[12];
    LandPart part[kLandParts];
};
// folds the parts into `head` (whose n_edges / n_band_entries the caller filled from the table)
void land_record_to_public(const LandRecord &r, aptgpu_land_mask_result head, aptgpu_land_mask_result *out);

// The table in HBM.  upload() copies when the generation or the band count differ from what it holds.
struct LandTable {
    apt::DeviceBuffer<uint32_t> off;
    apt::DeviceBuffer<apt::landmask::Edge> edges;
    std::shared_ptr<const apt::landmask::Table> host;  // what the device holds (kept while uploads may read it)
    void upload(hipStream_t s, const std::shared_ptr<const apt::landmask::Table> &t);
};

// k_land_mask<Plane>: n points of d_latlon (16-byte aligned) into d_mask; the record is reset first.
void land_mask_plane(hipStream_t s, const LandTable &t, const double *d_latlon, uint64_t n, uint8_t *d_mask,
                     LandRecord *rec);
// k_land_mask<Swath> behind the geolocation stage's track and row launches on the same stream (geoloc_track,
// geoloc_rows): the record's head, the frame and xoff come from geoloc_ws and dev; rows_cap rows of room in d_mask.
void land_mask_swath(hipStream_t s, const LandTable &t, const void *geoloc_ws, const apt::map::Device &dev,
                     uint32_t rows_cap, uint8_t *d_mask, LandRecord *rec);
// k_false_color_masked: h rows; d_palettes 3 * 65536 packed words; d_out h * 2080 * 4 bytes, 4-byte aligned
void false_color_masked(hipStream_t s, const uint8_t *d_image, uint32_t h, const uint8_t *d_mask,
                        const uint32_t *d_palettes, const apt::landmask::Tune &tune, uint8_t *d_out);

}  // namespace apt::gpu
#endif
