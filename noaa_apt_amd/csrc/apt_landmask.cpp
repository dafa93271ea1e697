// apt_landmask.cpp — the land / sea / lake mask on the CPU: the settings' checks, the acceleration table every form
// shares, and the definition of apt_kernels_landmask.hpp in plain C++ (aptgpu_land_mask_host,
// aptgpu_land_mask_plane_host, aptgpu_false_color_masked_host), which the kernels are tested against and which a
// stand-alone program can call without a GPU.
#include "apt_kernels_landmask.hpp"

#include <cmath>
#include <vector>

namespace apt::landmask {

namespace {

// calls fn(x1, y1, x2, y2) for every edge of the layer, in file order: consecutive pairs, then the closing edge of a part
// whose ends differ
template <typename Fn>
void for_each_edge(const apt::map::Layer &l, Fn &&fn)
{
    for (size_t k = 0; k + 1 < l.parts.size(); ++k) {
        const size_t p0 = l.parts[k], p1 = l.parts[k + 1];
        if (p1 <= p0) continue;
        for (size_t i = p0; i + 1 < p1; ++i) fn(l.xy[2 * i], l.xy[2 * i + 1], l.xy[2 * i + 2], l.xy[2 * i + 3]);
        const size_t a = p1 - 1, b = p0;
        if (l.xy[2 * a] != l.xy[2 * b] || l.xy[2 * a + 1] != l.xy[2 * b + 1])
            fn(l.xy[2 * a], l.xy[2 * a + 1], l.xy[2 * b], l.xy[2 * b + 1]);
    }
}

}  // namespace

int check_settings(const aptgpu_land_mask_settings *s)
{
    if (!s) return kDefaultBands;
    if (s->struct_size < sizeof(aptgpu_land_mask_settings))
        throw Error{ErrorKind::Invalid, "aptgpu_land_mask_settings: struct_size not set"};
    if (s->flags) throw Error{ErrorKind::Invalid, "land mask: unknown flag"};
    if (s->n_bands < 1 || s->n_bands > kMaxBands)
        throw Error{ErrorKind::Invalid, "land mask: n_bands must lie in [1, 7200]"};
    return s->n_bands;
}

Table build_table(const apt::map::Layers &layers, int nb)
{
    const int which[2] = {apt::map::Layers::kCountries, apt::map::Layers::kLakes};
    if (!layers.present[which[0]] && !layers.present[which[1]])
        throw Error{ErrorKind::Invalid, "land mask: the layer set holds neither countries nor lakes"};
    Table t;
    t.nb = nb;
    t.gen = layers.gen;
    const double scale = static_cast<double>(nb) / 180.0;
    std::vector<uint64_t> count(2 * static_cast<size_t>(nb) + 1, 0);
    for (int pass = 0; pass < 2; ++pass) {
        // pass 0 counts the entries per list, pass 1 writes them behind the lists' offsets
        std::vector<uint32_t> at;
        if (pass == 1) at.assign(t.off.begin(), t.off.end() - 1);
        for (int li = 0; li < 2; ++li) {
            if (!layers.present[which[li]]) continue;
            const apt::map::Layer &l = layers.layer[which[li]];
            if (pass == 0)
                for (double v : l.xy)
                    if (!std::isfinite(v))
                        throw Error{ErrorKind::Invalid, "land mask: a vertex of the layer set is not finite"};
            for_each_edge(l, [&](double x1, double y1, double x2, double y2) {
                if (y1 == y2) return;
                const int b0 = band_of(y1 < y2 ? y1 : y2, nb, scale), b1 = band_of(y1 < y2 ? y2 : y1, nb, scale);
                if (pass == 0) t.n_edges[li] += 1;
                for (int b = b0; b <= b1; ++b) {
                    const size_t list = static_cast<size_t>(li) * nb + b;
                    if (pass == 0) count[list] += 1;
                    else t.edges[at[list]++] = Edge{x1, y1, x2, y2};
                }
            });
        }
        if (pass == 0) {
            uint64_t total = 0;
            t.off.resize(count.size());
            for (size_t k = 0; k < count.size(); ++k) {
                if (total > 0xFFFFFFFFull) break;
                t.off[k] = static_cast<uint32_t>(total);
                total += count[k];
            }
            if (total > 0xFFFFFFFFull) throw Error{ErrorKind::Invalid, "land mask: 2^32 band entries or more"};
            t.edges.resize(static_cast<size_t>(total));
        }
    }
    return t;
}

void put_result(aptgpu_land_mask_result *out, aptgpu_land_mask_result r)
{
    if (!out) return;
    const uint32_t size = out->struct_size;
    r.struct_size = size;
    std::memcpy(out, &r, size < sizeof r ? size : sizeof r);
}

aptgpu_land_mask_result first_record(const Table &t, uint32_t height)
{
    aptgpu_land_mask_result r{};
    r.height = height;
    r.n_edges[0] = t.n_edges[0];
    r.n_edges[1] = t.n_edges[1];
    r.n_band_entries = t.edges.size();
    return r;
}

uint8_t classify(const Table &t, double lat, double lon)
{
    if (lat != lat || lon != lon) return kInvalid;
    const double py = lat * kDeg, px = lon * kDeg;
    const int b = band_of(py, t.nb, static_cast<double>(t.nb) / 180.0);
    bool odd[2];
    for (int li = 0; li < 2; ++li) {
        const size_t list = static_cast<size_t>(li) * t.nb + b;
        unsigned n = 0;
        for (uint32_t e = t.off[list]; e < t.off[list + 1]; ++e) n += crossing(t.edges[e], px, py) ? 1u : 0u;
        odd[li] = (n & 1u) != 0;
    }
    return class_of(odd[0], odd[1]);
}

void run_plane_host(const Table &t, const double *latlon, size_t n, uint8_t *mask, aptgpu_land_mask_result *rec)
{
    uint64_t cnt[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < n; ++i) {
        const uint8_t c = classify(t, latlon[2 * i], latlon[2 * i + 1]);
        mask[i] = c;
        cnt[c == kInvalid ? 3 : c] += 1;
    }
    rec->n_sea = cnt[0];
    rec->n_land = cnt[1];
    rec->n_lake = cnt[2];
    rec->n_invalid = cnt[3];
}

void run_swath_host(const Table &t, size_t h, const double *track, size_t count, const apt::geoloc::Geom &g,
                    uint8_t *mask, aptgpu_land_mask_result *info)
{
    aptgpu_land_mask_result rec = first_record(t, static_cast<uint32_t>(h));
    aptgpu_geoloc_result gi{};
    gi.struct_size = sizeof gi;
    std::vector<double> latlon(2 * h * apt::geoloc::kVideoN + 2);
    const apt::geoloc::Settings st{0, false, 0, 0.f, 0.f};
    try {
        apt::geoloc::run_host(nullptr, h * apt::geoloc::kPx, track, count, g, st, latlon.data(), nullptr, nullptr, &gi);
    } catch (const Error &) {
        rec.status = gi.status;
        rec.reason = gi.reason;
        put_result(info, rec);
        throw;
    }
    run_plane_host(t, latlon.data(), h * apt::geoloc::kVideoN, mask, &rec);
    put_result(info, rec);
}

void pack_palettes(const uint8_t *const *palettes, uint32_t *packed)
{
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < 65536; ++i) {
            const uint8_t *p = palettes[c] + 3 * i;
            packed[c * 65536 + i] = static_cast<uint32_t>(p[0]) | (static_cast<uint32_t>(p[1]) << 8) |
                                    (static_cast<uint32_t>(p[2]) << 16) | 0xff000000u;
        }
}

void false_color_masked_host(const uint8_t *image, size_t h, const uint8_t *mask, const uint8_t *const *palettes,
                             const float tunes[4], uint8_t *out)
{
    std::vector<uint32_t> pal(3 * 65536);
    pack_palettes(palettes, pal.data());
    const Tune tn = tune_of(tunes);
    constexpr uint32_t v0 = apt::geoloc::kVideo0, vn = apt::geoloc::kVideoN;
    for (size_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < static_cast<uint32_t>(apt::geoloc::kPx); ++x) {
            const bool video = x >= v0 && x < v0 + vn;
            const size_t i = y * apt::geoloc::kPx + x;
            const uint32_t g_b = video ? image[i + apt::geoloc::kHalfPx] : 0u;
            const uint32_t c = video ? mask[y * vn + (x - v0)] : 255u;
            const uint32_t px = masked_pixel(x, image[i], g_b, c, tn, pal.data());
            std::memcpy(out + 4 * i, &px, 4);
        }
}

}  // namespace apt::landmask
