// apt_geoloc.cpp — the geolocation stage on the CPU: the checks every entry point shares, the sun of one instant, and
// the definition of apt_kernels_geoloc.hpp in plain C++ (aptgpu_geolocate_host), which the kernels are tested against
// and which a stand-alone program can call without a GPU.
#include "apt_kernels_geoloc.hpp"

#include <cmath>
#include <vector>

namespace apt::geoloc {

namespace {

// latlon_to_rel_px's x (map.rs:71-100) with the C library's f64 functions: the text of apt_kernels_map_dev.hpp,
// which is device code, restated for the host
double rel_px_x(const apt::map::Scalars &s, double lat, double lon)
{
    const double dl = lon - s.start_lon, dl2 = s.start_lon - lon;
    const double az = std::atan2(std::sin(dl), std::cos(s.start_lat) * std::tan(lat) - std::sin(s.start_lat) * std::cos(dl));
    const double big_b = az - s.ref_az;
    double cc = std::sin(lat) * std::sin(s.start_lat) + std::cos(lat) * std::cos(s.start_lat) * std::cos(dl2);
    cc = std::fmin(std::fmax(cc, -1.), 1.);
    const double dist = std::acos(cc);
    const double c = std::fmin(std::fmax(dist, -kPi / 3.), kPi / 3.);
    const double b = std::asin(std::sin(big_b) * std::sin(c));
    return -b / s.x_res;
}

uint32_t bits_of(float v)
{
    uint32_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}

}  // namespace

Settings check_settings(const aptgpu_geoloc_settings *s)
{
    if (!s) throw Error{ErrorKind::Invalid, "geoloc: settings are required"};
    if (s->struct_size < sizeof(aptgpu_geoloc_settings))
        throw Error{ErrorKind::Invalid, "aptgpu_geoloc_settings: struct_size not set"};
    if (s->flags) throw Error{ErrorKind::Invalid, "geoloc: unknown flag"};
    if (s->channel != 0 && s->channel != 1) throw Error{ErrorKind::Invalid, "geoloc: channel must be 0 (A) or 1 (B)"};
    if (s->time_kind != APTGPU_REF_TIME_START && s->time_kind != APTGPU_REF_TIME_END)
        throw Error{ErrorKind::Invalid, "geoloc: unknown time_kind"};
    if (!std::isfinite(s->black_level)) throw Error{ErrorKind::Invalid, "geoloc: black_level must be finite"};
    if (!(s->max_zenith_deg > 0.f && s->max_zenith_deg < 90.f))
        throw Error{ErrorKind::Invalid, "geoloc: max_zenith_deg must lie in (0, 90)"};
    const float cmin = static_cast<float>(std::cos(static_cast<double>(s->max_zenith_deg) / 180. * kPi));
    return Settings{s->channel, s->time_kind == APTGPU_REF_TIME_END, s->unix_ms, s->black_level, cmin};
}

Geom check_geom(const aptgpu_map_settings *map)
{
    Geom g;
    if (!map) return g;
    if (map->struct_size < sizeof(aptgpu_map_settings))
        throw Error{ErrorKind::Invalid, "aptgpu_map_settings: struct_size not set"};
    g.yaw = map->yaw;
    g.hscale = map->hscale;
    g.vscale = map->vscale;
    return g;
}

void check_call(const void *positions, const void *orbit, bool want_rows, bool have_signal, size_t rows)
{
    if ((positions != nullptr) == (orbit != nullptr))
        throw Error{ErrorKind::Invalid, "geoloc: exactly one of sat_positions and orbit is required"};
    if (want_rows && !have_signal) throw Error{ErrorKind::Invalid, "geoloc: normalised rows need the signal"};
    if (rows > kMaxRows) throw Error{ErrorKind::Invalid, "geoloc: more than 2^22 rows"};
}

const char *reason_text(int reason)
{
    switch (reason) {
    case kReasonCount: return "geoloc: the number of satellite positions differs from the image height";
    case kReasonSgp4: return "satellite track: SGP4 failed for a row of the image (APTGPU_SAT_REASON_SGP4)";
    case kReasonHeight: return "geoloc: fewer than two rows, no direction of flight (APTGPU_GEOLOC_REASON_HEIGHT)";
    case kReasonDecode: return "geoloc: the decode before it failed (APTGPU_GEOLOC_REASON_DECODE)";
    default: return "geolocation stage failed";
    }
}

void sun_position(int64_t unix_ms, double out[2])
{
    double delta, lon;
    sun_angles(unix_ms, delta, lon);
    out[0] = delta;
    out[1] = std::atan2(std::sin(lon), std::cos(lon));
}

void put_result(aptgpu_geoloc_result *out, aptgpu_geoloc_result r)
{
    if (!out) return;
    const uint32_t size = out->struct_size;
    r.struct_size = size;
    std::memcpy(out, &r, size < sizeof r ? size : sizeof r);
}

void run_host(const float *x, size_t n, const double *track, size_t count, const Geom &g, const Settings &s,
              double *latlon, float *cos_sun, float *rows, aptgpu_geoloc_result *info)
{
    const size_t h = n / kPx;
    aptgpu_geoloc_result rec{};
    rec.height = static_cast<uint32_t>(h);
    rec.cos_min = rec.cos_max = quiet_nan();
    rec.reason = h < 2 ? kReasonHeight : count != h ? kReasonCount : 0;
    if (rec.reason) {
        rec.status = APTGPU_ERR_INTERNAL;
        put_result(info, rec);
        throw Error{ErrorKind::Internal, reason_text(rec.reason)};
    }
    const apt::map::Scalars sc = apt::map::scalars(track, count, g.yaw, g.hscale, g.vscale);
    const Frame f = frame_of(sc.start_lat, sc.start_lon, sc.ref_az, sc.x_res, sc.y_res, sc.yaw);
    const int64_t t0 = start_ms_of(s.ref_is_end, s.ref_ms, static_cast<uint32_t>(h));
    const int base = kHalfPx * s.channel;
    if (rows && rows != x) std::memcpy(rows, x, n * sizeof(float));
    Counters cnt;
    for (size_t r = 0; r < h; ++r) {
        const double xoff = xoff_of(rel_px_x(sc, track[2 * r], track[2 * r + 1]), static_cast<uint32_t>(r));
        double u[3];
        sun_of(t0 + kLineMs * static_cast<int64_t>(r), u);
        for (int k = 0; k < kVideoN; ++k) {
            const Point p = point_of(f, xoff, static_cast<uint32_t>(r), k);
            const size_t i = r * kVideoN + static_cast<size_t>(k);
            double lat = quiet_nan64(), lon = quiet_nan64();
            float c = quiet_nan();
            if (p.valid) {
                c = cos_sun_of(p, u);
                if (latlon) latlon_of(p, lat, lon);
                const uint32_t key = apt::despeckle::key_of_bits(bits_of(c));
                cnt.min_key = key < cnt.min_key ? key : cnt.min_key;
                cnt.max_key = key > cnt.max_key ? key : cnt.max_key;
                cnt.n_capped += c < s.cmin ? 1u : 0u;
                if (rows) {
                    float *px = rows + r * kPx + base + kVideo0 + k;
                    *px = normalised(*px, c, s.black, s.cmin, true);
                }
            } else {
                cnt.n_outside += 1;
            }
            if (latlon) {
                latlon[2 * i] = lat;
                latlon[2 * i + 1] = lon;
            }
            if (cos_sun) cos_sun[i] = c;
        }
    }
    rec.n_outside = cnt.n_outside;
    rec.n_capped = cnt.n_capped;
    if (cnt.min_key <= cnt.max_key) {
        const uint32_t lo = apt::despeckle::bits_of_key(cnt.min_key), hi = apt::despeckle::bits_of_key(cnt.max_key);
        std::memcpy(&rec.cos_min, &lo, sizeof lo);
        std::memcpy(&rec.cos_max, &hi, sizeof hi);
    }
    put_result(info, rec);
}

}  // namespace apt::geoloc
