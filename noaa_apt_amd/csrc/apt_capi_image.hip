// apt_capi_image.hip — extern "C" surface of include/aptgpu.h §4: the consumers of decode()'s
// pixel rows (contrast limits, u8 mapping, telemetry), host-buffer and device-resident forms.
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "apt_capi_util.hpp"
#include "apt_kernels_color.hpp"
#include "apt_kernels_despeckle.hpp"
#include "apt_kernels_eqfloat.hpp"
#include "apt_kernels_png.hpp"
#include "apt_kernels_project.hpp"
#include "apt_kernels_track.hpp"
#include "apt_map.hpp"
#include "apt_sat.hpp"

// the opaque handle of include/aptgpu.h
struct aptgpu_map_layers {
    apt::map::Layers layers;
};

namespace {

using namespace apt::capi;
using apt::gpu::ImageResult;

static_assert(sizeof(ImageResult) == sizeof(aptgpu_image_result), "ImageResult must mirror aptgpu_image_result");

const char *kZeroMin = "Can't get minimum of a zero length vector";
const char *kZeroMax = "Can't get maximum of a zero length vector";
const char *kTelemetryShort = "Recording too short for telemetry decoding";
const char *kBadPercent = "Percent given should be between 0 and 1";
const char *kNoLowBucket = "percent: no bucket reaches the low threshold (the reference panics here)";
const char *kMapOverflow = "map overlay: more than APTGPU_MAP_MAX_FRAGMENTS (2^21) fragments in one image";
const char *kMapWalk = "map overlay: a segment's walk is longer than APTGPU_MAP_MAX_WALK (2^20) steps or has a non-finite end";
const char *kMapPixel = "map overlay: more than APTGPU_MAP_MAX_PIXEL_FRAGMENTS (2^16) fragments on one pixel";
const char *kMapCount = "map overlay: the number of satellite positions differs from the image height";
const char *kSatSgp4 = "satellite track: SGP4 failed for a row of the image (APTGPU_SAT_REASON_SGP4)";
const char *kPngCapacity = "PNG encoding: the output buffer is smaller than the file (APTGPU_PNG_REASON_CAPACITY)";
const char *kProjectCapacity = "reprojection: the output buffer is smaller than width * height * 4 bytes (APTGPU_PROJECT_REASON_CAPACITY)";
const char *kChannelNames[9] = {"1", "2", "3a", "4", "5", "3b", "Unknown", "Unknown", "Unknown"};

// Rust's `{}` for an f32: shortest decimal that round-trips, never in exponent form.
std::string rust_display_f32(float v)
{
    if (std::isnan(v)) return "NaN";
    if (std::isinf(v)) return v > 0 ? "inf" : "-inf";
    char buf[64];
    int prec = 1;
    for (; prec <= 9; ++prec) {
        std::snprintf(buf, sizeof buf, "%.*e", prec - 1, static_cast<double>(v));
        if (std::strtof(buf, nullptr) == v) break;
    }
    std::string digits;
    bool neg = false;
    const char *p = buf;
    if (*p == '-') {
        neg = true;
        ++p;
    }
    for (; *p && *p != 'e'; ++p)
        if (*p != '.') digits.push_back(*p);
    const int exp10 = *p == 'e' ? std::atoi(p + 1) : 0;
    while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
    std::string out;
    const int point = exp10 + 1;  // digits before the decimal point
    if (point <= 0) {
        out = "0." + std::string(static_cast<size_t>(-point), '0') + digits;
    } else if (static_cast<size_t>(point) >= digits.size()) {
        out = digits + std::string(static_cast<size_t>(point) - digits.size(), '0');
    } else {
        out = digits.substr(0, static_cast<size_t>(point)) + "." + digits.substr(static_cast<size_t>(point));
    }
    if (digits == "0") out = "0";
    return neg ? "-" + out : out;
}

void throw_for(const ImageResult &r, int contrast)
{
    if (r.status == 0) return;
    switch (r.reason) {
    case 1: throw Error{ErrorKind::Internal, kZeroMin};
    case 2: throw Error{ErrorKind::Internal, kTelemetryShort};
    case 3: throw Error{ErrorKind::Internal, kNoLowBucket};
    case apt::map::kReasonOverflow: throw Error{ErrorKind::Internal, kMapOverflow};
    case apt::map::kReasonWalk: throw Error{ErrorKind::Internal, kMapWalk};
    case apt::map::kReasonCount: throw Error{ErrorKind::Internal, kMapCount};
    case apt::map::kReasonPixel: throw Error{ErrorKind::Internal, kMapPixel};
    case apt::sat::kReasonSgp4: throw Error{ErrorKind::Internal, kSatSgp4};
    case apt::png::kReasonCapacity: throw Error{ErrorKind::Internal, kPngCapacity};
    case apt::project::kReasonCapacity: throw Error{ErrorKind::Internal, kProjectCapacity};
    default: throw Error{ErrorKind::Internal, "image stage failed"};
    }
    (void)contrast;
}

// One host-buffer call: signal in HBM + scratch + record.
struct ImageCall {
    Scratch sc;
    apt::DeviceBuffer<float> d_x;
    apt::DeviceBuffer<char> ws;
    apt::DeviceBuffer<ImageResult> d_info;
    uint64_t n;
    ImageCall(const aptgpu_context *ctx, const float *signal, size_t n_) : sc(ctx), n(n_)
    {
        d_x = sc.upload(signal, n, 2080 + 16);
        ws.alloc(apt::gpu::image_ws_bytes(n));
        d_info.alloc(1);
        apt::gpu::image_begin(sc.stream, d_info.ptr);
    }
    ImageResult info()
    {
        ImageResult r{};
        apt::hip_check(hipMemcpyAsync(&r, d_info.ptr, sizeof r, hipMemcpyDeviceToHost, sc.stream),
                       "hipMemcpyAsync D2H");
        apt::hip_check(hipStreamSynchronize(sc.stream), "hipStreamSynchronize");
        return r;
    }
    void limits(float *low, float *high)
    {
        float lim[2] = {0.f, 0.f};
        const auto p = apt::gpu::image_ws_pointers(ws.ptr, n);
        apt::hip_check(hipMemcpyAsync(lim, p.limits, sizeof lim, hipMemcpyDeviceToHost, sc.stream),
                       "hipMemcpyAsync D2H");
        apt::hip_check(hipStreamSynchronize(sc.stream), "hipStreamSynchronize");
        *low = lim[0];
        *high = lim[1];
    }
    apt::Signal band(const float *d, size_t count)
    {
        apt::Signal h(count);
        if (count) {
            apt::hip_check(hipMemcpyAsync(h.data(), d, count * sizeof(float), hipMemcpyDeviceToHost, sc.stream),
                           "hipMemcpyAsync D2H");
            apt::hip_check(hipStreamSynchronize(sc.stream), "hipStreamSynchronize");
        }
        return h;
    }
};

void copy_out(aptgpu_image_result *dst, const ImageResult &r)
{
    if (dst) std::memcpy(dst, &r, sizeof r);
}

// read_telemetry's step exports, telemetry.rs:234-238 (same order, same ids)
void telemetry_steps(const aptgpu_context *ctx, ImageCall &c, const ImageResult &r)
{
    if (!ctx || !ctx->step) return;
    const auto p = apt::gpu::image_ws_pointers(c.ws.ptr, c.n);
    const size_t rows = c.n / 2080;
    const size_t nc = rows >= 200 ? rows - 200 : 0;
    (void)r;
    const apt::Signal a = c.band(p.mean_a, rows), b = c.band(p.mean_b, rows), v = c.band(p.variance, rows);
    const apt::Signal co = c.band(p.corr, nc), q = c.band(p.quality, nc);
    step(ctx, true, "telemetry_a", 0, a.data(), a.size(), 0);
    step(ctx, true, "telemetry_b", 0, b.data(), b.size(), 0);
    step(ctx, true, "telemetry_correlation", 0, co.data(), co.size(), 0);
    step(ctx, true, "telemetry_variance", 0, v.data(), v.size(), 0);
    step(ctx, true, "telemetry_quality", 0, q.data(), q.size(), 0);
}

// process()'s contrast limits (noaa_apt.rs:141-175) with its 0.1 status: every contrast but Telemetry
// leaves its error (if any) in the record for the caller's c.info() after the image kernels.  lab:
// Histogram with false colour, whose limits are misc::percent(signal, 0.98) once get_min / get_max
// have passed (noaa_apt.rs:170-175); their only error is the zero length, checked first.
void process_limits(const aptgpu_context *ctx, ImageCall &c, int contrast, float percent, aptgpu_image_result *info,
                    bool lab = false)
{
    hipStream_t s = c.sc.stream;
    const uint64_t n = c.n;
    if (contrast == APTGPU_CONTRAST_TELEMETRY) {
        status(ctx, 0.1f, "Adjusting contrast from telemetry");  // noaa_apt.rs:142
        apt::gpu::image_telemetry(s, c.d_x.ptr, nullptr, n, n, c.ws.ptr, c.d_info.ptr, true);
        const ImageResult r = c.info();
        copy_out(info, r);
        throw_for(r, contrast);
        telemetry_steps(ctx, c, r);
    } else if (contrast == APTGPU_CONTRAST_PERCENT) {
        // noaa_apt.rs:152-155
        status(ctx, 0.1f, "Adjusting contrast using " + rust_display_f32(percent * 100.f) + " percent");
        if (percent < 0.f || percent > 1.f) throw Error{ErrorKind::Internal, kBadPercent};
        if (n == 0) throw Error{ErrorKind::Internal, kZeroMin};
        apt::gpu::image_percent(s, c.d_x.ptr, nullptr, n, n, percent, c.ws.ptr, c.d_info.ptr);
    } else {
        status(ctx, 0.1f, "Mapping values");  // noaa_apt.rs:159 (MinMax and Histogram)
        if (n == 0) throw Error{ErrorKind::Internal, kZeroMin};
        if (lab)
            apt::gpu::image_percent(s, c.d_x.ptr, nullptr, n, n, 0.98f, c.ws.ptr, c.d_info.ptr);
        else
            apt::gpu::image_minmax(s, c.d_x.ptr, nullptr, n, n, c.ws.ptr, c.d_info.ptr);
    }
}

// The checks of aptgpu_process_image / aptgpu_plan_process_device_image, all before any status callback.
// Returns the folded tune values when false colour is on, and in *lab whether the Lab path runs.
bool color_args(int contrast, int rotate, const aptgpu_color_settings *color, int channels, apt::gpu::ColorTune *tune,
                bool *lab)
{
    *lab = false;
    if (contrast < APTGPU_CONTRAST_TELEMETRY || contrast > APTGPU_CONTRAST_HISTOGRAM_FLOAT)
        throw Error{ErrorKind::Invalid, "unknown contrast adjustment"};
    if (rotate != APTGPU_ROTATE_NO && rotate != APTGPU_ROTATE_YES)
        throw Error{ErrorKind::Unsupported, "Rotate::Orbit needs the satellite and the time: aptgpu_orbit_settings, the *_orbit entry points"};
    if (channels != 1 && channels != 4) throw Error{ErrorKind::Invalid, "channels must be 1 (gray) or 4 (RGBA)"};
    if (!color) return false;
    if (color->struct_size < sizeof(aptgpu_color_settings) || !color->palette_rgb)
        throw Error{ErrorKind::Invalid, "aptgpu_color_settings: struct_size or palette_rgb not set"};
    if (color->flags & ~APTGPU_COLOR_EQUALIZE_LAB) throw Error{ErrorKind::Invalid, "aptgpu_color_settings: unknown flags"};
    if (contrast == APTGPU_CONTRAST_HISTOGRAM_FLOAT)
        throw Error{ErrorKind::Unsupported,
                    "APTGPU_CONTRAST_HISTOGRAM_FLOAT equalises the gray image only: the reference has no float-domain "
                    "equalisation of a false-colour image (pass color = NULL)"};
    if (contrast == APTGPU_CONTRAST_HISTOGRAM) {
        if (!(color->flags & APTGPU_COLOR_EQUALIZE_LAB))
            throw Error{ErrorKind::Unsupported,
                        "histogram equalisation of a false-colour image (CIE Lab, imageext.rs:51-64) needs "
                        "APTGPU_COLOR_EQUALIZE_LAB in aptgpu_color_settings.flags"};
        *lab = true;
    }
    if (channels != 4) throw Error{ErrorKind::Invalid, "false colour needs channels = 4 (RGBA)"};
    // tune_input_values (processing.rs:126-140): the per-call part, f32 as the reference rounds it
    const float factor = 0.3f;
    const float s_a = color->ch_a_tune_start * factor, e_a = color->ch_a_tune_end * factor;
    const float s_b = color->ch_b_tune_start * factor, e_b = color->ch_b_tune_end * factor;
    tune->k_a = 1.f + e_a - s_a;
    tune->o_a = s_a * 255.f;
    tune->k_b = 1.f + e_b - s_b;
    tune->o_b = s_b * 255.f;
    return true;
}

int extreme(const aptgpu_context *ctx, const float *signal, size_t n, float *out, bool want_max, char *err,
            size_t err_cap)
{
    if ((!signal && n) || !out) return APTGPU_ERR_INVALID;
    return guarded(err, err_cap, [&] {
        if (n == 0) throw Error{ErrorKind::Internal, want_max ? kZeroMax : kZeroMin};
        ImageCall c(ctx, signal, n);
        apt::gpu::image_minmax(c.sc.stream, c.d_x.ptr, nullptr, n, n, c.ws.ptr, c.d_info.ptr);
        float lo, hi;
        c.limits(&lo, &hi);
        *out = want_max ? hi : lo;
        return APTGPU_OK;
    });
}

// The map overlay of one call (aptgpu_process_image_map / aptgpu_plan_process_device_image_map).
struct MapCall {
    const aptgpu_map_settings *settings;
    const apt::map::Layers *layers;
};

// The reprojection of one call or recording (the *_project entry points) after its checks: the grid, its graticule
// and the yaw / hscale / vscale of the geometry (the overlay's settings when one is drawn).
struct ProjectCall {
    apt::project::Grid grid;
    std::vector<uint8_t> flags;
    aptgpu_map_settings ms;
    uint64_t bytes() const { return static_cast<uint64_t>(grid.width) * grid.height * 4u; }
};

ProjectCall project_args(const aptgpu_projection_settings *proj, const aptgpu_map_settings *map)
{
    ProjectCall c;
    c.grid = apt::project::checked(proj);
    c.flags = apt::project::graticule(c.grid, proj->grid_deg);
    c.ms = aptgpu_map_settings{sizeof(aptgpu_map_settings), 0, 0., 1., 1.};
    if (map) {
        if (map->struct_size < sizeof(aptgpu_map_settings))
            throw Error{ErrorKind::Invalid, "aptgpu_map_settings: struct_size not set"};
        c.ms = *map;
    }
    return c;
}

// The projection reads the unrotated image and north is up by construction.
void project_rotate(int rotate)
{
    if (rotate != APTGPU_ROTATE_NO)
        throw Error{ErrorKind::Invalid, "a projection takes rotate = APTGPU_ROTATE_NO only: it reads the unrotated image and north is up by construction"};
}

// The checks of the map entry points, after color_args (so Rotate::Orbit stays Unsupported first).
void map_args(int channels, const aptgpu_map_settings *map, const aptgpu_map_layers *layers)
{
    if (!map || map->struct_size < sizeof(aptgpu_map_settings) || !layers)
        throw Error{ErrorKind::Invalid, "aptgpu_map_settings: struct_size not set, or no layer set"};
    if (channels != 4) throw Error{ErrorKind::Invalid, "the map overlay needs channels = 4 (RGBA)"};
}

int layer_index(int layer)
{
    if (layer < APTGPU_MAP_STATES || layer > APTGPU_MAP_LAKES) throw Error{ErrorKind::Invalid, "unknown map layer"};
    return layer;
}

apt::map::Scalars map_scalars(const MapCall &m, const double *positions, size_t count)
{
    return apt::map::scalars(positions, count, m.settings->yaw, m.settings->hscale, m.settings->vscale);
}

apt::map::Colors map_colors(const apt::map::Layers &l)
{
    return apt::map::Colors{{l.color[0], l.color[1], l.color[2]}};
}

// One recording's aptgpu_orbit_settings after its checks: the initialised satellite and the reference time for the
// kernels, the map settings (null: no overlay) and Rotate::Orbit's outcome.
struct SatCall {
    apt::sat::TrackCall call;
    const aptgpu_map_settings *draw_map;
};

// The checks of aptgpu_orbit_settings, then parse + sgp4init (cached for the last TLE and name).
SatCall orbit_args(const aptgpu_orbit_settings *orbit)
{
    if (!orbit || orbit->struct_size < sizeof(aptgpu_orbit_settings))
        throw Error{ErrorKind::Invalid, "aptgpu_orbit_settings: struct_size not set"};
    if (orbit->flags) throw Error{ErrorKind::Invalid, "aptgpu_orbit_settings: unknown flags"};
    if (!orbit->sat_name) throw Error{ErrorKind::Invalid, "aptgpu_orbit_settings: sat_name not set"};
    if (orbit->ref_kind != APTGPU_REF_TIME_START && orbit->ref_kind != APTGPU_REF_TIME_END)
        throw Error{ErrorKind::Invalid, "aptgpu_orbit_settings: unknown ref_kind"};
    if (!orbit->tle)
        throw Error{ErrorKind::Unsupported,
                    "aptgpu_orbit_settings: tle is NULL (the reference then downloads the current TLE, "
                    "misc::get_current_tle; pass the text)"};
    if (orbit->draw_map && orbit->draw_map->struct_size < sizeof(aptgpu_map_settings))
        throw Error{ErrorKind::Invalid, "aptgpu_map_settings: struct_size not set"};
    SatCall c{};
    c.call.rec = apt::sat::satrec_for(orbit->tle, orbit->sat_name);
    c.call.ref_ms = orbit->ref_unix_ms;
    c.call.ref_is_end = orbit->ref_kind == APTGPU_REF_TIME_END;
    c.draw_map = orbit->draw_map;
    return c;
}

// Rotate::Orbit -> Yes / No (noaa_apt.rs:229-234), before anything is launched
int resolve_rotate(int rotate, const SatCall &c)
{
    if (rotate != APTGPU_ROTATE_ORBIT) return rotate;
    return apt::sat::south_to_north_pass(c.call.rec, c.call.ref_ms) ? APTGPU_ROTATE_YES : APTGPU_ROTATE_NO;
}

// The checks of the PNG entry points' settings (nullable: flags 0).
void png_args(const aptgpu_png_settings *png)
{
    if (!png) return;
    if (png->struct_size < sizeof(aptgpu_png_settings))
        throw Error{ErrorKind::Invalid, "aptgpu_png_settings: struct_size not set"};
    if (png->flags) throw Error{ErrorKind::Invalid, "aptgpu_png_settings: unknown flags"};
}

// width, height, channels of an image the encoder takes; returns the filtered stream's bytes
uint64_t png_shape(uint32_t width, uint32_t height, int channels)
{
    if (width == 0 || height == 0) throw Error{ErrorKind::Invalid, "a PNG needs a width and a height of at least 1"};
    if (channels != 1 && channels != 4) throw Error{ErrorKind::Invalid, "channels must be 1 (gray) or 4 (RGBA)"};
    const uint64_t stream = apt::png::stream_bytes(width, height, channels);
    if (stream >= apt::png::kMaxStream) throw Error{ErrorKind::Invalid, "image too large for the PNG encoder (2^31 bytes)"};
    return stream;
}

// Copies the encoded file behind the call's stream to a malloc'd host buffer.
void png_to_host(hipStream_t s, const uint8_t *d_png, size_t len, uint8_t **png_out, size_t *n_out)
{
    uint8_t *h = host_alloc<uint8_t>(len);
    if (len && (hipMemcpyAsync(h, d_png, len, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipStreamSynchronize(s) != hipSuccess)) {
        std::free(h);
        throw Error{ErrorKind::Hip, "D2H copy failed"};
    }
    *png_out = h;
    *n_out = len;
}

// png: encode the image on the device and return the file instead of the pixels
int process_image(const aptgpu_context *ctx, const float *signal, size_t n, int contrast, float percent, int rotate,
                  const aptgpu_color_settings *color, int channels, const MapCall *map, const double *positions,
                  uint8_t **image_out, size_t *n_out, aptgpu_image_result *info, char *err, size_t err_cap,
                  bool png = false, const apt::sat::TrackCall *sat = nullptr, const ProjectCall *pj = nullptr)
{
    if ((!signal && n) || !image_out || !n_out) return APTGPU_ERR_INVALID;
    *image_out = nullptr;
    *n_out = 0;
    return guarded(err, err_cap, [&] {
        apt::gpu::ColorTune tune{};
        bool lab = false;
        const bool colored = color_args(contrast, rotate, color, channels, &tune, &lab);
        if (map && n / 2080 == 0 && n != 0)
            throw Error{ErrorKind::Internal, "map overlay: the image has no row to draw on"};
        if (png && n / 2080 == 0 && n != 0) throw Error{ErrorKind::Invalid, "PNG encoding: the image has no row"};
        if (pj && n / 2080 == 0 && n != 0) throw Error{ErrorKind::Internal, "reprojection: the image has no row to read"};
        std::vector<uint32_t> packed;  // (outlives the call's stream: ~ImageCall synchronises it)
        std::shared_ptr<const apt::lab::Tables> lab_tables;  // (likewise)
        apt::map::Device map_dev;  // (likewise)
        apt::project::Device project_dev;  // (likewise)
        ImageCall c(ctx, signal, n);
        hipStream_t s = c.sc.stream;
        process_limits(ctx, c, contrast, percent, info, lab);
        status(ctx, 0.3f, "Generating image");  // noaa_apt.rs:180
        const size_t bytes = n / 2080 * 2080 * static_cast<size_t>(channels);
        apt::DeviceBuffer<char> cws;
        cws.alloc(apt::gpu::color_ws_bytes());
        apt::hip_check(apt::gpu::color_ws_init(s, cws.ptr), "hipMemsetAsync");
        apt::DeviceBuffer<char> lws;
        if (lab) {
            lab_tables = apt::lab::tables_for(color->palette_rgb);
            lws.alloc(apt::gpu::lab_ws_bytes());
            apt::hip_check(hipMemcpyAsync(lws.ptr, lab_tables.get(), sizeof(apt::lab::Tables), hipMemcpyHostToDevice, s),
                           "hipMemcpyAsync H2D (Lab tables)");
        } else if (colored) {
            packed.resize(65536);
            apt::gpu::color_pack_palette(color->palette_rgb, packed.data());
            apt::hip_check(hipMemcpyAsync(apt::gpu::color_ws_palette(cws.ptr), packed.data(),
                                          packed.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s),
                           "hipMemcpyAsync H2D (palette)");
        }
        apt::DeviceBuffer<uint8_t> d_img;
        d_img.alloc(bytes + 16);
        const bool equalize = contrast == APTGPU_CONTRAST_HISTOGRAM;
        const bool eqfloat = contrast == APTGPU_CONTRAST_HISTOGRAM_FLOAT;
        apt::DeviceBuffer<char> fws;
        if (eqfloat) {
            fws.alloc(apt::gpu::eqfloat_ws_bytes());
            apt::gpu::image_equalize_float(s, c.d_x.ptr, nullptr, n, n, fws.ptr);
        } else if (lab) apt::gpu::image_equalize_lab(s, c.d_x.ptr, nullptr, n, n, c.ws.ptr, cws.ptr, lws.ptr, tune);
        else if (equalize) apt::gpu::image_equalize(s, c.d_x.ptr, nullptr, n, n, c.ws.ptr, cws.ptr);
        if (map) status(ctx, 0.5f, "Drawing map");                                    // noaa_apt.rs:205
        if (rotate == APTGPU_ROTATE_YES) status(ctx, 0.90f, "Rotating output image");  // noaa_apt.rs:229
        if (eqfloat)
            apt::gpu::image_color_float(s, c.d_x.ptr, nullptr, n, n, c.ws.ptr, fws.ptr, channels,
                                        rotate == APTGPU_ROTATE_YES, d_img.ptr, c.d_info.ptr);
        else
            apt::gpu::image_color(s, c.d_x.ptr, nullptr, n, n, c.ws.ptr, cws.ptr, equalize, colored ? &tune : nullptr,
                                  channels, rotate == APTGPU_ROTATE_YES, d_img.ptr, c.d_info.ptr, lab ? lws.ptr : nullptr);
        if (map) {
            const size_t height = n / 2080;
            map_dev.prepare(s, *map->layers, height);
            if (sat) {
                apt::map::image_map_overlay_sat(s, map_dev, *sat, map->settings->yaw, map->settings->hscale,
                                                map->settings->vscale, map_colors(*map->layers),
                                                rotate == APTGPU_ROTATE_YES, d_img.ptr, c.d_info.ptr);
            } else {
                map_dev.upload_track(s, positions, height);
                apt::map::image_map_overlay(s, map_dev, map_scalars(*map, positions, height),
                                            map_colors(*map->layers), static_cast<uint32_t>(height),
                                            rotate == APTGPU_ROTATE_YES, d_img.ptr, c.d_info.ptr);
            }
        } else if (pj) {  // no overlay: the track's x offsets and the call's checks alone
            const size_t height = n / 2080;
            map_dev.prepare_track(s, height);
            if (sat) {
                apt::map::image_map_track_sat(s, map_dev, *sat, pj->ms.yaw, pj->ms.hscale, pj->ms.vscale, c.d_info.ptr);
            } else {
                map_dev.upload_track(s, positions, height);
                apt::map::image_map_track(s, map_dev,
                                          apt::map::scalars(positions, height, pj->ms.yaw, pj->ms.hscale, pj->ms.vscale),
                                          static_cast<uint32_t>(height), c.d_info.ptr);
            }
        }
        apt::DeviceBuffer<char> pws;
        apt::DeviceBuffer<uint8_t> d_png, d_grid;
        if (pj) {
            d_grid.alloc(pj->bytes() + 16);
            project_dev.upload_flags(s, pj->flags);
            apt::map::Scalars host_sc{};
            if (!sat) host_sc = apt::map::scalars(positions, n / 2080, pj->ms.yaw, pj->ms.hscale, pj->ms.vscale);
            apt::project::image_project(s, project_dev, map_dev, sat ? nullptr : &host_sc, pj->grid, d_img.ptr, channels,
                                        d_grid.ptr, pj->bytes(), c.d_info.ptr);
            if (png) {
                png_shape(pj->grid.width, pj->grid.height, 4);
                const uint64_t cap = apt::png::bound(pj->grid.width, pj->grid.height, 4);
                d_png.alloc(cap);
                apt::project::image_project_png(s, project_dev, pj->grid, d_grid.ptr, d_png.ptr, cap, c.d_info.ptr);
            }
        } else if (png) {
            const uint32_t height = static_cast<uint32_t>(n / 2080);
            const uint64_t stream = png_shape(2080, height, channels);
            const uint64_t cap = apt::png::bound(2080, height, channels);
            pws.alloc(apt::png::ws_bytes(stream));
            d_png.alloc(cap);
            apt::png::encode(s, d_img.ptr, 2080, height, channels, pws.ptr, stream, d_png.ptr, cap, c.d_info.ptr, nullptr);
        }
        apt::hip_check(hipGetLastError(), "kernel launch (image stage)");
        const ImageResult r = c.info();
        copy_out(info, r);
        throw_for(r, contrast);
        if (png) {
            png_to_host(s, d_png.ptr, r.reserved, image_out, n_out);
            return APTGPU_OK;
        }
        const size_t out_bytes = pj ? static_cast<size_t>(pj->bytes()) : bytes;
        uint8_t *h = host_alloc<uint8_t>(out_bytes);
        if (out_bytes && (hipMemcpyAsync(h, pj ? d_grid.ptr : d_img.ptr, out_bytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
                          hipStreamSynchronize(s) != hipSuccess)) {
            std::free(h);
            throw Error{ErrorKind::Hip, "D2H copy failed"};
        }
        *image_out = h;
        *n_out = out_bytes;
        return APTGPU_OK;
    });
}

int plan_process_image(aptgpu_plan *plan, int count, const float *const *d_rows, const size_t *rows_cap, int contrast,
                       float percent, int rotate, const aptgpu_color_settings *color, int channels, const MapCall *map,
                       const double *const *positions, const size_t *n_positions, uint8_t *const *d_images, char *err,
                       size_t err_cap, uint8_t *const *d_png = nullptr, const size_t *png_cap = nullptr,
                       const aptgpu_orbit_settings *const *orbit = nullptr, const apt::map::Layers *orbit_layers = nullptr,
                       const std::vector<ProjectCall> *pj = nullptr, uint8_t *const *d_out = nullptr,
                       const size_t *out_cap = nullptr)
{
    if (!plan || count < 0 || !d_rows || !rows_cap || !d_images) return APTGPU_ERR_INVALID;
    if (map && count > 0 && (!positions || !n_positions)) return APTGPU_ERR_INVALID;
    return guarded(err, err_cap, [&] {
        apt::gpu::ColorTune tune{};
        bool lab = false;
        // the orbit form: every recording's satellite, time, map settings and Rotate::Orbit outcome, before any launch
        std::vector<SatCall> sats;
        std::vector<int> rotates(static_cast<size_t>(count), rotate);
        if (orbit) {
            for (int i = 0; i < count; ++i) {
                sats.push_back(orbit_args(orbit[i]));
                rotates[static_cast<size_t>(i)] = resolve_rotate(rotate, sats.back());
                if ((sats.back().draw_map != nullptr) != (sats.front().draw_map != nullptr))
                    throw Error{ErrorKind::Invalid, "draw_map must be set for every recording of the call or for none"};
            }
            // (with a projection the layer set alone asks for the overlay; its settings are the projection's)
            if (!sats.empty() && (pj ? orbit_layers != nullptr : sats.front().draw_map != nullptr)) {
                if (!orbit_layers) throw Error{ErrorKind::Invalid, "draw_map needs a layer set"};
                if (channels != 4) throw Error{ErrorKind::Invalid, "the map overlay needs channels = 4 (RGBA)"};
            }
            if (rotate == APTGPU_ROTATE_ORBIT) rotate = APTGPU_ROTATE_NO;  // (resolved per recording above)
        }
        const bool colored = color_args(contrast, rotate, color, channels, &tune, &lab);
        if (static_cast<size_t>(count) > plan->last_slots.size())
            throw Error{ErrorKind::Invalid, "count exceeds the recordings of the last decode call"};
        if (contrast == APTGPU_CONTRAST_PERCENT && (percent < 0.f || percent > 1.f))
            throw Error{ErrorKind::Internal, kBadPercent};
        const uintptr_t align = channels == 4 ? 15u : 3u;
        for (int i = 0; i < count; ++i) {
            if (!d_rows[i] || !d_images[i]) throw Error{ErrorKind::Invalid, "null device pointer"};
            if (map && !positions[i] && n_positions[i]) throw Error{ErrorKind::Invalid, "null sat_positions"};
            if (d_png && !d_png[i]) throw Error{ErrorKind::Invalid, "null device pointer (d_png)"};
            if (pj && !orbit && (!positions || !n_positions || (!positions[i] && n_positions[i])))
                throw Error{ErrorKind::Invalid, "null sat_positions"};
            if (pj && (!d_out[i] || (reinterpret_cast<uintptr_t>(d_out[i]) & 3u)))
                throw Error{ErrorKind::Invalid, "d_out must be non-null and 4-byte aligned"};
            if (reinterpret_cast<uintptr_t>(d_images[i]) & align)
                throw Error{ErrorKind::Invalid, channels == 4 ? "d_images must be 16-byte aligned for channels = 4"
                                                              : "d_images must be 4-byte aligned"};
        }
        apt::hip_check(hipSetDevice(plan->device), "hipSetDevice");
        if (colored) plan->set_palette(color->palette_rgb, lab);
        for (int i = 0; i < count; ++i)
            plan->enqueue_image_color(i, d_rows[i], static_cast<uint64_t>(rows_cap[i]) * 2080u, contrast, percent,
                                      rotates[static_cast<size_t>(i)] == APTGPU_ROTATE_YES, colored ? &tune : nullptr,
                                      channels, d_images[i], lab);
        const bool orbit_overlay = !sats.empty() && (pj ? orbit_layers != nullptr : sats.front().draw_map != nullptr);
        if (orbit_overlay)
            for (int i = 0; i < count; ++i)
                plan->enqueue_image_map_sat(i, static_cast<uint64_t>(rows_cap[i]) * 2080u, *orbit_layers,
                                            sats[static_cast<size_t>(i)].call,
                                            pj ? (*pj)[static_cast<size_t>(i)].ms : *sats[static_cast<size_t>(i)].draw_map,
                                            map_colors(*orbit_layers),
                                            rotates[static_cast<size_t>(i)] == APTGPU_ROTATE_YES, d_images[i]);
        if (map)
            for (int i = 0; i < count; ++i)
                plan->enqueue_image_map(i, static_cast<uint64_t>(rows_cap[i]) * 2080u, *map->layers,
                                        map_scalars(*map, positions[i], n_positions[i]), map_colors(*map->layers),
                                        positions[i], n_positions[i], rotate == APTGPU_ROTATE_YES, d_images[i]);
        if (pj) {
            for (int i = 0; i < count; ++i) {
                const ProjectCall &c = (*pj)[static_cast<size_t>(i)];
                plan->enqueue_image_project(i, static_cast<uint64_t>(rows_cap[i]) * 2080u, channels, d_images[i], c.grid,
                                            c.flags, c.ms, map != nullptr || orbit_overlay,
                                            positions ? positions[i] : nullptr, n_positions ? n_positions[i] : 0,
                                            orbit ? &sats[static_cast<size_t>(i)].call : nullptr, d_out[i], out_cap[i],
                                            d_png ? d_png[i] : nullptr, d_png ? png_cap[i] : 0);
            }
            return APTGPU_OK;
        }
        if (d_png)
            for (int i = 0; i < count; ++i)
                plan->enqueue_image_png(i, static_cast<uint64_t>(rows_cap[i]) * 2080u, channels, d_images[i], d_png[i],
                                        png_cap[i]);
        return APTGPU_OK;
    });
}

}  // namespace

extern "C" {

const char *aptgpu_channel_name(int index)
{
    return index >= 0 && index < 9 ? kChannelNames[index] : "";
}

int aptgpu_get_min(const aptgpu_context *ctx, const float *signal, size_t n, float *out, char *err,
                   size_t err_cap)
{
    return extreme(ctx, signal, n, out, false, err, err_cap);
}

int aptgpu_get_max(const aptgpu_context *ctx, const float *signal, size_t n, float *out, char *err,
                   size_t err_cap)
{
    return extreme(ctx, signal, n, out, true, err, err_cap);
}

int aptgpu_percent(const aptgpu_context *ctx, const float *signal, size_t n, float percent, float *low,
                   float *high, char *err, size_t err_cap)
{
    if ((!signal && n) || !low || !high) return APTGPU_ERR_INVALID;
    return guarded(err, err_cap, [&] {
        if (percent < 0.f || percent > 1.f) throw Error{ErrorKind::Internal, kBadPercent};  // misc.rs:120-124
        if (n == 0) throw Error{ErrorKind::Internal, kZeroMin};                            // misc.rs:135
        ImageCall c(ctx, signal, n);
        apt::gpu::image_percent(c.sc.stream, c.d_x.ptr, nullptr, n, n, percent, c.ws.ptr, c.d_info.ptr);
        throw_for(c.info(), APTGPU_CONTRAST_PERCENT);
        c.limits(low, high);
        return APTGPU_OK;
    });
}

int aptgpu_map_signal_u8(const aptgpu_context *ctx, const float *signal, size_t n, float low, float high,
                         uint8_t **out, char *err, size_t err_cap)
{
    if ((!signal && n) || !out) return APTGPU_ERR_INVALID;
    *out = nullptr;
    return guarded(err, err_cap, [&] {
        ImageCall c(ctx, signal, n);
        apt::DeviceBuffer<uint8_t> d_img;
        d_img.alloc(n + 16);
        apt::gpu::image_set_limits(c.sc.stream, c.ws.ptr, n, low, high);
        apt::gpu::image_map_u8(c.sc.stream, c.d_x.ptr, nullptr, n, n, c.ws.ptr, false, d_img.ptr, c.d_info.ptr);
        uint8_t *h = host_alloc<uint8_t>(n);
        if (n && (hipMemcpyAsync(h, d_img.ptr, n, hipMemcpyDeviceToHost, c.sc.stream) != hipSuccess ||
                  hipStreamSynchronize(c.sc.stream) != hipSuccess)) {
            std::free(h);
            throw Error{ErrorKind::Hip, "D2H copy failed"};
        }
        *out = h;
        return APTGPU_OK;
    });
}

int aptgpu_read_telemetry(const aptgpu_context *ctx, const float *signal, size_t n,
                          aptgpu_image_result *telemetry, char *err, size_t err_cap)
{
    if ((!signal && n) || !telemetry) return APTGPU_ERR_INVALID;
    return guarded(err, err_cap, [&] {
        ImageCall c(ctx, signal, n);
        apt::gpu::image_telemetry(c.sc.stream, c.d_x.ptr, nullptr, n, n, c.ws.ptr, c.d_info.ptr, false);
        const ImageResult r = c.info();
        copy_out(telemetry, r);
        throw_for(r, APTGPU_CONTRAST_TELEMETRY);
        telemetry_steps(ctx, c, r);
        return APTGPU_OK;
    });
}

int aptgpu_process_gray(const aptgpu_context *ctx, const float *signal, size_t n, int contrast, float percent,
                        int rotate, uint8_t **image_out, size_t *n_out, aptgpu_image_result *info, char *err,
                        size_t err_cap)
{
    if ((!signal && n) || !image_out || !n_out) return APTGPU_ERR_INVALID;
    *image_out = nullptr;
    *n_out = 0;
    return guarded(err, err_cap, [&] {
        if (contrast != APTGPU_CONTRAST_TELEMETRY && contrast != APTGPU_CONTRAST_PERCENT &&
            contrast != APTGPU_CONTRAST_MINMAX)
            throw Error{ErrorKind::Invalid, "unknown contrast adjustment"};
        if (rotate != APTGPU_ROTATE_NO && rotate != APTGPU_ROTATE_YES)
            throw Error{ErrorKind::Unsupported, "Rotate::Orbit needs the satellite and the time: aptgpu_orbit_settings, the *_orbit entry points"};
        ImageCall c(ctx, signal, n);
        hipStream_t s = c.sc.stream;
        process_limits(ctx, c, contrast, percent, info);
        status(ctx, 0.3f, "Generating image");  // noaa_apt.rs:180
        apt::DeviceBuffer<uint8_t> d_img;
        d_img.alloc(n + 16);
        if (rotate == APTGPU_ROTATE_YES) status(ctx, 0.90f, "Rotating output image");  // noaa_apt.rs:229
        apt::gpu::image_map_u8(s, c.d_x.ptr, nullptr, n, n, c.ws.ptr, rotate == APTGPU_ROTATE_YES, d_img.ptr,
                               c.d_info.ptr);
        const ImageResult r = c.info();
        copy_out(info, r);
        throw_for(r, contrast);
        uint8_t *h = host_alloc<uint8_t>(n);
        if (n && (hipMemcpyAsync(h, d_img.ptr, n, hipMemcpyDeviceToHost, s) != hipSuccess ||
                  hipStreamSynchronize(s) != hipSuccess)) {
            std::free(h);
            throw Error{ErrorKind::Hip, "D2H copy failed"};
        }
        *image_out = h;
        *n_out = n;
        return APTGPU_OK;
    });
}

int aptgpu_plan_process_device(aptgpu_plan *plan, int count, const float *const *d_rows,
                               const size_t *rows_cap, int contrast, float percent, int rotate,
                               uint8_t *const *d_images, char *err, size_t err_cap)
{
    if (!plan || count < 0 || !d_rows || !rows_cap || !d_images) return APTGPU_ERR_INVALID;
    return guarded(err, err_cap, [&] {
        if (static_cast<size_t>(count) > plan->last_slots.size())
            throw Error{ErrorKind::Invalid, "count exceeds the recordings of the last decode call"};
        if (contrast < APTGPU_CONTRAST_TELEMETRY || contrast > APTGPU_CONTRAST_MINMAX)
            throw Error{ErrorKind::Invalid, "unknown contrast adjustment"};
        if (rotate != APTGPU_ROTATE_NO && rotate != APTGPU_ROTATE_YES)
            throw Error{ErrorKind::Unsupported, "Rotate::Orbit needs the satellite and the time: aptgpu_orbit_settings, the *_orbit entry points"};
        if (contrast == APTGPU_CONTRAST_PERCENT && (percent < 0.f || percent > 1.f))
            throw Error{ErrorKind::Internal, kBadPercent};
        apt::hip_check(hipSetDevice(plan->device), "hipSetDevice");
        for (int i = 0; i < count; ++i) {
            if (!d_rows[i] || !d_images[i]) throw Error{ErrorKind::Invalid, "null device pointer"};
            plan->enqueue_image(i, d_rows[i], static_cast<uint64_t>(rows_cap[i]) * 2080u, contrast, percent, rotate == APTGPU_ROTATE_YES,
                                d_images[i]);
        }
        return APTGPU_OK;
    });
}

int aptgpu_process_image(const aptgpu_context *ctx, const float *signal, size_t n, int contrast, float percent,
                         int rotate, const aptgpu_color_settings *color, int channels, uint8_t **image_out,
                         size_t *n_out, aptgpu_image_result *info, char *err, size_t err_cap)
{
    return process_image(ctx, signal, n, contrast, percent, rotate, color, channels, nullptr, nullptr, image_out, n_out,
                         info, err, err_cap);
}

int aptgpu_plan_process_device_image(aptgpu_plan *plan, int count, const float *const *d_rows,
                                     const size_t *rows_cap, int contrast, float percent, int rotate,
                                     const aptgpu_color_settings *color, int channels,
                                     uint8_t *const *d_images, char *err, size_t err_cap)
{
    return plan_process_image(plan, count, d_rows, rows_cap, contrast, percent, rotate, color, channels, nullptr,
                              nullptr, nullptr, d_images, err, err_cap);
}

int aptgpu_process_image_map(const aptgpu_context *ctx, const float *signal, size_t n, int contrast,
                             float percent, int rotate, const aptgpu_color_settings *color, int channels,
                             const aptgpu_map_settings *map, const aptgpu_map_layers *layers,
                             const double *sat_positions, uint8_t **image_out, size_t *n_out,
                             aptgpu_image_result *info, char *err, size_t err_cap)
{
    if (!sat_positions && n >= 2080) return APTGPU_ERR_INVALID;
    int rc = guarded(err, err_cap, [&] {
        apt::gpu::ColorTune tune{};
        bool lab = false;
        color_args(contrast, rotate, color, channels, &tune, &lab);
        map_args(channels, map, layers);
        return APTGPU_OK;
    });
    if (rc != APTGPU_OK) return rc;
    const MapCall m{map, &layers->layers};
    return process_image(ctx, signal, n, contrast, percent, rotate, color, channels, &m, sat_positions, image_out,
                         n_out, info, err, err_cap);
}

int aptgpu_plan_process_device_image_map(aptgpu_plan *plan, int count, const float *const *d_rows,
                                         const size_t *rows_cap, int contrast, float percent, int rotate,
                                         const aptgpu_color_settings *color, int channels,
                                         const aptgpu_map_settings *map, const aptgpu_map_layers *layers,
                                         const double *const *sat_positions, const size_t *n_positions,
                                         uint8_t *const *d_images, char *err, size_t err_cap)
{
    int rc = guarded(err, err_cap, [&] {
        apt::gpu::ColorTune tune{};
        bool lab = false;
        color_args(contrast, rotate, color, channels, &tune, &lab);
        map_args(channels, map, layers);
        return APTGPU_OK;
    });
    if (rc != APTGPU_OK) return rc;
    const MapCall m{map, &layers->layers};
    return plan_process_image(plan, count, d_rows, rows_cap, contrast, percent, rotate, color, channels, &m,
                              sat_positions, n_positions, d_images, err, err_cap);
}

size_t aptgpu_png_bound(uint32_t width, uint32_t height, int channels)
{
    if (width == 0 || height == 0 || (channels != 1 && channels != 4)) return 0;
    if (apt::png::stream_bytes(width, height, channels) >= apt::png::kMaxStream) return 0;
    return static_cast<size_t>(apt::png::bound(width, height, channels));
}

int aptgpu_encode_png(const aptgpu_context *ctx, const uint8_t *image, uint32_t width, uint32_t height, int channels,
                      const aptgpu_png_settings *settings, uint8_t **png_out, size_t *n_out, char *err,
                      size_t err_cap)
{
    if (!png_out || !n_out) return APTGPU_ERR_INVALID;
    *png_out = nullptr;
    *n_out = 0;
    return guarded(err, err_cap, [&] {
        // (every check before the device is touched)
        png_args(settings);
        const uint64_t stream = png_shape(width, height, channels);
        if (!image) throw Error{ErrorKind::Invalid, "null image"};
        const size_t bytes = static_cast<size_t>(width) * height * static_cast<size_t>(channels);
        const uint64_t cap = apt::png::bound(width, height, channels);
        Scratch sc(ctx);
        hipStream_t s = sc.stream;
        apt::DeviceBuffer<uint8_t> d_img, d_png;
        apt::DeviceBuffer<char> ws;
        apt::DeviceBuffer<uint64_t> d_len;
        d_img.alloc(bytes + 16);
        d_png.alloc(cap);
        ws.alloc(apt::png::ws_bytes(stream));
        d_len.alloc(1);
        apt::hip_check(hipMemcpyAsync(d_img.ptr, image, bytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync H2D");
        apt::png::encode(s, d_img.ptr, width, height, channels, ws.ptr, stream, d_png.ptr, cap, nullptr, d_len.ptr);
        apt::hip_check(hipGetLastError(), "kernel launch (PNG encoder)");
        uint64_t len = 0;
        apt::hip_check(hipMemcpyAsync(&len, d_len.ptr, sizeof len, hipMemcpyDeviceToHost, s), "hipMemcpyAsync D2H");
        apt::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        if (len == 0 || len > cap) throw Error{ErrorKind::Internal, "PNG encoder: the file exceeds aptgpu_png_bound"};
        png_to_host(s, d_png.ptr, static_cast<size_t>(len), png_out, n_out);
        return APTGPU_OK;
    });
}

// map, layers and sat_positions of the PNG entry points: all given or none
bool png_map_given(const void *map, const void *layers, const void *positions, bool need_positions)
{
    if (!map && !layers && !positions) return false;
    if (!map || !layers || (!positions && need_positions))
        throw Error{ErrorKind::Invalid, "map, layers and sat_positions must be given together"};
    return true;
}

int aptgpu_process_image_png(const aptgpu_context *ctx, const float *signal, size_t n, int contrast, float percent,
                             int rotate, const aptgpu_color_settings *color, int channels,
                             const aptgpu_map_settings *map, const aptgpu_map_layers *layers,
                             const double *sat_positions, const aptgpu_png_settings *png, uint8_t **png_out,
                             size_t *n_out, aptgpu_image_result *info, char *err, size_t err_cap)
{
    bool with_map = false;
    int rc = guarded(err, err_cap, [&] {
        apt::gpu::ColorTune tune{};
        bool lab = false;
        color_args(contrast, rotate, color, channels, &tune, &lab);
        png_args(png);
        with_map = png_map_given(map, layers, sat_positions, n >= 2080);
        if (with_map) map_args(channels, map, layers);
        return APTGPU_OK;
    });
    if (rc != APTGPU_OK) return rc;
    MapCall m{map, with_map ? &layers->layers : nullptr};
    return process_image(ctx, signal, n, contrast, percent, rotate, color, channels, with_map ? &m : nullptr,
                         sat_positions, png_out, n_out, info, err, err_cap, true);
}

int aptgpu_plan_process_device_image_png(aptgpu_plan *plan, int count, const float *const *d_rows,
                                         const size_t *rows_cap, int contrast, float percent, int rotate,
                                         const aptgpu_color_settings *color, int channels,
                                         const aptgpu_map_settings *map, const aptgpu_map_layers *layers,
                                         const double *const *sat_positions, const size_t *n_positions,
                                         uint8_t *const *d_images, const aptgpu_png_settings *png,
                                         uint8_t *const *d_png, const size_t *png_cap, char *err, size_t err_cap)
{
    if (!d_png || !png_cap) return APTGPU_ERR_INVALID;
    bool with_map = false;
    int rc = guarded(err, err_cap, [&] {
        apt::gpu::ColorTune tune{};
        bool lab = false;
        color_args(contrast, rotate, color, channels, &tune, &lab);
        png_args(png);
        with_map = png_map_given(map, layers, sat_positions, true);
        if (with_map) map_args(channels, map, layers);
        return APTGPU_OK;
    });
    if (rc != APTGPU_OK) return rc;
    MapCall m{map, with_map ? &layers->layers : nullptr};
    return plan_process_image(plan, count, d_rows, rows_cap, contrast, percent, rotate, color, channels,
                              with_map ? &m : nullptr, sat_positions, n_positions, d_images, err, err_cap, d_png, png_cap);
}

int aptgpu_sat_track_host(const aptgpu_orbit_settings *orbit, uint32_t height, double *latlon_out, char *err,
                          size_t err_cap)
{
    if (!latlon_out && height) return APTGPU_ERR_INVALID;
    return guarded(err, err_cap, [&] {
        const SatCall c = orbit_args(orbit);
        apt::sat::track_host(c.call.rec, c.call.ref_is_end != 0, c.call.ref_ms, height, latlon_out);
        return APTGPU_OK;
    });
}

int aptgpu_sat_track(const aptgpu_context *ctx, const aptgpu_orbit_settings *orbit, uint32_t height,
                     double *latlon_out, char *err, size_t err_cap)
{
    if (!latlon_out && height) return APTGPU_ERR_INVALID;
    return guarded(err, err_cap, [&] {
        const SatCall c = orbit_args(orbit);
        if (height == 0) return APTGPU_OK;
        Scratch sc(ctx);
        apt::DeviceBuffer<double> d_track;
        apt::DeviceBuffer<uint32_t> d_err;
        d_track.alloc(2 * static_cast<size_t>(height));
        d_err.alloc(1);
        apt::hip_check(hipMemsetAsync(d_err.ptr, 0, sizeof(uint32_t), sc.stream), "hipMemsetAsync");
        apt::sat::track(sc.stream, c.call, nullptr, height, height, d_track.ptr, d_err.ptr);
        apt::hip_check(hipGetLastError(), "kernel launch (satellite track)");
        uint32_t e = 0;
        apt::hip_check(hipMemcpyAsync(&e, d_err.ptr, sizeof e, hipMemcpyDeviceToHost, sc.stream), "hipMemcpyAsync D2H");
        apt::hip_check(hipMemcpyAsync(latlon_out, d_track.ptr, 2 * static_cast<size_t>(height) * sizeof(double),
                                      hipMemcpyDeviceToHost, sc.stream),
                       "hipMemcpyAsync D2H");
        apt::hip_check(hipStreamSynchronize(sc.stream), "hipStreamSynchronize");
        if (e) throw Error{ErrorKind::Internal, apt::sat::error_text(static_cast<int32_t>(e))};
        return APTGPU_OK;
    });
}

int aptgpu_south_to_north_pass(const aptgpu_orbit_settings *orbit, int *out, char *err, size_t err_cap)
{
    if (!out) return APTGPU_ERR_INVALID;
    return guarded(err, err_cap, [&] {
        const SatCall c = orbit_args(orbit);
        *out = apt::sat::south_to_north_pass(c.call.rec, c.call.ref_ms) ? 1 : 0;
        return APTGPU_OK;
    });
}

int aptgpu_process_image_orbit(const aptgpu_context *ctx, const float *signal, size_t n, int contrast, float percent,
                               int rotate, const aptgpu_color_settings *color, int channels,
                               const aptgpu_orbit_settings *orbit, const aptgpu_map_layers *layers, int output,
                               const aptgpu_png_settings *png, uint8_t **out, size_t *n_out,
                               aptgpu_image_result *info, char *err, size_t err_cap)
{
    SatCall c{};
    const int rc = guarded(err, err_cap, [&] {
        if (output != APTGPU_OUTPUT_PIXELS && output != APTGPU_OUTPUT_PNG)
            throw Error{ErrorKind::Invalid, "unknown output kind"};
        c = orbit_args(orbit);
        rotate = resolve_rotate(rotate, c);
        if (output == APTGPU_OUTPUT_PNG) png_args(png);
        if (c.draw_map) map_args(channels, c.draw_map, layers);
        return APTGPU_OK;
    });
    if (rc != APTGPU_OK) return rc;
    MapCall m{c.draw_map, c.draw_map ? &layers->layers : nullptr};
    return process_image(ctx, signal, n, contrast, percent, rotate, color, channels, c.draw_map ? &m : nullptr,
                         nullptr, out, n_out, info, err, err_cap, output == APTGPU_OUTPUT_PNG, &c.call);
}

int aptgpu_plan_process_device_image_orbit(aptgpu_plan *plan, int count, const float *const *d_rows,
                                           const size_t *rows_cap, int contrast, float percent, int rotate,
                                           const aptgpu_color_settings *color, int channels,
                                           const aptgpu_orbit_settings *const *orbit, const aptgpu_map_layers *layers,
                                           uint8_t *const *d_images, const aptgpu_png_settings *png,
                                           uint8_t *const *d_png, const size_t *png_cap, char *err, size_t err_cap)
{
    if (!orbit || (d_png && !png_cap)) return APTGPU_ERR_INVALID;
    if (d_png) {
        const int rc = guarded(err, err_cap, [&] {
            png_args(png);
            return APTGPU_OK;
        });
        if (rc != APTGPU_OK) return rc;
    }
    return plan_process_image(plan, count, d_rows, rows_cap, contrast, percent, rotate, color, channels, nullptr,
                              nullptr, nullptr, d_images, err, err_cap, d_png, png_cap, orbit,
                              layers ? &layers->layers : nullptr);
}

int aptgpu_projection_fit(const double *track, size_t count, double hscale, int kind, double step_deg,
                          uint32_t max_width, aptgpu_projection_settings *out, char *err, size_t err_cap)
{
    if ((!track && count) || !out) return APTGPU_ERR_INVALID;
    return guarded(err, err_cap, [&] {
        apt::project::fit(track, count, hscale, kind, step_deg, max_width, out);
        return APTGPU_OK;
    });
}

int aptgpu_project_image(const aptgpu_context *ctx, const uint8_t *image, uint32_t height, int channels,
                         const double *sat_positions, size_t n_positions, const aptgpu_map_settings *map,
                         const aptgpu_projection_settings *proj, int output, const aptgpu_png_settings *png,
                         uint8_t **out, size_t *n_out, char *err, size_t err_cap)
{
    if (!out || !n_out) return APTGPU_ERR_INVALID;
    *out = nullptr;
    *n_out = 0;
    return guarded(err, err_cap, [&] {
        // (every check before the device is touched)
        if (output != APTGPU_OUTPUT_PIXELS && output != APTGPU_OUTPUT_PNG)
            throw Error{ErrorKind::Invalid, "unknown output kind"};
        if (output == APTGPU_OUTPUT_PNG) png_args(png);
        if (channels != 1 && channels != 4) throw Error{ErrorKind::Invalid, "channels must be 1 (gray) or 4 (RGBA)"};
        const ProjectCall pj = project_args(proj, map);
        if (!image || height == 0) throw Error{ErrorKind::Invalid, "reprojection: the image has no row to read"};
        if (!sat_positions) throw Error{ErrorKind::Invalid, "null sat_positions"};
        if (output == APTGPU_OUTPUT_PNG) png_shape(pj.grid.width, pj.grid.height, 4);
        const size_t bytes = static_cast<size_t>(height) * 2080u * static_cast<size_t>(channels);
        apt::map::Device map_dev;  // (outlive the call's stream: ~Scratch synchronises it)
        apt::project::Device project_dev;
        ImageResult rec{};
        rec.height = height;
        rec.channel_a = rec.channel_b = -1;
        rec.n_px = static_cast<uint64_t>(height) * 2080u;
        Scratch sc(ctx);
        hipStream_t s = sc.stream;
        apt::DeviceBuffer<uint8_t> d_img, d_grid, d_png;
        apt::DeviceBuffer<ImageResult> d_info;
        d_img.alloc(bytes + 16);
        d_grid.alloc(pj.bytes() + 16);
        d_info.alloc(1);
        apt::hip_check(hipMemcpyAsync(d_img.ptr, image, bytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync H2D");
        apt::hip_check(hipMemcpyAsync(d_info.ptr, &rec, sizeof rec, hipMemcpyHostToDevice, s), "hipMemcpyAsync H2D");
        map_dev.prepare_track(s, height);
        map_dev.upload_track(s, sat_positions, n_positions);
        const apt::map::Scalars msc = apt::map::scalars(sat_positions, n_positions, pj.ms.yaw, pj.ms.hscale, pj.ms.vscale);
        apt::map::image_map_track(s, map_dev, msc,
                                  n_positions < 0xffffffffu ? static_cast<uint32_t>(n_positions) : 0xffffffffu, d_info.ptr);
        project_dev.upload_flags(s, pj.flags);
        apt::project::image_project(s, project_dev, map_dev, &msc, pj.grid, d_img.ptr, channels, d_grid.ptr, pj.bytes(),
                                    d_info.ptr);
        if (output == APTGPU_OUTPUT_PNG) {
            const uint64_t cap = apt::png::bound(pj.grid.width, pj.grid.height, 4);
            d_png.alloc(cap);
            apt::project::image_project_png(s, project_dev, pj.grid, d_grid.ptr, d_png.ptr, cap, d_info.ptr);
        }
        apt::hip_check(hipGetLastError(), "kernel launch (reprojection)");
        ImageResult r{};
        apt::hip_check(hipMemcpyAsync(&r, d_info.ptr, sizeof r, hipMemcpyDeviceToHost, s), "hipMemcpyAsync D2H");
        apt::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        throw_for(r, APTGPU_CONTRAST_MINMAX);
        if (output == APTGPU_OUTPUT_PNG) {
            png_to_host(s, d_png.ptr, r.reserved, out, n_out);
            return APTGPU_OK;
        }
        png_to_host(s, d_grid.ptr, static_cast<size_t>(pj.bytes()), out, n_out);
        return APTGPU_OK;
    });
}

int aptgpu_process_image_project(const aptgpu_context *ctx, const float *signal, size_t n, int contrast, float percent,
                                 int rotate, const aptgpu_color_settings *color, int channels,
                                 const aptgpu_map_settings *map, const aptgpu_map_layers *layers,
                                 const double *sat_positions, const aptgpu_orbit_settings *orbit,
                                 const aptgpu_projection_settings *proj, int output, const aptgpu_png_settings *png,
                                 uint8_t **out, size_t *n_out, aptgpu_image_result *info, char *err, size_t err_cap)
{
    SatCall c{};
    ProjectCall pj{};
    const int rc = guarded(err, err_cap, [&] {
        if (output != APTGPU_OUTPUT_PIXELS && output != APTGPU_OUTPUT_PNG)
            throw Error{ErrorKind::Invalid, "unknown output kind"};
        project_rotate(rotate);
        if ((sat_positions != nullptr) == (orbit != nullptr))
            throw Error{ErrorKind::Invalid, "a projection needs exactly one of sat_positions and aptgpu_orbit_settings"};
        apt::gpu::ColorTune tune{};
        bool lab = false;
        color_args(contrast, rotate, color, channels, &tune, &lab);
        if (orbit) c = orbit_args(orbit);
        if (output == APTGPU_OUTPUT_PNG) png_args(png);
        pj = project_args(proj, map ? map : c.draw_map);
        if (layers) map_args(channels, &pj.ms, layers);
        if (output == APTGPU_OUTPUT_PNG) png_shape(pj.grid.width, pj.grid.height, 4);
        return APTGPU_OK;
    });
    if (rc != APTGPU_OK) return rc;
    MapCall m{&pj.ms, layers ? &layers->layers : nullptr};
    return process_image(ctx, signal, n, contrast, percent, rotate, color, channels, layers ? &m : nullptr, sat_positions,
                         out, n_out, info, err, err_cap, output == APTGPU_OUTPUT_PNG, orbit ? &c.call : nullptr, &pj);
}

int aptgpu_plan_process_device_image_project(aptgpu_plan *plan, int count, const float *const *d_rows,
                                             const size_t *rows_cap, int contrast, float percent, int rotate,
                                             const aptgpu_color_settings *color, int channels,
                                             const aptgpu_map_settings *map, const aptgpu_map_layers *layers,
                                             const double *const *sat_positions, const size_t *n_positions,
                                             const aptgpu_orbit_settings *const *orbit, uint8_t *const *d_images,
                                             const aptgpu_projection_settings *proj, uint8_t *const *d_out,
                                             const size_t *out_cap, const aptgpu_png_settings *png,
                                             uint8_t *const *d_png, const size_t *png_cap, char *err, size_t err_cap)
{
    if (count < 0 || (count > 0 && (!proj || !d_out || !out_cap)) || (d_png && !png_cap)) return APTGPU_ERR_INVALID;
    std::vector<ProjectCall> pj;
    const int rc = guarded(err, err_cap, [&] {
        project_rotate(rotate);
        if ((sat_positions != nullptr) == (orbit != nullptr) || (sat_positions && !n_positions))
            throw Error{ErrorKind::Invalid, "a projection needs exactly one of sat_positions and aptgpu_orbit_settings"};
        apt::gpu::ColorTune tune{};
        bool lab = false;
        color_args(contrast, rotate, color, channels, &tune, &lab);
        if (d_png) png_args(png);
        for (int i = 0; i < count; ++i) {
            if (orbit && !orbit[i]) throw Error{ErrorKind::Invalid, "aptgpu_orbit_settings: struct_size not set"};
            pj.push_back(project_args(proj + i, map ? map : (orbit ? orbit[i]->draw_map : nullptr)));
            if (d_png) png_shape(pj.back().grid.width, pj.back().grid.height, 4);
        }
        if (layers && count > 0) map_args(channels, &pj.front().ms, layers);
        return APTGPU_OK;
    });
    if (rc != APTGPU_OK) return rc;
    if (orbit)
        return plan_process_image(plan, count, d_rows, rows_cap, contrast, percent, rotate, color, channels, nullptr,
                                  nullptr, nullptr, d_images, err, err_cap, d_png, png_cap, orbit,
                                  layers ? &layers->layers : nullptr, &pj, d_out, out_cap);
    MapCall m{count > 0 ? &pj.front().ms : nullptr, layers ? &layers->layers : nullptr};
    return plan_process_image(plan, count, d_rows, rows_cap, contrast, percent, rotate, color, channels,
                              layers && count > 0 ? &m : nullptr, sat_positions, n_positions, d_images, err, err_cap, d_png,
                              png_cap, nullptr, nullptr, &pj, d_out, out_cap);
}

int aptgpu_map_layers_create(aptgpu_map_layers **out)
{
    if (!out) return APTGPU_ERR_INVALID;
    *out = nullptr;
    try {
        *out = new aptgpu_map_layers();
    } catch (const std::bad_alloc &) {
        return APTGPU_ERR_INVALID;
    }
    return APTGPU_OK;
}

void aptgpu_map_layers_destroy(aptgpu_map_layers *layers)
{
    delete layers;
}

int aptgpu_map_layers_load_dir(aptgpu_map_layers *layers, const char *dir, char *err, size_t err_cap)
{
    if (!layers || !dir) return APTGPU_ERR_INVALID;
    return guarded(err, err_cap, [&] {
        // res_path!("shapefiles", name): the directory joined with the file name
        std::string base(dir);
        if (!base.empty() && base.back() != '/') base += '/';
        apt::map::Layer st = apt::map::read_shp(base + "states.shp", apt::map::kShpPolyline);
        apt::map::Layer co = apt::map::read_shp(base + "countries.shp", apt::map::kShpPolygon);
        apt::map::Layer la = apt::map::read_shp(base + "lakes.shp", apt::map::kShpPolygon);
        apt::map::Layers &l = layers->layers;
        l.layer[0] = std::move(st);
        l.layer[1] = std::move(co);
        l.layer[2] = std::move(la);
        l.present[0] = l.present[1] = l.present[2] = true;
        l.flatten();
        return APTGPU_OK;
    });
}

int aptgpu_map_layers_set(aptgpu_map_layers *layers, int layer, const double *xy, size_t n_points,
                          const uint32_t *part_offsets, size_t n_parts, char *err, size_t err_cap)
{
    if (!layers || (!xy && n_points) || (!part_offsets && n_parts)) return APTGPU_ERR_INVALID;
    return guarded(err, err_cap, [&] {
        const int k = layer_index(layer);
        if (n_parts == 0) {
            if (n_points) throw Error{ErrorKind::Invalid, "layer: points without parts"};
            layers->layers.clear(k);
            return APTGPU_OK;
        }
        apt::map::Layer l;
        l.xy.assign(xy, xy + 2 * n_points);
        l.parts.assign(part_offsets, part_offsets + n_parts + 1);
        layers->layers.set(k, std::move(l));
        return APTGPU_OK;
    });
}

int aptgpu_map_layers_set_color(aptgpu_map_layers *layers, int layer, const uint8_t rgba[4])
{
    if (!layers || !rgba || layer < APTGPU_MAP_STATES || layer > APTGPU_MAP_LAKES) return APTGPU_ERR_INVALID;
    layers->layers.color[layer] = uint32_t(rgba[0]) | (uint32_t(rgba[1]) << 8) | (uint32_t(rgba[2]) << 16) |
                                  (uint32_t(rgba[3]) << 24);
    return APTGPU_OK;
}

int aptgpu_map_read_shapefile(const char *path, int shape_type, double **xy, size_t *n_points,
                              uint32_t **part_offsets, size_t *n_parts, char *err, size_t err_cap)
{
    if (!path || !xy || !n_points || !part_offsets || !n_parts) return APTGPU_ERR_INVALID;
    *xy = nullptr;
    *part_offsets = nullptr;
    *n_points = *n_parts = 0;
    return guarded(err, err_cap, [&] {
        const apt::map::Layer l = apt::map::read_shp(path, shape_type);
        double *h = host_alloc<double>(l.xy.size());
        uint32_t *o = static_cast<uint32_t *>(std::malloc(l.parts.size() * sizeof(uint32_t)));
        if (!o) {
            std::free(h);
            throw std::bad_alloc();
        }
        std::memcpy(h, l.xy.data(), l.xy.size() * sizeof(double));
        std::memcpy(o, l.parts.data(), l.parts.size() * sizeof(uint32_t));
        *xy = h;
        *part_offsets = o;
        *n_points = l.points();
        *n_parts = l.parts.size() - 1;
        return APTGPU_OK;
    });
}

int aptgpu_despeckle(const aptgpu_context *ctx, const float *signal, size_t n,
                     const aptgpu_despeckle_settings *settings, float **out, aptgpu_despeckle_result *info, char *err,
                     size_t err_cap)
{
    static_assert(sizeof(apt::gpu::DespeckleResult) == sizeof(aptgpu_despeckle_result),
                  "DespeckleResult must mirror aptgpu_despeckle_result");
    if ((!signal && n) || !out) return APTGPU_ERR_INVALID;
    *out = nullptr;
    return guarded(err, err_cap, [&] {
        const apt::despeckle::Settings st = apt::despeckle::check_settings(settings);
        ImageCall c(ctx, signal, n);
        hipStream_t s = c.sc.stream;
        apt::DeviceBuffer<float> d_out;
        apt::DeviceBuffer<apt::gpu::DespeckleResult> d_rec;
        d_out.alloc(n + 16);
        d_rec.alloc(1);
        if (st.threshold != 0.f && n >= 2080)  // (the limits of the unfiltered signal, as Percent(0.98) reports them)
            apt::gpu::image_percent(s, c.d_x.ptr, nullptr, n, n, 0.98f, c.ws.ptr, c.d_info.ptr);
        apt::gpu::despeckle(s, c.d_x.ptr, nullptr, n, n, st.radius, st.threshold,
                            apt::gpu::image_ws_pointers(c.ws.ptr, n).limits, c.d_info.ptr, d_out.ptr, d_rec.ptr);
        apt::hip_check(hipGetLastError(), "kernel launch (despeckle stage)");
        apt::gpu::DespeckleResult r{};
        apt::hip_check(hipMemcpyAsync(&r, d_rec.ptr, sizeof r, hipMemcpyDeviceToHost, s), "hipMemcpyAsync D2H");
        apt::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        if (info) std::memcpy(info, &r, sizeof r);
        if (r.status != 0) throw Error{ErrorKind::Internal, apt::despeckle::reason_text(r.reason)};
        *out = c.sc.download_malloc(d_out.ptr, n);
        return APTGPU_OK;
    });
}

int aptgpu_despeckle_host(const float *signal, size_t n, const aptgpu_despeckle_settings *settings, float **out,
                          aptgpu_despeckle_result *info, char *err, size_t err_cap)
{
    if ((!signal && n) || !out) return APTGPU_ERR_INVALID;
    *out = nullptr;
    return guarded(err, err_cap, [&] {
        const apt::despeckle::Settings st = apt::despeckle::check_settings(settings);
        float *h = host_alloc<float>(n);
        try {
            apt::despeckle::run_host(signal, n, st, h, info);
        } catch (...) {
            std::free(h);
            throw;
        }
        *out = h;
        return APTGPU_OK;
    });
}

int aptgpu_plan_despeckle_device(aptgpu_plan *plan, int count, const float *const *d_rows, const size_t *rows_cap,
                                 const aptgpu_despeckle_settings *settings, float *const *d_out, char *err,
                                 size_t err_cap)
{
    if (!plan || count < 0 || !d_rows || !rows_cap || !d_out) return APTGPU_ERR_INVALID;
    return guarded(err, err_cap, [&] {
        const apt::despeckle::Settings st = apt::despeckle::check_settings(settings);
        if (static_cast<size_t>(count) > plan->last_slots.size())
            throw Error{ErrorKind::Invalid, "count exceeds the recordings of the last decode call"};
        for (int i = 0; i < count; ++i) {
            if (!d_rows[i] || !d_out[i]) throw Error{ErrorKind::Invalid, "null device pointer"};
            const uintptr_t o0 = reinterpret_cast<uintptr_t>(d_out[i]);
            const uintptr_t o1 = o0 + rows_cap[i] * 2080u * sizeof(float);
            for (int j = 0; j < count; ++j) {
                const uintptr_t r0 = reinterpret_cast<uintptr_t>(d_rows[j]);
                const uintptr_t r1 = r0 + rows_cap[j] * 2080u * sizeof(float);
                if (r0 && ((o0 < r1 && r0 < o1) || o0 == r0)) throw Error{ErrorKind::Invalid, "d_out overlaps d_rows"};
            }
        }
        apt::hip_check(hipSetDevice(plan->device), "hipSetDevice");
        for (int i = 0; i < count; ++i)
            plan->enqueue_despeckle(i, d_rows[i], static_cast<uint64_t>(rows_cap[i]) * 2080u, st.radius, st.threshold,
                                    d_out[i]);
        return APTGPU_OK;
    });
}

int aptgpu_plan_despeckle_results(aptgpu_plan *plan, int count, aptgpu_despeckle_result *results)
{
    if (!plan || count < 0 || (!results && count)) return APTGPU_ERR_INVALID;
    if (static_cast<size_t>(count) > plan->last_slots.size()) return APTGPU_ERR_INVALID;
    for (int i = 0; i < count; ++i)
        if (!plan->slot_of(i).despeckle_ws.ptr) return APTGPU_ERR_INVALID;
    try {
        apt::hip_check(hipSetDevice(plan->device), "hipSetDevice");
        plan->sync_all();
        for (int i = 0; i < count; ++i)
            apt::hip_check(hipMemcpy(results + i, apt::gpu::despeckle_ws_record(plan->slot_of(i).despeckle_ws.ptr),
                                     sizeof(aptgpu_despeckle_result), hipMemcpyDeviceToHost),
                           "hipMemcpy");
    } catch (const apt::Error &) {
        return APTGPU_ERR_HIP;
    }
    return APTGPU_OK;
}

int aptgpu_plan_image_results(aptgpu_plan *plan, int count, aptgpu_image_result *results)
{
    if (!plan || count < 0 || (!results && count)) return APTGPU_ERR_INVALID;
    if (static_cast<size_t>(count) > plan->last_slots.size() || !plan->d_image_results.ptr)
        return APTGPU_ERR_INVALID;
    try {
        apt::hip_check(hipSetDevice(plan->device), "hipSetDevice");
        plan->sync_all();
        for (int i = 0; i < count; ++i)
            apt::hip_check(hipMemcpy(results + i,
                                     plan->d_image_results.ptr + plan->last_slots[static_cast<size_t>(i)],
                                     sizeof(aptgpu_image_result), hipMemcpyDeviceToHost),
                           "hipMemcpy");
    } catch (const apt::Error &) {
        return APTGPU_ERR_HIP;
    }
    return APTGPU_OK;
}

}  // extern "C"
