// apt_capi_image.hip — extern "C" surface of include/aptgpu.h §4: the consumers of decode()'s
// pixel rows (contrast limits, u8 mapping, telemetry), host-buffer and device-resident forms.
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "apt_capi_util.hpp"
#include "apt_kernels_color.hpp"
#include "apt_kernels_despeckle.hpp"
#include "apt_kernels_thermal.hpp"
#include "apt_kernels_eqfloat.hpp"
#include "apt_kernels_png.hpp"
#include "apt_kernels_project.hpp"
#include "apt_kernels_track.hpp"
#include "apt_map.hpp"
#include "apt_sat.hpp"

namespace {

using namespace apt::capi;
using apt::gpu::ImageResult;
using apt::ImageJob;
using apt::ImageRequest;
using Recording = apt::ImageRequest::Recording;
using Track = apt::ImageRequest::Track;

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
const char *kCompositePass = "composite: a pass failed, its position count differs from its height or SGP4 failed for a row (APTGPU_COMPOSITE_REASON_PASS)";
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
    case apt::composite::kReasonPass: throw Error{ErrorKind::Internal, kCompositePass};
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
    // the call as one job of the image stages: (res, n, cap) = (null, n, n)
    ImageJob job()
    {
        return ImageJob{sc.stream, d_x.ptr, nullptr, n, n, ws.ptr, d_info.ptr};
    }
    ImageResult info() { return read_record(sc.stream, d_info.ptr); }
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
                    bool lab)
{
    if (contrast == APTGPU_CONTRAST_TELEMETRY) {
        status(ctx, 0.1f, "Adjusting contrast from telemetry");  // noaa_apt.rs:142
    } else if (contrast == APTGPU_CONTRAST_PERCENT) {
        // noaa_apt.rs:152-155
        status(ctx, 0.1f, "Adjusting contrast using " + rust_display_f32(percent * 100.f) + " percent");
        if (percent < 0.f || percent > 1.f) throw Error{ErrorKind::Internal, kBadPercent};
        if (c.n == 0) throw Error{ErrorKind::Internal, kZeroMin};
    } else {
        status(ctx, 0.1f, "Mapping values");  // noaa_apt.rs:159 (MinMax and Histogram)
        if (c.n == 0) throw Error{ErrorKind::Internal, kZeroMin};
    }
    apt::enqueue_image_limits(nullptr, c.job(), lab ? APTGPU_CONTRAST_PERCENT : contrast, lab ? 0.98f : percent);
    if (contrast == APTGPU_CONTRAST_TELEMETRY) {
        const ImageResult r = c.info();
        copy_out(info, r);
        throw_for(r, contrast);
        telemetry_steps(ctx, c, r);
    }
}

void contrast_arg(int contrast, int last)
{
    if (contrast < APTGPU_CONTRAST_TELEMETRY || contrast > last) throw Error{ErrorKind::Invalid, "unknown contrast adjustment"};
}

void rotate_arg(int rotate)
{
    if (rotate != APTGPU_ROTATE_NO && rotate != APTGPU_ROTATE_YES)
        throw Error{ErrorKind::Unsupported, "Rotate::Orbit needs the satellite and the time: aptgpu_orbit_settings, the *_orbit entry points"};
}

void channels_arg(int channels)
{
    if (channels != 1 && channels != 4) throw Error{ErrorKind::Invalid, "channels must be 1 (gray) or 4 (RGBA)"};
}

// The checks of aptgpu_process_image / aptgpu_plan_process_device_image, all before any status callback.
// Fills the request's per-call part: the contrast, the channels and, with false colour, the folded tune values and
// whether the Lab path runs.
void color_args(ImageRequest &q, int contrast, float percent, int rotate, const aptgpu_color_settings *color, int channels)
{
    contrast_arg(contrast, APTGPU_CONTRAST_HISTOGRAM_FLOAT);
    rotate_arg(rotate);
    channels_arg(channels);
    q.contrast = contrast;
    q.percent = percent;
    q.channels = channels;
    if (!color) return;
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
        q.lab = true;
    }
    if (channels != 4) throw Error{ErrorKind::Invalid, "false colour needs channels = 4 (RGBA)"};
    // tune_input_values (processing.rs:126-140): the per-call part, f32 as the reference rounds it
    q.tune = apt::gpu::color_tune_of(color->ch_a_tune_start, color->ch_a_tune_end, color->ch_b_tune_start,
                                     color->ch_b_tune_end);
    q.colored = true;
    q.palette = color->palette_rgb;
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

// yaw / hscale / vscale of one recording's geometry (nullable: 0, 1, 1)
void geom_arg(Recording &r, const aptgpu_map_settings *map)
{
    if (!map) return;
    if (map->struct_size < sizeof(aptgpu_map_settings))
        throw Error{ErrorKind::Invalid, "aptgpu_map_settings: struct_size not set"};
    r.geom = *map;
}

// The reprojection of one recording (the *_project entry points): the grid, its graticule and the yaw / hscale / vscale
// of the geometry (`map`: the overlay's settings when one is drawn, nullable).
void project_args(Recording &r, const aptgpu_projection_settings *proj, const aptgpu_map_settings *map)
{
    r.grid = apt::project::checked(proj);
    r.flags = apt::project::graticule(r.grid, proj->grid_deg);
    geom_arg(r, map);
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
    channels_arg(channels);
    const uint64_t stream = apt::png::stream_bytes(width, height, channels);
    if (stream >= apt::png::kMaxStream) throw Error{ErrorKind::Invalid, "image too large for the PNG encoder (2^31 bytes)"};
    return stream;
}

// Copies `len` bytes of an output behind the call's stream to a malloc'd host buffer.
void to_host(hipStream_t s, const uint8_t *d, size_t len, uint8_t **out, size_t *n_out)
{
    uint8_t *h = host_alloc<uint8_t>(len);
    if (len && (hipMemcpyAsync(h, d, len, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipStreamSynchronize(s) != hipSuccess)) {
        std::free(h);
        throw Error{ErrorKind::Hip, "D2H copy failed"};
    }
    *out = h;
    *n_out = len;
}

// The composite of `count` passes onto one grid (the *_composite_* entry points), every check before the device is
// touched: the pass count, the settings struct, then per pass its image, its channels, its track (`positions` with
// `n_positions`, or `orbit`: exactly one array is given) and its geometry (map and its entries nullable); the grid and
// its graticule go to the first recording.  Fills q.rec, which it sizes, and the per-call part of q.comp.
void composite_args(ImageRequest &q, int count, const uint8_t *const *images, const uint32_t *heights,
                    const int *channels, const double *const *positions, const size_t *n_positions,
                    const aptgpu_orbit_settings *const *orbit, const aptgpu_map_settings *const *map,
                    const aptgpu_projection_settings *proj, const aptgpu_composite_settings *composite)
{
    if (count < 1 || count > APTGPU_COMPOSITE_MAX_PASSES)
        throw Error{ErrorKind::Invalid, "a composite takes 1 to APTGPU_COMPOSITE_MAX_PASSES (16) passes"};
    if (!composite || composite->struct_size < sizeof(aptgpu_composite_settings))
        throw Error{ErrorKind::Invalid, "aptgpu_composite_settings: struct_size not set"};
    if (composite->blend < APTGPU_COMPOSITE_FIRST || composite->blend > APTGPU_COMPOSITE_FEATHER)
        throw Error{ErrorKind::Invalid, "aptgpu_composite_settings: unknown blend"};
    if (composite->reserved) throw Error{ErrorKind::Invalid, "aptgpu_composite_settings: reserved must be 0"};
    if (!images || !heights || !channels) throw Error{ErrorKind::Invalid, "composite: null images, heights or channels"};
    if ((positions != nullptr) == (orbit != nullptr) || (positions && !n_positions))
        throw Error{ErrorKind::Invalid, "a composite needs exactly one of sat_positions and aptgpu_orbit_settings"};
    q.composite = true;
    q.comp.blend = composite->blend;
    q.rec.resize(static_cast<size_t>(count));
    for (int i = 0; i < count; ++i) {
        Recording &r = q.rec[static_cast<size_t>(i)];
        if (!images[i] || heights[i] == 0) throw Error{ErrorKind::Invalid, "composite: a pass has no image or no row"};
        channels_arg(channels[i]);
        if (positions && !positions[i]) throw Error{ErrorKind::Invalid, "null sat_positions"};
        if (orbit && !orbit[i]) throw Error{ErrorKind::Invalid, "aptgpu_orbit_settings: struct_size not set"};
        const aptgpu_map_settings *m = map ? map[i] : nullptr;
        if (i == 0)
            project_args(r, proj, nullptr);
        geom_arg(r, m ? m : (orbit ? orbit[i]->draw_map : nullptr));
        r.channels = channels[i];
        if (positions) {
            r.track = Track::Positions;
            r.positions = positions[i];
            r.n_positions = n_positions[i];
        }
    }
    // (SGP4 initialisation last: it is the only check with a cost)
    if (orbit)
        for (int i = 0; i < count; ++i) {
            q.rec[static_cast<size_t>(i)].track = Track::Sat;
            q.rec[static_cast<size_t>(i)].sat = orbit_args(orbit[i]).call;
        }
}

// APTGPU_OUTPUT_*: whether the PNG file is asked for
bool output_arg(int output)
{
    if (output != APTGPU_OUTPUT_PIXELS && output != APTGPU_OUTPUT_PNG)
        throw Error{ErrorKind::Invalid, "unknown output kind"};
    return output == APTGPU_OUTPUT_PNG;
}

// map, layers and sat_positions of the PNG entry points: all given or none
bool png_map_given(const void *map, const void *layers, const void *positions, bool need_positions)
{
    if (!map && !layers && !positions) return false;
    if (!map || !layers || (!positions && need_positions))
        throw Error{ErrorKind::Invalid, "map, layers and sat_positions must be given together"};
    return true;
}

// The overlay is drawn over every recording of the request, with `map`'s yaw / hscale / vscale where given (a
// projection's or an orbit's settings are in the recordings already).
void set_overlay(ImageRequest &q, const aptgpu_map_layers *layers, const aptgpu_map_settings *map)
{
    q.overlay = true;
    q.layers = &layers->layers;
    if (map)
        for (Recording &r : q.rec) r.geom = *map;
}

// The bare checks of a one-shot entry point's buffers.
bool host_call_ok(const float *signal, size_t n, uint8_t **out, size_t *n_out)
{
    return !((!signal && n) || !out || !n_out);
}

// ... and its outputs before anything is computed (a call that lacks one of them touches neither)
void clear_outputs(uint8_t **out, size_t *n_out)
{
    if (!out || !n_out) return;
    *out = nullptr;
    *n_out = 0;
}

// One host-buffer call under its checked request (one recording): the limits with their status callbacks and host-side
// errors, Telemetry's step export, the stages on call-local buffers, then the record and the download.  The runner
// finishes the recording the entry point built: n_positions (the height), the destinations and their capacities.
int process_image(const aptgpu_context *ctx, const float *signal, size_t n, ImageRequest &q, uint8_t **image_out,
                  size_t *n_out, aptgpu_image_result *info)
{
    Recording &r = q.rec.front();
    const size_t height = n / 2080;
    if (height == 0 && n != 0) {
        if (q.overlay) throw Error{ErrorKind::Internal, "map overlay: the image has no row to draw on"};
        if (q.png) throw Error{ErrorKind::Invalid, "PNG encoding: the image has no row"};
        if (q.project) throw Error{ErrorKind::Internal, "reprojection: the image has no row to read"};
    }
    r.n_positions = height;  // (host positions: one pair per row)
    std::vector<uint32_t> packed;  // (outlives the call's stream: ~ImageCall synchronises it)
    std::shared_ptr<const apt::lab::Tables> lab_tables;  // (likewise)
    apt::map::Device map_dev;  // (likewise)
    apt::project::Device project_dev;  // (likewise)
    ImageCall c(ctx, signal, n);
    hipStream_t s = c.sc.stream;
    process_limits(ctx, c, q.contrast, q.percent, info, q.lab);
    status(ctx, 0.3f, "Generating image");  // noaa_apt.rs:180
    const size_t bytes = height * 2080 * static_cast<size_t>(q.channels);
    apt::DeviceBuffer<char> cws, lws, fws, pws;
    apt::DeviceBuffer<uint8_t> d_img, d_grid, d_png;
    cws.alloc(apt::gpu::color_ws_bytes());
    apt::hip_check(apt::gpu::color_ws_init(s, cws.ptr), "hipMemsetAsync");
    if (q.lab) {
        lab_tables = apt::lab::tables_for(q.palette);
        lws.alloc(apt::gpu::lab_ws_bytes());
        apt::hip_check(hipMemcpyAsync(lws.ptr, lab_tables.get(), sizeof(apt::lab::Tables), hipMemcpyHostToDevice, s),
                       "hipMemcpyAsync H2D (Lab tables)");
    } else if (q.colored) {
        packed.resize(65536);
        apt::gpu::color_pack_palette(q.palette, packed.data());
        apt::hip_check(hipMemcpyAsync(apt::gpu::color_ws_palette(cws.ptr), packed.data(),
                                      packed.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s),
                       "hipMemcpyAsync H2D (palette)");
    }
    d_img.alloc(bytes + 16);
    if (q.contrast == APTGPU_CONTRAST_HISTOGRAM_FLOAT) fws.alloc(apt::gpu::eqfloat_ws_bytes());
    ImageJob j = c.job();
    if (q.project) {
        r.out_cap = r.grid_bytes();
        d_grid.alloc(r.out_cap + 16);
        if (q.png) r.png_cap = apt::png::bound(r.grid.width, r.grid.height, 4);
    } else if (q.png) {  // (the scratch sized by the exact stream)
        j.stream_cap = png_shape(2080, static_cast<uint32_t>(height), q.channels);
        r.png_cap = apt::png::bound(2080, height, q.channels);
        pws.alloc(apt::png::ws_bytes(j.stream_cap));
    }
    d_png.alloc(r.png_cap);
    j.color_ws = cws.ptr;
    j.lab_ws = lws.ptr;
    j.eqfloat_ws = fws.ptr;
    j.png_ws = pws.ptr;
    j.map = &map_dev;
    j.project = &project_dev;
    r.d_image = d_img.ptr;
    r.d_out = d_grid.ptr;
    r.d_png = d_png.ptr;
    if (q.overlay) status(ctx, 0.5f, "Drawing map");           // noaa_apt.rs:205
    if (r.rotate) status(ctx, 0.90f, "Rotating output image");  // noaa_apt.rs:229
    apt::enqueue_image_color(nullptr, q, r, j);
    apt::enqueue_image_outputs(nullptr, q, &j, 1);
    apt::hip_check(hipGetLastError(), "kernel launch (image stage)");
    const ImageResult res = c.info();
    copy_out(info, res);
    throw_for(res, q.contrast);
    if (q.png)
        to_host(s, d_png.ptr, res.reserved, image_out, n_out);
    else if (q.project)
        to_host(s, d_grid.ptr, r.out_cap, image_out, n_out);
    else
        to_host(s, d_img.ptr, bytes, image_out, n_out);
    return APTGPU_OK;
}

// The bare checks every plan form shares.
bool plan_call_ok(const aptgpu_plan *plan, int count, const float *const *d_rows, const size_t *rows_cap,
                  uint8_t *const *d_images)
{
    return plan && count >= 0 && d_rows && rows_cap && d_images;
}

// The fillers of a plan call's recordings.  Each writes its own fields of the q.rec the entry point has sized and reads
// nothing of the request, so their order among themselves does not matter.
// `rotate` (the orbit forms resolve their own after), the image destinations and, when d_png is given, the PNG files':
void plan_recordings(ImageRequest &q, int rotate, uint8_t *const *d_images, uint8_t *const *d_png, const size_t *png_cap)
{
    q.png = d_png != nullptr;
    for (size_t i = 0; i < q.rec.size(); ++i) {
        q.rec[i].rotate = rotate == APTGPU_ROTATE_YES;
        q.rec[i].d_image = d_images[i];
        q.rec[i].d_png = q.png ? d_png[i] : nullptr;
        q.rec[i].png_cap = q.png ? png_cap[i] : 0;
    }
}

// their tracks on the host:
void plan_positions(ImageRequest &q, const double *const *positions, const size_t *n_positions)
{
    for (size_t i = 0; i < q.rec.size(); ++i) {
        q.rec[i].track = Track::Positions;
        q.rec[i].positions = positions[i];
        q.rec[i].n_positions = n_positions[i];
    }
}

// or every recording's satellite, time and Rotate::Orbit outcome (the orbit forms), before any launch.  Returns the
// first recording's draw_map: set for every recording of the call or for none.
const aptgpu_map_settings *plan_orbits(ImageRequest &q, const aptgpu_orbit_settings *const *orbit, int rotate)
{
    const aptgpu_map_settings *first = nullptr;
    for (size_t i = 0; i < q.rec.size(); ++i) {
        const SatCall c = orbit_args(orbit[i]);
        Recording &r = q.rec[i];
        r.track = Track::Sat;
        r.sat = c.call;
        r.rotate = resolve_rotate(rotate, c) == APTGPU_ROTATE_YES;
        if (i == 0) first = c.draw_map;
        if ((c.draw_map != nullptr) != (first != nullptr))
            throw Error{ErrorKind::Invalid, "draw_map must be set for every recording of the call or for none"};
    }
    return first;
}

// The rest of a plan call under its checked request: the checks that need the live plan, then the stages.
int plan_process_image(aptgpu_plan *plan, int count, const float *const *d_rows, const size_t *rows_cap,
                       const ImageRequest &q)
{
    if (static_cast<size_t>(count) > plan->last_slots.size())
        throw Error{ErrorKind::Invalid, "count exceeds the recordings of the last decode call"};
    if (q.contrast == APTGPU_CONTRAST_PERCENT && (q.percent < 0.f || q.percent > 1.f))
        throw Error{ErrorKind::Internal, kBadPercent};
    const uintptr_t align = q.channels == 4 ? 15u : 3u;
    for (int i = 0; i < count; ++i) {
        const Recording &r = q.rec[static_cast<size_t>(i)];
        const bool no_positions = r.track == Track::Positions && !r.positions && r.n_positions;
        if (!d_rows[i] || !r.d_image) throw Error{ErrorKind::Invalid, "null device pointer"};
        if (q.overlay && no_positions) throw Error{ErrorKind::Invalid, "null sat_positions"};
        if (q.png && !r.d_png) throw Error{ErrorKind::Invalid, "null device pointer (d_png)"};
        if (q.project && no_positions) throw Error{ErrorKind::Invalid, "null sat_positions"};
        if (q.project && (!r.d_out || (reinterpret_cast<uintptr_t>(r.d_out) & 3u)))
            throw Error{ErrorKind::Invalid, "d_out must be non-null and 4-byte aligned"};
        if (reinterpret_cast<uintptr_t>(r.d_image) & align)
            throw Error{ErrorKind::Invalid, q.channels == 4 ? "d_images must be 16-byte aligned for channels = 4"
                                                            : "d_images must be 4-byte aligned"};
    }
    apt::hip_check(hipSetDevice(plan->device), "hipSetDevice");
    if (q.colored) plan->set_palette(q.palette, q.lab);
    plan->enqueue_images(q, count, d_rows, rows_cap);
    return APTGPU_OK;
}


// the kernel-argument forms of the caller's coefficients and table
apt::gpu::ThermalCoeffs thermal_coeffs(const aptgpu_thermal_coeffs &c)
{
    apt::gpu::ThermalCoeffs k;
    std::memcpy(k.prt, c.prt, sizeof k.prt);
    std::memcpy(k.channel, c.channel, sizeof k.channel);
    return k;
}
apt::gpu::ThermalTable thermal_table(const apt::thermal::Settings &st)
{
    apt::gpu::ThermalTable t{};
    t.has_palette = st.palette ? 1u : 0u;
    if (st.palette) std::memcpy(t.rgb, st.palette, sizeof t.rgb);
    return t;
}
apt::gpu::ThermalLaunch thermal_launch(const apt::thermal::Settings &st, const float *x, float *kelvin, uint8_t *image)
{
    return apt::gpu::ThermalLaunch{x,          nullptr,   0,         0,      st.channel, st.channel_id, st.image_channels,
                                   st.cold_white, st.t_low, st.t_high, kelvin, image};
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
        size_t n_out = 0;
        to_host(c.sc.stream, d_img.ptr, n, out, &n_out);
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
        contrast_arg(contrast, APTGPU_CONTRAST_MINMAX);
        rotate_arg(rotate);
        ImageCall c(ctx, signal, n);
        hipStream_t s = c.sc.stream;
        process_limits(ctx, c, contrast, percent, info, false);
        status(ctx, 0.3f, "Generating image");  // noaa_apt.rs:180
        apt::DeviceBuffer<uint8_t> d_img;
        d_img.alloc(n + 16);
        if (rotate == APTGPU_ROTATE_YES) status(ctx, 0.90f, "Rotating output image");  // noaa_apt.rs:229
        apt::gpu::image_map_u8(s, c.d_x.ptr, nullptr, n, n, c.ws.ptr, rotate == APTGPU_ROTATE_YES, d_img.ptr,
                               c.d_info.ptr);
        const ImageResult r = c.info();
        copy_out(info, r);
        throw_for(r, contrast);
        to_host(s, d_img.ptr, n, image_out, n_out);
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
        contrast_arg(contrast, APTGPU_CONTRAST_MINMAX);
        rotate_arg(rotate);
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
    if (!host_call_ok(signal, n, image_out, n_out)) return APTGPU_ERR_INVALID;
    clear_outputs(image_out, n_out);
    return guarded(err, err_cap, [&] {
        ImageRequest q(1);
        color_args(q, contrast, percent, rotate, color, channels);
        q.rec[0].rotate = rotate == APTGPU_ROTATE_YES;
        return process_image(ctx, signal, n, q, image_out, n_out, info);
    });
}

int aptgpu_plan_process_device_image(aptgpu_plan *plan, int count, const float *const *d_rows,
                                     const size_t *rows_cap, int contrast, float percent, int rotate,
                                     const aptgpu_color_settings *color, int channels,
                                     uint8_t *const *d_images, char *err, size_t err_cap)
{
    if (!plan_call_ok(plan, count, d_rows, rows_cap, d_images)) return APTGPU_ERR_INVALID;
    return guarded(err, err_cap, [&] {
        ImageRequest q;
        color_args(q, contrast, percent, rotate, color, channels);
        q.rec.resize(static_cast<size_t>(count));
        plan_recordings(q, rotate, d_images, nullptr, nullptr);
        return plan_process_image(plan, count, d_rows, rows_cap, q);
    });
}

int aptgpu_process_image_map(const aptgpu_context *ctx, const float *signal, size_t n, int contrast,
                             float percent, int rotate, const aptgpu_color_settings *color, int channels,
                             const aptgpu_map_settings *map, const aptgpu_map_layers *layers,
                             const double *sat_positions, uint8_t **image_out, size_t *n_out,
                             aptgpu_image_result *info, char *err, size_t err_cap)
{
    if (!sat_positions && n >= 2080) return APTGPU_ERR_INVALID;
    clear_outputs(image_out, n_out);
    return guarded(err, err_cap, [&] {
        ImageRequest q(1);
        color_args(q, contrast, percent, rotate, color, channels);
        map_args(channels, map, layers);
        if (!host_call_ok(signal, n, image_out, n_out)) return APTGPU_ERR_INVALID;
        q.rec[0].rotate = rotate == APTGPU_ROTATE_YES;
        q.rec[0].track = Track::Positions;
        q.rec[0].positions = sat_positions;
        set_overlay(q, layers, map);
        return process_image(ctx, signal, n, q, image_out, n_out, info);
    });
}

int aptgpu_plan_process_device_image_map(aptgpu_plan *plan, int count, const float *const *d_rows,
                                         const size_t *rows_cap, int contrast, float percent, int rotate,
                                         const aptgpu_color_settings *color, int channels,
                                         const aptgpu_map_settings *map, const aptgpu_map_layers *layers,
                                         const double *const *sat_positions, const size_t *n_positions,
                                         uint8_t *const *d_images, char *err, size_t err_cap)
{
    return guarded(err, err_cap, [&] {
        ImageRequest q;
        color_args(q, contrast, percent, rotate, color, channels);
        map_args(channels, map, layers);
        if (!plan_call_ok(plan, count, d_rows, rows_cap, d_images)) return APTGPU_ERR_INVALID;
        if (count > 0 && (!sat_positions || !n_positions)) return APTGPU_ERR_INVALID;
        q.rec.resize(static_cast<size_t>(count));
        plan_recordings(q, rotate, d_images, nullptr, nullptr);
        plan_positions(q, sat_positions, n_positions);
        set_overlay(q, layers, map);
        return plan_process_image(plan, count, d_rows, rows_cap, q);
    });
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
        to_host(s, d_png.ptr, static_cast<size_t>(len), png_out, n_out);
        return APTGPU_OK;
    });
}

int aptgpu_process_image_png(const aptgpu_context *ctx, const float *signal, size_t n, int contrast, float percent,
                             int rotate, const aptgpu_color_settings *color, int channels,
                             const aptgpu_map_settings *map, const aptgpu_map_layers *layers,
                             const double *sat_positions, const aptgpu_png_settings *png, uint8_t **png_out,
                             size_t *n_out, aptgpu_image_result *info, char *err, size_t err_cap)
{
    clear_outputs(png_out, n_out);
    return guarded(err, err_cap, [&] {
        ImageRequest q(1);
        color_args(q, contrast, percent, rotate, color, channels);
        png_args(png);
        const bool with_map = png_map_given(map, layers, sat_positions, n >= 2080);
        if (with_map) map_args(channels, map, layers);
        if (!host_call_ok(signal, n, png_out, n_out)) return APTGPU_ERR_INVALID;
        q.png = true;
        q.rec[0].rotate = rotate == APTGPU_ROTATE_YES;
        if (with_map) {
            q.rec[0].track = Track::Positions;
            q.rec[0].positions = sat_positions;
            set_overlay(q, layers, map);
        }
        return process_image(ctx, signal, n, q, png_out, n_out, info);
    });
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
    return guarded(err, err_cap, [&] {
        ImageRequest q;
        color_args(q, contrast, percent, rotate, color, channels);
        png_args(png);
        const bool with_map = png_map_given(map, layers, sat_positions, true);
        if (with_map) map_args(channels, map, layers);
        if (!plan_call_ok(plan, count, d_rows, rows_cap, d_images)) return APTGPU_ERR_INVALID;
        if (with_map && count > 0 && !n_positions) return APTGPU_ERR_INVALID;
        q.rec.resize(static_cast<size_t>(count));
        plan_recordings(q, rotate, d_images, d_png, png_cap);
        if (with_map) {
            plan_positions(q, sat_positions, n_positions);
            set_overlay(q, layers, map);
        }
        return plan_process_image(plan, count, d_rows, rows_cap, q);
    });
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
    clear_outputs(out, n_out);
    return guarded(err, err_cap, [&] {
        ImageRequest q(1);
        Recording &r = q.rec[0];
        q.png = output_arg(output);
        const SatCall c = orbit_args(orbit);
        rotate = resolve_rotate(rotate, c);
        if (q.png) png_args(png);
        if (c.draw_map) map_args(channels, c.draw_map, layers);
        if (!host_call_ok(signal, n, out, n_out)) return APTGPU_ERR_INVALID;
        color_args(q, contrast, percent, rotate, color, channels);
        r.rotate = rotate == APTGPU_ROTATE_YES;
        r.track = Track::Sat;
        r.sat = c.call;
        if (c.draw_map) set_overlay(q, layers, c.draw_map);
        return process_image(ctx, signal, n, q, out, n_out, info);
    });
}

int aptgpu_plan_process_device_image_orbit(aptgpu_plan *plan, int count, const float *const *d_rows,
                                           const size_t *rows_cap, int contrast, float percent, int rotate,
                                           const aptgpu_color_settings *color, int channels,
                                           const aptgpu_orbit_settings *const *orbit, const aptgpu_map_layers *layers,
                                           uint8_t *const *d_images, const aptgpu_png_settings *png,
                                           uint8_t *const *d_png, const size_t *png_cap, char *err, size_t err_cap)
{
    if (!orbit || (d_png && !png_cap)) return APTGPU_ERR_INVALID;
    return guarded(err, err_cap, [&] {
        ImageRequest q;
        if (d_png) png_args(png);
        if (!plan_call_ok(plan, count, d_rows, rows_cap, d_images)) return APTGPU_ERR_INVALID;
        q.rec.resize(static_cast<size_t>(count));
        plan_recordings(q, rotate, d_images, d_png, png_cap);
        if (plan_orbits(q, orbit, rotate)) {
            if (!layers) throw Error{ErrorKind::Invalid, "draw_map needs a layer set"};
            if (channels != 4) throw Error{ErrorKind::Invalid, "the map overlay needs channels = 4 (RGBA)"};
            for (int i = 0; i < count; ++i) q.rec[static_cast<size_t>(i)].geom = *orbit[i]->draw_map;
            set_overlay(q, layers, nullptr);
        }
        // (Rotate::Orbit is resolved per recording above)
        color_args(q, contrast, percent, rotate == APTGPU_ROTATE_ORBIT ? APTGPU_ROTATE_NO : rotate, color, channels);
        return plan_process_image(plan, count, d_rows, rows_cap, q);
    });
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
        ImageRequest q(1);
        Recording &r = q.rec[0];
        q.png = output_arg(output);
        if (q.png) png_args(png);
        channels_arg(channels);
        project_args(r, proj, map);
        if (!image || height == 0) throw Error{ErrorKind::Invalid, "reprojection: the image has no row to read"};
        if (!sat_positions) throw Error{ErrorKind::Invalid, "null sat_positions"};
        if (q.png) png_shape(r.grid.width, r.grid.height, 4);
        q.project = true;
        q.channels = channels;
        r.track = Track::Positions;
        r.positions = sat_positions;
        r.n_positions = n_positions;
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
        r.out_cap = r.grid_bytes();
        if (q.png) r.png_cap = apt::png::bound(r.grid.width, r.grid.height, 4);
        d_img.alloc(bytes + 16);
        d_grid.alloc(r.out_cap + 16);
        d_png.alloc(r.png_cap);
        d_info.alloc(1);
        r.d_image = d_img.ptr;
        r.d_out = d_grid.ptr;
        r.d_png = d_png.ptr;
        // the finished image as a job behind its colour stage, with a hand-made record
        ImageJob j{};
        j.stream = s;
        j.cap = rec.n_px;
        j.info = d_info.ptr;
        j.map = &map_dev;
        j.project = &project_dev;
        apt::hip_check(hipMemcpyAsync(d_img.ptr, image, bytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync H2D");
        apt::hip_check(hipMemcpyAsync(d_info.ptr, &rec, sizeof rec, hipMemcpyHostToDevice, s), "hipMemcpyAsync H2D");
        apt::enqueue_image_outputs(nullptr, q, &j, 1);
        apt::hip_check(hipGetLastError(), "kernel launch (reprojection)");
        const ImageResult res = read_record(s, d_info.ptr);
        throw_for(res, APTGPU_CONTRAST_MINMAX);
        if (q.png)
            to_host(s, d_png.ptr, res.reserved, out, n_out);
        else
            to_host(s, d_grid.ptr, r.out_cap, out, n_out);
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
    clear_outputs(out, n_out);
    return guarded(err, err_cap, [&] {
        ImageRequest q(1);
        Recording &r = q.rec[0];
        q.png = output_arg(output);
        project_rotate(rotate);
        if ((sat_positions != nullptr) == (orbit != nullptr))
            throw Error{ErrorKind::Invalid, "a projection needs exactly one of sat_positions and aptgpu_orbit_settings"};
        color_args(q, contrast, percent, rotate, color, channels);
        SatCall c{};
        if (orbit) c = orbit_args(orbit);
        if (q.png) png_args(png);
        project_args(r, proj, map ? map : c.draw_map);
        if (layers) map_args(channels, &r.geom, layers);
        if (q.png) png_shape(r.grid.width, r.grid.height, 4);
        if (!host_call_ok(signal, n, out, n_out)) return APTGPU_ERR_INVALID;
        q.project = true;
        r.track = orbit ? Track::Sat : Track::Positions;
        r.sat = c.call;
        r.positions = sat_positions;
        if (layers) set_overlay(q, layers, nullptr);
        return process_image(ctx, signal, n, q, out, n_out, info);
    });
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
    return guarded(err, err_cap, [&] {
        ImageRequest q;
        project_rotate(rotate);
        if ((sat_positions != nullptr) == (orbit != nullptr) || (sat_positions && !n_positions))
            throw Error{ErrorKind::Invalid, "a projection needs exactly one of sat_positions and aptgpu_orbit_settings"};
        color_args(q, contrast, percent, rotate, color, channels);
        if (d_png) png_args(png);
        q.project = true;
        q.rec.resize(static_cast<size_t>(count));
        for (int i = 0; i < count; ++i) {
            Recording &r = q.rec[static_cast<size_t>(i)];
            if (orbit && !orbit[i]) throw Error{ErrorKind::Invalid, "aptgpu_orbit_settings: struct_size not set"};
            project_args(r, proj + i, map ? map : (orbit ? orbit[i]->draw_map : nullptr));
            if (d_png) png_shape(r.grid.width, r.grid.height, 4);
            r.d_out = d_out[i];
            r.out_cap = out_cap[i];
        }
        if (layers && count > 0) map_args(channels, &q.rec[0].geom, layers);
        if (!plan_call_ok(plan, count, d_rows, rows_cap, d_images)) return APTGPU_ERR_INVALID;
        plan_recordings(q, rotate, d_images, d_png, png_cap);
        if (orbit)
            plan_orbits(q, orbit, rotate);
        else
            plan_positions(q, sat_positions, n_positions);
        if (layers && count > 0) set_overlay(q, layers, nullptr);
        return plan_process_image(plan, count, d_rows, rows_cap, q);
    });
}

int aptgpu_projection_fit_many(const double *const *tracks, const size_t *counts, size_t n_tracks, double hscale,
                               int kind, double step_deg, uint32_t max_width, aptgpu_projection_settings *out,
                               char *err, size_t err_cap)
{
    if (!tracks || !counts || !out) return APTGPU_ERR_INVALID;
    for (size_t t = 0; t < n_tracks; ++t)
        if (!tracks[t] && counts[t]) return APTGPU_ERR_INVALID;
    return guarded(err, err_cap, [&] {
        apt::project::fit_many(tracks, counts, n_tracks, hscale, kind, step_deg, max_width, out);
        return APTGPU_OK;
    });
}

int aptgpu_composite_images(const aptgpu_context *ctx, int count, const uint8_t *const *images,
                            const uint32_t *heights, const int *channels, const double *const *sat_positions,
                            const size_t *n_positions, const aptgpu_map_settings *const *map,
                            const aptgpu_projection_settings *proj, const aptgpu_composite_settings *composite,
                            int output, const aptgpu_png_settings *png, uint8_t **out, size_t *n_out,
                            uint8_t **coverage, char *err, size_t err_cap)
{
    if (!out || !n_out) return APTGPU_ERR_INVALID;
    *out = nullptr;
    *n_out = 0;
    if (coverage) *coverage = nullptr;
    return guarded(err, err_cap, [&] {
        // (every check before the device is touched)
        ImageRequest q;
        q.png = output_arg(output);
        if (q.png) png_args(png);
        if (!sat_positions) throw Error{ErrorKind::Invalid, "null sat_positions"};
        composite_args(q, count, images, heights, channels, sat_positions, n_positions, nullptr, map, proj, composite);
        const apt::project::Grid &g = q.rec[0].grid;
        if (q.png) png_shape(g.width, g.height, 4);
        const size_t k = static_cast<size_t>(count), pixels = static_cast<size_t>(g.width) * g.height;
        std::vector<std::unique_ptr<apt::map::Device>> maps(k);  // (outlive the call's stream: ~Scratch synchronises it)
        apt::composite::Device dev;
        std::vector<ImageResult> recs(k);
        Scratch sc(ctx);
        hipStream_t s = sc.stream;
        std::vector<apt::DeviceBuffer<uint8_t>> d_img(k);
        apt::DeviceBuffer<uint8_t> d_grid, d_cov, d_png;
        apt::DeviceBuffer<ImageResult> d_info;
        q.comp.dev = &dev;
        q.comp.out_cap = q.rec[0].grid_bytes();
        if (q.png) q.comp.png_cap = apt::png::bound(g.width, g.height, 4);
        d_grid.alloc(q.comp.out_cap + 16);
        d_png.alloc(q.comp.png_cap);
        if (coverage) d_cov.alloc(pixels);
        d_info.alloc(k);
        q.comp.d_out = d_grid.ptr;
        q.comp.d_coverage = d_cov.ptr;
        q.comp.d_png = d_png.ptr;
        // every finished image as a job behind its colour stage, with a hand-made record
        std::vector<ImageJob> jobs(k);
        for (size_t i = 0; i < k; ++i) {
            Recording &r = q.rec[i];
            const size_t bytes = static_cast<size_t>(heights[i]) * 2080u * static_cast<size_t>(r.channels);
            recs[i].height = heights[i];
            recs[i].channel_a = recs[i].channel_b = -1;
            recs[i].n_px = static_cast<uint64_t>(heights[i]) * 2080u;
            maps[i] = std::make_unique<apt::map::Device>();
            d_img[i].alloc(bytes + 16);
            apt::hip_check(hipMemcpyAsync(d_img[i].ptr, images[i], bytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync H2D");
            r.d_image = d_img[i].ptr;
            jobs[i].stream = s;
            jobs[i].cap = recs[i].n_px;
            jobs[i].info = d_info.ptr + i;
            jobs[i].map = maps[i].get();
        }
        apt::hip_check(hipMemcpyAsync(d_info.ptr, recs.data(), k * sizeof(ImageResult), hipMemcpyHostToDevice, s),
                       "hipMemcpyAsync H2D");
        apt::enqueue_image_outputs(nullptr, q, jobs.data(), count);
        apt::hip_check(hipGetLastError(), "kernel launch (composite)");
        const ImageResult res = read_record(s, dev.info);
        throw_for(res, APTGPU_CONTRAST_MINMAX);
        HostPtr<uint8_t> cov;
        if (coverage) {
            uint8_t *h = nullptr;
            size_t n_cov = 0;
            to_host(s, d_cov.ptr, pixels, &h, &n_cov);
            cov.reset(h);
        }
        if (q.png)
            to_host(s, d_png.ptr, res.reserved, out, n_out);
        else
            to_host(s, d_grid.ptr, q.comp.out_cap, out, n_out);
        if (coverage) *coverage = cov.release();
        return APTGPU_OK;
    });
}

int aptgpu_plan_composite_device_images(aptgpu_plan *plan, int count, const uint8_t *const *d_images,
                                        const uint32_t *heights, const int *channels,
                                        const double *const *sat_positions, const size_t *n_positions,
                                        const aptgpu_orbit_settings *const *orbit,
                                        const aptgpu_map_settings *const *map, const aptgpu_projection_settings *proj,
                                        const aptgpu_composite_settings *composite, uint8_t *d_out, size_t out_cap,
                                        uint8_t *d_coverage, const aptgpu_png_settings *png, uint8_t *d_png,
                                        size_t png_cap, char *err, size_t err_cap)
{
    return guarded(err, err_cap, [&] {
        ImageRequest q;
        q.png = d_png != nullptr;
        if (q.png) png_args(png);
        composite_args(q, count, d_images, heights, channels, sat_positions, n_positions, orbit, map, proj, composite);
        if (q.png) png_shape(q.rec[0].grid.width, q.rec[0].grid.height, 4);
        if (!plan) return APTGPU_ERR_INVALID;
        if (!d_out || (reinterpret_cast<uintptr_t>(d_out) & 3u))
            throw Error{ErrorKind::Invalid, "d_out must be non-null and 4-byte aligned"};
        if (static_cast<size_t>(count) > plan->last_slots.size())
            throw Error{ErrorKind::Invalid, "count exceeds the recordings of the last decode call"};
        if (!plan->d_image_results.ptr)
            throw Error{ErrorKind::Invalid, "composite: no image stage has run on this plan (aptgpu_plan_process_device_image first)"};
        for (int i = 0; i < count; ++i) {
            Recording &r = q.rec[static_cast<size_t>(i)];
            if (r.channels == 4 && (reinterpret_cast<uintptr_t>(d_images[i]) & 3u))
                throw Error{ErrorKind::Invalid, "d_images must be 4-byte aligned for channels = 4"};
            r.d_image = const_cast<uint8_t *>(d_images[i]);
        }
        q.comp.d_out = d_out;
        q.comp.out_cap = out_cap;
        q.comp.d_coverage = d_coverage;
        q.comp.d_png = d_png;
        q.comp.png_cap = png_cap;
        apt::hip_check(hipSetDevice(plan->device), "hipSetDevice");
        plan->enqueue_composite(q, count, heights);
        return APTGPU_OK;
    });
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
        HostPtr<double> h(host_alloc<double>(l.xy.size()));
        HostPtr<uint32_t> o(host_alloc<uint32_t>(l.parts.size()));
        std::memcpy(h.get(), l.xy.data(), l.xy.size() * sizeof(double));
        std::memcpy(o.get(), l.parts.data(), l.parts.size() * sizeof(uint32_t));
        *xy = h.release();
        *part_offsets = o.release();
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
        apt::DeviceBuffer<float> d_out;
        apt::DeviceBuffer<apt::gpu::DespeckleResult> d_rec;
        d_out.alloc(n + 16);
        d_rec.alloc(1);
        apt::enqueue_despeckle(nullptr, c.job(), st.radius, st.threshold, d_out.ptr, d_rec.ptr);
        const apt::gpu::DespeckleResult r = read_record(c.sc.stream, d_rec.ptr);
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
        HostSignal h(host_alloc<float>(n));
        apt::despeckle::run_host(signal, n, st, h.get(), info);
        *out = h.release();
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
            if (overlaps_rows(d_out[i], rows_cap[i] * 2080u * sizeof(float), count, d_rows, rows_cap))
                throw Error{ErrorKind::Invalid, "d_out overlaps d_rows"};
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
    return plan_results(
        plan, count, results,
        [&](int i) -> apt::gpu::DespeckleResult * {
            void *ws = plan->slot_of(i).despeckle_ws.ptr;
            return ws ? apt::gpu::despeckle_ws_record(ws) : nullptr;
        },
        [&](int i, const apt::gpu::DespeckleResult &r) { std::memcpy(results + i, &r, sizeof r); });
}

int aptgpu_calibrate_thermal(const aptgpu_context *ctx, const float *signal, size_t n,
                             const aptgpu_thermal_coeffs *coeffs, const aptgpu_thermal_settings *settings,
                             float **kelvin, uint8_t **image, aptgpu_thermal_result *info, char *err, size_t err_cap)
{
    if ((!signal && n) || !kelvin) return APTGPU_ERR_INVALID;
    *kelvin = nullptr;
    if (image) *image = nullptr;
    return guarded(err, err_cap, [&] {
        const apt::thermal::Settings st = apt::thermal::check_settings(coeffs, settings);
        if ((st.image_channels != 0) != (image != nullptr))
            throw Error{ErrorKind::Invalid, "thermal: image is required exactly when image_channels is not 0"};
        ImageCall c(ctx, signal, n);
        hipStream_t s = c.sc.stream;
        const size_t h = n / 2080u;
        const size_t image_bytes = h * 2080u * static_cast<size_t>(st.image_channels);
        apt::DeviceBuffer<float> d_kelvin;
        apt::DeviceBuffer<uint8_t> d_image;
        apt::DeviceBuffer<char> ws;
        d_kelvin.alloc(h * APTGPU_THERMAL_PX + 16);
        d_image.alloc(image_bytes + 16);
        ws.alloc(apt::gpu::thermal_ws_bytes());
        apt::enqueue_thermal(nullptr, c.job(),
                             thermal_launch(st, c.d_x.ptr, d_kelvin.ptr, st.image_channels ? d_image.ptr : nullptr),
                             thermal_coeffs(*coeffs), thermal_table(st), ws.ptr);
        const apt::gpu::ThermalRecord r = read_record(s, apt::gpu::thermal_ws_record(ws.ptr));
        if (info) apt::gpu::thermal_record_to_public(r, info);
        if (r.status != 0) throw Error{ErrorKind::Internal, apt::thermal::reason_text(r.reason)};
        HostSignal hk(c.sc.download_malloc(d_kelvin.ptr, h * APTGPU_THERMAL_PX));
        size_t n_out = 0;
        if (st.image_channels) to_host(s, d_image.ptr, image_bytes, image, &n_out);
        *kelvin = hk.release();
        return APTGPU_OK;
    });
}

int aptgpu_calibrate_thermal_host(const float *signal, size_t n, const aptgpu_thermal_coeffs *coeffs,
                                  const aptgpu_thermal_settings *settings, float **kelvin, uint8_t **image,
                                  aptgpu_thermal_result *info, char *err, size_t err_cap)
{
    if ((!signal && n) || !kelvin) return APTGPU_ERR_INVALID;
    *kelvin = nullptr;
    if (image) *image = nullptr;
    return guarded(err, err_cap, [&] {
        const apt::thermal::Settings st = apt::thermal::check_settings(coeffs, settings);
        if ((st.image_channels != 0) != (image != nullptr))
            throw Error{ErrorKind::Invalid, "thermal: image is required exactly when image_channels is not 0"};
        const size_t h = n / 2080u;
        HostSignal hk(host_alloc<float>(h * APTGPU_THERMAL_PX));
        HostPtr<uint8_t> hi(st.image_channels ? host_alloc<uint8_t>(h * 2080u * static_cast<size_t>(st.image_channels)) : nullptr);
        apt::thermal::run_host(signal, n, *coeffs, st, hk.get(), hi.get(), info);
        *kelvin = hk.release();
        if (image) *image = hi.release();
        return APTGPU_OK;
    });
}

int aptgpu_plan_calibrate_thermal_device(aptgpu_plan *plan, int count, const float *const *d_rows,
                                         const size_t *rows_cap, const aptgpu_thermal_coeffs *coeffs,
                                         const aptgpu_thermal_settings *settings, float *const *d_kelvin,
                                         uint8_t *const *d_images, char *err, size_t err_cap)
{
    if (!plan || count < 0 || !d_rows || !rows_cap || !d_kelvin) return APTGPU_ERR_INVALID;
    return guarded(err, err_cap, [&] {
        const apt::thermal::Settings st = apt::thermal::check_settings(coeffs, settings);
        if ((st.image_channels != 0) != (d_images != nullptr))
            throw Error{ErrorKind::Invalid, "thermal: d_images is required exactly when image_channels is not 0"};
        if (static_cast<size_t>(count) > plan->last_slots.size())
            throw Error{ErrorKind::Invalid, "count exceeds the recordings of the last decode call"};
        for (int i = 0; i < count; ++i) {
            if (!d_rows[i] || !d_kelvin[i] || (d_images && !d_images[i]))
                throw Error{ErrorKind::Invalid, "null device pointer"};
            if (overlaps_rows(d_kelvin[i], rows_cap[i] * APTGPU_THERMAL_PX * sizeof(float), count, d_rows, rows_cap))
                throw Error{ErrorKind::Invalid, "d_kelvin overlaps d_rows"};
            if (d_images && overlaps_rows(d_images[i], rows_cap[i] * 2080u * static_cast<size_t>(st.image_channels), count,
                                          d_rows, rows_cap))
                throw Error{ErrorKind::Invalid, "d_images overlaps d_rows"};
            if (st.image_channels == 4 && (reinterpret_cast<uintptr_t>(d_images[i]) & 3u))
                throw Error{ErrorKind::Invalid, "d_images must be 4-byte aligned"};
        }
        apt::hip_check(hipSetDevice(plan->device), "hipSetDevice");
        const apt::gpu::ThermalCoeffs kc = thermal_coeffs(*coeffs);
        const apt::gpu::ThermalTable table = thermal_table(st);
        for (int i = 0; i < count; ++i)
            plan->enqueue_thermal(i, static_cast<uint64_t>(rows_cap[i]) * 2080u,
                                  thermal_launch(st, d_rows[i], d_kelvin[i], d_images ? d_images[i] : nullptr), kc, table);
        return APTGPU_OK;
    });
}

int aptgpu_plan_thermal_results(aptgpu_plan *plan, int count, aptgpu_thermal_result *results)
{
    return plan_results(
        plan, count, results,
        [&](int i) -> apt::gpu::ThermalRecord * {
            void *ws = plan->slot_of(i).thermal_ws.ptr;
            return ws ? apt::gpu::thermal_ws_record(ws) : nullptr;
        },
        [&](int i, const apt::gpu::ThermalRecord &r) { apt::gpu::thermal_record_to_public(r, results + i); });
}

int aptgpu_plan_image_results(aptgpu_plan *plan, int count, aptgpu_image_result *results)
{
    if (!plan || count < 0 || (!results && count) || !plan->d_image_results.ptr) return APTGPU_ERR_INVALID;
    // one record past the passes of the latest composite: the composite's own, read behind the passes'
    const bool with_composite = plan->composite_count >= 0 && count == plan->composite_count + 1;
    if (with_composite) --count;
    const int rc = plan_results(
        plan, count, results, [&](int i) { return plan->d_image_results.ptr + plan->last_slots[static_cast<size_t>(i)]; },
        [&](int i, const ImageResult &r) { copy_out(results + i, r); });
    if (rc != APTGPU_OK || !with_composite) return rc;
    if (hipMemcpy(results + count, plan->composite[static_cast<size_t>(plan->last_stream)]->info,
                  sizeof(aptgpu_image_result), hipMemcpyDeviceToHost) != hipSuccess)
        return APTGPU_ERR_HIP;
    return APTGPU_OK;
}

}  // extern "C"
