// apt_capi_fit.hip — extern "C" surface of the overlay fit (include/aptgpu.h §4, "fitting the map overlay to the
// image"): a host image on the GPU, an image already on the device, the same on the CPU, and the
// sampler alone.
#include <memory>
#include <vector>

#include "apt_capi_util.hpp"
#include "apt_kernels_fit.hpp"

namespace {

using namespace apt::capi;
namespace fit = apt::fit;

void clear(void **scores_out, size_t *n_scores)
{
    if (scores_out) *scores_out = nullptr;
    if (n_scores) *n_scores = 0;
}

// the checks every form shares, in the order the header gives them; none touches a device
struct Checked {
    fit::Settings st;
    apt::geoloc::Geom geom;
    std::vector<double> points;
};
Checked checked(const void *image, size_t h, const void *positions, const aptgpu_orbit_settings *orbit,
                const aptgpu_map_layers *layers, const aptgpu_map_settings *map, const aptgpu_fit_settings *settings)
{
    Checked c{fit::check_settings(settings), apt::geoloc::check_geom(map), {}};
    if (!image) throw Error{ErrorKind::Invalid, "fit: the image is required"};
    if (!layers) throw Error{ErrorKind::Invalid, "fit: the layer set is required"};
    fit::check_call(positions, orbit, h, c.st);
    c.points = fit::sample_points(layers->layers, c.st.mask, c.st.spacing);
    return c;
}

// the orbit as the long track's: row -M's time as a start time
SatCall long_track_call(const aptgpu_orbit_settings *orbit, size_t h, const fit::Settings &st)
{
    SatCall sat = orbit_args(orbit);
    const int64_t start = apt::geoloc::start_ms_of(sat.call.ref_is_end != 0, sat.call.ref_ms, static_cast<uint32_t>(h));
    sat.call.ref_ms = start - fit::kLineMs * st.margin;
    sat.call.ref_is_end = 0;
    return sat;
}

// a record no launch is needed for: the position count
void check_count(const Checked &c, size_t h, const void *positions, size_t n_positions, aptgpu_fit_result *info)
{
    if (!positions || n_positions == h + 2 * static_cast<size_t>(c.st.margin)) return;
    aptgpu_fit_result r = fit::first_record(static_cast<uint32_t>(h), c.geom, c.st, static_cast<uint32_t>(c.points.size() / 2));
    r.status = APTGPU_ERR_INTERNAL;
    r.reason = apt::geoloc::kReasonCount;
    r.done = 1;
    fit::put_result(info, r);
    throw Error{ErrorKind::Internal, fit::reason_text(apt::geoloc::kReasonCount)};
}

int fit_device(const aptgpu_context *ctx, hipStream_t s, const uint8_t *d_image, size_t h, const Checked &c,
               const double *positions, size_t n_positions, const aptgpu_orbit_settings *orbit, aptgpu_fit_result *info,
               void **scores_out, size_t *n_scores)
{
    SatCall sat{};
    if (orbit) sat = long_track_call(orbit, h, c.st);
    apt::gpu::FitLaunch l{};
    l.image = d_image;
    l.h = static_cast<uint32_t>(h);
    l.positions = positions;
    l.n_positions = n_positions;
    l.sat = orbit ? &sat.call : nullptr;
    l.points = c.points.data();
    l.n_points = static_cast<uint32_t>(c.points.size() / 2);
    l.geom = c.geom;
    l.st = c.st;
    struct Free {
        void operator()(apt::gpu::FitWorkspace *w) const { apt::gpu::fit_ws_destroy(w); }
    };
    std::unique_ptr<apt::gpu::FitWorkspace, Free> ws(apt::gpu::fit_ws_create(l));
    float ms[4] = {0.f, 0.f, 0.f, 0.f};
    apt::gpu::fit_enqueue(s, l, ws.get(), c.st.timing ? ms : nullptr);
    aptgpu_fit_result r = read_record(s, apt::gpu::fit_ws_record(ws.get()));
    r.ms_edge = ms[0];
    r.ms_angles = ms[1];
    r.ms_score = ms[2];
    r.ms_pick = ms[3];
    fit::put_result(info, r);
    if (r.status != 0) throw Error{ErrorKind::Internal, fit::reason_text(r.reason)};
    if (scores_out) {
        const size_t n = static_cast<size_t>(c.st.rounds) * c.st.grid.total();
        HostPtr<fit::Sum> out(host_alloc<fit::Sum>(n));
        apt::hip_check(hipMemcpyAsync(out.get(), apt::gpu::fit_ws_scores(ws.get()), n * sizeof(fit::Sum), hipMemcpyDeviceToHost, s),
                       "hipMemcpyAsync D2H");
        apt::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        *scores_out = out.release();
        if (n_scores) *n_scores = n;
    }
    return APTGPU_OK;
}

}  // namespace

extern "C" {

void aptgpu_fit_default_settings(aptgpu_fit_settings *out)
{
    if (!out) return;
    aptgpu_fit_settings s{};
    s.struct_size = sizeof s;
    s.margin_rows = 120;
    s.rounds = 4;
    s.radius = 2;
    s.min_points = 64;
    s.shift_step = 8;
    s.n_shift = 15;
    s.n_yaw = s.n_hscale = s.n_vscale = 3;
    s.yaw_step = 0.02;
    s.hscale_step = s.vscale_step = 0.04;
    s.spacing_deg = 0.05;
    *out = s;
}

int aptgpu_fit_sample_points(const aptgpu_map_layers *layers, uint32_t layer_mask, double spacing_deg, double **xy,
                             size_t *n_points, char *err, size_t err_cap)
{
    if (xy) *xy = nullptr;
    if (n_points) *n_points = 0;
    return guarded(err, err_cap, [&] {
        if (!layers || !xy || !n_points) throw Error{ErrorKind::Invalid, "fit: null argument"};
        aptgpu_fit_settings s{};
        aptgpu_fit_default_settings(&s);
        s.layer_mask = layer_mask;
        s.spacing_deg = spacing_deg;
        const fit::Settings st = fit::check_settings(&s);
        const std::vector<double> pts = fit::sample_points(layers->layers, st.mask, st.spacing);
        HostPtr<double> out(host_alloc<double>(pts.size()));
        if (!pts.empty()) std::memcpy(out.get(), pts.data(), pts.size() * sizeof(double));
        *xy = out.release();
        *n_points = pts.size() / 2;
        return APTGPU_OK;
    });
}

int aptgpu_fit_overlay_host(const uint8_t *image, size_t height, const double *sat_positions, size_t n_positions,
                            const aptgpu_orbit_settings *orbit, const aptgpu_map_layers *layers,
                            const aptgpu_map_settings *map, const aptgpu_fit_settings *settings,
                            aptgpu_fit_result *info, void **scores_out, size_t *n_scores, char *err, size_t err_cap)
{
    clear(scores_out, n_scores);
    return guarded(err, err_cap, [&] {
        const Checked c = checked(image, height, sat_positions, orbit, layers, map, settings);
        std::vector<double> own;
        const double *track = sat_positions;
        size_t count = n_positions;
        if (orbit) {
            const SatCall sat = long_track_call(orbit, height, c.st);
            count = height + 2 * static_cast<size_t>(c.st.margin);
            own.resize(2 * count);
            apt::sat::track_host(sat.call.rec, false, sat.call.ref_ms, static_cast<uint32_t>(count), own.data());
            track = own.data();
        }
        const size_t n = static_cast<size_t>(c.st.rounds) * c.st.grid.total();
        HostPtr<fit::Sum> scores(scores_out ? host_alloc<fit::Sum>(n) : nullptr);
        fit::run_host(image, height, track, count, c.points, c.geom, c.st, scores.get(), info);
        if (scores_out) {
            *scores_out = scores.release();
            if (n_scores) *n_scores = n;
        }
        return APTGPU_OK;
    });
}

int aptgpu_fit_overlay(const aptgpu_context *ctx, const uint8_t *image, size_t height, const double *sat_positions,
                       size_t n_positions, const aptgpu_orbit_settings *orbit, const aptgpu_map_layers *layers,
                       const aptgpu_map_settings *map, const aptgpu_fit_settings *settings, aptgpu_fit_result *info,
                       void **scores_out, size_t *n_scores, char *err, size_t err_cap)
{
    clear(scores_out, n_scores);
    return guarded(err, err_cap, [&] {
        const Checked c = checked(image, height, sat_positions, orbit, layers, map, settings);
        check_count(c, height, sat_positions, n_positions, info);
        Scratch sc(ctx);
        apt::DeviceBuffer<uint8_t> d_image;
        d_image.alloc(height * 2080u);
        apt::hip_check(hipMemcpyAsync(d_image.ptr, image, height * 2080u, hipMemcpyHostToDevice, sc.stream), "hipMemcpyAsync H2D");
        return fit_device(ctx, sc.stream, d_image.ptr, height, c, sat_positions, n_positions, orbit, info, scores_out, n_scores);
    });
}

int aptgpu_fit_overlay_device(const aptgpu_context *ctx, const uint8_t *d_image, size_t height, void *stream,
                              const double *sat_positions, size_t n_positions, const aptgpu_orbit_settings *orbit,
                              const aptgpu_map_layers *layers, const aptgpu_map_settings *map,
                              const aptgpu_fit_settings *settings, aptgpu_fit_result *info, void **scores_out,
                              size_t *n_scores, char *err, size_t err_cap)
{
    clear(scores_out, n_scores);
    return guarded(err, err_cap, [&] {
        const Checked c = checked(d_image, height, sat_positions, orbit, layers, map, settings);
        check_count(c, height, sat_positions, n_positions, info);
        apt::hip_check(hipSetDevice(ctx ? ctx->device : 0), "hipSetDevice");
        return fit_device(ctx, static_cast<hipStream_t>(stream), d_image, height, c, sat_positions, n_positions, orbit, info,
                          scores_out, n_scores);
    });
}

}  // extern "C"
