// apt_capi_geoloc.hip — extern "C" surface of the geolocation stage (include/aptgpu.h §4, "geolocation of the swath";
// DESIGN.md §25): host-array form on the GPU, the same on the CPU, the sun of one instant, and the device-resident
// form chained behind a plan's decode.
#include <memory>
#include <vector>

#include "apt_capi_util.hpp"
#include "apt_kernels_geoloc.hpp"

namespace {

using namespace apt::capi;
namespace geo = apt::geoloc;

void clear(double **latlon, float **cos_sun, float **rows_out)
{
    if (latlon) *latlon = nullptr;
    if (cos_sun) *cos_sun = nullptr;
    if (rows_out) *rows_out = nullptr;
}

// the checks every form shares, in the order the header gives them; none touches a device
struct Checked {
    geo::Settings st;
    geo::Geom geom;
};
Checked checked(const aptgpu_geoloc_settings *settings, const aptgpu_map_settings *map, const void *positions,
                const void *orbit, bool want_rows, bool have_signal, size_t rows)
{
    Checked c{geo::check_settings(settings), geo::check_geom(map)};
    geo::check_call(positions, orbit, want_rows, have_signal, rows);
    return c;
}

}  // namespace

extern "C" {

int aptgpu_sun_position(int64_t unix_ms, double out[2])
{
    if (!out) return APTGPU_ERR_INVALID;
    geo::sun_position(unix_ms, out);
    return APTGPU_OK;
}

int aptgpu_geolocate_host(const float *signal, size_t n, const double *sat_positions, size_t n_positions,
                          const aptgpu_orbit_settings *orbit, const aptgpu_map_settings *map,
                          const aptgpu_geoloc_settings *settings, double **latlon, float **cos_sun, float **rows_out,
                          aptgpu_geoloc_result *info, char *err, size_t err_cap)
{
    clear(latlon, cos_sun, rows_out);
    return guarded(err, err_cap, [&] {
        const size_t h = n / 2080u;
        Checked c = checked(settings, map, sat_positions, orbit, rows_out != nullptr, signal != nullptr, h);
        std::vector<double> own;
        const double *track = sat_positions;
        size_t count = n_positions;
        if (orbit) {
            const SatCall sat = orbit_args(orbit);
            own.resize(2 * (h ? h : 1));
            apt::sat::track_host(sat.call.rec, sat.call.ref_is_end != 0, sat.call.ref_ms, static_cast<uint32_t>(h), own.data());
            track = own.data();
            count = h;
            c.st.ref_is_end = sat.call.ref_is_end != 0;
            c.st.ref_ms = sat.call.ref_ms;
        }
        HostPtr<double> hl(latlon ? host_alloc<double>(h * 2 * APTGPU_GEOLOC_PX) : nullptr);
        HostSignal hc(cos_sun ? host_alloc<float>(h * APTGPU_GEOLOC_PX) : nullptr);
        HostSignal hr(rows_out ? host_alloc<float>(n) : nullptr);
        geo::run_host(signal, n, track, count, c.geom, c.st, hl.get(), hc.get(), hr.get(), info);
        if (latlon) *latlon = hl.release();
        if (cos_sun) *cos_sun = hc.release();
        if (rows_out) *rows_out = hr.release();
        return APTGPU_OK;
    });
}

int aptgpu_geolocate(const aptgpu_context *ctx, const float *signal, size_t n, const double *sat_positions,
                     size_t n_positions, const aptgpu_orbit_settings *orbit, const aptgpu_map_settings *map,
                     const aptgpu_geoloc_settings *settings, double **latlon, float **cos_sun, float **rows_out,
                     aptgpu_geoloc_result *info, char *err, size_t err_cap)
{
    clear(latlon, cos_sun, rows_out);
    return guarded(err, err_cap, [&] {
        const size_t h = n / 2080u;
        const Checked c = checked(settings, map, sat_positions, orbit, rows_out != nullptr, signal != nullptr, h);
        SatCall sat{};
        if (orbit) sat = orbit_args(orbit);
        Scratch sc(ctx);
        hipStream_t s = sc.stream;
        const size_t px = h * APTGPU_GEOLOC_PX;
        apt::DeviceBuffer<double> d_latlon;
        apt::DeviceBuffer<float> d_cos, d_rows;
        apt::DeviceBuffer<char> ws;
        apt::map::Device dev;
        if (latlon) d_latlon.alloc(2 * px + 2);
        if (cos_sun) d_cos.alloc(px + 16);
        if (rows_out) d_rows = sc.upload(signal, n);  // normalised in place, then copied back
        ws.alloc(apt::gpu::geoloc_ws_bytes(h));
        apt::gpu::GeolocLaunch l{};
        l.x = d_rows.ptr;
        l.positions = sat_positions;
        l.n_positions = n_positions;
        l.sat = orbit ? &sat.call : nullptr;
        l.geom = c.geom;
        l.st = c.st;
        l.latlon = d_latlon.ptr;
        l.cos_sun = d_cos.ptr;
        l.rows = d_rows.ptr;
        // the call as one job of the row stages: whole rows only, (res, n, cap) = (null, h * 2080, h * 2080)
        apt::enqueue_geoloc(nullptr, apt::ImageJob{s, d_rows.ptr, nullptr, h * 2080u, h * 2080u}, l, dev, ws.ptr);
        const apt::gpu::GeolocRecord r = read_record(s, apt::gpu::geoloc_ws_record(ws.ptr));
        apt::gpu::geoloc_record_to_public(r, info);
        if (r.status != 0) throw Error{ErrorKind::Internal, geo::reason_text(r.reason)};
        HostPtr<double> hl(latlon ? host_alloc<double>(2 * px) : nullptr);
        if (latlon && px)
            apt::hip_check(hipMemcpyAsync(hl.get(), d_latlon.ptr, 2 * px * sizeof(double), hipMemcpyDeviceToHost, s),
                           "hipMemcpyAsync D2H");
        HostSignal hc(cos_sun ? sc.download_malloc(d_cos.ptr, px) : nullptr);
        HostSignal hr(rows_out ? sc.download_malloc(d_rows.ptr, n) : nullptr);
        apt::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        if (latlon) *latlon = hl.release();
        if (cos_sun) *cos_sun = hc.release();
        if (rows_out) *rows_out = hr.release();
        return APTGPU_OK;
    });
}

int aptgpu_plan_geolocate_device(aptgpu_plan *plan, int count, const float *const *d_rows, const size_t *rows_cap,
                                 const double *const *sat_positions, const size_t *n_positions,
                                 const aptgpu_orbit_settings *const *orbit, const aptgpu_map_settings *map,
                                 const aptgpu_geoloc_settings *settings, double *const *d_latlon,
                                 float *const *d_cos, float *const *d_out, char *err, size_t err_cap)
{
    if (count < 0 || !d_rows || !rows_cap) return APTGPU_ERR_INVALID;
    return guarded(err, err_cap, [&] {
        // (the checks of the arguments come before the plan is looked at: none of them needs a device)
        const Checked c = checked(settings, map, sat_positions, orbit, d_out != nullptr, true, 0);
        if (sat_positions && !n_positions) throw Error{ErrorKind::Invalid, "geoloc: n_positions is required with sat_positions"};
        // every buffer of the call as (start, bytes)
        struct Span {
            const void *p;
            size_t bytes;
            bool rows;  // a rows buffer: read only, or rewritten in place
        };
        std::vector<Span> spans;
        for (int i = 0; i < count; ++i) {
            const size_t rows = rows_cap[i];
            if (!d_rows[i] || (sat_positions && !sat_positions[i]) || (orbit && !orbit[i]) ||
                (d_latlon && !d_latlon[i]) || (d_cos && !d_cos[i]) || (d_out && !d_out[i]))
                throw Error{ErrorKind::Invalid, "null pointer in a per-recording array"};
            if (rows > geo::kMaxRows) throw Error{ErrorKind::Invalid, "geoloc: more than 2^22 rows"};
            if (d_latlon && (reinterpret_cast<uintptr_t>(d_latlon[i]) & 15u))
                throw Error{ErrorKind::Invalid, "d_latlon must be 16-byte aligned"};
            if ((d_cos && (reinterpret_cast<uintptr_t>(d_cos[i]) & 3u)) || (d_out && (reinterpret_cast<uintptr_t>(d_out[i]) & 3u)) ||
                (reinterpret_cast<uintptr_t>(d_rows[i]) & 3u))
                throw Error{ErrorKind::Invalid, "d_rows, d_cos and d_out must be 4-byte aligned"};
            spans.push_back({d_rows[i], rows * 2080u * sizeof(float), true});
            if (d_latlon) spans.push_back({d_latlon[i], rows * APTGPU_GEOLOC_PX * 2 * sizeof(double), false});
            if (d_cos) spans.push_back({d_cos[i], rows * APTGPU_GEOLOC_PX * sizeof(float), false});
            if (d_out && d_out[i] != d_rows[i]) spans.push_back({d_out[i], rows * 2080u * sizeof(float), false});
        }
        // (rows buffers may coincide with each other, as far as this stage is concerned: it only reads them, or
        // rewrites them in place, which the d_out == d_rows case above left out of the list)
        for (size_t a = 0; a < spans.size(); ++a)
            for (size_t b = a + 1; b < spans.size(); ++b)
                if (!(spans[a].rows && spans[b].rows) && overlaps(spans[a].p, spans[a].bytes, spans[b].p, spans[b].bytes))
                    throw Error{ErrorKind::Invalid, "geoloc: an output overlaps a rows buffer or another output"};
        if (!plan) throw Error{ErrorKind::Invalid, "geoloc: no plan"};
        if (static_cast<size_t>(count) > plan->last_slots.size())
            throw Error{ErrorKind::Invalid, "count exceeds the recordings of the last decode call"};
        std::vector<SatCall> sats(static_cast<size_t>(count));
        if (orbit)
            for (int i = 0; i < count; ++i) sats[static_cast<size_t>(i)] = orbit_args(orbit[i]);
        apt::hip_check(hipSetDevice(plan->device), "hipSetDevice");
        for (int i = 0; i < count; ++i) {
            apt::gpu::GeolocLaunch l{};
            l.x = d_rows[i];
            l.positions = sat_positions ? sat_positions[i] : nullptr;
            l.n_positions = sat_positions ? n_positions[i] : 0;
            l.sat = orbit ? &sats[static_cast<size_t>(i)].call : nullptr;
            l.geom = c.geom;
            l.st = c.st;
            l.latlon = d_latlon ? d_latlon[i] : nullptr;
            l.cos_sun = d_cos ? d_cos[i] : nullptr;
            l.rows = d_out ? d_out[i] : nullptr;
            plan->enqueue_geoloc(i, static_cast<uint64_t>(rows_cap[i]) * 2080u, l);
        }
        return APTGPU_OK;
    });
}

int aptgpu_plan_geoloc_results(aptgpu_plan *plan, int count, aptgpu_geoloc_result *results)
{
    return plan_results(
        plan, count, results,
        [&](int i) -> apt::gpu::GeolocRecord * {
            void *ws = plan->slot_of(i).geoloc_ws.ptr;
            return ws ? apt::gpu::geoloc_ws_record(ws) : nullptr;
        },
        [&](int i, const apt::gpu::GeolocRecord &r) { apt::gpu::geoloc_record_to_public(r, results + i); });
}

}  // extern "C"
