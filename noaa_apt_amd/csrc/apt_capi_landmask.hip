// apt_capi_landmask.hip — extern "C" surface of the land / sea / lake mask and of the map-coloured false colour
// (include/aptgpu.h §4, "land / sea / lake mask of the swath"): the swath and plane forms on the GPU, the
// same on the CPU, the device-resident form chained behind a plan's decode, and the colouriser.
#include <memory>
#include <vector>

#include "apt_capi_util.hpp"
#include "apt_kernels_landmask.hpp"

namespace {

using namespace apt::capi;
namespace geo = apt::geoloc;
namespace lm = apt::landmask;
using TablePtr = std::shared_ptr<const lm::Table>;

// The layer set's table for nb bands: the cached one while the layers' generation and the band count are its own.
TablePtr table_of(const aptgpu_map_layers *layers, int nb)
{
    if (!layers) throw Error{ErrorKind::Invalid, "land mask: the layer set is required"};
    std::lock_guard<std::mutex> lock(layers->land_mutex);
    auto cur = std::static_pointer_cast<const lm::Table>(layers->land_table);
    if (cur && cur->gen == layers->layers.gen && cur->nb == nb) return cur;
    TablePtr t = std::make_shared<const lm::Table>(lm::build_table(layers->layers, nb));
    layers->land_table = t;
    return t;
}

// the checks the swath forms share, in the order the header gives them; none touches a device
struct Checked {
    TablePtr table;
    geo::Geom geom;
};
Checked checked(const aptgpu_map_layers *layers, const aptgpu_land_mask_settings *settings,
                const aptgpu_map_settings *map, const void *positions, const void *orbit, size_t rows)
{
    const int nb = lm::check_settings(settings);
    Checked c{table_of(layers, nb), geo::check_geom(map)};
    geo::check_call(positions, orbit, false, false, rows);
    return c;
}

TablePtr checked_plane(const double *latlon, const aptgpu_map_layers *layers, const aptgpu_land_mask_settings *settings)
{
    const int nb = lm::check_settings(settings);
    TablePtr t = table_of(layers, nb);
    if (!latlon) throw Error{ErrorKind::Invalid, "land mask: the lat / lon plane is required"};
    if (reinterpret_cast<uintptr_t>(latlon) & 7u) throw Error{ErrorKind::Invalid, "land mask: the lat / lon plane must be 8-byte aligned"};
    return t;
}

void check_color(const uint8_t *image, size_t height, const uint8_t *mask, size_t mask_height,
                 const uint8_t *const *palettes, const size_t *palette_bytes, const float *tunes, uint8_t **rgba)
{
    if (!image || !mask || !palettes || !palette_bytes || !tunes || !rgba)
        throw Error{ErrorKind::Invalid, "false colour (masked): null argument"};
    for (int k = 0; k < 3; ++k) {
        if (!palettes[k]) throw Error{ErrorKind::Invalid, "false colour (masked): null palette"};
        if (palette_bytes[k] != static_cast<size_t>(lm::kPaletteBytes))
            throw Error{ErrorKind::Invalid, "false colour (masked): a palette is 256 x 256 x 3 bytes"};
    }
    if (mask_height != height) throw Error{ErrorKind::Invalid, "false colour (masked): the mask's height differs from the image's"};
    if (height > geo::kMaxRows) throw Error{ErrorKind::Invalid, "false colour (masked): more than 2^22 rows"};
}

// what the land mask stage keeps in a plan slot
struct SlotState {
    apt::gpu::LandTable table;
    apt::DeviceBuffer<char> geoloc_ws;  // the geolocation stage's scratch of this stage's own track and row launches
    size_t geoloc_rows = 0;
    apt::DeviceBuffer<apt::gpu::LandRecord> rec;
    aptgpu_land_mask_result head{};     // the table's part of the record of the latest call
};

apt::gpu::GeolocLaunch geoloc_launch(const double *positions, size_t n_positions, const SatCall *sat, const geo::Geom &geom)
{
    apt::gpu::GeolocLaunch l{};
    l.positions = positions;
    l.n_positions = n_positions;
    l.sat = sat ? &sat->call : nullptr;
    l.geom = geom;
    l.st = geo::Settings{0, false, 0, 0.f, 0.f};
    return l;
}

// The swath form's launches on s: the geolocation stage's track and rows, then k_land_mask<Swath>.  res / n / cap as the
// row stages take them.
void enqueue_swath(aptgpu_plan *plan, hipStream_t s, apt::gpu::GeolocLaunch l, const apt::gpu::Result *res, uint64_t n,
                   uint64_t cap, apt::map::Device &dev, void *geoloc_ws, const apt::gpu::LandTable &table,
                   uint8_t *d_mask, apt::gpu::LandRecord *rec)
{
    l.res = res;
    l.n = n;
    l.cap = cap;
    auto timed = [&](const char *name, auto &&fn) { plan ? plan->timed(s, name, fn) : fn(); };
    dev.prepare_track(s, static_cast<size_t>(cap / 2080u));
    timed("image_geoloc_track", [&] { apt::gpu::geoloc_track(s, l, dev, geoloc_ws); });
    timed("image_geoloc_rows", [&] { apt::gpu::geoloc_rows(s, l, dev, geoloc_ws); });
    timed("image_land_mask", [&] {
        apt::gpu::land_mask_swath(s, table, geoloc_ws, dev, static_cast<uint32_t>(cap / 2080u), d_mask, rec);
    });
    apt::hip_check(hipGetLastError(), "kernel launch (land mask stage)");
}

uint8_t *download_bytes(hipStream_t s, const uint8_t *d, size_t n)
{
    HostPtr<uint8_t> h(host_alloc<uint8_t>(n));
    if (n) apt::hip_check(hipMemcpyAsync(h.get(), d, n, hipMemcpyDeviceToHost, s), "hipMemcpyAsync D2H");
    apt::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
    return h.release();
}

}  // namespace

extern "C" {

int aptgpu_land_mask_host(size_t height, const double *sat_positions, size_t n_positions,
                          const aptgpu_orbit_settings *orbit, const aptgpu_map_settings *map,
                          const aptgpu_map_layers *layers, const aptgpu_land_mask_settings *settings, uint8_t **mask,
                          aptgpu_land_mask_result *info, char *err, size_t err_cap)
{
    if (mask) *mask = nullptr;
    return guarded(err, err_cap, [&] {
        const Checked c = checked(layers, settings, map, sat_positions, orbit, height);
        if (!mask) throw Error{ErrorKind::Invalid, "land mask: null argument"};
        std::vector<double> own;
        const double *track = sat_positions;
        size_t count = n_positions;
        if (orbit) {
            const SatCall sat = orbit_args(orbit);
            own.resize(2 * (height ? height : 1));
            apt::sat::track_host(sat.call.rec, sat.call.ref_is_end != 0, sat.call.ref_ms, static_cast<uint32_t>(height), own.data());
            track = own.data();
            count = height;
        }
        HostPtr<uint8_t> out(host_alloc<uint8_t>(height * APTGPU_GEOLOC_PX));
        lm::run_swath_host(*c.table, height, track, count, c.geom, out.get(), info);
        *mask = out.release();
        return APTGPU_OK;
    });
}

int aptgpu_land_mask(const aptgpu_context *ctx, size_t height, const double *sat_positions, size_t n_positions,
                     const aptgpu_orbit_settings *orbit, const aptgpu_map_settings *map,
                     const aptgpu_map_layers *layers, const aptgpu_land_mask_settings *settings, uint8_t **mask,
                     aptgpu_land_mask_result *info, char *err, size_t err_cap)
{
    if (mask) *mask = nullptr;
    return guarded(err, err_cap, [&] {
        const Checked c = checked(layers, settings, map, sat_positions, orbit, height);
        if (!mask) throw Error{ErrorKind::Invalid, "land mask: null argument"};
        SatCall sat{};
        if (orbit) sat = orbit_args(orbit);
        Scratch sc(ctx);
        hipStream_t s = sc.stream;
        const size_t px = height * APTGPU_GEOLOC_PX;
        apt::gpu::LandTable table;
        apt::DeviceBuffer<char> ws;
        apt::DeviceBuffer<uint8_t> d_mask;
        apt::DeviceBuffer<apt::gpu::LandRecord> rec;
        apt::map::Device dev;
        table.upload(s, c.table);
        ws.alloc(apt::gpu::geoloc_ws_bytes(height));
        d_mask.alloc(px + 16);
        rec.alloc(1);
        enqueue_swath(nullptr, s, geoloc_launch(sat_positions, n_positions, orbit ? &sat : nullptr, c.geom), nullptr,
                      height * 2080u, height * 2080u, dev, ws.ptr, table, d_mask.ptr, rec.ptr);
        const apt::gpu::LandRecord r = read_record(s, rec.ptr);
        apt::gpu::land_record_to_public(r, lm::first_record(*c.table, 0), info);
        if (r.status != 0) throw Error{ErrorKind::Internal, geo::reason_text(r.reason)};
        *mask = download_bytes(s, d_mask.ptr, px);
        return APTGPU_OK;
    });
}

int aptgpu_land_mask_plane_host(const double *latlon, size_t n, const aptgpu_map_layers *layers,
                                const aptgpu_land_mask_settings *settings, uint8_t **mask,
                                aptgpu_land_mask_result *info, char *err, size_t err_cap)
{
    if (mask) *mask = nullptr;
    return guarded(err, err_cap, [&] {
        const TablePtr t = checked_plane(latlon, layers, settings);
        if (!mask) throw Error{ErrorKind::Invalid, "land mask: null argument"};
        HostPtr<uint8_t> out(host_alloc<uint8_t>(n));
        aptgpu_land_mask_result rec = lm::first_record(*t, 0);
        lm::run_plane_host(*t, latlon, n, out.get(), &rec);
        lm::put_result(info, rec);
        *mask = out.release();
        return APTGPU_OK;
    });
}

int aptgpu_land_mask_plane(const aptgpu_context *ctx, const double *latlon, size_t n, const aptgpu_map_layers *layers,
                           const aptgpu_land_mask_settings *settings, uint8_t **mask, aptgpu_land_mask_result *info,
                           char *err, size_t err_cap)
{
    if (mask) *mask = nullptr;
    return guarded(err, err_cap, [&] {
        const TablePtr t = checked_plane(latlon, layers, settings);
        if (!mask) throw Error{ErrorKind::Invalid, "land mask: null argument"};
        Scratch sc(ctx);
        hipStream_t s = sc.stream;
        apt::gpu::LandTable table;
        apt::DeviceBuffer<double> d_ll;
        apt::DeviceBuffer<uint8_t> d_mask;
        apt::DeviceBuffer<apt::gpu::LandRecord> rec;
        table.upload(s, t);
        d_ll.alloc(2 * n + 2);
        d_mask.alloc(n + 16);
        rec.alloc(1);
        if (n) apt::hip_check(hipMemcpyAsync(d_ll.ptr, latlon, 2 * n * sizeof(double), hipMemcpyHostToDevice, s), "hipMemcpyAsync H2D");
        apt::gpu::land_mask_plane(s, table, d_ll.ptr, n, d_mask.ptr, rec.ptr);
        apt::hip_check(hipGetLastError(), "kernel launch (land mask stage)");
        const apt::gpu::LandRecord r = read_record(s, rec.ptr);
        apt::gpu::land_record_to_public(r, lm::first_record(*t, 0), info);
        *mask = download_bytes(s, d_mask.ptr, n);
        return APTGPU_OK;
    });
}

int aptgpu_plan_land_mask_device(aptgpu_plan *plan, int count, const float *const *d_rows, const size_t *rows_cap,
                                 const double *const *sat_positions, const size_t *n_positions,
                                 const aptgpu_orbit_settings *const *orbit, const aptgpu_map_settings *map,
                                 const aptgpu_map_layers *layers, const aptgpu_land_mask_settings *settings,
                                 uint8_t *const *d_mask, char *err, size_t err_cap)
{
    if (count < 0 || !d_rows || !rows_cap || !d_mask) return APTGPU_ERR_INVALID;
    return guarded(err, err_cap, [&] {
        // (the checks of the arguments come before the plan is looked at: none of them needs a device)
        const Checked c = checked(layers, settings, map, sat_positions, orbit, 0);
        if (sat_positions && !n_positions) throw Error{ErrorKind::Invalid, "land mask: n_positions is required with sat_positions"};
        for (int i = 0; i < count; ++i) {
            if (!d_rows[i] || (sat_positions && !sat_positions[i]) || (orbit && !orbit[i]) || !d_mask[i])
                throw Error{ErrorKind::Invalid, "null pointer in a per-recording array"};
            if (rows_cap[i] > geo::kMaxRows) throw Error{ErrorKind::Invalid, "land mask: more than 2^22 rows"};
            const size_t bytes = rows_cap[i] * APTGPU_GEOLOC_PX;
            if (overlaps_rows(d_mask[i], bytes, count, d_rows, rows_cap))
                throw Error{ErrorKind::Invalid, "land mask: a mask overlaps a rows buffer"};
            for (int j = 0; j < i; ++j)
                if (overlaps(d_mask[i], bytes, d_mask[j], rows_cap[j] * APTGPU_GEOLOC_PX))
                    throw Error{ErrorKind::Invalid, "land mask: a mask overlaps another"};
        }
        if (!plan) throw Error{ErrorKind::Invalid, "land mask: no plan"};
        if (static_cast<size_t>(count) > plan->last_slots.size())
            throw Error{ErrorKind::Invalid, "count exceeds the recordings of the last decode call"};
        std::vector<SatCall> sats(static_cast<size_t>(count));
        if (orbit)
            for (int i = 0; i < count; ++i) sats[static_cast<size_t>(i)] = orbit_args(orbit[i]);
        apt::hip_check(hipSetDevice(plan->device), "hipSetDevice");
        for (int i = 0; i < count; ++i) {
            const aptgpu_plan::ImageTarget t = plan->image_target(i, static_cast<uint64_t>(rows_cap[i]) * 2080u);
            aptgpu_plan::Slot &sl = t.slot;
            if (!sl.landmask) sl.landmask = std::make_shared<SlotState>();
            SlotState &st = *static_cast<SlotState *>(sl.landmask.get());
            const size_t rows = static_cast<size_t>(t.cap / 2080u);
            if (!st.geoloc_ws.ptr || st.geoloc_rows < rows) {
                st.geoloc_ws.alloc(apt::gpu::geoloc_ws_bytes(rows));
                st.geoloc_rows = rows;
            }
            if (!st.rec.ptr) st.rec.alloc(1);
            if (!sl.map) sl.map = std::make_unique<apt::map::Device>();
            st.table.upload(t.stream, c.table);
            st.head = lm::first_record(*c.table, 0);
            enqueue_swath(plan, t.stream,
                          geoloc_launch(sat_positions ? sat_positions[i] : nullptr, sat_positions ? n_positions[i] : 0,
                                        orbit ? &sats[static_cast<size_t>(i)] : nullptr, c.geom),
                          t.res, 0, t.cap, *sl.map, st.geoloc_ws.ptr, st.table, d_mask[i], st.rec.ptr);
        }
        return APTGPU_OK;
    });
}

int aptgpu_plan_land_mask_results(aptgpu_plan *plan, int count, aptgpu_land_mask_result *results)
{
    auto state = [&](int i) { return static_cast<SlotState *>(plan->slot_of(i).landmask.get()); };
    return plan_results(
        plan, count, results,
        [&](int i) -> apt::gpu::LandRecord * {
            SlotState *st = state(i);
            return st ? st->rec.ptr : nullptr;
        },
        [&](int i, const apt::gpu::LandRecord &r) { apt::gpu::land_record_to_public(r, state(i)->head, results + i); });
}

int aptgpu_false_color_masked_host(const uint8_t *image, size_t height, const uint8_t *mask, size_t mask_height,
                                   const uint8_t *const *palettes, const size_t *palette_bytes, const float tunes[4],
                                   uint8_t **rgba, char *err, size_t err_cap)
{
    if (rgba) *rgba = nullptr;
    return guarded(err, err_cap, [&] {
        check_color(image, height, mask, mask_height, palettes, palette_bytes, tunes, rgba);
        HostPtr<uint8_t> out(host_alloc<uint8_t>(height * 2080u * 4u));
        lm::false_color_masked_host(image, height, mask, palettes, tunes, out.get());
        *rgba = out.release();
        return APTGPU_OK;
    });
}

int aptgpu_false_color_masked(const aptgpu_context *ctx, const uint8_t *image, size_t height, const uint8_t *mask,
                              size_t mask_height, const uint8_t *const *palettes, const size_t *palette_bytes,
                              const float tunes[4], uint8_t **rgba, char *err, size_t err_cap)
{
    if (rgba) *rgba = nullptr;
    return guarded(err, err_cap, [&] {
        check_color(image, height, mask, mask_height, palettes, palette_bytes, tunes, rgba);
        std::vector<uint32_t> packed(3 * 65536);
        lm::pack_palettes(palettes, packed.data());
        Scratch sc(ctx);
        hipStream_t s = sc.stream;
        const size_t px = height * 2080u, mpx = height * APTGPU_GEOLOC_PX;
        apt::DeviceBuffer<uint8_t> d_image, d_mask, d_out;
        apt::DeviceBuffer<uint32_t> d_pal;
        d_image.alloc(px + 16);
        d_mask.alloc(mpx + 16);
        d_out.alloc(px * 4 + 16);
        d_pal.alloc(packed.size());
        if (px) {
            apt::hip_check(hipMemcpyAsync(d_image.ptr, image, px, hipMemcpyHostToDevice, s), "hipMemcpyAsync H2D");
            apt::hip_check(hipMemcpyAsync(d_mask.ptr, mask, mpx, hipMemcpyHostToDevice, s), "hipMemcpyAsync H2D");
        }
        apt::hip_check(hipMemcpyAsync(d_pal.ptr, packed.data(), packed.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s),
                       "hipMemcpyAsync H2D");
        if (px) apt::gpu::false_color_masked(s, d_image.ptr, static_cast<uint32_t>(height), d_mask.ptr, d_pal.ptr, lm::tune_of(tunes), d_out.ptr);
        apt::hip_check(hipGetLastError(), "kernel launch (masked false colour)");
        *rgba = download_bytes(s, d_out.ptr, px * 4);
        return APTGPU_OK;
    });
}

}  // extern "C"
