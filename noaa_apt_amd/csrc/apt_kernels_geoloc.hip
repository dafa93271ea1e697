// apt_kernels_geoloc.hip — the gfx950 kernels of the geolocation stage (definition: apt_kernels_geoloc.hpp,
// include/aptgpu.h).  Per recording, behind the track's launches (apt_kernels_map.hpp: the track, its
// x offsets and the call's checks, from the caller's positions or from SGP4 on the device):
//
//  k_geoloc_head  one wave in front of them: the height record they read, from the decode record on the device, and
//                 fresh partial records.
//  k_geoloc_rows  one thread per row: the sun's unit vector at the row's time into a per-row table.  Thread 0 also
//                 computes the call's nine frame doubles S, T, R from the scalars (the host's by value, or
//                 k_sat_scalars' in device memory) and writes the record's head.
//  k_geoloc<OUT>  the hot path.  One thread per pixel of the flattened h x 909 index (r = i / 909, k = i % 909), so
//                 every wave is full and touches at most two rows; xoff[r] and the row's sun vector come from L2.  Every
//                 store is contiguous across the wave: 16 bytes per lane into the interleaved lat / lon plane, 4 bytes
//                 into cos_sun, a 4-byte load and store in the rows.  OUT is a mask of the outputs: a call that asks
//                 for the rows alone issues neither atan2.  The record's counters stay in registers, are reduced per
//                 wave with shuffles and reach one of 64 partial records with at most four integer atomics per wave.
#include "apt_kernels_geoloc.hpp"

#include "apt_kernels_map_dev.hpp"

#include <cstddef>

#pragma clang fp contract(off)

namespace apt::gpu {

namespace {

using namespace apt::geoloc;
using apt::despeckle::bits_of_key;
using apt::despeckle::key_of_bits;
using apt::map::Scalars;

constexpr int kThreads = 256;

// What the stage keeps per recording; `sun` (3 doubles per row) lies behind it.
struct Workspace {
    GeolocRecord rec;
    Frame frame;
    ImageResult height;  // status and height alone: what the track's launches read
};
constexpr size_t kSunOffset = (sizeof(Workspace) + 255u) & ~static_cast<size_t>(255u);

inline Workspace *view(void *ws) { return static_cast<Workspace *>(ws); }
inline double *sun_table(void *ws) { return reinterpret_cast<double *>(static_cast<char *>(ws) + kSunOffset); }

__global__ __launch_bounds__(64) void k_geoloc_head(const Result *res, uint64_t n_host, uint64_t cap,
                                                    ImageResult *height, GeolocRecord *rec)
{
    const int t = threadIdx.x;
    if (t < kGeolocParts) {
        GeolocPart z{};
        z.min_key = 0xFFFFFFFFu;
        rec->part[t] = z;
    }
    if (t != 0) return;
    const bool failed = res && res->status != 0;
    uint64_t n = res ? (failed ? 0 : res->n_out) : n_host;
    n = n < cap ? n : cap;
    ImageResult r{};
    r.status = failed ? 1 : 0;
    r.reason = failed ? 4 : 0;
    r.height = static_cast<uint32_t>(n / kPx);
    r.channel_a = r.channel_b = -1;
    *height = r;
}

// ctl: the map device's control words ([1]: kSkip, kReasonCount or kReasonSgp4 from the track's launches)
__global__ __launch_bounds__(kThreads) void k_geoloc_rows(const ImageResult *height, const uint32_t *ctl, Scalars sc,
                                                          const Scalars *scp, int ref_is_end, int64_t ref_ms,
                                                          uint32_t rows_cap, double *sun, Frame *frame,
                                                          GeolocRecord *rec)
{
    const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t h = height->height;
    if (r == 0) {
        if (scp) sc = *scp;
        *frame = frame_of(sc.start_lat, sc.start_lon, sc.ref_az, sc.x_res, sc.y_res, sc.yaw);
        const uint32_t c = ctl[1];
        const int32_t reason = height->status != 0 ? kReasonDecode : h < 2 ? kReasonHeight : static_cast<int32_t>(c);
        rec->status = reason ? 1 : 0;
        rec->reason = reason;
        rec->height = h;
        rec->reserved = 0;
    }
    if (r >= h || r >= rows_cap) return;
    double u[3];
    sun_of(start_ms_of(ref_is_end != 0, ref_ms, h) + kLineMs * static_cast<int64_t>(r), u);
    sun[3 * r] = u[0];
    sun[3 * r + 1] = u[1];
    sun[3 * r + 2] = u[2];
}

__device__ inline uint32_t shfl_down_u32(uint32_t v, int d) { return static_cast<uint32_t>(__shfl_down(static_cast<int>(v), d)); }

// rows: holds the input rows already (the caller's buffer in place, or the copy in front of this launch)
template <unsigned OUT>
__global__ __launch_bounds__(kThreads) void k_geoloc(const GeolocRecord *rec_in, const Frame *__restrict__ frame,
                                                     const double *__restrict__ xoff, const double *__restrict__ sun,
                                                     uint32_t rows_cap, int base, float black, float cmin,
                                                     double2 *__restrict__ latlon, float *__restrict__ cos_sun,
                                                     float *rows, GeolocRecord *rec)
{
    const uint32_t h = rec_in->height < rows_cap ? rec_in->height : rows_cap;
    const bool ok = rec_in->status == 0;
    // (kMaxRows * 909 < 2^32: the flattened index fits 32 bits, and so does its division)
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    const bool in = i < h * static_cast<uint32_t>(kVideoN);

    uint32_t n_outside = 0, n_capped = 0, min_key = 0xFFFFFFFFu, max_key = 0u;
    if (in) {
        const uint32_t r = i / static_cast<uint32_t>(kVideoN);
        const int k = static_cast<int>(i - r * static_cast<uint32_t>(kVideoN));
        double lat = quiet_nan64(), lon = quiet_nan64();
        float c = quiet_nan();
        bool valid = false;
        if (ok) {
            const Frame f = *frame;
            const Point p = point_of(f, xoff_of(xoff[r], r), r, k);
            valid = p.valid;
            const float cs = cos_sun_of(p, sun + 3 * r);
            if (valid) {
                c = cs;
                if (OUT & kOutLatLon) latlon_of(p, lat, lon);
                const uint32_t key = key_of_bits(__float_as_uint(c));
                min_key = key;
                max_key = key;
                n_capped = c < cmin ? 1u : 0u;
            } else {
                n_outside = 1u;
            }
        }
        if (OUT & kOutLatLon) latlon[i] = make_double2(lat, lon);
        if (OUT & kOutCos) cos_sun[i] = c;
        if ((OUT & kOutRows) && valid) {
            float *px = rows + static_cast<uint64_t>(r) * kPx + base + kVideo0 + k;
            *px = normalised(*px, c, black, cmin, true);
        }
    }

    // ---- per wave, then at most four integer atomics per wave, on one of the partial records
    for (int d = 32; d >= 1; d >>= 1) {
        n_outside += shfl_down_u32(n_outside, d);
        n_capped += shfl_down_u32(n_capped, d);
        const uint32_t a = shfl_down_u32(min_key, d), b = shfl_down_u32(max_key, d);
        min_key = a < min_key ? a : min_key;
        max_key = b > max_key ? b : max_key;
    }
    if ((threadIdx.x & 63) == 0) {
        const uint64_t wave = static_cast<uint64_t>(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6);
        GeolocPart *part = &rec->part[wave % kGeolocParts];
        if (n_outside) atomicAdd(&part->n_outside, static_cast<unsigned long long>(n_outside));
        if (n_capped) atomicAdd(&part->n_capped, static_cast<unsigned long long>(n_capped));
        if (min_key <= max_key) {
            atomicMin(&part->min_key, min_key);
            atomicMax(&part->max_key, max_key);
        }
    }
}

uint32_t blocks(uint64_t n, uint32_t per)
{
    const uint64_t b = (n + per - 1) / per;
    return static_cast<uint32_t>(b ? b : 1);
}

uint32_t rows_of(const GeolocLaunch &l)
{
    const uint64_t rows = l.cap / kPx;
    return static_cast<uint32_t>(rows < kMaxRows ? rows : kMaxRows);
}

template <unsigned OUT>
void launch_pixels(hipStream_t s, const GeolocLaunch &l, apt::map::Device &dev, void *ws)
{
    Workspace *w = view(ws);
    const uint32_t rows = rows_of(l);
    hipLaunchKernelGGL(k_geoloc<OUT>, dim3(blocks(static_cast<uint64_t>(rows) * kVideoN, kThreads)), dim3(kThreads), 0,
                       s, &w->rec, &w->frame, dev.xoff, sun_table(ws), rows, kHalfPx * l.st.channel, l.st.black,
                       l.st.cmin, reinterpret_cast<double2 *>(l.latlon), l.cos_sun, l.rows, &w->rec);
}

}  // namespace

size_t geoloc_ws_bytes(size_t rows) { return kSunOffset + 3 * (rows ? rows : 1) * sizeof(double); }
GeolocRecord *geoloc_ws_record(void *ws) { return &view(ws)->rec; }
const apt::geoloc::Frame *geoloc_ws_frame(void *ws) { return &view(ws)->frame; }

void geoloc_record_to_public(const GeolocRecord &r, aptgpu_geoloc_result *out)
{
    aptgpu_geoloc_result v{};
    v.status = r.status;
    v.reason = r.reason;
    v.height = r.height;
    uint32_t min_key = 0xFFFFFFFFu, max_key = 0u;
    for (const GeolocPart &p : r.part) {
        v.n_outside += p.n_outside;
        v.n_capped += p.n_capped;
        min_key = p.min_key < min_key ? p.min_key : min_key;
        max_key = p.max_key > max_key ? p.max_key : max_key;
    }
    v.cos_min = v.cos_max = quiet_nan();
    if (min_key <= max_key) {
        const uint32_t lo = bits_of_key(min_key), hi = bits_of_key(max_key);
        std::memcpy(&v.cos_min, &lo, sizeof lo);
        std::memcpy(&v.cos_max, &hi, sizeof hi);
    }
    put_result(out, v);
}

void geoloc_track(hipStream_t s, const GeolocLaunch &l, apt::map::Device &dev, void *ws)
{
    Workspace *w = view(ws);
    hipLaunchKernelGGL(k_geoloc_head, dim3(1), dim3(64), 0, s, l.res, l.n, l.cap, &w->height, &w->rec);
    if (l.sat) {
        apt::map::image_map_track_sat(s, dev, *l.sat, l.geom.yaw, l.geom.hscale, l.geom.vscale, &w->height);
    } else {
        dev.upload_track(s, l.positions, l.n_positions);
        const Scalars sc = apt::map::scalars(l.positions, l.n_positions, l.geom.yaw, l.geom.hscale, l.geom.vscale);
        const uint32_t count = l.n_positions > 0xFFFFFFFFu ? 0xFFFFFFFFu : static_cast<uint32_t>(l.n_positions);
        apt::map::image_map_track(s, dev, sc, count, &w->height);
    }
}

void geoloc_rows(hipStream_t s, const GeolocLaunch &l, apt::map::Device &dev, void *ws)
{
    Workspace *w = view(ws);
    const uint32_t rows = rows_of(l);
    Scalars sc{};
    if (!l.sat) sc = apt::map::scalars(l.positions, l.n_positions, l.geom.yaw, l.geom.hscale, l.geom.vscale);
    hipLaunchKernelGGL(k_geoloc_rows, dim3(blocks(rows, kThreads)), dim3(kThreads), 0, s, &w->height, dev.ctl, sc,
                       l.sat ? dev.scalars : nullptr, l.sat ? l.sat->ref_is_end : (l.st.ref_is_end ? 1 : 0),
                       l.sat ? l.sat->ref_ms : l.st.ref_ms, rows, sun_table(ws), &w->frame, &w->rec);
}

void geoloc_pixels(hipStream_t s, const GeolocLaunch &l, apt::map::Device &dev, void *ws)
{
    const unsigned out = (l.latlon ? kOutLatLon : 0u) | (l.cos_sun ? kOutCos : 0u) | (l.rows ? kOutRows : 0u);
    if (l.rows && l.rows != l.x) {
        // (all cap floats: the consumer behind reads what the decode wrote, whatever the height turns out to be)
        const uint64_t floats = static_cast<uint64_t>(rows_of(l)) * kPx;
        if (floats)
            apt::hip_check(hipMemcpyAsync(l.rows, l.x, floats * sizeof(float), hipMemcpyDeviceToDevice, s),
                           "hipMemcpyAsync D2D (geoloc rows)");
    }
    switch (out) {
    case 0: launch_pixels<0>(s, l, dev, ws); break;  // (the record's counters alone)
    case 1: launch_pixels<1>(s, l, dev, ws); break;
    case 2: launch_pixels<2>(s, l, dev, ws); break;
    case 3: launch_pixels<3>(s, l, dev, ws); break;
    case 4: launch_pixels<4>(s, l, dev, ws); break;
    case 5: launch_pixels<5>(s, l, dev, ws); break;
    case 6: launch_pixels<6>(s, l, dev, ws); break;
    default: launch_pixels<7>(s, l, dev, ws); break;
    }
}

}  // namespace apt::gpu
