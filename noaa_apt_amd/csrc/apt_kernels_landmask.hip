// apt_kernels_landmask.hip — the gfx950 kernels of the land / sea / lake mask and of the map-coloured false colour
// (definition: apt_kernels_landmask.hpp, include/aptgpu.h).
//
//  k_land_mask<SRC>      the hot path.  One thread per point of the flattened index, so every wave is full and, in the
//                        swath form, touches at most two rows.  Each wave reduces the lowest and highest band over its
//                        valid lanes with shuffles and walks the records of those bands with a wave-uniform index: the
//                        32-byte records come through the scalar data cache (s_load_dwordx2, no per-lane vector load)
//                        and every lane tests every record.  A lane counts a crossing only while the walk is in its own
//                        band (an edge that spans several bands is listed in each of them), and the straddle test
//                        rejects the rest.  What the listing shows per record: y1 and y2 are fetched and compared
//                        first, and the wave branches on the result (s_and_saveexec, s_cbranch_execz): where no lane
//                        straddles, which is most records of a band, x1, x2 and the seven f64 operations of d are
//                        skipped; where one does, a second pair of scalar loads and a second wait follow.  So the lanes
//                        never diverge from each other in what they fetch, but the walk is not branch-free.  The
//                        branch-free form (one s_load_dwordx8, & for && in crossing()) was built and measured: 0.67
//                        against 0.48 ms per recording, the f64 work it no longer skips costs more than the second
//                        wait.  No LDS.
//                        A wave without a valid lane skips the walk.  One byte per lane is stored,
//                        contiguous across the wave; the four counts come from ballots and reach one of 64 partial
//                        records with at most four integer atomics per wave.
//                        SRC = Plane reads the point from an (n, 2) f64 plane; SRC = Swath computes it from the track
//                        and the geometry with the geolocation stage's own text, behind that stage's track and row
//                        launches, so the lat / lon plane never exists.
//  k_false_color_masked  one thread per pixel of the un-rotated image: gray, or inside channel A's video the palette of
//                        the pixel's class.
#include "apt_kernels_landmask.hpp"

#include "apt_kernels_map_dev.hpp"

#include <cstddef>

#pragma clang fp contract(off)

namespace apt::gpu {

namespace {

using namespace apt::landmask;
namespace geo = apt::geoloc;

constexpr int kThreads = 256;

struct Plane {
    const double2 *latlon;
    uint64_t n;
    // the point of index i; false: i lies behind the end
    __device__ bool in(uint64_t i) const { return i < n; }
    __device__ bool point(uint64_t i, double &lat, double &lon) const
    {
        const double2 v = latlon[i];
        lat = v.x;
        lon = v.y;
        return true;
    }
    __device__ void head(LandRecord *rec) const
    {
        rec->status = 0;
        rec->reason = 0;
        rec->height = 0;
        rec->reserved = 0;
    }
};

struct Swath {
    const GeolocRecord *grec;  // the geolocation stage's record: status, reason, height
    const geo::Frame *frame;
    const double *xoff;
    uint32_t rows_cap;
    __device__ uint32_t height() const { return grec->height < rows_cap ? grec->height : rows_cap; }
    // (kMaxRows * 909 < 2^32: the flattened index fits 32 bits, and so does its division)
    __device__ bool in(uint64_t i) const { return i < static_cast<uint64_t>(height()) * geo::kVideoN; }
    // false: the stage in front failed, every pixel of the rows is invalid
    __device__ bool point(uint64_t i, double &lat, double &lon) const
    {
        lat = lon = geo::quiet_nan64();
        if (grec->status != 0) return false;
        const uint32_t r = static_cast<uint32_t>(i) / static_cast<uint32_t>(geo::kVideoN);
        const int k = static_cast<int>(static_cast<uint32_t>(i) - r * static_cast<uint32_t>(geo::kVideoN));
        const geo::Frame f = *frame;
        const geo::Point p = geo::point_of(f, geo::xoff_of(xoff[r], r), r, k);
        if (p.valid) geo::latlon_of(p, lat, lon);
        return true;
    }
    __device__ void head(LandRecord *rec) const
    {
        rec->status = grec->status;
        rec->reason = grec->reason;
        rec->height = grec->height;
        rec->reserved = 0;
    }
};

// min and max of an int over the wave, in every lane
__device__ inline void wave_min_max(int &lo, int &hi)
{
    for (int d = 32; d >= 1; d >>= 1) {
        const int a = __shfl_xor(lo, d), b = __shfl_xor(hi, d);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
}

// off: 2 * nb + 1 offsets (countries' bands, then the lakes'); edges: the records
template <typename SRC>
__global__ __launch_bounds__(kThreads) void k_land_mask(SRC src, const uint32_t *__restrict__ off,
                                                        const Edge *__restrict__ edges, int nb, double scale,
                                                        uint8_t *__restrict__ mask, LandRecord *rec)
{
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i == 0) src.head(rec);
    const bool in = src.in(i);
    double lat = geo::quiet_nan64(), lon = geo::quiet_nan64();
    if (in) src.point(i, lat, lon);
    const bool valid = in && lat == lat && lon == lon;
    const double py = lat * kDeg, px = lon * kDeg;
    const int band = valid ? band_of(py, nb, scale) : -1;

    int lo = valid ? band : 0x7FFFFFFF, hi = band;
    wave_min_max(lo, hi);
    const int bmin = __builtin_amdgcn_readfirstlane(lo), bmax = __builtin_amdgcn_readfirstlane(hi);

    uint32_t odd[2] = {0u, 0u};
    for (int b = bmin; b <= bmax; ++b) {  // (no valid lane: 0x7FFFFFFF > -1, no trip)
        const bool mine = b == band;
        for (int li = 0; li < 2; ++li) {
            const uint32_t e0 = __builtin_amdgcn_readfirstlane(off[li * nb + b]);
            const uint32_t e1 = __builtin_amdgcn_readfirstlane(off[li * nb + b + 1]);
            uint32_t n = 0;
            for (uint32_t e = e0; e < e1; ++e) {
                const Edge ed = edges[e];
                n += crossing(ed, px, py) ? 1u : 0u;
            }
            odd[li] ^= mine ? (n & 1u) : 0u;
        }
    }
    const uint32_t cls = valid ? class_of(odd[0] != 0u, odd[1] != 0u) : kInvalid;
    if (in) mask[i] = static_cast<uint8_t>(cls);

    // ---- per wave: four ballots, then at most four integer atomics on one of the partial records
    const unsigned long long m_sea = __ballot(in && cls == kSea), m_land = __ballot(in && cls == kLand);
    const unsigned long long m_lake = __ballot(in && cls == kLake), m_inv = __ballot(in && cls == kInvalid);
    if ((threadIdx.x & 63) == 0) {
        const uint64_t wave = static_cast<uint64_t>(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6);
        LandPart *part = &rec->part[wave % kLandParts];
        if (m_sea) atomicAdd(&part->n[0], static_cast<unsigned long long>(__popcll(m_sea)));
        if (m_land) atomicAdd(&part->n[1], static_cast<unsigned long long>(__popcll(m_land)));
        if (m_lake) atomicAdd(&part->n[2], static_cast<unsigned long long>(__popcll(m_lake)));
        if (m_inv) atomicAdd(&part->n[3], static_cast<unsigned long long>(__popcll(m_inv)));
    }
}

__global__ __launch_bounds__(kThreads) void k_false_color_masked(const uint8_t *__restrict__ image, uint32_t h,
                                                                 const uint8_t *__restrict__ mask,
                                                                 const uint32_t *__restrict__ pal, Tune tn,
                                                                 uint32_t *__restrict__ out)
{
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= static_cast<uint64_t>(h) * geo::kPx) return;
    const uint64_t y = i / geo::kPx;
    const uint32_t x = static_cast<uint32_t>(i - y * geo::kPx);
    const bool video = x >= static_cast<uint32_t>(geo::kVideo0) && x < static_cast<uint32_t>(geo::kVideo0 + geo::kVideoN);
    const uint32_t g_b = video ? image[i + geo::kHalfPx] : 0u;
    const uint32_t c = video ? mask[y * geo::kVideoN + (x - geo::kVideo0)] : 255u;
    out[i] = masked_pixel(x, image[i], g_b, c, tn, pal);
}

uint32_t blocks(uint64_t n, uint32_t per)
{
    const uint64_t b = (n + per - 1) / per;
    return static_cast<uint32_t>(b ? b : 1);
}

template <typename SRC>
void launch(hipStream_t s, const LandTable &t, const SRC &src, uint64_t points, uint8_t *d_mask, LandRecord *rec)
{
    apt::hip_check(hipMemsetAsync(rec, 0, sizeof(LandRecord), s), "hipMemsetAsync (land mask record)");
    const int nb = t.host->nb;
    hipLaunchKernelGGL(k_land_mask<SRC>, dim3(blocks(points, kThreads)), dim3(kThreads), 0, s, src, t.off.ptr,
                       t.edges.ptr, nb, static_cast<double>(nb) / 180.0, d_mask, rec);
}

}  // namespace

void land_record_to_public(const LandRecord &r, aptgpu_land_mask_result head, aptgpu_land_mask_result *out)
{
    head.status = r.status;
    head.reason = r.reason;
    head.height = r.height;
    head.n_sea = head.n_land = head.n_lake = head.n_invalid = 0;
    for (const LandPart &p : r.part) {
        head.n_sea += p.n[0];
        head.n_land += p.n[1];
        head.n_lake += p.n[2];
        head.n_invalid += p.n[3];
    }
    apt::landmask::put_result(out, head);
}

void LandTable::upload(hipStream_t s, const std::shared_ptr<const Table> &t)
{
    if (host && host->gen == t->gen && host->nb == t->nb && off.ptr) return;
    if (off.count < t->off.size()) off.alloc(t->off.size());
    if (edges.count < t->edges.size() + 1) edges.alloc(t->edges.size() + 1);
    apt::hip_check(hipMemcpyAsync(off.ptr, t->off.data(), t->off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s),
                   "hipMemcpyAsync H2D (land mask table)");
    if (!t->edges.empty())
        apt::hip_check(hipMemcpyAsync(edges.ptr, t->edges.data(), t->edges.size() * sizeof(Edge), hipMemcpyHostToDevice, s),
                       "hipMemcpyAsync H2D (land mask table)");
    host = t;
}

void land_mask_plane(hipStream_t s, const LandTable &t, const double *d_latlon, uint64_t n, uint8_t *d_mask,
                     LandRecord *rec)
{
    launch(s, t, Plane{reinterpret_cast<const double2 *>(d_latlon), n}, n, d_mask, rec);
}

void land_mask_swath(hipStream_t s, const LandTable &t, const void *geoloc_ws, const apt::map::Device &dev,
                     uint32_t rows_cap, uint8_t *d_mask, LandRecord *rec)
{
    void *ws = const_cast<void *>(geoloc_ws);
    const uint32_t rows = rows_cap < geo::kMaxRows ? rows_cap : geo::kMaxRows;
    launch(s, t, Swath{geoloc_ws_record(ws), geoloc_ws_frame(ws), dev.xoff, rows},
           static_cast<uint64_t>(rows) * geo::kVideoN, d_mask, rec);
}

void false_color_masked(hipStream_t s, const uint8_t *d_image, uint32_t h, const uint8_t *d_mask,
                        const uint32_t *d_palettes, const Tune &tune, uint8_t *d_out)
{
    hipLaunchKernelGGL(k_false_color_masked, dim3(blocks(static_cast<uint64_t>(h) * geo::kPx, kThreads)), dim3(kThreads),
                       0, s, d_image, h, d_mask, d_palettes, tune, reinterpret_cast<uint32_t *>(d_out));
}

}  // namespace apt::gpu
