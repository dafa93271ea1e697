// apt_kernels_map.hip — gfx950 kernels of the map overlay (apt_kernels_map.hpp; map.rs:14-200).
//
// One call is eleven launches on the image's stream, none of them waiting on the host (with the track computed on the
// device, apt_kernels_track.hpp, two more in front, and the first two below read their scalars from device memory):
//   k_map_track    x offset of every track row (map.rs:110-114), and the call's checks (count == height)
//   k_map_project  latlon_to_rel_px of every vertex, once (map.rs:71-100); both segments that share a vertex
//                  read the same value, as the reference's two evaluations of one input give
//   k_map_count    per segment draw_line(pt, prev_pt): offset correction, the point-1 cull, and the number of
//                  fragments its Xiaolin Wu walk draws (one thread per segment: the walk accumulates y += gradient
//                  sequentially and cannot be split without changing the rounding)
//   scan (3)       exclusive prefix sum of the counts = every fragment's place in the global draw order
//   k_map_emit     the same walk again, writing the fragments in draw order
//   k_map_link     the two copies of every fragment (columns x + 539, x + 1579, through the rotation when it is
//                  folded into the image) are counted per pixel; each copy keeps its arrival slot there
//   k_map_alloc    the first arrival at every pixel reserves a contiguous run of the pixel's count (one atomic per
//                  workgroup) and checks the per-pixel bound
//   k_map_scatter  every copy writes its index into its pixel's run at its slot
//   k_map_blend    the first arrival sorts its pixel's run by copy index (= draw order: insertion sort for short
//                  runs, heapsort otherwise, O(k log k)) and blends in that order (image 0.24.7's Rgba::blend is
//                  order-dependent), then zeroes the pixel's count for the next call
//
// f64 math is the reference's, operation for operation (contract off); sin/cos/tan/atan/asin/acos/atan2 are the
// device library's, which may differ from glibc by an ulp (the parity contract of DESIGN.md §12).  The blend is
// f32, one rounding per operation, as the crate's.
#include "apt_kernels_map.hpp"

#include "apt_kernels_map_dev.hpp"
#include "apt_kernels_track.hpp"

#include <cmath>
#include <cstring>

#pragma clang fp contract(off)

namespace apt::map {

namespace {

using apt::gpu::ImageResult;

constexpr int kPx = 2080;
constexpr int kThreads = 256;
constexpr int kScanItems = 8;
constexpr int kScanBlock = kThreads * kScanItems;
constexpr int kListBlocks = 1024;

// line_drawing 1.0.0's XiaolinWu<f64, i32> from (sx, sy) to (ex, ey), calling emit(x, y, value) for the points
// that pass map.rs's band test x in (-456, 456), y in (0, h).  Stops once the major axis has left the band (nothing
// later can pass).  false: a non-finite end or more than kMaxWalk steps (the caller reports it).
template <typename Emit>
__device__ inline bool walk(double sx, double sy, double ex, double ey, int h, Emit &&emit)
{
    if (!(isfinite(sx) && isfinite(sy) && isfinite(ex) && isfinite(ey))) return false;
    const bool steep = fabs(ey - sy) > fabs(ex - sx);
    if (steep) {
        double t = sx; sx = sy; sy = t;
        t = ex; ex = ey; ey = t;
    }
    if (sx > ex) {
        double t = sx; sx = ex; ex = t;
        t = sy; sy = ey; ey = t;
    }
    const double dx = ex - sx;
    if (!(dx <= static_cast<double>(kMaxWalk))) return false;
    const double gradient = dx == 0. ? 1. : (ey - sy) / dx;
    int x = static_cast<int>(round(sx));
    const int end_x = static_cast<int>(round(ex));
    const int stop = steep ? h : 456;
    double y = sy;
    bool lower = false;
    while (x <= end_x && x < stop) {
        const double fpart = y - floor(y);
        int yi = static_cast<int>(y);  // NumCast: truncation toward zero
        if (lower) yi += 1;
        const int px = steep ? yi : x, py = steep ? x : yi;
        double value;
        if (lower) {
            lower = false;
            x += 1;
            y += gradient;
            value = fpart;
        } else {
            if (fpart > 0.) {
                lower = true;
            } else {
                x += 1;
                y += gradient;
            }
            value = 1. - fpart;
        }
        if (px > -456 && px < 456 && py > 0 && py < h) emit(px, py, value);
    }
    return true;
}

// draw_line(latlon1, latlon2) up to the walk: offset correction and the point-1 cull (map.rs:107-124).  The
// `±456` clause of the cull is inside the `±600` one.
struct Seg {
    double x1, y1, x2, y2;
    bool drawn;
};

__device__ inline Seg segment(const double *proj, const int32_t *meta, const double *xoff, uint32_t v, uint32_t h)
{
    const uint32_t p = static_cast<uint32_t>(meta[2 * v]);
    Seg s;
    s.x1 = proj[2 * v];
    s.y1 = proj[2 * v + 1];
    s.x2 = proj[2 * p];
    s.y2 = proj[2 * p + 1];
    s.x1 -= xoff[est_row(s.y1, h)];
    s.x2 -= xoff[est_row(s.y2, h)];
    s.drawn = s.x1 > -600. && s.x1 < 600. && s.y1 > 0. && s.y1 < static_cast<double>(h);
    return s;
}

__device__ inline uint32_t alpha_u8(double value, uint32_t a)
{
    const double v = value * static_cast<double>(a);  // `as u8` saturates; value is in [0, 1]
    return v >= 255. ? 255u : (v > 0. ? static_cast<uint32_t>(v) : 0u);
}

// fragment: y (32 bits) | x + 456 (10) | alpha (8) | layer (2)
__device__ inline uint64_t pack(int x, int y, uint32_t alpha, uint32_t layer)
{
    return static_cast<uint64_t>(static_cast<uint32_t>(y)) | (static_cast<uint64_t>(x + 456) << 32) |
           (static_cast<uint64_t>(alpha) << 42) | (static_cast<uint64_t>(layer) << 50);
}

__device__ inline void set_error(uint32_t *ctl, uint32_t reason)
{
    atomicCAS(&ctl[1], 0u, reason);
}

__global__ __launch_bounds__(kThreads) void k_map_track(const double *track, uint32_t count, uint32_t rows,
                                                        Scalars sc, double *xoff, const ImageResult *info,
                                                        uint32_t *ctl)
{
    const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
    if (r == 0) {
        ctl[0] = 0;
        ctl[2] = 0;
        ctl[1] = info->status != 0 ? kSkip : (count == 0 || count > rows || count != info->height ? kReasonCount : 0u);
    }
    if (r >= rows || r >= count) return;
    double x, y;
    rel_px(sc, track[2 * r], track[2 * r + 1], x, y);
    xoff[r] = x;
}

__global__ __launch_bounds__(kThreads) void k_map_project(const double *verts, uint32_t n, Scalars sc, double *proj)
{
    const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= n) return;
    // (pt.y / 180. * PI, pt.x / 180. * PI), map.rs:142-143
    const double lat = verts[2 * v + 1] / 180. * kPi, lon = verts[2 * v] / 180. * kPi;
    double x, y;
    rel_px(sc, lat, lon, x, y);
    proj[2 * v] = x;
    proj[2 * v + 1] = y;
}

// The two kernels above fed from the device: the scalars and the row count are k_sat_scalars' (the height itself, so
// the count check can only fail on the capacity), ctl[3] holds k_sat_track's SGP4 error.
__global__ __launch_bounds__(kThreads) void k_map_track_dev(const double *track, uint32_t rows_cap, const Scalars *scp,
                                                            double *xoff, const ImageResult *info, uint32_t *ctl)
{
    const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t count = ctl[4];
    if (r == 0) {
        ctl[0] = 0;
        ctl[2] = 0;
        ctl[1] = info->status != 0 ? kSkip
                 : ctl[3] != 0     ? static_cast<uint32_t>(apt::sat::kReasonSgp4)
                                   : (count == 0 || count > rows_cap ? kReasonCount : 0u);
        ctl[3] = 0;  // (zero between calls, as k_sat_track expects it)
    }
    if (r >= rows_cap || r >= count) return;
    const Scalars sc = *scp;
    double x, y;
    rel_px(sc, track[2 * r], track[2 * r + 1], x, y);
    xoff[r] = x;
}

__global__ __launch_bounds__(kThreads) void k_map_project_dev(const double *verts, uint32_t n, const Scalars *scp,
                                                              double *proj)
{
    const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= n) return;
    const Scalars sc = *scp;
    const double lat = verts[2 * v + 1] / 180. * kPi, lon = verts[2 * v] / 180. * kPi;
    double x, y;
    rel_px(sc, lat, lon, x, y);
    proj[2 * v] = x;
    proj[2 * v + 1] = y;
}

__global__ __launch_bounds__(kThreads) void k_map_count(const double *proj, const int32_t *meta, uint32_t n,
                                                        const double *xoff, const ImageResult *info, uint32_t *ctl,
                                                        uint64_t *seg)
{
    const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
    if (v > n) return;
    uint64_t cnt = 0;
    if (v < n && ctl[1] == 0) {
        const uint32_t h = info->height;
        const Seg s = segment(proj, meta, xoff, v, h);
        if (s.drawn && !walk(s.x1, s.y1, s.x2, s.y2, static_cast<int>(h), [&](int, int, double) { ++cnt; }))
            set_error(ctl, kReasonWalk);
    }
    seg[v] = cnt;  // seg[n] = 0: the scan's total lands there
}

__global__ __launch_bounds__(kThreads) void k_map_emit(const double *proj, const int32_t *meta, uint32_t n,
                                                       const double *xoff, const ImageResult *info,
                                                       const uint32_t *ctl, const uint64_t *seg, Colors colors,
                                                       uint64_t *frags)
{
    const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= n || ctl[1] != 0) return;
    const uint32_t h = info->height;
    const Seg s = segment(proj, meta, xoff, v, h);
    if (!s.drawn) return;
    const uint32_t layer = static_cast<uint32_t>(meta[2 * v + 1]);
    const uint32_t a = colors.c[layer] >> 24;
    uint64_t o = seg[v];
    walk(s.x1, s.y1, s.x2, s.y2, static_cast<int>(h), [&](int x, int y, double value) {
        if (o < kMaxFragments) frags[o] = pack(x, y, alpha_u8(value, a), layer);
        ++o;
    });
}

// ---- exclusive scan of n + 1 u64 counts (the last is 0), total -> ctl[0]
__global__ __launch_bounds__(kThreads) void k_scan_local(uint64_t *a, uint32_t n, uint64_t *sums)
{
    __shared__ uint64_t s[kThreads];
    const uint32_t base = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
    uint64_t v[kScanItems], t = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        v[k] = base + k < n ? a[base + k] : 0;
        t += v[k];
    }
    s[threadIdx.x] = t;
    __syncthreads();
    for (int off = 1; off < kThreads; off <<= 1) {
        const uint64_t add = threadIdx.x >= static_cast<uint32_t>(off) ? s[threadIdx.x - off] : 0;
        __syncthreads();
        s[threadIdx.x] += add;
        __syncthreads();
    }
    uint64_t e = s[threadIdx.x] - t;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        if (base + k < n) a[base + k] = e;
        e += v[k];
    }
    if (threadIdx.x == kThreads - 1) sums[blockIdx.x] = s[kThreads - 1];
}

__global__ __launch_bounds__(1024) void k_scan_sums(uint64_t *sums, uint32_t nb, uint32_t *ctl)
{
    __shared__ uint64_t s[1024];
    const uint32_t per = (nb + 1023) / 1024;
    const uint32_t b0 = threadIdx.x * per;
    uint64_t t = 0;
    for (uint32_t k = 0; k < per; ++k)
        if (b0 + k < nb) t += sums[b0 + k];
    s[threadIdx.x] = t;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const uint64_t add = threadIdx.x >= static_cast<uint32_t>(off) ? s[threadIdx.x - off] : 0;
        __syncthreads();
        s[threadIdx.x] += add;
        __syncthreads();
    }
    uint64_t e = s[threadIdx.x] - t;
    for (uint32_t k = 0; k < per; ++k)
        if (b0 + k < nb) {
            const uint64_t x = sums[b0 + k];
            sums[b0 + k] = e;
            e += x;
        }
    if (threadIdx.x == 1023) {
        const uint64_t total = s[1023];
        if (total > kMaxFragments) set_error(ctl, kReasonOverflow);
        ctl[0] = ctl[1] == 0 ? static_cast<uint32_t>(total) : 0u;
    }
}

__global__ __launch_bounds__(kThreads) void k_scan_add(uint64_t *a, uint32_t n, const uint64_t *sums)
{
    const uint32_t base = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
    const uint64_t add = sums[blockIdx.x];
#pragma unroll
    for (int k = 0; k < kScanItems; ++k)
        if (base + k < n) a[base + k] += add;
}

// the pixel a fragment copy lands on, after the rotation when it is folded in (processing.rs:21-37: sub-images
// [86, 995) and [1126, 2035) turn by 180 degrees; columns 84, 85, 1124, 1125 of the overlay keep their row)
__device__ inline uint32_t pixel_of(uint64_t f, uint32_t copy, uint32_t h, bool rotate)
{
    uint32_t y = static_cast<uint32_t>(f);
    int col = static_cast<int>((f >> 32) & 1023u) - 456 + (copy ? 1579 : 539);
    if (rotate) {
        if (col >= 86 && col < 995) {
            col = 1080 - col;
            y = h - 1 - y;
        } else if (col >= 1126 && col < 2035) {
            col = 3160 - col;
            y = h - 1 - y;
        }
    }
    return y * kPx + static_cast<uint32_t>(col);
}

__global__ __launch_bounds__(kThreads) void k_map_link(const uint64_t *frags, const uint32_t *ctl,
                                                       const ImageResult *info_in, ImageResult *info, bool rotate,
                                                       uint32_t *cnt, uint32_t *slot)
{
    const uint32_t e = ctl[1];
    if (blockIdx.x == 0 && threadIdx.x == 0 && e != 0 && e != kSkip) {
        info->status = 1;
        info->reason = static_cast<int32_t>(e);
    }
    if (e != 0) return;
    const uint32_t total = ctl[0], h = info_in->height;
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < 2 * total; i += kListBlocks * kThreads) {
        const uint32_t p = pixel_of(frags[i >> 1], i & 1u, h, rotate);
        slot[i] = atomicAdd(&cnt[p], 1u);
    }
}

// Runs are placed in arrival order of the workgroups (their order in `runs` does not matter, only that each is
// contiguous): a workgroup scans its owners' counts in LDS and reserves them with one atomic.
__global__ __launch_bounds__(kThreads) void k_map_alloc(const uint64_t *frags, uint32_t *ctl, const ImageResult *info,
                                                        bool rotate, const uint32_t *cnt, const uint32_t *slot,
                                                        uint32_t *base)
{
    __shared__ uint32_t s[kThreads];
    __shared__ uint32_t skip, block_base;
    if (threadIdx.x == 0) skip = ctl[1];
    __syncthreads();
    if (skip != 0) return;  // (uniform per workgroup)
    const uint32_t n = 2 * ctl[0], h = info->height;
    for (uint32_t b0 = blockIdx.x * kThreads; b0 < n; b0 += kListBlocks * kThreads) {
        const uint32_t i = b0 + threadIdx.x;
        uint32_t c = 0, p = 0;
        if (i < n && slot[i] == 0) {
            p = pixel_of(frags[i >> 1], i & 1u, h, rotate);
            c = cnt[p];
            if (c > kMaxPixelFragments) set_error(ctl, kReasonPixel);
        }
        s[threadIdx.x] = c;
        __syncthreads();
        for (int off = 1; off < kThreads; off <<= 1) {
            const uint32_t add = threadIdx.x >= static_cast<uint32_t>(off) ? s[threadIdx.x - off] : 0u;
            __syncthreads();
            s[threadIdx.x] += add;
            __syncthreads();
        }
        if (threadIdx.x == kThreads - 1) block_base = atomicAdd(&ctl[2], s[kThreads - 1]);
        __syncthreads();
        if (c) base[p] = block_base + s[threadIdx.x] - c;
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreads) void k_map_scatter(const uint64_t *frags, const uint32_t *ctl,
                                                          const ImageResult *info, bool rotate, const uint32_t *slot,
                                                          const uint32_t *base, uint32_t *runs)
{
    if (ctl[1] != 0) return;
    const uint32_t n = 2 * ctl[0], h = info->height;
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < n; i += kListBlocks * kThreads) {
        const uint32_t p = pixel_of(frags[i >> 1], i & 1u, h, rotate);
        runs[base[p] + slot[i]] = i;
    }
}

__device__ inline void sift_down(uint32_t *a, uint32_t root, uint32_t n)
{
    const uint32_t v = a[root];
    for (;;) {
        uint32_t c = 2 * root + 1;
        if (c >= n) break;
        if (c + 1 < n && a[c + 1] > a[c]) ++c;
        if (a[c] <= v) break;
        a[root] = a[c];
        root = c;
    }
    a[root] = v;
}

// ascending, in place: insertion sort for short runs (the common case: a handful of copies), heapsort otherwise
__device__ inline void sort_run(uint32_t *a, uint32_t n)
{
    if (n <= 32) {
        for (uint32_t j = 1; j < n; ++j) {
            const uint32_t v = a[j];
            uint32_t k = j;
            for (; k > 0 && a[k - 1] > v; --k) a[k] = a[k - 1];
            a[k] = v;
        }
        return;
    }
    for (uint32_t r = n / 2; r-- > 0;) sift_down(a, r, n);
    for (uint32_t end = n; end-- > 1;) {
        const uint32_t t = a[0];
        a[0] = a[end];
        a[end] = t;
        sift_down(a, 0, end);
    }
}

// The first arrival at each pixel blends its run in draw order.  After a per-pixel overflow (found by k_map_alloc)
// nothing is blended, but the counts are still zeroed so the next call starts clean.
__global__ __launch_bounds__(kThreads) void k_map_blend(const uint64_t *frags, const uint32_t *ctl, ImageResult *info,
                                                        bool rotate, Colors colors, uint32_t *cnt, const uint32_t *slot,
                                                        const uint32_t *base, uint32_t *runs, uint32_t *img)
{
    const uint32_t e = ctl[1];
    if (e != 0 && e != static_cast<uint32_t>(kReasonPixel)) return;
    if (blockIdx.x == 0 && threadIdx.x == 0 && e != 0) {
        info->status = 1;
        info->reason = static_cast<int32_t>(e);
    }
    const uint32_t n = 2 * ctl[0], h = info->height;
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < n; i += kListBlocks * kThreads) {
        if (slot[i] != 0) continue;  // another copy owns this pixel
        const uint32_t p = pixel_of(frags[i >> 1], i & 1u, h, rotate);
        if (e == 0) {
            const uint32_t k = cnt[p];
            uint32_t *run = runs + base[p];
            sort_run(run, k);
            uint32_t px = img[p];
            for (uint32_t j = 0; j < k; ++j) {
                const uint64_t fr = frags[run[j] >> 1];
                const uint32_t layer = static_cast<uint32_t>(fr >> 50) & 3u;
                const uint32_t alpha = static_cast<uint32_t>(fr >> 42) & 255u;
                px = blend(px, (colors.c[layer] & 0x00ffffffu) | (alpha << 24));
            }
            img[p] = px;
        }
        cnt[p] = 0;
    }
}

uint32_t blocks(uint64_t n, uint32_t per)
{
    const uint64_t b = (n + per - 1) / per;
    return static_cast<uint32_t>(b ? b : 1);
}

template <typename T>
void dev_alloc(T *&p, size_t n, const char *what)
{
    if (p) (void)hipFree(p);
    p = nullptr;
    apt::hip_check(hipMalloc(reinterpret_cast<void **>(&p), (n ? n : 1) * sizeof(T)), what);
}

}  // namespace

Device::~Device()
{
    for (void *p : {static_cast<void *>(verts), static_cast<void *>(meta), static_cast<void *>(proj),
                    static_cast<void *>(seg), static_cast<void *>(sums), static_cast<void *>(track),
                    static_cast<void *>(xoff), static_cast<void *>(frags), static_cast<void *>(slot),
                    static_cast<void *>(runs), static_cast<void *>(cnt), static_cast<void *>(base),
                    static_cast<void *>(ctl), static_cast<void *>(scalars)})
        if (p) (void)hipFree(p);
    for (int k = 0; k < kTrackRing; ++k) {
        if (track_ev[k]) (void)hipEventDestroy(track_ev[k]);
        if (track_host[k]) (void)hipHostFree(track_host[k]);
    }
}

void Device::prepare_control(hipStream_t s)
{
    if (ctl) return;
    dev_alloc(ctl, kCtlWords, "hipMalloc (map control)");
    dev_alloc(scalars, 1, "hipMalloc (map control)");
    apt::hip_check(hipMemsetAsync(ctl, 0, kCtlWords * sizeof(uint32_t), s), "hipMemsetAsync");
}

void Device::prepare_track(hipStream_t s, size_t rows)
{
    prepare_control(s);
    if (rows_cap >= rows && track) return;
    // (the overlay's per-pixel lists are sized by rows_cap too: prepare() makes them anew when it finds them gone)
    for (void *p : {static_cast<void *>(cnt), static_cast<void *>(base)})
        if (p) (void)hipFree(p);
    cnt = base = nullptr;
    rows_cap = rows > rows_cap ? rows : rows_cap;
    dev_alloc(track, 2 * rows_cap, "hipMalloc (map track)");
    dev_alloc(xoff, rows_cap, "hipMalloc (map track)");
    for (int k = 0; k < kTrackRing; ++k) {
        if (track_ev[k]) apt::hip_check(hipEventSynchronize(track_ev[k]), "hipEventSynchronize");
        if (track_host[k]) (void)hipHostFree(track_host[k]);
        track_host[k] = nullptr;
    }
}

void Device::prepare(hipStream_t s, const Layers &layers, size_t rows)
{
    const size_t n = layers.xy.size() / 2;
    if (!frag_ready) {
        dev_alloc(frags, kMaxFragments, "hipMalloc (map fragments)");
        dev_alloc(slot, 2 * static_cast<size_t>(kMaxFragments), "hipMalloc (map runs)");
        dev_alloc(runs, 2 * static_cast<size_t>(kMaxFragments), "hipMalloc (map runs)");
        prepare_control(s);
        frag_ready = true;
    }
    if (vert_cap < n + 1 || !verts) {
        vert_cap = n + 1;
        dev_alloc(verts, 2 * vert_cap, "hipMalloc (map vertices)");
        dev_alloc(meta, 2 * vert_cap, "hipMalloc (map vertices)");
        dev_alloc(proj, 2 * vert_cap, "hipMalloc (map projection)");
        dev_alloc(seg, vert_cap, "hipMalloc (map segments)");
        dev_alloc(sums, blocks(vert_cap, kScanBlock), "hipMalloc (map scan)");
        gen = 0;
    }
    if (gen != layers.gen) {
        if (n) {
            apt::hip_check(hipMemcpyAsync(verts, layers.xy.data(), 2 * n * sizeof(double), hipMemcpyHostToDevice, s),
                           "hipMemcpyAsync H2D (map vertices)");
            apt::hip_check(hipMemcpyAsync(meta, layers.meta.data(), 2 * n * sizeof(int32_t), hipMemcpyHostToDevice, s),
                           "hipMemcpyAsync H2D (map vertices)");
        }
        n_vert = n;
        gen = layers.gen;
    }
    if (rows_cap < rows || !cnt) {
        rows_cap = rows > rows_cap ? rows : rows_cap;
        dev_alloc(track, 2 * rows_cap, "hipMalloc (map track)");
        dev_alloc(xoff, rows_cap, "hipMalloc (map track)");
        dev_alloc(cnt, rows_cap * kPx, "hipMalloc (map pixel counts)");
        dev_alloc(base, rows_cap * kPx, "hipMalloc (map pixel runs)");
        apt::hip_check(hipMemsetAsync(cnt, 0, rows_cap * kPx * sizeof(uint32_t), s), "hipMemsetAsync");
        // the staging buffers are sized by rows_cap: drop them, upload_track makes new ones as it needs them
        for (int k = 0; k < kTrackRing; ++k) {
            if (track_ev[k]) apt::hip_check(hipEventSynchronize(track_ev[k]), "hipEventSynchronize");
            if (track_host[k]) (void)hipHostFree(track_host[k]);
            track_host[k] = nullptr;
        }
    }
}

void Device::upload_track(hipStream_t s, const double *positions, size_t count)
{
    const size_t rows = count < rows_cap ? count : rows_cap;
    if (!rows) return;
    const int k = track_next;
    track_next = (track_next + 1) % kTrackRing;
    // the upload from this buffer kTrackRing calls ago: normally long done, so no wait in steady state
    if (track_ev[k]) apt::hip_check(hipEventSynchronize(track_ev[k]), "hipEventSynchronize");
    else apt::hip_check(hipEventCreateWithFlags(&track_ev[k], hipEventDisableTiming), "hipEventCreate");
    if (!track_host[k])
        apt::hip_check(hipHostMalloc(reinterpret_cast<void **>(&track_host[k]), 2 * rows_cap * sizeof(double)),
                       "hipHostMalloc (map track)");
    std::memcpy(track_host[k], positions, 2 * rows * sizeof(double));
    apt::hip_check(hipMemcpyAsync(track, track_host[k], 2 * rows * sizeof(double), hipMemcpyHostToDevice, s),
                   "hipMemcpyAsync H2D (map track)");
    apt::hip_check(hipEventRecord(track_ev[k], s), "hipEventRecord");
}

namespace {

// the nine launches behind the projection, shared by both forms
void overlay_tail(hipStream_t s, Device &d, uint32_t n, const Colors &colors, bool rotate, uint8_t *img,
                  ImageResult *info);

}  // namespace

void image_map_overlay(hipStream_t s, Device &d, const Scalars &sc, const Colors &colors, uint32_t count,
                       bool rotate, uint8_t *img, ImageResult *info)
{
    const uint32_t n = static_cast<uint32_t>(d.n_vert);
    const uint32_t rows = static_cast<uint32_t>(d.rows_cap < count ? d.rows_cap : count);
    k_map_track<<<blocks(rows, kThreads), kThreads, 0, s>>>(d.track, count, rows, sc, d.xoff, info, d.ctl);
    k_map_project<<<blocks(n, kThreads), kThreads, 0, s>>>(d.verts, n, sc, d.proj);
    overlay_tail(s, d, n, colors, rotate, img, info);
}

void image_map_track(hipStream_t s, Device &d, const Scalars &sc, uint32_t count, ImageResult *info)
{
    const uint32_t rows = static_cast<uint32_t>(d.rows_cap < count ? d.rows_cap : count);
    k_map_track<<<blocks(rows, kThreads), kThreads, 0, s>>>(d.track, count, rows, sc, d.xoff, info, d.ctl);
}

void image_map_track_sat(hipStream_t s, Device &d, const apt::sat::TrackCall &call, double yaw, double hscale,
                         double vscale, ImageResult *info)
{
    const uint32_t rows = static_cast<uint32_t>(d.rows_cap < 0xffffffffu ? d.rows_cap : 0xffffffffu);
    apt::sat::track(s, call, info, 0, rows, d.track, d.ctl + 3);
    apt::sat::scalars(s, d.track, info, rows, yaw, hscale, vscale, d.scalars, d.ctl + 4);
    k_map_track_dev<<<blocks(rows, kThreads), kThreads, 0, s>>>(d.track, rows, d.scalars, d.xoff, info, d.ctl);
}

void image_map_overlay_sat(hipStream_t s, Device &d, const apt::sat::TrackCall &call, double yaw, double hscale,
                           double vscale, const Colors &colors, bool rotate, uint8_t *img, ImageResult *info)
{
    const uint32_t n = static_cast<uint32_t>(d.n_vert);
    const uint32_t rows = static_cast<uint32_t>(d.rows_cap < 0xffffffffu ? d.rows_cap : 0xffffffffu);
    apt::sat::track(s, call, info, 0, rows, d.track, d.ctl + 3);
    apt::sat::scalars(s, d.track, info, rows, yaw, hscale, vscale, d.scalars, d.ctl + 4);
    k_map_track_dev<<<blocks(rows, kThreads), kThreads, 0, s>>>(d.track, rows, d.scalars, d.xoff, info, d.ctl);
    k_map_project_dev<<<blocks(n, kThreads), kThreads, 0, s>>>(d.verts, n, d.scalars, d.proj);
    overlay_tail(s, d, n, colors, rotate, img, info);
}

namespace {

void overlay_tail(hipStream_t s, Device &d, uint32_t n, const Colors &colors, bool rotate, uint8_t *img,
                  ImageResult *info)
{
    k_map_count<<<blocks(n + 1, kThreads), kThreads, 0, s>>>(d.proj, d.meta, n, d.xoff, info, d.ctl, d.seg);
    const uint32_t nb = blocks(n + 1, kScanBlock);
    k_scan_local<<<nb, kThreads, 0, s>>>(d.seg, n + 1, d.sums);
    k_scan_sums<<<1, 1024, 0, s>>>(d.sums, nb, d.ctl);
    k_scan_add<<<nb, kThreads, 0, s>>>(d.seg, n + 1, d.sums);
    k_map_emit<<<blocks(n, kThreads), kThreads, 0, s>>>(d.proj, d.meta, n, d.xoff, info, d.ctl, d.seg, colors,
                                                         d.frags);
    k_map_link<<<kListBlocks, kThreads, 0, s>>>(d.frags, d.ctl, info, info, rotate, d.cnt, d.slot);
    k_map_alloc<<<kListBlocks, kThreads, 0, s>>>(d.frags, d.ctl, info, rotate, d.cnt, d.slot, d.base);
    k_map_scatter<<<kListBlocks, kThreads, 0, s>>>(d.frags, d.ctl, info, rotate, d.slot, d.base, d.runs);
    k_map_blend<<<kListBlocks, kThreads, 0, s>>>(d.frags, d.ctl, info, rotate, colors, d.cnt, d.slot, d.base, d.runs,
                                                 reinterpret_cast<uint32_t *>(img));
}

}  // namespace

}  // namespace apt::map
