// apt_kernels_project.hip — gfx950 kernels of the reprojection (apt_kernels_project.hpp): the step the
// reference's to-do list names after the overlay (docs/development.md:112 "Draw image over mercator (or at least
// equirectangular) projection", :99 "Add latitude longitude grid").
//
// One launch per image.  One thread per output pixel in tiles of 64 x 4 (a wave is 64 neighbours of one output row, so
// its RGBA stores are one contiguous 256 bytes).  Per pixel:
//   (lat, lon) of the grid    -> latlon_to_rel_px, map.rs:71-100 (apt_kernels_map_dev.hpp: the overlay's source text)
//   x -= xoff[est_row(y, h)]     the offset correction of map.rs:105-111, with the step at integer y it has
//   band -456 < x < 456, 0 < y < h (map.rs:116-121), and geo::distance(latlon, start) < PI / 3 unclamped: beyond it
//   latlon_to_rel_px's clamp would alias every point onto one image row
//   nearest or bilinear sample of channel A (x + 539) or B (x + 1579) of the unrotated image, then the graticule
// lat and its sin / cos / tan depend on the output row alone and sin / cos of the longitude differences on the column
// alone: a tile evaluates them once per row and once per column into LDS (the same library calls on the same
// arguments as a per-pixel evaluation, so the same bits), which leaves atan2, acos, tan, atan, asin and two sin / cos
// per pixel.  The source reads are gathers from an image of at most a few MB that the L2 holds; it is not staged.
//
// f64 math is the reference's, operation for operation (contract off); the transcendentals are the device library's,
// which may differ from glibc by an ulp (the parity contract of DESIGN.md §15, §12's).
#include "apt_kernels_project.hpp"

#include "apt_kernels_map_dev.hpp"
#include "apt_kernels_project_dev.hpp"
#include "apt_kernels_png.hpp"

#include <cstring>

#pragma clang fp contract(off)

namespace apt::project {

namespace {

using apt::gpu::ImageResult;
using apt::map::kPi;
using apt::map::kSkip;
using apt::map::Scalars;

__global__ __launch_bounds__(kThreads) void k_project(Grid g, Scalars sc_host, const Scalars *scp, const double *xoff,
                                                      const uint32_t *ctl, ImageResult *info, const uint8_t *src,
                                                      int src_channels, const uint8_t *flags, uint32_t *out,
                                                      uint64_t out_cap)
{
    __shared__ double s_row[kTileH][3];  // sin, cos, tan of the row's latitude
    __shared__ double s_col[kTileW][3];  // sin(dl), cos(dl), cos(dl2) of the column's longitude
    __shared__ double s_start[2];        // sin, cos of the start latitude
    __shared__ uint32_t s_why;
    const uint32_t tid = threadIdx.y * kTileW + threadIdx.x;
    if (tid == 0) {
        // the overlay's or the track launch's finding, a record that already carries a status, or the capacity
        const uint32_t e = ctl[1];
        uint32_t why = e;
        if (why == 0 && info->status != 0) why = kSkip;
        if (why == 0 && out_cap < static_cast<uint64_t>(g.width) * g.height * 4u) why = static_cast<uint32_t>(kReasonCapacity);
        if (blockIdx.x == 0 && blockIdx.y == 0 && why != 0 && why != kSkip && info->status == 0) {
            info->status = 1;
            info->reason = static_cast<int32_t>(why);
        }
        s_why = why;
    }
    __syncthreads();
    if (s_why != 0) return;  // (uniform per workgroup)
    const Scalars sc = scp ? *scp : sc_host;
    if (tid < kTileH) {
        row_terms(g, blockIdx.y * kTileH + tid, s_row[tid]);
    } else if (tid >= 64 && tid < 64 + kTileW) {
        col_terms(g, blockIdx.x * kTileW + (tid - 64), sc.start_lon, s_col[tid - 64]);
    } else if (tid == 128) {
        s_start[0] = sin(sc.start_lat);
        s_start[1] = cos(sc.start_lat);
    }
    __syncthreads();
    const uint32_t i = blockIdx.y * kTileH + threadIdx.y, j = blockIdx.x * kTileW + threadIdx.x;
    if (i >= g.height || j >= g.width) return;
    double x;
    uint32_t px = 0;  // (stays 0 where the swath does not cover the pixel)
    sample_pass(g, sc, s_start, s_row[threadIdx.y], s_col[threadIdx.x], xoff, info->height, src, src_channels, x, px);
    // a row and a column that cross are blended once
    if (g.graticule && (flags[j] | flags[g.width + i])) px = apt::map::blend(px, g.grid_color);
    out[static_cast<size_t>(i) * g.width + j] = px;
}

// the record the encoder reads: the grid's height under the call's status
__global__ void k_project_png_begin(const ImageResult *info, ImageResult *grid_info, uint32_t height)
{
    grid_info->status = info->status;
    grid_info->reason = info->reason;
    grid_info->height = height;
    grid_info->reserved = 0;
}

__global__ void k_project_png_end(const ImageResult *grid_info, ImageResult *info)
{
    info->reserved = grid_info->reserved;
    if (info->status == 0 && grid_info->status != 0) {
        info->status = grid_info->status;
        info->reason = grid_info->reason;
    }
}

}  // namespace

Device::~Device()
{
    if (flags_ev) {
        (void)hipEventSynchronize(flags_ev);
        (void)hipEventDestroy(flags_ev);
    }
    if (flags) (void)hipFree(flags);
    if (flags_host) (void)hipHostFree(flags_host);
    if (grid_info) (void)hipFree(grid_info);
    if (png_ws) (void)hipFree(png_ws);
}

void Device::upload_flags(hipStream_t s, const std::vector<uint8_t> &f)
{
    if (f.empty()) return;
    if (flags_ev) apt::hip_check(hipEventSynchronize(flags_ev), "hipEventSynchronize");
    else apt::hip_check(hipEventCreateWithFlags(&flags_ev, hipEventDisableTiming), "hipEventCreate");
    if (flags_cap < f.size()) {
        if (flags) (void)hipFree(flags);
        if (flags_host) (void)hipHostFree(flags_host);
        flags = flags_host = nullptr;
        flags_cap = f.size();
        apt::hip_check(hipMalloc(reinterpret_cast<void **>(&flags), flags_cap), "hipMalloc (graticule)");
        apt::hip_check(hipHostMalloc(reinterpret_cast<void **>(&flags_host), flags_cap), "hipHostMalloc (graticule)");
    }
    std::memcpy(flags_host, f.data(), f.size());
    apt::hip_check(hipMemcpyAsync(flags, flags_host, f.size(), hipMemcpyHostToDevice, s), "hipMemcpyAsync H2D (graticule)");
    apt::hip_check(hipEventRecord(flags_ev, s), "hipEventRecord");
}

void image_project(hipStream_t s, Device &dev, const apt::map::Device &map, const Scalars *sc, const Grid &g,
                   const uint8_t *src, int src_channels, uint8_t *out, uint64_t out_cap, ImageResult *info)
{
    const dim3 grid((g.width + kTileW - 1) / kTileW, (g.height + kTileH - 1) / kTileH), block(kTileW, kTileH);
    k_project<<<grid, block, 0, s>>>(g, sc ? *sc : Scalars{}, sc ? nullptr : map.scalars, map.xoff, map.ctl, info, src,
                                     src_channels, dev.flags, reinterpret_cast<uint32_t *>(out), out_cap);
}

void image_project_png(hipStream_t s, Device &dev, const Grid &g, const uint8_t *grid_rgba, uint8_t *d_png,
                       uint64_t png_cap, ImageResult *info)
{
    const uint64_t stream = apt::png::stream_bytes(g.width, g.height, 4);
    if (!dev.grid_info)
        apt::hip_check(hipMalloc(reinterpret_cast<void **>(&dev.grid_info), sizeof(ImageResult)), "hipMalloc (projection record)");
    if (dev.png_stream_cap < stream) {
        if (dev.png_ws) (void)hipFree(dev.png_ws);
        dev.png_ws = nullptr;
        apt::hip_check(hipMalloc(reinterpret_cast<void **>(&dev.png_ws), apt::png::ws_bytes(stream)), "hipMalloc (PNG scratch)");
        dev.png_stream_cap = stream;
    }
    k_project_png_begin<<<1, 1, 0, s>>>(info, dev.grid_info, g.height);
    apt::png::encode(s, grid_rgba, g.width, g.height, 4, dev.png_ws, dev.png_stream_cap, d_png, png_cap, dev.grid_info,
                     nullptr);
    k_project_png_end<<<1, 1, 0, s>>>(dev.grid_info, info);
}

}  // namespace apt::project
