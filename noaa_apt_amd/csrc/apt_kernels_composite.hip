// apt_kernels_composite.hip — the gfx950 kernel of the composite (apt_kernels_composite.hpp): several
// passes, each with its own track, geometry and image, combined onto one north-up grid.
//
// One launch per composite.  One thread per output pixel in k_project's tiles of 64 x 4 (a wave is 64 neighbours of
// one output row, so its RGBA stores are one contiguous 256 bytes and its coverage stores 64).  A tile evaluates
//   sin / cos / tan of its 4 row latitudes                      once (they depend on neither the column nor the pass)
//   sin(dl), cos(dl), cos(dl2) of its 64 columns, per pass      count x 64 x 3 doubles
//   sin / cos of every pass's start latitude                    count x 2 doubles
// into LDS before one barrier: dynamic shared memory sized by the call's pass count, 1552 B per pass (24.3 KB at 16).
// Each value is the library call k_project makes on the argument k_project makes it on (the functions of
// apt_kernels_project_dev.hpp), so a pass's x, y and dist carry k_project's bits.  Behind the barrier every thread
// walks the passes in list order -- the loop is wave-uniform, `count` and `blend` are kernel arguments -- through
// sample_pass, the very text of k_project's steps 2-4, and keeps what its blend needs: the first covering sample,
// the sample of the smallest |x| (strictly smaller replaces, so the lower index wins a tie), or the f64 sums of
// (456 - |x|) c per channel and of (456 - |x|).  FIRST leaves the loop once every live lane of the wave is covered
// and nobody asked for the coverage; NADIR and FEATHER never leave it early.
//
// f64, contraction off, as k_project.
#include "apt_kernels_composite.hpp"

#include "apt_kernels_map_dev.hpp"
#include "apt_kernels_project_dev.hpp"

#include <cstring>

#pragma clang fp contract(off)

namespace apt::composite {

namespace {

using apt::gpu::ImageResult;
using apt::map::kSkip;
using apt::map::Scalars;
using apt::project::col_terms;
using apt::project::Grid;
using apt::project::row_terms;
using apt::project::sample_pass;
using apt::project::kThreads;
using apt::project::kTileH;
using apt::project::kTileW;

constexpr size_t kPassDoubles = kTileW * 3 + 2;  // LDS per pass: the column terms, then sin / cos of the start latitude

__global__ void k_composite_begin(ImageResult *info, uint32_t width, uint32_t height)
{
    ImageResult z{};
    z.channel_a = z.channel_b = -1;
    z.height = height;
    z.n_px = static_cast<uint64_t>(width) * height;
    *info = z;
}

__global__ __launch_bounds__(kThreads) void k_composite(Grid g, const Pass *passes, uint32_t count, int blend,
                                                        ImageResult *info, const uint8_t *flags, uint32_t *out,
                                                        uint64_t out_cap, uint8_t *coverage)
{
    extern __shared__ double s_pass[];   // [count][kPassDoubles]
    __shared__ double s_row[kTileH][3];  // sin, cos, tan of the row's latitude
    __shared__ uint32_t s_why;
    const uint32_t tid = threadIdx.y * kTileW + threadIdx.x;
    if (tid == 0) {
        // every pass's finding as k_project reads it; any of them fails the composite, then the capacity
        const bool first = blockIdx.x == 0 && blockIdx.y == 0;
        uint32_t why = 0;
        for (uint32_t p = 0; p < count; ++p) {
            ImageResult *pi = passes[p].info;
            uint32_t e = passes[p].ctl[1];
            if (e == 0 && pi->status != 0) e = kSkip;
            if (first && e != 0 && e != kSkip && pi->status == 0) {
                pi->status = 1;
                pi->reason = static_cast<int32_t>(e);
            }
            if (e != 0) why = static_cast<uint32_t>(kReasonPass);
        }
        if (why == 0 && out_cap < static_cast<uint64_t>(g.width) * g.height * 4u)
            why = static_cast<uint32_t>(apt::project::kReasonCapacity);
        if (first && why != 0) {
            info->status = 1;
            info->reason = static_cast<int32_t>(why);
        }
        s_why = why;
    }
    __syncthreads();
    if (s_why != 0) return;  // (uniform per workgroup)
    if (tid < kTileH) row_terms(g, blockIdx.y * kTileH + tid, s_row[tid]);
    if (tid >= 64 && tid < 64 + count) {
        const Pass &ps = passes[tid - 64];
        const double start_lat = ps.scp ? ps.scp->start_lat : ps.sc.start_lat;
        double *st = s_pass + (tid - 64) * kPassDoubles + kTileW * 3;
        st[0] = sin(start_lat);
        st[1] = cos(start_lat);
    }
#pragma clang loop unroll(disable)
    for (uint32_t k = tid; k < count * kTileW; k += kThreads) {
        const uint32_t p = k / kTileW, c = k % kTileW;
        const Pass &ps = passes[p];
        const double start_lon = ps.scp ? ps.scp->start_lon : ps.sc.start_lon;
        col_terms(g, blockIdx.x * kTileW + c, start_lon, s_pass + p * kPassDoubles + c * 3);
    }
    __syncthreads();
    const uint32_t i = blockIdx.y * kTileH + threadIdx.y, j = blockIdx.x * kTileW + threadIdx.x;
    if (i >= g.height || j >= g.width) return;
    uint32_t px = 0, n = 0;
    double best = 0., wsum = 0., acc[4] = {0., 0., 0., 0.};
#pragma clang loop unroll(disable)
    for (uint32_t p = 0; p < count; ++p) {
        const Pass &ps = passes[p];
        const Scalars sc = ps.scp ? *ps.scp : ps.sc;
        const double *lds = s_pass + p * kPassDoubles;
        double x;
        uint32_t c;
        if (sample_pass(g, sc, lds + kTileW * 3, s_row[threadIdx.y], lds + threadIdx.x * 3, ps.xoff, ps.info->height,
                        ps.src, ps.channels, x, c)) {
            const double ax = fabs(x);
            if (blend == APTGPU_COMPOSITE_FEATHER) {
                const double w = 456. - ax;
                wsum = wsum + w;
                for (int k = 0; k < 4; ++k) acc[k] = acc[k] + w * static_cast<double>((c >> (8 * k)) & 255u);
            } else if (n == 0 || (blend == APTGPU_COMPOSITE_NADIR && ax < best)) {
                px = c;
                best = ax;
            }
            ++n;
        }
        if (blend == APTGPU_COMPOSITE_FIRST && !coverage && __all(n != 0)) break;
    }
    if (blend == APTGPU_COMPOSITE_FEATHER && n != 0) {
        for (int k = 0; k < 4; ++k) {
            const double r = floor(acc[k] / wsum + 0.5);
            px |= (r >= 255. ? 255u : (r > 0. ? static_cast<uint32_t>(r) : 0u)) << (8 * k);
        }
    }
    // a row and a column that cross are blended once
    if (g.graticule && (flags[j] | flags[g.width + i])) px = apt::map::blend(px, g.grid_color);
    const size_t at = static_cast<size_t>(i) * g.width + j;
    out[at] = px;
    if (coverage) coverage[at] = static_cast<uint8_t>(n);
}

}  // namespace

Device::~Device()
{
    if (table_ev) {
        (void)hipEventSynchronize(table_ev);
        (void)hipEventDestroy(table_ev);
    }
    for (hipEvent_t ev : pass_ev)
        if (ev) (void)hipEventDestroy(ev);
    if (table) (void)hipFree(table);
    if (table_host) (void)hipHostFree(table_host);
    if (info) (void)hipFree(info);
}

void Device::prepare()
{
    if (table) return;
    apt::hip_check(hipMalloc(reinterpret_cast<void **>(&table), kMaxPasses * sizeof(Pass)), "hipMalloc (pass table)");
    apt::hip_check(hipHostMalloc(reinterpret_cast<void **>(&table_host), kMaxPasses * sizeof(Pass)),
                   "hipHostMalloc (pass table)");
    apt::hip_check(hipMalloc(reinterpret_cast<void **>(&info), sizeof(ImageResult)), "hipMalloc (composite record)");
}

void Device::upload_table(hipStream_t s, const Pass *passes, int count)
{
    prepare();
    if (table_ev) apt::hip_check(hipEventSynchronize(table_ev), "hipEventSynchronize");
    else apt::hip_check(hipEventCreateWithFlags(&table_ev, hipEventDisableTiming), "hipEventCreate");
    std::memcpy(table_host, passes, static_cast<size_t>(count) * sizeof(Pass));
    apt::hip_check(hipMemcpyAsync(table, table_host, static_cast<size_t>(count) * sizeof(Pass), hipMemcpyHostToDevice, s),
                   "hipMemcpyAsync H2D (pass table)");
    apt::hip_check(hipEventRecord(table_ev, s), "hipEventRecord");
}

void wait_for_pass(hipStream_t s, Device &dev, int p, hipStream_t other)
{
    if (other == s) return;
    hipEvent_t &ev = dev.pass_ev[p];
    if (!ev) apt::hip_check(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate");
    apt::hip_check(hipEventRecord(ev, other), "hipEventRecord");
    apt::hip_check(hipStreamWaitEvent(s, ev, 0), "hipStreamWaitEvent");
}

void image_composite(hipStream_t s, Device &dev, int count, int blend, const Grid &g, uint8_t *out, uint64_t out_cap,
                     uint8_t *coverage)
{
    const dim3 grid((g.width + kTileW - 1) / kTileW, (g.height + kTileH - 1) / kTileH), block(kTileW, kTileH);
    const size_t lds = static_cast<size_t>(count) * kPassDoubles * sizeof(double);
    k_composite_begin<<<1, 1, 0, s>>>(dev.info, g.width, g.height);
    k_composite<<<grid, block, lds, s>>>(g, dev.table, static_cast<uint32_t>(count), blend, dev.info, dev.grid.flags,
                                         reinterpret_cast<uint32_t *>(out), out_cap, coverage);
}

}  // namespace apt::composite
