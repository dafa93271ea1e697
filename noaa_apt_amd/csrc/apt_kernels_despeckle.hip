// apt_kernels_despeckle.hip — k_despeckle<R>, the gfx950 kernel of the despeckle stage (definition:
// apt_kernels_despeckle.hpp).  One launch per recording, exact: integer min / max on totalOrder keys,
// one f32 subtraction and one comparison per sample.
//
// A workgroup of 256 threads filters a tile of 8 rows x 128 columns; a thread owns 4 horizontally consecutive pixels
// (one 16-byte load and store).  The tile plus R halo rows above and below and one halo quad left and right is staged
// in LDS as u32 keys, rows clamped to the image while loading.  A thread sorts each of its 4 + 2R columns vertically
// once (min3 / med3 / max3 for R = 1); neighbouring windows share them, and the band clamp only selects which sorted
// column a window reads (compile-time register indices, v_cndmask).  R = 1 then takes
// med3(max3(lows), med3(mids), min3(highs)); R = 2 runs a forgetful selection over the 25 keys.
#include "apt_kernels_despeckle.hpp"

#include <cmath>

#pragma clang fp contract(off)

namespace apt::gpu {

namespace {

using namespace apt::despeckle;

constexpr int kThreads = 256;
constexpr int kTileRows = 8;
constexpr int kTileQuads = 32;                                      // 128 columns
constexpr int kRowQuads = kPx / 4;                                  // 520
constexpr int kColTiles = (kRowQuads + kTileQuads - 1) / kTileQuads;  // 17
constexpr int kLdsQuads = kTileQuads + 2;                           // one halo quad on each side
// Row stride in dwords: >= 4 * kLdsQuads, a multiple of 4 (ds_read_b128 / ds_write_b128) and = 32 mod 64, so that the
// two tile rows a wave reads at once (lanes 0-31 and 32-63) start half a bank row apart.
constexpr int kLdsStride = 160;
static_assert(kLdsStride >= 4 * kLdsQuads && kLdsStride % 64 == 32, "LDS row stride");
static_assert(kTileRows * kTileQuads == kThreads, "one thread per quad of the tile");

// samples this launch works on; 0 when the decode failed
__device__ inline uint64_t px_count(const Result *res, uint64_t n_host, uint64_t cap)
{
    uint64_t n = n_host;
    if (res) n = res->status == 0 ? res->n_out : 0;
    return n < cap ? n : cap;
}

__device__ inline uint32_t key_of(float v) { return key_of_bits(__float_as_uint(v)); }

// One sorted column per image column x0 - R + j, j < 4 + 2R, of the thread's row.
template <int R>
struct Columns {
    uint32_t c[4 + 2 * R][2 * R + 1];
};

__device__ inline void sort_column(uint32_t (&v)[3])
{
    const uint32_t a = v[0], b = v[1], c = v[2];
    v[0] = umin3(a, b, c);
    v[1] = umed3(a, b, c);
    v[2] = umax3(a, b, c);
}

__device__ inline void sort_column(uint32_t (&v)[5])
{
    // 9 compare-exchanges, the optimal network for 5 keys
    detail::cx(v[0], v[1]);
    detail::cx(v[3], v[4]);
    detail::cx(v[2], v[4]);
    detail::cx(v[2], v[3]);
    detail::cx(v[0], v[3]);
    detail::cx(v[0], v[2]);
    detail::cx(v[1], v[4]);
    detail::cx(v[1], v[3]);
    detail::cx(v[1], v[2]);
}

// The sorted column the window of pixel P reads at offset DX: column clamp(x + DX, b0, b1 - 1), which lies between
// x + DX and x, so the choice is among |DX| + 1 registers known at compile time.  lo = b0 - (x0 - R) and
// hi = b1 - 1 - (x0 - R) are the band's ends as column indices.
template <int R, int P, int DX>
__device__ inline void pick(const Columns<R> &cols, int lo, int hi, uint32_t (&w)[2 * R + 1])
{
    constexpr int K = 2 * R + 1;
    constexpr int centre = P + R;
    int j = centre + DX;
    j = j < lo ? lo : j;
    j = j > hi ? hi : j;
#pragma unroll
    for (int k = 0; k < K; ++k) w[k] = cols.c[centre][k];
    if constexpr (DX != 0) {
        constexpr int step = DX < 0 ? -1 : 1;
#pragma unroll
        for (int d = 1; d <= (DX < 0 ? -DX : DX); ++d) {
            const bool take = j == centre + step * d;
#pragma unroll
            for (int k = 0; k < K; ++k) w[k] = take ? cols.c[centre + step * d][k] : w[k];
        }
    }
}

template <int P>
__device__ inline uint32_t window_median(const Columns<1> &cols, int lo, int hi)
{
    uint32_t a[3], b[3], c[3];
    pick<1, P, -1>(cols, lo, hi, a);
    pick<1, P, 0>(cols, lo, hi, b);
    pick<1, P, 1>(cols, lo, hi, c);
    return median9_sorted_columns(a, b, c);
}

template <int P>
__device__ inline uint32_t window_median(const Columns<2> &cols, int lo, int hi)
{
    uint32_t v[25], w[5];
    // (the order in which the keys enter the selection is free: the centre column and its neighbours first)
    pick<2, P, 0>(cols, lo, hi, w);
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = w[k];
    pick<2, P, -1>(cols, lo, hi, w);
#pragma unroll
    for (int k = 0; k < 5; ++k) v[5 + k] = w[k];
    pick<2, P, 1>(cols, lo, hi, w);
#pragma unroll
    for (int k = 0; k < 5; ++k) v[10 + k] = w[k];
    pick<2, P, -2>(cols, lo, hi, w);
#pragma unroll
    for (int k = 0; k < 5; ++k) v[15 + k] = w[k];
    pick<2, P, 2>(cols, lo, hi, w);
#pragma unroll
    for (int k = 0; k < 5; ++k) v[20 + k] = w[k];
    return median25(v);
}

// the rule for one sample; counts a replacement
__device__ inline float decide(float x, uint32_t med_key, float t, bool filter, uint32_t &replaced)
{
    const float med = __uint_as_float(bits_of_key(med_key));
    const bool take = filter && med == med && !(fabsf(x - med) <= t);
    replaced += take ? 1u : 0u;
    return take ? med : x;
}

template <int R, int P>
__device__ inline float filter_pixel(const Columns<R> &cols, int x0, float x, float t, bool filter, uint32_t &replaced)
{
    int b0, b1;
    band_of(x0 + P, &b0, &b1);
    return decide(x, window_median<P>(cols, b0 - (x0 - R), b1 - 1 - (x0 - R)), t, filter, replaced);
}

template <int R>
__global__ __launch_bounds__(kThreads) void k_despeckle(const float *__restrict__ x, const Result *res, uint64_t n_host,
                                                        uint64_t cap, float threshold, const float *limits,
                                                        const ImageResult *lim_info, float *__restrict__ out,
                                                        DespeckleResult *rec)
{
    constexpr int K = 2 * R + 1;
    constexpr int kLdsRows = kTileRows + 2 * R;
    __shared__ __attribute__((aligned(16))) uint32_t s_key[kLdsRows * kLdsStride];
    __shared__ uint32_t s_count[kThreads / 64];

    const uint64_t n = px_count(res, n_host, cap);
    const uint64_t h = n / kPx;
    const bool decode_failed = res && res->status != 0;
    // the limits of the unfiltered signal (only looked at when there is something to filter with a threshold)
    const bool want_limits = threshold != 0.f && h > 0;
    const bool limits_failed = want_limits && lim_info->status != 0;
    const float low = want_limits && !limits_failed ? limits[0] : 0.f;
    const float high = want_limits && !limits_failed ? limits[1] : 0.f;
    const float t = want_limits && !limits_failed ? threshold * (high - low) : 0.f;
    const bool filter = !limits_failed;

    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) {  // (the record was zeroed in front of the launch; `replaced` is only ever added to)
            rec->status = (decode_failed || limits_failed) ? 1 : 0;
            rec->reason = decode_failed ? 4 : (limits_failed ? lim_info->reason : 0);
            rec->height = static_cast<uint32_t>(h);
            rec->low = low;
            rec->high = high;
            rec->t = t;
        }
        // the samples past the last whole row: copied bit for bit (fewer than 2080)
        const uint32_t *xb = reinterpret_cast<const uint32_t *>(x);
        uint32_t *ob = reinterpret_cast<uint32_t *>(out);
        for (uint64_t i = h * kPx + threadIdx.x; i < n; i += kThreads) ob[i] = xb[i];
    }

    const uint64_t row_tile = blockIdx.x / kColTiles;
    const int col_tile = static_cast<int>(blockIdx.x % kColTiles);
    const uint64_t y0 = row_tile * kTileRows;
    if (y0 >= h) return;  // (the whole workgroup: the launch is sized for the buffer's capacity)
    const int q0 = col_tile * kTileQuads;  // first quad of the tile
    const bool vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0;

    // ---- stage rows y0 - R .. y0 + 7 + R (clamped to the image), quads q0 - 1 .. q0 + 32, as keys
    for (int e = threadIdx.x; e < kLdsRows * kLdsQuads; e += kThreads) {
        const int r = e / kLdsQuads, c = e % kLdsQuads;
        const int q = q0 - 1 + c;
        int64_t gy = static_cast<int64_t>(y0) - R + r;
        gy = gy < 0 ? 0 : gy;
        gy = gy > static_cast<int64_t>(h) - 1 ? static_cast<int64_t>(h) - 1 : gy;
        uint4 k4 = make_uint4(0u, 0u, 0u, 0u);  // (quads outside the row are never selected: a band ends at the row's)
        if (q >= 0 && q < kRowQuads) {
            const float *src = x + static_cast<uint64_t>(gy) * kPx + 4 * q;
            float4 v;
            if (vec) {
                v = *reinterpret_cast<const float4 *>(src);
            } else {
                v = make_float4(src[0], src[1], src[2], src[3]);
            }
            k4 = make_uint4(key_of(v.x), key_of(v.y), key_of(v.z), key_of(v.w));
        }
        *reinterpret_cast<uint4 *>(&s_key[r * kLdsStride + 4 * c]) = k4;
    }
    __syncthreads();

    const int tx = threadIdx.x % kTileQuads, ty = threadIdx.x / kTileQuads;
    const int q = q0 + tx;
    const uint64_t y = y0 + ty;
    uint32_t replaced = 0;
    if (q < kRowQuads && y < h) {
        // ---- this thread's 4 + 2R columns, image columns x0 - R .. x0 + 3 + R, each sorted vertically
        const int x0 = 4 * q;
        Columns<R> cols;
        uint32_t centre[4];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t *row = &s_key[(ty + k) * kLdsStride + 4 * tx + 4];  // column x0 of LDS row ty + k
            const uint4 m = *reinterpret_cast<const uint4 *>(row);
            cols.c[R + 0][k] = m.x;
            cols.c[R + 1][k] = m.y;
            cols.c[R + 2][k] = m.z;
            cols.c[R + 3][k] = m.w;
            if constexpr (R == 1) {
                cols.c[0][k] = row[-1];
                cols.c[5][k] = row[4];
            } else {
                const uint2 l = *reinterpret_cast<const uint2 *>(row - 2);
                const uint2 g = *reinterpret_cast<const uint2 *>(row + 4);
                cols.c[0][k] = l.x;
                cols.c[1][k] = l.y;
                cols.c[6][k] = g.x;
                cols.c[7][k] = g.y;
            }
            if (k == R) {
                centre[0] = m.x;
                centre[1] = m.y;
                centre[2] = m.z;
                centre[3] = m.w;
            }
        }
#pragma unroll
        for (int j = 0; j < 4 + 2 * R; ++j) sort_column(cols.c[j]);

        float4 o;
        o.x = filter_pixel<R, 0>(cols, x0, __uint_as_float(bits_of_key(centre[0])), t, filter, replaced);
        o.y = filter_pixel<R, 1>(cols, x0, __uint_as_float(bits_of_key(centre[1])), t, filter, replaced);
        o.z = filter_pixel<R, 2>(cols, x0, __uint_as_float(bits_of_key(centre[2])), t, filter, replaced);
        o.w = filter_pixel<R, 3>(cols, x0, __uint_as_float(bits_of_key(centre[3])), t, filter, replaced);
        float *dst = out + y * kPx + x0;
        if (vec) {
            *reinterpret_cast<float4 *>(dst) = o;
        } else {
            dst[0] = o.x;
            dst[1] = o.y;
            dst[2] = o.z;
            dst[3] = o.w;
        }
    }

    // ---- one integer atomic per workgroup
    for (int d = 32; d >= 1; d >>= 1) replaced += __shfl_down(replaced, d);
    if ((threadIdx.x & 63) == 0) s_count[threadIdx.x >> 6] = replaced;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        for (int w = 0; w < kThreads / 64; ++w) total += s_count[w];
        if (total) atomicAdd(reinterpret_cast<unsigned long long *>(&rec->replaced), static_cast<unsigned long long>(total));
    }
}

}  // namespace

size_t despeckle_ws_bytes() { return 64 + sizeof(ImageResult); }
DespeckleResult *despeckle_ws_record(void *ws) { return static_cast<DespeckleResult *>(ws); }
ImageResult *despeckle_ws_limits_info(void *ws)
{
    static_assert(sizeof(DespeckleResult) <= 64, "record slot");
    return reinterpret_cast<ImageResult *>(static_cast<char *>(ws) + 64);
}

void despeckle(hipStream_t s, const float *x, const Result *res, uint64_t n, uint64_t cap, int radius, float threshold,
               const float *limits, const ImageResult *lim_info, float *out, DespeckleResult *rec)
{
    (void)hipMemsetAsync(rec, 0, sizeof(DespeckleResult), s);
    const uint64_t row_tiles = (cap / kPx + kTileRows - 1) / kTileRows;
    const uint64_t blocks = row_tiles * kColTiles;
    const dim3 grid(static_cast<unsigned>(blocks < 1 ? 1 : blocks));  // (block 0 also writes the record and the tail)
    if (radius == 1)
        hipLaunchKernelGGL(k_despeckle<1>, grid, dim3(kThreads), 0, s, x, res, n, cap, threshold, limits, lim_info, out, rec);
    else
        hipLaunchKernelGGL(k_despeckle<2>, grid, dim3(kThreads), 0, s, x, res, n, cap, threshold, limits, lim_info, out, rec);
}

}  // namespace apt::gpu
