// apt_kernels_color.hip — gfx950 kernels for the colour layer of process() (apt_kernels_color.hpp):
// histogram equalisation of the two channel halves and palette false colour over channel A.
//
// Bit-exact with the reference: the histograms are integer counts (exact in any order), the scans
// are integer prefix sums, and every f32 operation of the reference is one f32 operation here,
// rounded on its own (contract off; the Makefile's -fhip-fp32-correctly-rounded-divide-sqrt makes
// the table's division correctly rounded).
//
// The stage reads the f32 rows twice (histogram pass, output pass) and maps them to u8 in both,
// with the arithmetic of k_map_u8: a u8 staging image would move 4 + 1 + 1 bytes per pixel through
// HBM against 4 + 4 here, but costs a third launch over the whole image and a buffer per slot, and
// at 10 MB of rows per recording the stage is bound by launches, not bytes.
#include "apt_kernels_color.hpp"

#include <cmath>
#include <cstring>

#pragma clang fp contract(off)

namespace apt::gpu {

namespace {

constexpr int kPx = 2080;         // PX_PER_ROW, decode.rs:14
constexpr int kHalf = 1040;       // PX_PER_CHANNEL: histogram_equalization's two sub-images
constexpr int kColorStart = 86;   // PX_SYNC_FRAME + PX_SPACE_DATA (processing.rs:123)
constexpr int kColorEnd = 995;    // + PX_CHANNEL_IMAGE_DATA (909)
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kBins = 2 * 256;    // channel A bins, then channel B bins
constexpr int kHistBlocks = 256;  // at most one workgroup per CU: every one ends with <= 512 global atomics

// workspace layout (color_ws_bytes)
constexpr size_t kHistOff = 0;
constexpr size_t kLutOff = kHistOff + kBins * sizeof(uint32_t);
constexpr size_t kPaletteOff = kLutOff + kBins;
constexpr size_t kWsBytes = kPaletteOff + 65536 * sizeof(uint32_t);

// as apt_kernels_image.hip
__device__ inline uint64_t px_count(const Result *res, uint64_t n_host, uint64_t cap)
{
    uint64_t n = n_host;
    if (res) n = res->status == 0 ? res->n_out : 0;
    return n < cap ? n : cap;
}

// map_signal_u8 (noaa_apt.rs:249-259), the arithmetic of k_map_u8
__device__ inline uint32_t map_px(float v, float low, float range)
{
    float t = (v - low) / range * 255.f;
    t = fmaxf(t, 0.f);  // NaN -> 0
    t = fminf(t, 255.f);
    return static_cast<uint32_t>(roundf(t));
}

// processing::rotate (processing.rs:21-37), as k_map_u8: source pixel of output (r, c)
__device__ inline uint64_t rotate_src(uint64_t r, uint32_t c, uint64_t rows)
{
    constexpr uint32_t kOff = 39 + 47, kW = 909, kCh = 1040;
    uint32_t base = ~0u;
    if (c >= kOff && c < kOff + kW) base = kOff;
    else if (c >= kOff + kCh && c < kOff + kCh + kW) base = kOff + kCh;
    if (base == ~0u) return r * kPx + c;
    return (rows - 1 - r) * kPx + base + (kW - 1 - (c - base));
}

// tune_input_values (processing.rs:126-140): `(in * k - o).clamp(0., 255.) as u32`; clamp keeps a
// NaN and `as u32` makes it 0
__device__ inline uint32_t tune(uint32_t in, float k, float o)
{
    const float t = static_cast<float>(in) * k - o;
    if (t != t) return 0u;
    const float c = t < 0.f ? 0.f : (t > 255.f ? 255.f : t);
    return static_cast<uint32_t>(c);
}

__device__ inline bool aligned16(const void *p)
{
    return (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

// Histograms of both halves of the u8 image.  Per-wave sub-histograms in LDS: APT rows have long
// runs of one value (sync, space, telemetry, saturated cloud), and lanes adding to one LDS word
// serialise; four copies cut that by the number of waves.  Then one global add per non-zero bin.
__global__ __launch_bounds__(kThreads) void k_eq_histogram(const float *__restrict__ x, const Result *res,
                                                           uint64_t n_host, uint64_t cap, const float *limits,
                                                           uint32_t *hist)
{
    __shared__ uint32_t s_h[kWaves][kBins];
    for (int k = threadIdx.x; k < kWaves * kBins; k += kThreads) (&s_h[0][0])[k] = 0u;
    __syncthreads();
    const uint64_t rows = px_count(res, n_host, cap) / kPx;
    const uint64_t quads = rows * (kPx / 4);  // whole rows: the reference's Image has n / 2080 rows (noaa_apt.rs:182)
    const float low = limits[0];
    const float range = limits[1] - limits[0];
    uint32_t *h = s_h[threadIdx.x >> 6];
    const uint64_t gtid = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    const bool vec = aligned16(x);
    for (uint64_t q = gtid; q < quads; q += stride) {
        // 2080 and 1040 are multiples of 4: a quad lies in one half of one row
        const uint32_t half = static_cast<uint32_t>(q % (kPx / 4)) < kHalf / 4 ? 0u : 256u;
        float v0, v1, v2, v3;
        if (vec) {
            const float4 v = reinterpret_cast<const float4 *>(x)[q];
            v0 = v.x, v1 = v.y, v2 = v.z, v3 = v.w;
        } else {
            v0 = x[4 * q], v1 = x[4 * q + 1], v2 = x[4 * q + 2], v3 = x[4 * q + 3];
        }
        atomicAdd(&h[half + map_px(v0, low, range)], 1u);
        atomicAdd(&h[half + map_px(v1, low, range)], 1u);
        atomicAdd(&h[half + map_px(v2, low, range)], 1u);
        atomicAdd(&h[half + map_px(v3, low, range)], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < kBins; b += kThreads) {
        uint32_t c = 0;
        for (int w = 0; w < kWaves; w++) c += s_h[w][b];
        if (c) atomicAdd(&hist[b], c);
    }
}

// equalize_histogram_grayscale (imageext.rs:21-45): cum = inclusive scan, total = cum[255] as f32,
// v -> (255. * (cum[v] as f32 / total)) as u8.  One workgroup; thread t owns bin t of both halves.
// Leaves the histogram zeroed for the next call on this workspace.
__global__ __launch_bounds__(kThreads) void k_eq_lut(uint32_t *hist, uint8_t *lut)
{
    __shared__ uint32_t s_wave[2][kWaves];
    __shared__ uint32_t s_total[2];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint32_t a = hist[t], b = hist[256 + t];
    hist[t] = 0u;
    hist[256 + t] = 0u;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t oa = __shfl_up(a, d), ob = __shfl_up(b, d);
        if (lane >= d) {
            a += oa;
            b += ob;
        }
    }
    if (lane == 63) {
        s_wave[0][wave] = a;
        s_wave[1][wave] = b;
    }
    __syncthreads();
    for (int w = 0; w < wave; w++) {
        a += s_wave[0][w];
        b += s_wave[1][w];
    }
    if (t == 255) {
        s_total[0] = a;
        s_total[1] = b;
    }
    __syncthreads();
    const uint32_t cum[2] = {a, b};
    for (int ch = 0; ch < 2; ch++) {
        const float total = static_cast<float>(s_total[ch]);
        uint32_t v = 0;
        if (s_total[ch] != 0u) {  // (an empty image has no pixel to look the table up)
            const float fraction = static_cast<float>(cum[ch]) / total;
            v = static_cast<uint32_t>(255.f * fraction);  // in [0, 255]: cum <= total survives the rounding
        }
        lut[ch * 256 + t] = static_cast<uint8_t>(v);
    }
}

// The output pass, 4 output pixels per thread (a quad never straddles a row or a half).
template <int kCh>
__global__ __launch_bounds__(kThreads) void k_color(const float *__restrict__ x, const Result *res, uint64_t n_host,
                                                    uint64_t cap, const float *limits, const uint8_t *lut,
                                                    const uint32_t *__restrict__ palette, ColorTune tn,
                                                    int rotate, uint8_t *__restrict__ out, ImageResult *info)
{
    __shared__ uint8_t s_lut[kBins];
    if (lut) {
        for (int k = threadIdx.x; k < kBins / 4; k += kThreads)
            reinterpret_cast<uint32_t *>(s_lut)[k] = reinterpret_cast<const uint32_t *>(lut)[k];
        __syncthreads();
    }
    const uint64_t n = px_count(res, n_host, cap);
    const uint64_t rows = n / kPx;
    const uint64_t npx = rows * kPx;
    const float low = limits[0];
    const float range = limits[1] - limits[0];
    const uint64_t q = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (q == 0) {
        info->low = limits[0];
        info->high = limits[1];
        info->height = static_cast<uint32_t>(rows);
        info->n_px = info->status == 0 ? npx : 0;
    }
    if (info->status != 0) return;
    const uint64_t i0 = q * 4;
    if (i0 >= npx) return;
    const uint64_t r = i0 / kPx;
    const uint32_t c0 = static_cast<uint32_t>(i0 - r * kPx);
    const bool colored = palette && c0 + 3 >= kColorStart && c0 < kColorEnd;
    float v[4], w[4] = {0.f, 0.f, 0.f, 0.f};  // the pixel, and its channel-B partner 1040 columns on
    if (!rotate && aligned16(x)) {
        const float4 a = *reinterpret_cast<const float4 *>(x + i0);
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
        if (colored) {
            const float4 b = *reinterpret_cast<const float4 *>(x + i0 + kHalf);
            w[0] = b.x, w[1] = b.y, w[2] = b.z, w[3] = b.w;
        }
    } else {
        for (int k = 0; k < 4; k++) {
            const uint64_t src = rotate ? rotate_src(r, c0 + k, rows) : i0 + k;
            v[k] = x[src];
            if (colored) {
                const uint32_t c = c0 + k;
                if (c >= kColorStart && c < kColorEnd) w[k] = x[src + kHalf];
            }
        }
    }
    const uint32_t half = c0 < kHalf ? 0u : 256u;
    uint32_t px[4];
    for (int k = 0; k < 4; k++) {
        const uint32_t c = c0 + k;
        uint32_t g = map_px(v[k], low, range);
        if (colored && c >= kColorStart && c < kColorEnd) {
            // palette_img.get_pixel(val_a, val_b) (processing.rs:153-158)
            const uint32_t ta = tune(g, tn.k_a, tn.o_a);
            const uint32_t tb = tune(map_px(w[k], low, range), tn.k_b, tn.o_b);
            px[k] = palette[tb * 256u + ta];
            continue;
        }
        if (lut) g = s_lut[half + g];
        px[k] = kCh == 4 ? (g * 0x010101u) | 0xff000000u : g;
    }
    if (kCh == 4) {
        *reinterpret_cast<uint4 *>(out + i0 * 4) = make_uint4(px[0], px[1], px[2], px[3]);
    } else {
        *reinterpret_cast<uint32_t *>(out + i0) = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
    }
}

inline unsigned blocks_for(uint64_t n, unsigned per_block, unsigned max_blocks)
{
    uint64_t b = (n + per_block - 1) / per_block;
    if (b < 1) b = 1;
    return static_cast<unsigned>(b < max_blocks ? b : max_blocks);
}

}  // namespace

size_t color_ws_bytes()
{
    return kWsBytes;
}

hipError_t color_ws_init(hipStream_t s, void *color_ws)
{
    return hipMemsetAsync(static_cast<char *>(color_ws) + kHistOff, 0, kBins * sizeof(uint32_t), s);
}

uint32_t *color_ws_palette(void *color_ws)
{
    return reinterpret_cast<uint32_t *>(static_cast<char *>(color_ws) + kPaletteOff);
}

void color_pack_palette(const uint8_t *rgb, uint32_t *packed)
{
    for (int i = 0; i < 65536; i++)
        packed[i] = static_cast<uint32_t>(rgb[3 * i]) | (static_cast<uint32_t>(rgb[3 * i + 1]) << 8) |
                    (static_cast<uint32_t>(rgb[3 * i + 2]) << 16) | 0xff000000u;
}

void image_equalize(hipStream_t s, const float *x, const Result *res, uint64_t n, uint64_t cap, void *image_ws,
                    void *color_ws)
{
    const float *limits = image_ws_pointers(image_ws, cap).limits;
    char *ws = static_cast<char *>(color_ws);
    uint32_t *hist = reinterpret_cast<uint32_t *>(ws + kHistOff);
    const unsigned nb = blocks_for(cap / 4, kThreads * 16, kHistBlocks);
    hipLaunchKernelGGL(k_eq_histogram, dim3(nb), dim3(kThreads), 0, s, x, res, n, cap, limits, hist);
    hipLaunchKernelGGL(k_eq_lut, dim3(1), dim3(kThreads), 0, s, hist, reinterpret_cast<uint8_t *>(ws + kLutOff));
}

void image_color(hipStream_t s, const float *x, const Result *res, uint64_t n, uint64_t cap, void *image_ws,
                 const void *color_ws, bool equalize, const ColorTune *tune_p, int channels, bool rotate,
                 uint8_t *out, ImageResult *info)
{
    const float *limits = image_ws_pointers(image_ws, cap).limits;
    const char *ws = static_cast<const char *>(color_ws);
    const uint8_t *lut = equalize ? reinterpret_cast<const uint8_t *>(ws + kLutOff) : nullptr;
    const uint32_t *palette = tune_p ? reinterpret_cast<const uint32_t *>(ws + kPaletteOff) : nullptr;
    const ColorTune tn = tune_p ? *tune_p : ColorTune{0.f, 0.f, 0.f, 0.f};
    const dim3 grid(blocks_for((cap + 3) / 4, kThreads, 1u << 30));
    if (channels == 4)
        hipLaunchKernelGGL(k_color<4>, grid, dim3(kThreads), 0, s, x, res, n, cap, limits, lut, palette, tn,
                           rotate ? 1 : 0, out, info);
    else
        hipLaunchKernelGGL(k_color<1>, grid, dim3(kThreads), 0, s, x, res, n, cap, limits, lut, palette, tn,
                           rotate ? 1 : 0, out, info);
}

}  // namespace apt::gpu
