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
//
// Histogram + false colour (the opt-in Lab path, apt_lab.hpp): channel A's pixels are looked up by
// their table index (palette colour tb*256 + ta inside [86, 995), gray 65536 + v elsewhere), the
// histogram counts the index's L bin, k_eq_lut also makes the 101 equalised L values, and
// k_lab_rgba turns every index into its RGBA once per call, so the output pass only gathers.
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

// Lab workspace layout (lab_ws_bytes): the host's lab::Tables first (one upload), then the per-call
// equalised L values and RGBA table
constexpr size_t kLabLpOff = (sizeof(lab::Tables) + 255) & ~size_t(255);
constexpr size_t kLabRgbaOff = kLabLpOff + 128 * sizeof(float);
constexpr size_t kLabWsBytes = kLabRgbaOff + lab::kEntries * sizeof(uint32_t);
constexpr int kLabIndexBlocks = (lab::kEntries + kThreads - 1) / kThreads;

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

// (tune_input_values, processing.rs:126-140: tune() of apt_color_tune.hpp)

__device__ inline bool aligned16(const void *p)
{
    return (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

// channel A's index into the Lab tables: palette colour inside the image columns, gray elsewhere
__device__ inline uint32_t lab_index(uint32_t c, uint32_t g_a, uint32_t g_b, const ColorTune &tn)
{
    if (c >= kColorStart && c < kColorEnd) return tune(g_b, tn.k_b, tn.o_b) * 256u + tune(g_a, tn.k_a, tn.o_a);
    return lab::kPaletteEntries + g_a;
}

// Histograms of both halves of the u8 image.  Per-wave sub-histograms in LDS: APT rows have long
// runs of one value (sync, space, telemetry, saturated cloud), and lanes adding to one LDS word
// serialise; four copies cut that by the number of waves.  Then one global add per non-zero bin.
// kLab: channel A counts the L bin (< 101) of each pixel's Lab table index instead of its value.
template <bool kLab>
__global__ __launch_bounds__(kThreads) void k_eq_histogram(const float *__restrict__ x, const Result *res,
                                                           uint64_t n_host, uint64_t cap, const float *limits,
                                                           uint32_t *hist, const uint8_t *__restrict__ lab_bin,
                                                           ColorTune tn)
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
        if (kLab && half == 0u) {
            const uint32_t c0 = static_cast<uint32_t>(q % (kPx / 4)) * 4u;
            float w[4] = {0.f, 0.f, 0.f, 0.f};  // channel B partners, 1040 columns on in the same row
            if (c0 + 3 >= kColorStart && c0 < kColorEnd) {
                const uint64_t qb = q + kHalf / 4;
                if (vec) {
                    const float4 b = reinterpret_cast<const float4 *>(x)[qb];
                    w[0] = b.x, w[1] = b.y, w[2] = b.z, w[3] = b.w;
                } else {
                    for (int k = 0; k < 4; k++) w[k] = x[4 * qb + k];
                }
            }
            const float v[4] = {v0, v1, v2, v3};
            for (int k = 0; k < 4; k++) {
                const uint32_t idx = lab_index(c0 + k, map_px(v[k], low, range), map_px(w[k], low, range), tn);
                atomicAdd(&h[lab_bin[idx]], 1u);
            }
            continue;
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
// lprime (Lab path): channel A's bins 0..100 are L bins, and l' = 100f32 * (cum[bin] as f32 / cum[100] as
// f32) (imageext.rs:56-62); bins 101..255 are empty there, so cum[100] is the total.
__global__ __launch_bounds__(kThreads) void k_eq_lut(uint32_t *hist, uint8_t *lut, float *lprime)
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
    if (lprime && t < lab::kBins) {
        float lp = 0.f;
        if (s_total[0] != 0u) lp = 100.f * (static_cast<float>(a) / static_cast<float>(s_total[0]));
        lprime[t] = lp;
    }
}

// Lab::to_rgb of every table index with its equalised L: (l'[bin], a, b) -> RGBA, A = 255
// (lab_to_rgb_mut keeps the alpha of the RgbaImage, which is 255 everywhere).
__global__ __launch_bounds__(kThreads) void k_lab_rgba(const lab::Tables *__restrict__ tab, const float *lprime,
                                                       uint32_t *__restrict__ rgba)
{
    __shared__ float s_thr[256];
    __shared__ float s_lp[lab::kBins];
    for (int k = threadIdx.x; k < 256; k += kThreads) s_thr[k] = tab->thr[k];
    for (int k = threadIdx.x; k < lab::kBins; k += kThreads) s_lp[k] = lprime[k];
    __syncthreads();
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= static_cast<uint32_t>(lab::kEntries)) return;
    const uint32_t bin = tab->bin[i];  // <= 100 (lab::bin_of)
    rgba[i] = lab::to_rgba(s_lp[bin], tab->ab[i][0], tab->ab[i][1], s_thr);
}

// The output pass, 4 output pixels per thread (a quad never straddles a row or a half).
template <int kCh>
__global__ __launch_bounds__(kThreads) void k_color(const float *__restrict__ x, const Result *res, uint64_t n_host,
                                                    uint64_t cap, const float *limits, const uint8_t *lut,
                                                    const uint32_t *__restrict__ palette, ColorTune tn,
                                                    const uint32_t *__restrict__ lab_rgba, int rotate,
                                                    uint8_t *__restrict__ out, ImageResult *info)
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
    const bool colored = (palette || lab_rgba) && c0 + 3 >= kColorStart && c0 < kColorEnd;
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
            px[k] = lab_rgba ? lab_rgba[tb * 256u + ta] : palette[tb * 256u + ta];
            continue;
        }
        if (lab_rgba && half == 0u) {  // channel A's gray columns go through Lab as well
            px[k] = lab_rgba[lab::kPaletteEntries + g];
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
    hipLaunchKernelGGL(k_eq_histogram<false>, dim3(nb), dim3(kThreads), 0, s, x, res, n, cap, limits, hist,
                       nullptr, ColorTune{0.f, 0.f, 0.f, 0.f});
    hipLaunchKernelGGL(k_eq_lut, dim3(1), dim3(kThreads), 0, s, hist, reinterpret_cast<uint8_t *>(ws + kLutOff),
                       nullptr);
}

size_t lab_ws_bytes()
{
    return kLabWsBytes;
}

void image_equalize_lab(hipStream_t s, const float *x, const Result *res, uint64_t n, uint64_t cap, void *image_ws,
                        void *color_ws, void *lab_ws, const ColorTune &tn)
{
    const float *limits = image_ws_pointers(image_ws, cap).limits;
    char *ws = static_cast<char *>(color_ws);
    char *lw = static_cast<char *>(lab_ws);
    const auto *tab = reinterpret_cast<const lab::Tables *>(lw);
    float *lprime = reinterpret_cast<float *>(lw + kLabLpOff);
    uint32_t *hist = reinterpret_cast<uint32_t *>(ws + kHistOff);
    const unsigned nb = blocks_for(cap / 4, kThreads * 16, kHistBlocks);
    hipLaunchKernelGGL(k_eq_histogram<true>, dim3(nb), dim3(kThreads), 0, s, x, res, n, cap, limits, hist,
                       tab->bin, tn);
    hipLaunchKernelGGL(k_eq_lut, dim3(1), dim3(kThreads), 0, s, hist, reinterpret_cast<uint8_t *>(ws + kLutOff),
                       lprime);
    hipLaunchKernelGGL(k_lab_rgba, dim3(kLabIndexBlocks), dim3(kThreads), 0, s, tab, lprime,
                       reinterpret_cast<uint32_t *>(lw + kLabRgbaOff));
}

void image_color(hipStream_t s, const float *x, const Result *res, uint64_t n, uint64_t cap, void *image_ws,
                 const void *color_ws, bool equalize, const ColorTune *tune_p, int channels, bool rotate,
                 uint8_t *out, ImageResult *info, const void *lab_ws)
{
    const float *limits = image_ws_pointers(image_ws, cap).limits;
    const char *ws = static_cast<const char *>(color_ws);
    const uint8_t *lut = equalize ? reinterpret_cast<const uint8_t *>(ws + kLutOff) : nullptr;
    const uint32_t *lab_rgba =
        lab_ws ? reinterpret_cast<const uint32_t *>(static_cast<const char *>(lab_ws) + kLabRgbaOff) : nullptr;
    const uint32_t *palette = tune_p && !lab_ws ? reinterpret_cast<const uint32_t *>(ws + kPaletteOff) : nullptr;
    const ColorTune tn = tune_p ? *tune_p : ColorTune{0.f, 0.f, 0.f, 0.f};
    const dim3 grid(blocks_for((cap + 3) / 4, kThreads, 1u << 30));
    if (channels == 4)
        hipLaunchKernelGGL(k_color<4>, grid, dim3(kThreads), 0, s, x, res, n, cap, limits, lut, palette, tn,
                           lab_rgba, rotate ? 1 : 0, out, info);
    else
        hipLaunchKernelGGL(k_color<1>, grid, dim3(kThreads), 0, s, x, res, n, cap, limits, lut, palette, tn,
                           lab_rgba, rotate ? 1 : 0, out, info);
}

}  // namespace apt::gpu
