// apt_kernels_eqfloat.hip — gfx950 kernels of APTGPU_CONTRAST_HISTOGRAM_FLOAT (apt_kernels_eqfloat.hpp):
// histogram equalisation of the two channel halves on the f32 signal itself.
//
// Per half, out(p) = #{v in 1..255 : key(p) >= T_v}: the image needs the 255 order statistics T_v (the c_v-th
// smallest keys), not a sort.  They come from a radix multi-select over the 32-bit keys in three levels of
// 11 + 11 + 10 bits: count one level's digit below the prefixes chosen so far, then (a launch of its own) scan the
// counters and push every v's prefix one digit down.  Every counter is an integer, so the result does not depend on
// the order of the atomics.  The kernel boundary is the hand-over between a count and its select.
//
// Every f32 operation of level() is one f32 operation, rounded on its own (contract off; the Makefile's
// -fhip-fp32-correctly-rounded-divide-sqrt makes the division correctly rounded), as in k_eq_lut.
#include "apt_kernels_eqfloat.hpp"

#pragma clang fp contract(off)

namespace apt::gpu {

namespace {

constexpr int kPx = 2080;      // PX_PER_ROW, decode.rs:14
constexpr int kHalf = 1040;    // PX_PER_CHANNEL: the two sub-images of histogram_equalization
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kV = 255;        // the levels 1..255 that have a threshold
constexpr int kBins1 = 2048, kBins2 = 2048, kBins3 = 1024;  // key bits 31..21, 20..10, 9..0
constexpr int kCountBlocks = 256;  // at most one workgroup per CU, as k_eq_histogram

// workspace layout, in u32 words (eqfloat_ws_bytes)
constexpr size_t kCnt1Off = 0;                                   // [2][2048]
constexpr size_t kCnt2Off = kCnt1Off + 2 * kBins1;               // [2][255][2048]
constexpr size_t kCnt3Off = kCnt2Off + size_t(2) * kV * kBins2;  // [2][255][1024]
constexpr size_t kCntWords = kCnt3Off + size_t(2) * kV * kBins3;
constexpr size_t kPref1Off = kCntWords;        // [2][256]: every v's 11-bit prefix (select 1)
constexpr size_t kRank1Off = kPref1Off + 512;  // [2][256]: its rank among the samples under that prefix, >= 1
constexpr size_t kPref2Off = kRank1Off + 512;  // [2][256]: 22-bit prefix (select 2)
constexpr size_t kRank2Off = kPref2Off + 512;
constexpr size_t kThrOff = kRank2Off + 512;    // [2][255]: T_1..T_255 per half (select 3)
constexpr size_t kWsWords = kThrOff + 512;

static_assert(kCntWords * sizeof(uint32_t) == 6283264, "the counters of DESIGN.md §16");

// as apt_kernels_image.hip
__device__ inline uint64_t px_count(const Result *res, uint64_t n_host, uint64_t cap)
{
    uint64_t n = n_host;
    if (res) n = res->status == 0 ? res->n_out : 0;
    return n < cap ? n : cap;
}

// samples of one half: N of the definition (`as u32`)
__device__ inline uint32_t half_total(const Result *res, uint64_t n_host, uint64_t cap)
{
    return static_cast<uint32_t>(px_count(res, n_host, cap) / kPx * kHalf);
}

// IEEE totalOrder as an unsigned compare
__device__ inline uint32_t key_of(float v)
{
    const uint32_t b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// imageext.rs:33,38: (255f32 * (cum as f32 / total as f32)) as u8; in [0, 255] for c <= N
__device__ inline uint32_t level(uint32_t c, float total)
{
    return static_cast<uint32_t>(255.f * (static_cast<float>(c) / total));
}

__device__ inline bool aligned16(const void *p)
{
    return (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

// processing::rotate (processing.rs:21-37), as k_color: source pixel of output (r, c)
__device__ inline uint64_t rotate_src(uint64_t r, uint32_t c, uint64_t rows)
{
    constexpr uint32_t kOff = 39 + 47, kW = 909, kCh = 1040;
    uint32_t base = ~0u;
    if (c >= kOff && c < kOff + kW) base = kOff;
    else if (c >= kOff + kCh && c < kOff + kCh + kW) base = kOff + kCh;
    if (base == ~0u) return r * kPx + c;
    return (rows - 1 - r) * kPx + base + (kW - 1 - (c - base));
}

// Inclusive sum of one value per thread over the workgroup.  s_wave: kWaves words; the caller synchronises before
// it reuses them.
__device__ inline uint32_t block_scan(uint32_t a, uint32_t *s_wave)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(a, d);
        if (lane >= d) a += o;
    }
    if (lane == 63) s_wave[wave] = a;
    __syncthreads();
    for (int w = 0; w < wave; w++) a += s_wave[w];
    return a;
}

// The prefixes of v = 1..255 are non-decreasing in v (s_p[0..254]); equal ones share a counter row.  Returns the row
// id of thread t's v = t + 1 (t < 255), writes the distinct prefixes in order to s_u[0..*s_n) and their number to
// *s_n (<= 255).  Every thread of the workgroup calls it; it ends with a barrier.
__device__ inline uint32_t compact_ids(const uint32_t *s_p, uint32_t *s_u, uint32_t *s_wave, uint32_t *s_n)
{
    const int t = threadIdx.x;
    const uint32_t flag = t < kV && (t == 0 || s_p[t] != s_p[t - 1]) ? 1u : 0u;
    const uint32_t a = block_scan(flag, s_wave);
    if (flag) s_u[a - 1] = s_p[t];
    if (t == kThreads - 1) *s_n = a;
    __syncthreads();
    return a - 1;
}

// number of entries of the sorted s[0..n) that are <= p (n <= 255): 8 steps, no branch
__device__ inline uint32_t count_le(const uint32_t *s, uint32_t n, uint32_t p)
{
    uint32_t lo = 0;
#pragma unroll
    for (uint32_t step = 128; step; step >>= 1) {
        const uint32_t m = lo + step;  // <= 255
        if (m <= n && s[m - 1] <= p) lo = m;
    }
    return lo;
}

// One add per run of equal addresses over neighbouring lanes (a == ~0u: nothing to count).  APT rows hold long runs
// of one value (sync, space, telemetry, saturated cloud), and one lane's quad is four consecutive samples, so a run
// along the row is a run along the lanes; equal addresses that are not neighbours are added on their own.
__device__ inline void add_runs(uint32_t *cnt, uint32_t a)
{
    const int lane = threadIdx.x & 63;
    const uint32_t prev = __shfl_up(a, 1);
    const bool head = lane == 0 || a != prev;
    const uint64_t heads = __ballot(head);
    if (head && a != ~0u) {
        const uint64_t rest = lane == 63 ? 0ull : heads >> (lane + 1);
        const uint32_t len = rest ? static_cast<uint32_t>(__ffsll(static_cast<unsigned long long>(rest)))
                                  : static_cast<uint32_t>(64 - lane);
        atomicAdd(&cnt[a], len);
    }
}

// Level 1: the histogram of key >> 21 of both halves.  k_eq_histogram's shape: grid-stride over quads that never
// straddle a row or a half, sub-histograms in LDS (one per pair of waves: 2 x 2 x 2048 words), one global add per
// non-zero bin and workgroup.
__global__ __launch_bounds__(kThreads) void k_eqf_count1(const float *__restrict__ x, const Result *res,
                                                         uint64_t n_host, uint64_t cap, uint32_t *cnt)
{
    __shared__ uint32_t s_h[2][2 * kBins1];
    for (int k = threadIdx.x; k < 2 * 2 * kBins1; k += kThreads) (&s_h[0][0])[k] = 0u;
    __syncthreads();
    const uint64_t quads = px_count(res, n_host, cap) / kPx * (kPx / 4);
    uint32_t *h = s_h[threadIdx.x >> 7];
    const uint64_t gtid = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    const bool vec = aligned16(x);
    for (uint64_t q = gtid; q < quads; q += stride) {
        const uint32_t half = static_cast<uint32_t>(q % (kPx / 4)) < kHalf / 4 ? 0u : static_cast<uint32_t>(kBins1);
        float v0, v1, v2, v3;
        if (vec) {
            const float4 v = reinterpret_cast<const float4 *>(x)[q];
            v0 = v.x, v1 = v.y, v2 = v.z, v3 = v.w;
        } else {
            v0 = x[4 * q], v1 = x[4 * q + 1], v2 = x[4 * q + 2], v3 = x[4 * q + 3];
        }
        atomicAdd(&h[half + (key_of(v0) >> 21)], 1u);
        atomicAdd(&h[half + (key_of(v1) >> 21)], 1u);
        atomicAdd(&h[half + (key_of(v2) >> 21)], 1u);
        atomicAdd(&h[half + (key_of(v3) >> 21)], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < 2 * kBins1; b += kThreads) {
        const uint32_t c = s_h[0][b] + s_h[1][b];
        if (c) atomicAdd(&cnt[b], c);
    }
}

// Levels 2 and 3: samples whose bits above the level's digit are one of the (at most 255) prefixes the previous select
// chose count their digit into that prefix's row.  kShift: the digit's lowest bit; kBins: its range.
template <int kShift, int kBins>
__global__ __launch_bounds__(kThreads) void k_eqf_count(const float *__restrict__ x, const Result *res, uint64_t n_host,
                                                        uint64_t cap, const uint32_t *pref, uint32_t *cnt)
{
    __shared__ uint32_t s_p[2][kThreads], s_u[2][kThreads], s_wave[2][kWaves], s_n[2];
    constexpr int kUp = kShift == 0 ? 10 : 21;  // the prefix is key >> kUp
    const int t = threadIdx.x;
    s_p[0][t] = t < kV ? pref[t] : 0u;
    s_p[1][t] = t < kV ? pref[kThreads + t] : 0u;
    __syncthreads();
    compact_ids(s_p[0], s_u[0], s_wave[0], &s_n[0]);
    compact_ids(s_p[1], s_u[1], s_wave[1], &s_n[1]);
    const uint64_t quads = px_count(res, n_host, cap) / kPx * (kPx / 4);
    const uint64_t gtid = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    const bool vec = aligned16(x);
    // (every lane of a wave makes the same number of trips: add_runs shuffles across the whole wave)
    const uint64_t trips = (quads + stride - 1) / stride;
    for (uint64_t k = 0; k < trips; k++) {
        const uint64_t q = gtid + k * stride;
        uint32_t a[4] = {~0u, ~0u, ~0u, ~0u};
        if (q < quads) {
            const uint32_t hf = static_cast<uint32_t>(q % (kPx / 4)) < kHalf / 4 ? 0u : 1u;
            float v[4];
            if (vec) {
                const float4 f = reinterpret_cast<const float4 *>(x)[q];
                v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
            } else {
                for (int j = 0; j < 4; j++) v[j] = x[4 * q + j];
            }
            const uint32_t n = s_n[hf];
            for (int j = 0; j < 4; j++) {
                const uint32_t key = key_of(v[j]);
                const uint32_t p = key >> kUp;
                const uint32_t le = count_le(s_u[hf], n, p);
                if (le != 0u && s_u[hf][le - 1] == p)  // row le - 1 < n <= 255
                    a[j] = (hf * kV + (le - 1)) * kBins + ((key >> kShift) & (kBins - 1));
            }
        }
        for (int j = 0; j < 4; j++) add_runs(cnt, a[j]);
    }
}

// The select of one level, one workgroup per (counter row, half); thread t owns v = t + 1.  It scans its row and, for
// every v whose prefix is the row's, finds the digit under which v's rank falls: the smallest d with
// cum[d] >= rank.  The prefix grows by d and the rank becomes the rank among the samples of that digit.
// kLevel 1: one row per half, and the ranks are the c_v themselves, found here by bisection over level() (the smallest
// c in [1, N] with level(c) >= v; level is non-decreasing and level(N) = 255).  kLevel 3: the prefixes are the keys T_v.
template <int kLevel>
__global__ __launch_bounds__(kThreads) void k_eqf_select(const Result *res, uint64_t n_host, uint64_t cap,
                                                         const uint32_t *cnt, const uint32_t *pref_in,
                                                         const uint32_t *rank_in, uint32_t *pref_out,
                                                         uint32_t *rank_out)
{
    constexpr int kBins = kLevel == 3 ? kBins3 : kBins1;
    constexpr int kBits = kLevel == 3 ? 10 : 11;
    constexpr int kPer = kBins / kThreads;
    constexpr int kOutStride = kLevel == 3 ? kV : kThreads;
    __shared__ uint32_t s_p[kThreads], s_u[kThreads], s_wave[kWaves], s_wave2[kWaves], s_n, s_cum[kBins];
    const int t = threadIdx.x;
    const uint32_t hf = blockIdx.y, row = blockIdx.x;
    const uint32_t total = half_total(res, n_host, cap);
    if (total == 0u) return;  // no pixel reads a threshold
    uint32_t id = 0, rank = 0, p = 0;
    if (kLevel == 1) {
        if (t < kV) {
            const float ftotal = static_cast<float>(total);
            const uint32_t v = static_cast<uint32_t>(t) + 1u;
            uint32_t lo = 1, hi = total;
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (level(mid, ftotal) >= v) hi = mid;
                else lo = mid + 1;
            }
            rank = lo;
        }
    } else {
        s_p[t] = t < kV ? pref_in[hf * kThreads + t] : 0u;
        __syncthreads();
        id = compact_ids(s_p, s_u, s_wave, &s_n);
        if (row >= s_n) return;
        if (t < kV) {
            rank = rank_in[hf * kThreads + t];
            p = s_p[t];
        }
    }
    const uint32_t *c = cnt + (static_cast<size_t>(hf) * (kLevel == 1 ? 1 : kV) + row) * kBins;
    uint32_t own[kPer], sum = 0;
    for (int j = 0; j < kPer; j++) {
        own[j] = c[t * kPer + j];
        sum += own[j];
    }
    uint32_t cum = block_scan(sum, s_wave2) - sum;
    for (int j = 0; j < kPer; j++) {
        cum += own[j];
        s_cum[t * kPer + j] = cum;
    }
    __syncthreads();
    if (t < kV && id == row) {
        uint32_t lo = 0, hi = kBins - 1;  // (rank <= s_cum[kBins - 1]: the row counted every sample under its prefix)
        while (lo < hi) {
            const uint32_t mid = (lo + hi) / 2;
            if (s_cum[mid] >= rank) hi = mid;
            else lo = mid + 1;
        }
        pref_out[hf * kOutStride + t] = (p << kBits) | lo;
        if (kLevel != 3) rank_out[hf * kThreads + t] = rank - (lo ? s_cum[lo - 1] : 0u);
    }
}

// The output pass, k_color's shape: 4 output pixels per thread (a quad never straddles a row or a half), both
// halves' thresholds in LDS, the level of a pixel = the number of its half's thresholds <= its key.
template <int kCh>
__global__ __launch_bounds__(kThreads) void k_color_float(const float *__restrict__ x, const Result *res,
                                                          uint64_t n_host, uint64_t cap, const float *limits,
                                                          const uint32_t *thr, int rotate, uint8_t *__restrict__ out,
                                                          ImageResult *info)
{
    __shared__ uint32_t s_t[2][kThreads];
    s_t[0][threadIdx.x] = threadIdx.x < kV ? thr[threadIdx.x] : 0xFFFFFFFFu;
    s_t[1][threadIdx.x] = threadIdx.x < kV ? thr[kV + threadIdx.x] : 0xFFFFFFFFu;
    __syncthreads();
    const uint64_t n = px_count(res, n_host, cap);
    const uint64_t rows = n / kPx;
    const uint64_t npx = rows * kPx;
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
    float v[4];
    if (!rotate && aligned16(x)) {
        const float4 a = *reinterpret_cast<const float4 *>(x + i0);
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
    } else {
        for (int k = 0; k < 4; k++) v[k] = x[rotate ? rotate_src(r, c0 + k, rows) : i0 + k];  // (stays in its half)
    }
    const uint32_t *th = s_t[c0 < kHalf ? 0 : 1];
    uint32_t px[4];
    for (int k = 0; k < 4; k++) {
        const uint32_t g = count_le(th, kV, key_of(v[k]));
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

size_t eqfloat_ws_bytes()
{
    return kWsWords * sizeof(uint32_t);
}

const uint32_t *eqfloat_ws_thresholds(const void *eq_ws)
{
    return static_cast<const uint32_t *>(eq_ws) + kThrOff;
}

void image_equalize_float(hipStream_t s, const float *x, const Result *res, uint64_t n, uint64_t cap, void *eq_ws)
{
    uint32_t *ws = static_cast<uint32_t *>(eq_ws);
    uint32_t *cnt1 = ws + kCnt1Off, *cnt2 = ws + kCnt2Off, *cnt3 = ws + kCnt3Off;
    uint32_t *pref1 = ws + kPref1Off, *rank1 = ws + kRank1Off, *pref2 = ws + kPref2Off, *rank2 = ws + kRank2Off;
    (void)hipMemsetAsync(ws, 0, kCntWords * sizeof(uint32_t), s);
    const dim3 nb(blocks_for(cap / 4, kThreads * 16, kCountBlocks)), th(kThreads);
    hipLaunchKernelGGL(k_eqf_count1, nb, th, 0, s, x, res, n, cap, cnt1);
    hipLaunchKernelGGL(k_eqf_select<1>, dim3(1, 2), th, 0, s, res, n, cap, cnt1, nullptr, nullptr, pref1, rank1);
    hipLaunchKernelGGL((k_eqf_count<10, kBins2>), nb, th, 0, s, x, res, n, cap, pref1, cnt2);
    hipLaunchKernelGGL(k_eqf_select<2>, dim3(kV, 2), th, 0, s, res, n, cap, cnt2, pref1, rank1, pref2, rank2);
    hipLaunchKernelGGL((k_eqf_count<0, kBins3>), nb, th, 0, s, x, res, n, cap, pref2, cnt3);
    hipLaunchKernelGGL(k_eqf_select<3>, dim3(kV, 2), th, 0, s, res, n, cap, cnt3, pref2, rank2, ws + kThrOff, nullptr);
}

void image_color_float(hipStream_t s, const float *x, const Result *res, uint64_t n, uint64_t cap, void *image_ws,
                       const void *eq_ws, int channels, bool rotate, uint8_t *out, ImageResult *info)
{
    const float *limits = image_ws_pointers(image_ws, cap).limits;
    const uint32_t *thr = eqfloat_ws_thresholds(eq_ws);
    const dim3 grid(blocks_for((cap + 3) / 4, kThreads, 1u << 30));
    if (channels == 4)
        hipLaunchKernelGGL(k_color_float<4>, grid, dim3(kThreads), 0, s, x, res, n, cap, limits, thr, rotate ? 1 : 0, out,
                           info);
    else
        hipLaunchKernelGGL(k_color_float<1>, grid, dim3(kThreads), 0, s, x, res, n, cap, limits, thr, rotate ? 1 : 0, out,
                           info);
}

}  // namespace apt::gpu
