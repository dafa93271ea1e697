// apt_kernels_thermal.hip — the gfx950 kernels of the thermal calibration stage (definition: apt_kernels_thermal.hpp,
// include/aptgpu.h).  Three launches per recording behind the telemetry stage's:
//
//  k_thermal_space  128 threads, one per row of the space view: the sequential f32 mean of its 38 columns.
//  k_thermal_setup  one workgroup of 128 threads ranks the means by counting (totalOrder keys in LDS, ties by row);
//                   thread 0 adds the 96 kept means in row order in f64, runs the scalar chain (scalars_of, the very
//                   function the CPU runs) and writes the record and the f32 pixel parameters.
//  k_thermal_map    the hot path.  A workgroup of 256 threads walks rows (grid stride); a thread takes quads of four
//                   consecutive image columns, 16-byte groups of the row image that are 4-byte aligned loads
//                   (f4_a4, as the row gather's: the buffer is only known to be float aligned, and neither is
//                   column 86 on a 16-byte boundary of the Kelvin plane's rows of 909).  One pass writes the Kelvin
//                   plane and, when asked, the scale image through a 256-entry RGBA table in LDS: four bytes (gray)
//                   or one 16-byte store (RGBA) per quad, zero quads outside the video columns.  NaN count and the
//                   finite extremes (as totalOrder keys) stay in registers over all rows of a thread, are reduced
//                   per wave with shuffles and reach one of the record's 64 partial records with at most three integer atomics per wave.
#include "apt_kernels_thermal.hpp"

#include "apt_kernels.hpp"

#include <cstddef>

#pragma clang fp contract(off)

namespace apt::gpu {

namespace {

using namespace apt::thermal;
using apt::despeckle::bits_of_key;
using apt::despeckle::key_of_bits;

constexpr int kMapThreads = 256;
constexpr int kMapMaxBlocks = 512;  // two workgroups per CU: rows beyond that are walked with a grid stride
constexpr int kRowQuads = kPx / 4;  // 520

typedef float f4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t u4_a4 __attribute__((ext_vector_type(4), aligned(4)));

// What the stage keeps per recording besides the record.
struct Workspace {
    ThermalRecord rec;           // with its partial records
    PixelParams params;          // 64 bytes
    ImageResult telemetry;       // the telemetry stage's record
    float means[kSpaceRows];
};

// samples this launch works on; 0 when the decode failed
__device__ inline uint64_t px_count(const Result *res, uint64_t n_host, uint64_t cap)
{
    uint64_t n = n_host;
    if (res) n = res->status == 0 ? res->n_out : 0;
    return n < cap ? n : cap;
}

__global__ __launch_bounds__(kSpaceRows) void k_thermal_space(const float *__restrict__ x, const ImageResult *tel,
                                                              int base, float *means)
{
    if (tel->status != 0) return;  // (no frame: the setup kernel reports it)
    // a frame is 200 rows inside the image, so the 128 rows from its start are too
    const float *p = x + (static_cast<uint64_t>(tel->telemetry_row) + threadIdx.x) * kPx + base + kSpace0;
    float sum = 0.f;
    for (int i = 0; i < kSpaceN; ++i) sum += p[i];
    means[threadIdx.x] = sum / static_cast<float>(kSpaceN);
}

__global__ __launch_bounds__(kSpaceRows) void k_thermal_setup(const Result *res, uint64_t n_host, uint64_t cap,
                                                              const ImageResult *tel, const float *means,
                                                              ThermalCoeffs coeffs, int channel, int channel_id,
                                                              ThermalRecord *rec, PixelParams *params)
{
    __shared__ uint32_t s_key[kSpaceRows];
    __shared__ uint32_t s_keep[kSpaceRows];
    __shared__ float s_mean[kSpaceRows];
    const bool have_frame = tel->status == 0;
    const int t = threadIdx.x;
    s_mean[t] = have_frame ? means[t] : 0.f;
    s_key[t] = key_of_bits(__float_as_uint(s_mean[t]));
    if (t < kThermalParts) {  // fresh partial records for the map kernel's waves
        ThermalPart z{};
        z.t_min_key = 0xFFFFFFFFu;
        rec->part[t] = z;
    }
    __syncthreads();
    const uint32_t mine = s_key[t];
    int rank = 0;
    for (int j = 0; j < kSpaceRows; ++j) {
        const uint32_t k = s_key[j];
        rank += (k < mine || (k == mine && j < t)) ? 1 : 0;
    }
    s_keep[t] = (rank >= kTrim && rank < kSpaceRows - kTrim) ? 1u : 0u;
    __syncthreads();
    if (t != 0) return;

    // (the record's head only: the partial records behind it are other threads')
    struct Head {
        int32_t status, reason;
        uint32_t height, telemetry_row;
        int32_t channel_id;
        uint32_t reserved;
        unsigned long long n_nan;
        double slope, icpt, space, c_space, c_bb, t_bb, n_bb;
        uint32_t t_min_key, t_max_key;
    } r{};
    static_assert(sizeof(Head) == sizeof(aptgpu_thermal_result) && offsetof(ThermalRecord, pad) == sizeof(Head), "record head");
    r.height = static_cast<uint32_t>(px_count(res, n_host, cap) / kPx);
    r.channel_id = channel_id;
    r.t_min_key = 0xFFFFFFFFu;
    r.t_max_key = 0u;
    PixelParams pp{};
    if (!have_frame) {
        r.status = 1;
        r.reason = tel->reason;  // 2 too short, 4 the decode failed
    } else {
        r.telemetry_row = tel->telemetry_row;
        if (channel_id == -1) r.channel_id = channel == 0 ? tel->channel_a : tel->channel_b;
        const int set = set_of_identity(r.channel_id);
        if (set < 0) {
            r.status = 1;
            r.reason = kReasonChannel;
        } else {
            double sum = 0.;
            for (int j = 0; j < kSpaceRows; ++j)
                if (s_keep[j]) sum = sum + static_cast<double>(s_mean[j]);
            const double space = sum / static_cast<double>(kSpaceRows - 2 * kTrim);
            const float *v = channel == 0 ? tel->values_a : tel->values_b;
            float vv[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) vv[k] = v[k];
            // (the set is chosen by copying: a run-time index into the argument struct would put it in scratch)
            double ch[7];
#pragma unroll
            for (int k = 0; k < 7; ++k)
                ch[k] = set == 0 ? coeffs.channel[0][k] : set == 1 ? coeffs.channel[1][k] : coeffs.channel[2][k];
            const Scalars sc = scalars_of(vv, space, coeffs.prt, ch);
            r.slope = sc.slope;
            r.icpt = sc.icpt;
            r.space = sc.space;
            r.c_space = sc.c_space;
            r.c_bb = sc.c_bb;
            r.t_bb = sc.t_bb;
            r.n_bb = sc.n_bb;
            if (!sc.ok) {
                r.status = 1;
                r.reason = kReasonDegenerate;
            }
            pp = pixel_params(sc, ch);
        }
    }
    if (r.status != 0) pp.ok = 0;
    *reinterpret_cast<Head *>(rec) = r;
    *params = pp;
}

__device__ inline uint32_t shfl_down_u32(uint32_t v, int d) { return static_cast<uint32_t>(__shfl_down(static_cast<int>(v), d)); }

// CH: bytes per pixel of the scale image (0: none)
template <int CH>
__global__ __launch_bounds__(kMapThreads) void k_thermal_map(const float *__restrict__ x, const Result *res,
                                                             uint64_t n_host, uint64_t cap, ThermalRecord *rec,
                                                             const PixelParams *__restrict__ params, int base,
                                                             int cold_white, float t_low, float t_high,
                                                             ThermalTable table, float *__restrict__ kelvin,
                                                             uint8_t *__restrict__ image)
{
    __shared__ uint32_t s_rgba[256];
    const uint64_t h = px_count(res, n_host, cap) / kPx;
    if (CH == 4) {
        // the table by level: the caller's RGB (read from the kernel-argument segment), or gray; A = 255
        const uint32_t l = threadIdx.x;
        const uint8_t *e = table.rgb + 3 * l;
        s_rgba[l] = table.has_palette ? (uint32_t(e[0]) | (uint32_t(e[1]) << 8) | (uint32_t(e[2]) << 16) | 0xFF000000u)
                                       : (l * 0x010101u | 0xFF000000u);
        __syncthreads();
    }
    const PixelParams pp = *params;
    const bool ok = pp.ok != 0;
    const int lo = base + kVideo0, hi = lo + kVideoN;  // the video columns [lo, hi)
    // quads that hold a video column; without a scale image nothing else is visited
    const int q_first = CH ? 0 : lo / 4, q_last = CH ? kRowQuads - 1 : (hi - 1) / 4;
    const bool gray_vec = (reinterpret_cast<uintptr_t>(image) & 3u) == 0;

    uint32_t n_nan = 0, min_key = 0xFFFFFFFFu, max_key = 0u;
    for (uint64_t y = blockIdx.x; y < h; y += gridDim.x) {
        const float *row = x + y * kPx;
        float *krow = kelvin + y * kVideoN;
        for (int q = q_first + static_cast<int>(threadIdx.x); q <= q_last; q += kMapThreads) {
            const int c0 = 4 * q;
            uint32_t out[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) out[j] = CH == 4 ? 0xFF000000u : 0u;
            if (c0 + 3 >= lo && c0 < hi) {
                const f4_a4 v4 = *reinterpret_cast<const f4_a4 *>(row + c0);  // (c0 + 3 < 2080: inside row y < h)
                const float v[4] = {v4.x, v4.y, v4.z, v4.w};
                float t[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool in = c0 + j >= lo && c0 + j < hi;
                    t[j] = ok ? kelvin_of(v[j], pp) : quiet_nan();
                    const bool nan = t[j] != t[j];
                    const bool finite = t[j] - t[j] == 0.f;
                    const uint32_t key = key_of_bits(__float_as_uint(t[j]));
                    n_nan += (in && nan) ? 1u : 0u;
                    min_key = (in && finite && key < min_key) ? key : min_key;
                    max_key = (in && finite && key > max_key) ? key : max_key;
                    if (CH) {
                        const uint32_t level = nan ? 0u : level_of(t[j], t_low, t_high, cold_white != 0);
                        const uint32_t px = CH == 4 ? (nan ? 0u : s_rgba[level]) : level;
                        out[j] = in ? px : out[j];
                    }
                }
                if (c0 >= lo && c0 + 3 < hi) {
                    f4_a4 o;
                    o.x = t[0];
                    o.y = t[1];
                    o.z = t[2];
                    o.w = t[3];
                    *reinterpret_cast<f4_a4 *>(krow + (c0 - lo)) = o;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (c0 + j >= lo && c0 + j < hi) krow[c0 + j - lo] = t[j];
                }
            }
            if (CH == 4) {
                u4_a4 o;
                o.x = out[0];
                o.y = out[1];
                o.z = out[2];
                o.w = out[3];
                *reinterpret_cast<u4_a4 *>(image + (y * kPx + static_cast<uint64_t>(c0)) * 4u) = o;
            } else if (CH == 1) {
                uint8_t *dst = image + y * kPx + static_cast<uint64_t>(c0);
                if (gray_vec) {
                    *reinterpret_cast<uint32_t *>(dst) = out[0] | (out[1] << 8) | (out[2] << 16) | (out[3] << 24);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) dst[j] = static_cast<uint8_t>(out[j]);
                }
            }
        }
    }

    // ---- per wave, then at most three integer atomics per wave, on one of the partial records
    for (int d = 32; d >= 1; d >>= 1) {
        n_nan += shfl_down_u32(n_nan, d);
        const uint32_t a = shfl_down_u32(min_key, d), b = shfl_down_u32(max_key, d);
        min_key = a < min_key ? a : min_key;
        max_key = b > max_key ? b : max_key;
    }
    if ((threadIdx.x & 63) == 0) {
        ThermalPart *part = &rec->part[(blockIdx.x * (kMapThreads / 64) + (threadIdx.x >> 6)) % kThermalParts];
        if (n_nan) atomicAdd(&part->n_nan, static_cast<unsigned long long>(n_nan));
        if (min_key <= max_key) {
            atomicMin(&part->t_min_key, min_key);
            atomicMax(&part->t_max_key, max_key);
        }
    }
}

inline Workspace *view(void *ws) { return static_cast<Workspace *>(ws); }

}  // namespace

size_t thermal_ws_bytes() { return sizeof(Workspace); }
ThermalRecord *thermal_ws_record(void *ws) { return &view(ws)->rec; }
ImageResult *thermal_ws_telemetry(void *ws) { return &view(ws)->telemetry; }

void thermal_record_to_public(const ThermalRecord &r, aptgpu_thermal_result *out)
{
    static_assert(offsetof(ThermalRecord, pad) == sizeof(aptgpu_thermal_result), "ThermalRecord's head must mirror aptgpu_thermal_result");
    std::memcpy(out, &r, sizeof *out);
    uint32_t min_key = 0xFFFFFFFFu, max_key = 0u;
    out->n_nan = 0;
    for (const ThermalPart &p : r.part) {
        out->n_nan += p.n_nan;
        min_key = p.t_min_key < min_key ? p.t_min_key : min_key;
        max_key = p.t_max_key > max_key ? p.t_max_key : max_key;
    }
    const bool any = min_key <= max_key;
    const uint32_t lo = bits_of_key(min_key), hi = bits_of_key(max_key);
    out->t_min = out->t_max = quiet_nan();
    if (any) {
        std::memcpy(&out->t_min, &lo, sizeof lo);
        std::memcpy(&out->t_max, &hi, sizeof hi);
    }
}

void thermal_space(hipStream_t s, const ThermalLaunch &l, void *ws)
{
    Workspace *w = view(ws);
    hipLaunchKernelGGL(k_thermal_space, dim3(1), dim3(kSpaceRows), 0, s, l.x, &w->telemetry, kHalfPx * l.channel,
                       w->means);
}

void thermal_setup(hipStream_t s, const ThermalLaunch &l, const ThermalCoeffs &c, void *ws)
{
    Workspace *w = view(ws);
    hipLaunchKernelGGL(k_thermal_setup, dim3(1), dim3(kSpaceRows), 0, s, l.res, l.n, l.cap, &w->telemetry, w->means, c,
                       l.channel, l.channel_id, &w->rec, &w->params);
}

void thermal_map(hipStream_t s, const ThermalLaunch &l, const ThermalTable &table, void *ws)
{
    Workspace *w = view(ws);
    const uint64_t rows = l.cap / kPx;
    const dim3 grid(static_cast<unsigned>(rows < 1 ? 1 : rows < kMapMaxBlocks ? rows : kMapMaxBlocks));
    const int base = kHalfPx * l.channel;
    if (l.image_channels == 4) {
        // (the table travels by value in the kernel-argument segment: the caller's bytes are read before this returns)
        hipLaunchKernelGGL(k_thermal_map<4>, grid, dim3(kMapThreads), 0, s, l.x, l.res, l.n, l.cap, &w->rec, &w->params,
                           base, l.cold_white ? 1 : 0, l.t_low, l.t_high, table, l.kelvin, l.image);
    } else if (l.image_channels == 1) {
        hipLaunchKernelGGL(k_thermal_map<1>, grid, dim3(kMapThreads), 0, s, l.x, l.res, l.n, l.cap, &w->rec, &w->params,
                           base, l.cold_white ? 1 : 0, l.t_low, l.t_high, table, l.kelvin, l.image);
    } else {
        hipLaunchKernelGGL(k_thermal_map<0>, grid, dim3(kMapThreads), 0, s, l.x, l.res, l.n, l.cap, &w->rec, &w->params,
                           base, l.cold_white ? 1 : 0, l.t_low, l.t_high, table, l.kelvin, l.image);
    }
}

}  // namespace apt::gpu
