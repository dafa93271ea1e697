// apt_kernels_afc.hpp — AFC in front of the FM demodulator: follow the carrier of an IQ recording block by block and
// demodulate with an NCO that reads a table (apt_kernels_afc.hip and apt_kernels_fm_tracked.hip on the GPU, apt_afc.cpp
// on the CPU).  The reference has nothing comparable, so this is the definition (include/aptgpu.h §4b'
// states it in full; tests/np_afc_model.py in numpy).  The per-frame and per-block arithmetic is written once, here,
// for both sides; they differ only in atan2 and in the cos / sin of a block's step.
//
//  A  sums   per block of B frames, with components as integers (u8: 2 raw - 255): the lag-L autocorrelation
//            re + j im = sum x[i + L] conj(x[i]) and the energy en = sum |x[i]|^2, exact in int64 (F32: in f64).
//  B  table  windowed sums over W blocks -> coherence, the phase increment the window's angle stands for, good / not,
//            hold of the nearest good block, the uint32 prefix sum of the phase and the f32 step of every block.
//  C  demod  §4b with the phase of frame i taken from the table: phase0[b] + (uint32)(i - b B) * pw[b], b = i / B.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <vector>

#include "apt_kernels_fm.hpp"

namespace apt::afc {

constexpr uint32_t kMinBlock = 64, kMaxBlock = 1u << 20, kMaxLag = 64, kMaxSmooth = 1023;
constexpr uint64_t kMaxBlocks = 1ull << 20;
constexpr double kTwo32 = 4294967296.0, kPi = 3.14159265358979323846;

using Record = aptgpu_afc_record;  // {pw, phase0, step_re, step_im}
static_assert(sizeof(Record) == 16, "aptgpu_afc_record is 16 bytes");

// What the settings come to, once (design_of, apt_afc.cpp).  Plain data: the kernels take it by value.
struct Design {
    uint32_t B = 0, log2_B = 0, L = 0, W = 0;
    uint32_t pw_base = 0, fs = 0;
    double max_offset_hz = 0., min_coherence = 0.;
};

APT_FM_HD uint64_t blocks_of(uint64_t n_frames, uint32_t log2_B)
{
    return (n_frames + ((1ull << log2_B) - 1u)) >> log2_B;
}

// ---- stage A: one component as the integer the sums are made of
template <int FMT>
APT_FM_HD int32_t int_component(uint32_t raw)
{
    if constexpr (FMT == APTGPU_IQ_U8)
        return 2 * static_cast<int32_t>(raw & 0xFFu) - 255;
    else if constexpr (FMT == APTGPU_IQ_S8)
        return static_cast<int8_t>(raw & 0xFFu);
    else
        return static_cast<int16_t>(raw & 0xFFFFu);
}

// The three running sums of a block: int64 for the integer formats (every product pair widened first: 2 * 32768^2 is
// already past int32), f64 for F32.
template <int FMT>
struct Sums {
    using T = std::conditional_t<FMT == APTGPU_IQ_F32, double, int64_t>;
    T re = 0, im = 0, en = 0;
    // frame (i0, q0) is x[i]; energy alone
    APT_FM_HD void energy(T i0, T q0) { en += i0 * i0 + q0 * q0; }
    // ... and (i1, q1) is x[i + L]
    APT_FM_HD void lagged(T i0, T q0, T i1, T q1)
    {
        re += i1 * i0 + q1 * q0;
        im += q1 * i0 - i1 * q0;
    }
};
template <int FMT>
APT_FM_HD typename Sums<FMT>::T sum_component(uint32_t raw)
{
    if constexpr (FMT == APTGPU_IQ_F32)
        return static_cast<double>(apt::fm::component<APTGPU_IQ_F32>(raw));
    else
        return int_component<FMT>(raw);
}

// ---- stage B.  Everything is f64, rounded product by product and sum by sum (both sides are built without contraction).
struct Estimate {
    double coherence;  // NaN where the window's sums are not finite
    uint32_t est;      // pw_base + rel (meaningless unless finite)
    bool good;
};
APT_FM_HD bool finite64(double v) { return v - v == 0.; }

// the window sums of block b (ascending block order from a zero accumulator) -> its estimate
APT_FM_HD Estimate estimate_block(const double *sums, uint64_t nb, uint64_t b, const Design &d)
{
    const uint64_t half = d.W / 2u;
    const uint64_t lo = b >= half ? b - half : 0, hi = b + half < nb ? b + half : nb - 1;
    double rre = 0., rim = 0., e = 0.;
    for (uint64_t j = lo; j <= hi; ++j) {
        rre += sums[3 * j];
        rim += sums[3 * j + 1];
        e += sums[3 * j + 2];
    }
    Estimate r{0., d.pw_base, false};
    if (e != 0.) r.coherence = sqrt(rre * rre + rim * rim) / e;  // (NaN == 0. is false)
    if (!(finite64(rre) && finite64(rim) && finite64(e))) return r;
    const double turns = atan2(rim, rre) / (2. * kPi);
    const uint32_t q = static_cast<uint32_t>(static_cast<int64_t>(llrint(turns * kTwo32)));
    const int32_t dq = static_cast<int32_t>(q - d.L * d.pw_base);
    const int64_t rel = static_cast<int64_t>(llround(static_cast<double>(dq) / static_cast<double>(d.L)));
    r.est = d.pw_base + static_cast<uint32_t>(rel);
    const double off = fabs(static_cast<double>(rel)) * static_cast<double>(d.fs) / kTwo32;
    r.good = r.coherence >= d.min_coherence && off <= d.max_offset_hz;
    return r;
}
// coherence as it is returned: f32, one NaN
APT_FM_HD float coherence_out(double c)
{
    if (c != c) {
#if defined(__HIP_DEVICE_COMPILE__)
        return __uint_as_float(0x7FC00000u);
#else
        const uint32_t bits = 0x7FC00000u;
        float v;
        std::memcpy(&v, &bits, sizeof v);
        return v;
#endif
    }
    return static_cast<float>(c);
}
// design_of's step of a phase increment (apt_fm.cpp): f64 cos / -sin, rounded to f32
APT_FM_HD Record record_of(uint32_t pw, uint32_t phase0)
{
    const double t1 = static_cast<double>(static_cast<int32_t>(pw)) * (kPi / 2147483648.);
    return Record{pw, phase0, static_cast<float>(cos(t1)), static_cast<float>(-sin(t1))};
}

// ---- the host side (apt_afc.cpp)
void default_settings(aptgpu_afc_settings *s);
// Every refusal of the definition's settings table, on the host; throws Error{Invalid} naming the field.
Design design_of(const apt::fm::Design &fm, float deviation_hz, const aptgpu_afc_settings *s);
// nb of a recording; throws Error{Invalid} above 2^20
uint64_t checked_blocks(const Design &d, uint64_t n_frames);
// The twin.  sums: 3 nb doubles {re, im, en} per block.
void sums_host(const apt::fm::Design &fm, const Design &d, const void *iq, size_t n_frames, double *sums);
void table_host(const Design &d, const double *sums, uint64_t nb, Record *table, float *coherence, uint8_t *good);
void tracked_host(const apt::fm::Design &fm, const Design &d, const void *iq, size_t n_frames, const Record *table,
                  float *audio);

}  // namespace apt::afc

#if defined(__HIPCC__)
namespace apt::gpu {

struct AfcRecording {
    const uint8_t *iq;
    uint64_t n_frames;
    double *sums;                // 3 nb
    apt::afc::Record *table;     // nb
    float *coherence;            // nb
    uint8_t *good;               // nb
};
struct AfcBatch {
    AfcRecording r[apt::fm::kMaxBatch];
};
struct AfcTables {
    const apt::afc::Record *table[apt::fm::kMaxBatch];
    uint32_t log2_B;
};
// stage A: grid (blocks of the longest recording, count)
void afc_sums(hipStream_t stream, int format, bool swap, const apt::afc::Design &d, const AfcBatch &batch, int count,
              uint32_t max_blocks);
// stage B: one workgroup per recording
void afc_table(hipStream_t stream, const apt::afc::Design &d, const AfcBatch &batch, int count);
// stage C (apt_kernels_fm_tracked.hip): k_fm's launch with the phase of every run taken from the recording's table
void fm_demodulate_tracked(hipStream_t stream, int format, const apt::fm::Tile &tile, const FmBatch &batch,
                           const AfcTables &tables, int count, uint32_t max_tiles, const FmParams &p);
void fm_tracked_prepare(int format, const apt::fm::Tile &tile);

}  // namespace apt::gpu
#endif
