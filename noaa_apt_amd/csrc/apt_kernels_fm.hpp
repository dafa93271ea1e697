// apt_kernels_fm.hpp — the FM demodulator in front of the decode: an IQ recording in, audio at fs / D out
// (apt_kernels_fm.hip on the GPU, apt_fm.cpp on the CPU).  The reference reads audio only, so this is
// the definition (include/aptgpu.h states it in full; tests/np_fm_model.py in numpy f64).  The per-sample arithmetic
// is written once, here, for both sides; they differ only in the sincos of a run's first phasor and in atan2.
//
//  Convert  one component of a frame `as f32`, never scaled (u8: minus 127.5); SWAP_IQ exchanges I and Q.
//  Mix      u[i] = x[i] * e^{-j theta_i}, theta_i = 2 pi ((uint32) i * pw) / 2^32.  Frames are mixed in runs of 8
//           that start at multiples of 8 of the absolute index i: the run's first phasor comes from its integer phase,
//           each next one is the previous times e^{-j theta_1} (one complex multiply).  A frame's phasor so depends on
//           i alone: not on the tile, the recording's place in a batch or the pointer.
//  Filter   v[m] = sum_j hr[j] * u[m D + j], hr[j] = h[T - 1 - j], j ascending from a zero accumulator.
//  Discriminate  a[m] = g * atan2(Im p, Re p), p = v[m + 1] * conj(v[m]); 0 for p == 0; NaN where a component of
//           v[m] or v[m + 1] is not finite.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/aptgpu.h"
#include "apt_host.hpp"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define APT_FM_HD __host__ __device__ inline
#else
#define APT_FM_HD inline
#endif

namespace apt::fm {

constexpr uint32_t kMaxTaps = 4096, kMaxDecimation = 4096;
constexpr int kRun = 8;          // frames per phasor run (and per lane of the tile load)
constexpr int kMaxBatch = APTGPU_FM_MAX_BATCH;

struct Cx {
    float re, im;
};

// On the device the object is built with -ffp-contract=fast, under which `a b - c d` may be fused around either
// product, and which one the compiler takes has changed with the code around it.  The fused forms are therefore
// written out: the ones k_fm has always had (one rounding of a.re's product, the other product rounded first).
APT_FM_HD Cx cmul(Cx a, Cx b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return Cx{__fmaf_rn(a.re, b.re, -(a.im * b.im)), __fmaf_rn(a.re, b.im, a.im * b.re)};
#else
    return Cx{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
#endif
}

// bytes of one component
APT_FM_HD uint32_t component_bytes(int format)
{
    return format == APTGPU_IQ_S16 ? 2u : format == APTGPU_IQ_F32 ? 4u : 1u;
}

// one component from its raw bits (the low 8 / 16 / 32 of `raw`)
template <int FMT>
APT_FM_HD float component(uint32_t raw)
{
    if constexpr (FMT == APTGPU_IQ_U8) {
        return static_cast<float>(raw & 0xFFu) - 127.5f;
    } else if constexpr (FMT == APTGPU_IQ_S8) {
        return static_cast<float>(static_cast<int8_t>(raw & 0xFFu));
    } else if constexpr (FMT == APTGPU_IQ_S16) {
        return static_cast<float>(static_cast<int16_t>(raw & 0xFFFFu));
    } else {
        float v;
#if defined(__HIP_DEVICE_COMPILE__)
        v = __uint_as_float(raw);
#else
        std::memcpy(&v, &raw, sizeof v);
#endif
        return v;
    }
}

// e^{-j theta} of an integer phase (theta = 2 pi phase / 2^32): the one place besides atan2 where the sides differ
APT_FM_HD Cx phasor_of_phase(uint32_t phase)
{
#if defined(__HIP_DEVICE_COMPILE__)
    float s, c;
    sincospif(static_cast<float>(static_cast<int32_t>(phase)) * 4.656612873077393e-10f, &s, &c);  // * 2^-31
    return Cx{c, -s};
#else
    const double t = static_cast<double>(static_cast<int32_t>(phase)) * (3.14159265358979323846 / 2147483648.0);
    return Cx{static_cast<float>(std::cos(t)), static_cast<float>(-std::sin(t))};
#endif
}

APT_FM_HD bool finite32(float v) { return v - v == 0.f; }

APT_FM_HD float discriminate(Cx v0, Cx v1, float gain)
{
    if (!(finite32(v0.re) && finite32(v0.im) && finite32(v1.re) && finite32(v1.im))) {
#if defined(__HIP_DEVICE_COMPILE__)
        return __uint_as_float(0x7FC00000u);
#else
        return std::nanf("");
#endif
    }
#if defined(__HIP_DEVICE_COMPILE__)  // (fused as cmul is, for the same reason)
    const float re = __fmaf_rn(v1.re, v0.re, v1.im * v0.im);
    const float im = __fmaf_rn(v1.im, v0.re, -(v1.re * v0.im));
#else
    const float re = v1.re * v0.re + v1.im * v0.im;
    const float im = v1.im * v0.re - v1.re * v0.im;
#endif
    if (re == 0.f && im == 0.f) return 0.f;
    return gain * atan2f(im, re);
}

// What create() derives from the settings, once.
struct Design {
    int format = 0;
    bool swap = false;
    uint32_t fs = 0, fs_out = 0, D = 1, T = 0;
    uint32_t pw = 0;
    double shift_used = 0.;
    Cx step{1.f, 0.f};  // e^{-j theta_1}
    float gain = 0.f;   // fs_out / (2 pi deviation_hz)
    float deviation_hz = 0.f;
    Signal taps;        // h
    Signal taps_rev;    // hr[j] = h[T - 1 - j]
};

// Every refusal of the definition, on the host; throws Error{Invalid} naming the field.
Design design_of(const aptgpu_fm_settings *s);
inline size_t out_len(const Design &d, size_t n_frames)
{
    if (n_frames < d.T) return 0;
    const size_t m = (n_frames - d.T) / d.D + 1;
    return m - 1;
}
// The twin: plain C++.  iq: n_frames * 2 components; audio: out_len floats.
void run_host(const Design &d, const void *iq, size_t n_frames, float *audio);
// ... with the phase of every run of 8 from a table of one record per block of 2^log2_block frames (§4b', stage C);
// table: ceil(n_frames / 2^log2_block) records.  The mix is always made.
void run_host_tracked(const Design &d, const void *iq, size_t n_frames, const aptgpu_afc_record *table,
                      uint32_t log2_block, float *audio);

// The tile of one workgroup: nv consecutive v[m] (nv - 1 outputs), frames [m0 D, m0 D + (nv - 1) D + T) in LDS as
// D rows (the frame's phase, local index mod D) of R complex columns (local index / D); every 8 rows the image is
// skewed by one element (tile_index), which keeps the load's stores on distinct banks.
struct Tile {
    uint32_t nv, vpt, R, threads;
    size_t lds_bytes;
};
constexpr uint32_t kThreads = 256;       // at most; a tile of fewer v takes fewer waves
constexpr uint32_t kTileComplex = 8192;  // 64 KiB of float2
APT_FM_HD uint32_t tile_index(uint32_t row, uint32_t col, uint32_t R) { return row * R + (row >> 3) + col; }
inline Tile tile_of(uint32_t D, uint32_t T)
{
    const uint32_t halo = (T + D - 1) / D;                       // columns the taps reach past a v's own
    const uint32_t r_max = (kTileComplex - (D >> 3) - 1) / D;    // columns 64 KiB hold
    uint32_t nv = r_max > halo ? r_max - halo + 1 : 2;           // R = nv - 1 + halo <= r_max
    if (nv < 2) nv = 2;
    Tile t{};
    t.vpt = nv >= 4 * kThreads ? 4 : nv >= 2 * kThreads ? 2 : 1;
    t.nv = nv > t.vpt * kThreads ? t.vpt * kThreads : nv;
    t.threads = t.nv >= kThreads ? kThreads : (t.nv + 63u) / 64u * 64u;
    t.R = t.nv - 1 + halo;
    t.lds_bytes = (static_cast<size_t>(D) * t.R + (D >> 3) + 1u) * 8u;
    return t;
}
// where tap j reads, relative to a thread's column: frame j of the tile is at row j % D, column j / D
inline std::vector<uint32_t> tap_offsets(uint32_t D, uint32_t T, uint32_t R)
{
    std::vector<uint32_t> off(T);
    for (uint32_t j = 0; j < T; ++j) off[j] = tile_index(j % D, j / D, R);
    return off;
}

}  // namespace apt::fm

#if defined(__HIPCC__)
namespace apt::gpu {

struct FmRecording {
    const uint8_t *iq;
    float *audio;
    uint64_t n_frames;
};
struct FmBatch {
    FmRecording r[apt::fm::kMaxBatch];
};
struct FmParams {
    const float *taps_rev;
    const uint32_t *offsets;  // tap_offsets()
    uint32_t T, D, R, nv;
    uint32_t pw, swap;
    float step_re, step_im, gain;
};
// One launch for `count` recordings: grid (tiles of the longest, count).
void fm_demodulate(hipStream_t stream, int format, bool mix, const apt::fm::Tile &tile, const FmBatch &batch, int count,
                   uint32_t max_tiles, const FmParams &p);
// create(): a tile above 64 KiB (D rows that do not divide it well) needs the kernel's dynamic-LDS limit raised
void fm_prepare(int format, bool mix, const apt::fm::Tile &tile);

}  // namespace apt::gpu
#endif
