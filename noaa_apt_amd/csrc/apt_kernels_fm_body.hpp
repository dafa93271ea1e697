// apt_kernels_fm_body.hpp — the one text of the FM tile: load / filter / discriminate over a frame source, for k_fm
// (apt_kernels_fm.hip: one recording) and k_fm_stream (apt_kernels_fm_stream.hip: carry ++ chunk).  Both objects are
// built with -ffp-contract=fast; convert, cmul, the phasor, the tap loop and discriminate exist once, here, so that
// both kernels contract and order them alike.
//
// The phasors of a run come from a phase policy: UniformPhase is §4b (k_fm, k_fm_stream), TablePhase the tracked
// demodulator of §4b' (apt_kernels_fm_tracked.hip).
//
// A source states where its frame 0 stands on the absolute frame axis (base(): the phase of frame i is
// (uint32) i * pw and the runs of 8 start at multiples of 8 of that axis), how many frames it has, and how the run of
// 8 frames at an absolute multiple of 8 is fetched: 16 raw component words, zero for frames outside the source.
#pragma once

#include "apt_kernels_fm.hpp"

namespace apt::gpu::fm_body {

using apt::fm::Cx;
using apt::fm::kRun;

template <int FMT>
inline constexpr uint32_t kComponentBytes = FMT == APTGPU_IQ_S16 ? 2u : FMT == APTGPU_IQ_F32 ? 4u : 1u;

// a whole run from one, two or four 16-byte loads at p (16-byte aligned)
template <int FMT>
__device__ __forceinline__ void load_wide(const uint8_t *__restrict__ p, uint32_t (&raw)[2 * kRun])
{
    constexpr uint32_t cb = kComponentBytes<FMT>;
    constexpr int kWide = static_cast<int>(2u * cb * kRun / 16u);
    uint32_t w[4 * kWide];
#pragma unroll
    for (int k = 0; k < kWide; ++k) {
        const uint4 q = reinterpret_cast<const uint4 *>(p)[k];
        w[4 * k] = q.x;
        w[4 * k + 1] = q.y;
        w[4 * k + 2] = q.z;
        w[4 * k + 3] = q.w;
    }
#pragma unroll
    for (int k = 0; k < 2 * kRun; ++k) {
        if constexpr (cb == 1u)
            raw[k] = (w[k / 4] >> (8 * (k % 4))) & 0xFFu;
        else if constexpr (cb == 2u)
            raw[k] = (w[k / 2] >> (16 * (k % 2))) & 0xFFFFu;
        else
            raw[k] = w[k];
    }
}

// component k of the frames at p
template <int FMT>
__device__ __forceinline__ uint32_t load_component(const uint8_t *__restrict__ p, int k)
{
    constexpr uint32_t cb = kComponentBytes<FMT>;
    if constexpr (cb == 1u)
        return p[k];
    else if constexpr (cb == 2u)
        return reinterpret_cast<const uint16_t *>(p)[k];
    else
        return reinterpret_cast<const uint32_t *>(p)[k];
}

// One recording whose frame 0 is absolute frame 0.
struct OneSegment {
    const uint8_t *iq;
    uint64_t n_frames;
    bool aligned16;
    __device__ __forceinline__ OneSegment(const uint8_t *p, uint64_t n)
        : iq(p), n_frames(n), aligned16((reinterpret_cast<uintptr_t>(p) & 15u) == 0)
    {
    }
    __device__ __forceinline__ uint64_t base() const { return 0; }
    __device__ __forceinline__ uint64_t frames() const { return n_frames; }
    template <int FMT>
    __device__ __forceinline__ void load_run(uint64_t i0, uint32_t (&raw)[2 * kRun]) const
    {
        const uint8_t *p = iq + i0 * (2u * kComponentBytes<FMT>);
        if (aligned16 && i0 + kRun <= n_frames) {
            load_wide<FMT>(p, raw);
        } else {
#pragma unroll
            for (int k = 0; k < 2 * kRun; ++k) {
                uint32_t v = 0;
                if (i0 + static_cast<uint64_t>(k / 2) < n_frames) v = load_component<FMT>(p, k);
                raw[k] = v;
            }
        }
    }
};

// The virtual recording carry ++ chunk of a stream's push, read in place.  Its frame 0 is absolute frame `first`; the
// carry's slot 0 holds absolute frame first - first % 8 (the slots in front of frame 0 are stale and never used), so a
// run inside the carry is 16-byte aligned.  The chunk begins at absolute frame first + n_carry.
struct TwoSegment {
    const uint8_t *carry, *chunk;
    uint64_t first, n_total;
    uint32_t n_carry;
    __device__ __forceinline__ uint64_t base() const { return first; }
    __device__ __forceinline__ uint64_t frames() const { return n_total; }
    template <int FMT>
    __device__ __forceinline__ void load_run(uint64_t i0, uint32_t (&raw)[2 * kRun]) const
    {
        constexpr uint32_t fb = 2u * kComponentBytes<FMT>;  // bytes of a frame
        const int64_t r = static_cast<int64_t>(i0 - first);  // the run's first frame in the virtual recording: >= -7
        const int64_t nc = n_carry, n = static_cast<int64_t>(n_total);
        const int64_t lead = static_cast<int64_t>(first & 7u);  // the carry's slot of frame 0
        const uint8_t *pc = carry + (r + lead) * fb;            // (r + lead >= 0: i0 is at or behind slot 0)
        const uint8_t *px = chunk + (r - nc) * fb;              // (dereferenced for frames of the chunk only)
        if (r + kRun <= nc) {
            load_wide<FMT>(pc, raw);
        } else if (r >= nc && r + kRun <= n && (reinterpret_cast<uintptr_t>(px) & 15u) == 0) {
            load_wide<FMT>(px, raw);
        } else {  // across the seam, at either end, or a chunk whose runs are not 16-byte aligned
#pragma unroll
            for (int k = 0; k < 2 * kRun; ++k) {
                const int64_t f = r + k / 2;
                uint32_t v = 0;
                if (f >= 0 && f < nc)
                    v = load_component<FMT>(pc, k);
                else if (f >= nc && f < n)
                    v = load_component<FMT>(px, k);
                raw[k] = v;
            }
        }
    }
};

// Where the phasors of the run of 8 at absolute frame i0 come from: the first one and the step to each next.
struct RunPhasors {
    Cx first, step;
};
// §4b: one increment for the whole recording, the phase of frame i is (uint32) i * pw
struct UniformPhase {
    __device__ __forceinline__ RunPhasors run(uint64_t i0, const FmParams &P) const
    {
        return RunPhasors{apt::fm::phasor_of_phase(static_cast<uint32_t>(i0) * P.pw), Cx{P.step_re, P.step_im}};
    }
};
// §4b' stage C: one record {pw, phase0, step} per block of 2^log2_block frames (a run of 8 lies inside one block)
struct TablePhase {
    const aptgpu_afc_record *table;
    uint32_t log2_block;
    __device__ __forceinline__ RunPhasors run(uint64_t i0, const FmParams &) const
    {
        const uint4 r = *reinterpret_cast<const uint4 *>(table + (i0 >> log2_block));  // one 16-byte load
        const uint32_t in_block = static_cast<uint32_t>(i0) & ((1u << log2_block) - 1u);
        return RunPhasors{apt::fm::phasor_of_phase(r.y + in_block * r.x), Cx{__uint_as_float(r.z), __uint_as_float(r.w)}};
    }
};

// The tile of workgroup `block`: nv consecutive v[m] of the source from m0 = block (P.nv - 1) on, audio[m0 ...] out.
template <int FMT, bool MIX, int VPT, class Source, class Phase = UniformPhase>
__device__ __forceinline__ void fm_tile(const Source &src, float *__restrict__ audio, const FmParams &P, float2 *tile,
                                        uint32_t block, const Phase &phase = Phase{})
{
    const uint32_t T = P.T, D = P.D, R = P.R;
    const uint64_t n_frames = src.frames();
    if (n_frames < T) return;
    const uint64_t n_v = (n_frames - T) / D + 1;  // M
    const uint64_t m0 = static_cast<uint64_t>(block) * (P.nv - 1);
    if (m0 + 1 >= n_v) return;  // no output left (uniform over the workgroup)
    const uint32_t nv = static_cast<uint32_t>(n_v - m0 < P.nv ? n_v - m0 : P.nv);  // >= 2
    const uint64_t s = src.base() + m0 * D;                                        // the tile's first frame, absolute
    const uint32_t frames = (nv - 1) * D + T;                                      // all inside the source
    const uint32_t tid = threadIdx.x, threads = blockDim.x;

    // ---- load: runs of 8 by absolute index
    {
        const uint64_t g0 = s / kRun;
        const uint32_t runs = static_cast<uint32_t>((s + frames - 1) / kRun - g0) + 1;
        const bool swap = P.swap != 0;
        for (uint32_t g = tid; g < runs; g += threads) {
            const uint64_t i0 = (g0 + g) * kRun;
            uint32_t raw[2 * kRun];
            src.template load_run<FMT>(i0, raw);
            Cx ph{1.f, 0.f}, step{1.f, 0.f};
            if constexpr (MIX) {
                const RunPhasors rp = phase.run(i0, P);
                ph = rp.first;
                step = rp.step;
            }
            // local index of the run's first frame (negative: frames in front of the tile, dropped)
            const int64_t l0 = static_cast<int64_t>(i0) - static_cast<int64_t>(s);
            uint32_t row = 0, col = 0;
            if (l0 > 0) {
                col = static_cast<uint32_t>(l0) / D;
                row = static_cast<uint32_t>(l0) - col * D;
            }
#pragma unroll
            for (int k = 0; k < kRun; ++k) {
                const float ci = apt::fm::component<FMT>(raw[2 * k]), cq = apt::fm::component<FMT>(raw[2 * k + 1]);
                Cx x{swap ? cq : ci, swap ? ci : cq};
                if constexpr (MIX) {
                    x = apt::fm::cmul(x, ph);
                    ph = apt::fm::cmul(ph, step);
                }
                const int64_t l = l0 + k;
                if (l >= 0 && l < static_cast<int64_t>(frames)) {
                    tile[apt::fm::tile_index(row, col, R)] = make_float2(x.re, x.im);
                    if (++row == D) {
                        row = 0;
                        ++col;
                    }
                }
            }
        }
    }
    __syncthreads();

    // ---- filter: thread c, columns c + r * blockDim.x
    uint32_t c[VPT];
    float re[VPT], im[VPT];
#pragma unroll
    for (int r = 0; r < VPT; ++r) {
        const uint32_t cc = tid + static_cast<uint32_t>(r) * threads;
        c[r] = cc < nv ? cc : nv - 1;  // (lanes past the tile's v repeat its last one; their sums are dropped)
        re[r] = 0.f;
        im[r] = 0.f;
    }
    {
        const float *__restrict__ hr = P.taps_rev;
        const uint32_t *__restrict__ off = P.offsets;
        auto tap = [&](float h, uint32_t o) {
#pragma unroll
            for (int r = 0; r < VPT; ++r) {
                const float2 u = tile[o + c[r]];
                re[r] += h * u.x;
                im[r] += h * u.y;
            }
        };
        uint32_t j = 0;
        for (; j + 8 <= T; j += 8) {
            float h[8];
            uint32_t o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                h[k] = hr[j + k];
                o[k] = off[j + k];
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) tap(h[k], o[k]);
        }
        for (; j < T; ++j) tap(hr[j], off[j]);
    }
    __syncthreads();

    // ---- discriminate
#pragma unroll
    for (int r = 0; r < VPT; ++r) {
        const uint32_t cc = tid + static_cast<uint32_t>(r) * threads;
        if (cc < nv) tile[cc] = make_float2(re[r], im[r]);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < VPT; ++r) {
        const uint32_t cc = tid + static_cast<uint32_t>(r) * threads;
        if (cc + 1 < nv) {
            const float2 v0 = tile[cc], v1 = tile[cc + 1];
            audio[m0 + cc] = apt::fm::discriminate(Cx{v0.x, v0.y}, Cx{v1.x, v1.y}, P.gain);
        }
    }
}

}  // namespace apt::gpu::fm_body
