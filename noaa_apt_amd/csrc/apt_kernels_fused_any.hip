// apt_kernels_fused_any.hip — fused front end for ANY (input rate, profile): resample ->
// envelope -> low-pass -> sync correlation (+ group maxima) in one launch, all run-time
// parameters.  Used when no compile-time specialisation of k_fused (apt_kernels_fused.hip)
// matches: 11 025 Hz (L = 832) and 44 100 Hz (L = 208) recordings, the fast / slow profiles,
// odd rates.  Same outputs, same bit-exact arithmetic (separately rounded products and sums in
// the reference's order); about 2x the instructions of the specialised kernel because nothing
// is packed or unrolled against compile-time tap positions.
//
// One workgroup = one tile of KT = NTHR*KPT work samples:
//
//   tile index:   0 ......... PRE ........................ PRE+OWN ....... KT
//                 | history    | owned: F, C, GM go to HBM  | look-ahead   |
//                 | (low-pass) |                            | (sync frame) |
//
//   stage 0  polyphase table (phase-major, row stride odd -> conflict-free) and the input
//            tile -> LDS, coalesced
//   stage 1  R[k] = sum_i coeff[p + i*l] * x[x0 + i]      (dsp.rs:252-263), one output per
//            thread and step, taps and samples from LDS
//   stage 2  D[k] = envelope(R[k-1], R[k])                (dsp.rs:369-377)
//   stage 3  F[k] = sum_{j<T2} D[k-j] * h[j]              (dsp.rs:396-404), KPT consecutive
//            outputs per thread: a sliding register window cuts LDS reads per tap to 1/KPT
//   stage 4  bounds of max C over groups of 52 positions, C[k] = sum_{j<G} +-F[k+j] (decode.rs:225-233): the
//            correlation from pulse sums (apt_sync_corr.hpp) widened by the rounding bound slack * sum|F|; the
//            picker evaluates the exact chain where it matters (apt_kernels_sync.hip)
//   stage 5  owned F -> HBM (coalesced), GM[g] = [lo, hi]
//
// LDS layout of A and B: logical index i lives at i + i/KPT (one pad word after every KPT), so a
// thread's block of KPT consecutive outputs starts at an ODD multiple-of-words stride from its
// neighbour's: the register-blocked stages read conflict-free (unpadded, a stride of 8 floats
// put 64 lanes on 4 banks and made stage 4 three times slower than everything else together).
//
// Why zero-filling is exact: a running sum that starts at +0.0 can never be -0.0 (x + y is
// -0.0 only if both are), so adding the +-0.0 product of a zero-filled sample (inputs at or
// past n, which the reference skips, dsp.rs:257; D[k <= 0], which the `i > j` guard of
// dsp.rs:399 excludes and which is 0.0 anyway) leaves every bit unchanged.
#include "apt_kernels_fused_any_launch.hpp"

#include <type_traits>

#pragma clang fp contract(off)

namespace apt::gpu {

bool fused_any_front_end(hipStream_t s, uint32_t l, uint32_t m, uint32_t t1, uint32_t t2, uint32_t pw, bool pcm16,
                         const CallArgs &call, const SlotPtrs *d_slots, uint64_t max_w, const float *table,
                         const float *h2, const float *h2p, float cosphi2, float sinphi, float inv_sinphi, bool want_gm,
                         float gm_slack_scale)
{
    AnyCandidate c;
    AnyGeom g;
    size_t lds;
    if (call.count == 0) return true;
    if (!any_choose(l, m, t1, t2, pw, &c, &g, &lds)) return false;
    g.gm_slack_scale = gm_slack_scale;
    if (pcm16)
        for (uint32_t i = 0; i < call.count; ++i)
            if (reinterpret_cast<uintptr_t>(call.rec[i].x) & 1u) return false;
    const int prof = (t2 == 37 && pw == 3) ? 1 : (t2 == 43 && pw == 4) ? 2 : (t2 == 61 && pw == 5) ? 3 : 0;
    if (c.nthr == 256 && c.kpt == 8)
        fused_any_launch<256, 8>(s, call, d_slots, max_w, pcm16, table, h2, h2p, cosphi2, sinphi, inv_sinphi, want_gm, g, lds, prof);
    else if (c.nthr == 1024 && c.kpt == 8)
        fused_any_launch<1024, 8>(s, call, d_slots, max_w, pcm16, table, h2, h2p, cosphi2, sinphi, inv_sinphi, want_gm, g, lds, prof);
    else if (c.nthr == 1024 && c.kpt == 4)
        fused_any_launch<1024, 4>(s, call, d_slots, max_w, pcm16, table, h2, h2p, cosphi2, sinphi, inv_sinphi, want_gm, g, lds, prof);
    else if (c.nthr == 256 && c.kpt == 4)
        fused_any_launch<256, 4>(s, call, d_slots, max_w, pcm16, table, h2, h2p, cosphi2, sinphi, inv_sinphi, want_gm, g, lds, prof);
    else
        return false;
    return true;
}

}  // namespace apt::gpu
