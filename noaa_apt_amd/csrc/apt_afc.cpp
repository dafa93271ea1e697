// apt_afc.cpp — AFC on the CPU: the checks and the design every entry point shares, and the definition of
// apt_kernels_afc.hpp in plain C++ (the *_host entry points of include/aptgpu.h §4b'), which the kernels are tested
// against and which a stand-alone program can call without a GPU.
#include "apt_kernels_afc.hpp"

namespace apt::afc {

namespace {
[[noreturn]] void refuse(const std::string &text) { throw Error{ErrorKind::Invalid, "aptgpu_afc_settings: " + text}; }

template <int FMT>
void sums_of(bool swap, const Design &d, const uint8_t *iq, size_t n, double *sums)
{
    const size_t cb = apt::fm::component_bytes(FMT);
    const int a = swap ? 1 : 0;
    auto frame = [&](size_t i, typename Sums<FMT>::T &ci, typename Sums<FMT>::T &cq) {
        uint32_t raw[2] = {0, 0};
        std::memcpy(&raw[0], iq + 2 * i * cb, cb);  // little endian
        std::memcpy(&raw[1], iq + (2 * i + 1) * cb, cb);
        ci = sum_component<FMT>(raw[a]);
        cq = sum_component<FMT>(raw[1 - a]);
    };
    const uint64_t nb = blocks_of(n, d.log2_B);
    for (uint64_t b = 0; b < nb; ++b) {
        const size_t lo = static_cast<size_t>(b) << d.log2_B;
        const size_t hi = lo + d.B < n ? lo + d.B : n;
        Sums<FMT> s;
        for (size_t i = lo; i < hi; ++i) {
            typename Sums<FMT>::T i0, q0, i1, q1;
            frame(i, i0, q0);
            s.energy(i0, q0);
            if (i + d.L < n) {
                frame(i + d.L, i1, q1);
                s.lagged(i0, q0, i1, q1);
            }
        }
        sums[3 * b] = static_cast<double>(s.re);
        sums[3 * b + 1] = static_cast<double>(s.im);
        sums[3 * b + 2] = static_cast<double>(s.en);
    }
}
}  // namespace

void default_settings(aptgpu_afc_settings *s)
{
    *s = aptgpu_afc_settings{};
    s->struct_size = sizeof(aptgpu_afc_settings);
    s->block_frames = 4096;
    s->lag = 0;
    s->smooth_blocks = 15;
    s->max_offset_hz = 15000.f;
    s->min_coherence = 0.05f;
}

Design design_of(const apt::fm::Design &fm, float deviation_hz, const aptgpu_afc_settings *s)
{
    if (!s) refuse("settings are required");
    if (s->struct_size < sizeof(aptgpu_afc_settings)) refuse("struct_size not set");
    const uint32_t B = s->block_frames;
    if (B < kMinBlock || B > kMaxBlock || (B & (B - 1u)) != 0) refuse("block_frames must be a power of two in 64 ... 2^20");
    if (s->lag > kMaxLag) refuse("lag must be 1 ... 64, or 0 for auto");
    if (s->smooth_blocks < 1 || s->smooth_blocks > kMaxSmooth || s->smooth_blocks % 2u == 0)
        refuse("smooth_blocks must be odd and in 1 ... 1023");
    if (!std::isfinite(s->max_offset_hz) || !(s->max_offset_hz > 0.f)) refuse("max_offset_hz must be finite and positive");
    if (!(s->min_coherence >= 0.f && s->min_coherence < 1.f)) refuse("min_coherence must be in [0, 1)");
    Design d;
    d.B = B;
    while ((1u << d.log2_B) < B) ++d.log2_B;
    d.W = s->smooth_blocks;
    d.fs = fm.fs;
    d.pw_base = fm.pw;
    d.max_offset_hz = static_cast<double>(s->max_offset_hz);
    d.min_coherence = static_cast<double>(s->min_coherence);
    d.L = s->lag;
    if (d.L == 0) {
        const double l = std::floor(static_cast<double>(fm.fs) / (4. * (d.max_offset_hz + static_cast<double>(deviation_hz))));
        d.L = l < 1. ? 1u : l > static_cast<double>(kMaxLag) ? kMaxLag : static_cast<uint32_t>(l);
    }
    return d;
}

uint64_t checked_blocks(const Design &d, uint64_t n_frames)
{
    const uint64_t nb = blocks_of(n_frames, d.log2_B);
    if (nb > kMaxBlocks) throw Error{ErrorKind::Invalid, "afc: n_frames has more than 2^20 blocks of block_frames"};
    return nb;
}

void sums_host(const apt::fm::Design &fm, const Design &d, const void *iq, size_t n_frames, double *sums)
{
    const uint8_t *p = static_cast<const uint8_t *>(iq);
    switch (fm.format) {
    case APTGPU_IQ_U8: return sums_of<APTGPU_IQ_U8>(fm.swap, d, p, n_frames, sums);
    case APTGPU_IQ_S8: return sums_of<APTGPU_IQ_S8>(fm.swap, d, p, n_frames, sums);
    case APTGPU_IQ_S16: return sums_of<APTGPU_IQ_S16>(fm.swap, d, p, n_frames, sums);
    default: return sums_of<APTGPU_IQ_F32>(fm.swap, d, p, n_frames, sums);
    }
}

void table_host(const Design &d, const double *sums, uint64_t nb, Record *table, float *coherence, uint8_t *good)
{
    std::vector<uint32_t> est(nb);
    std::vector<uint8_t> ok(nb);
    for (uint64_t b = 0; b < nb; ++b) {
        const Estimate e = estimate_block(sums, nb, b, d);
        est[b] = e.est;
        ok[b] = e.good ? 1 : 0;
        if (coherence) coherence[b] = coherence_out(e.coherence);
        if (good) good[b] = ok[b];
    }
    uint64_t first = nb;  // the first good block
    for (uint64_t b = 0; b < nb && first == nb; ++b)
        if (ok[b]) first = b;
    uint32_t held = first < nb ? est[first] : d.pw_base, phase0 = 0;
    for (uint64_t b = 0; b < nb; ++b) {
        if (ok[b]) held = est[b];
        table[b] = record_of(held, phase0);
        phase0 += d.B * held;
    }
}

void tracked_host(const apt::fm::Design &fm, const Design &d, const void *iq, size_t n_frames, const Record *table,
                  float *audio)
{
    apt::fm::run_host_tracked(fm, iq, n_frames, table, d.log2_B, audio);
}

}  // namespace apt::afc
