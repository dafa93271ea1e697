// apt_fm.cpp — the FM demodulator on the CPU: the checks and the design every entry point shares, and the definition of
// apt_kernels_fm.hpp in plain C++ (aptgpu_fm_demodulate_host), which the kernel is tested against and which a
// stand-alone program can call without a GPU.
#include "apt_kernels_fm.hpp"

#include <cstdio>

#include "apt_kernels_fm_stream.hpp"

namespace apt::fm {

namespace {
[[noreturn]] void refuse(const std::string &text) { throw Error{ErrorKind::Invalid, "aptgpu_fm_settings: " + text}; }

bool positive(float v) { return std::isfinite(v) && v > 0.f; }

// where the phasors come from: the design's one increment (§4b) ...
struct UniformPhase {
    const Design &d;
    bool mix() const { return d.pw != 0; }
    Cx first(uint64_t i0) const { return phasor_of_phase(static_cast<uint32_t>(i0) * d.pw); }
    Cx step(uint64_t) const { return d.step; }
};
// ... or a table of one record per block of 2^log2_block frames (§4b', apt_afc.cpp): always mixed
struct TablePhase {
    const aptgpu_afc_record *table;
    uint32_t log2_block;
    bool mix() const { return true; }
    const aptgpu_afc_record &of(uint64_t i0) const { return table[i0 >> log2_block]; }
    Cx first(uint64_t i0) const
    {
        const aptgpu_afc_record &r = of(i0);
        return phasor_of_phase(r.phase0 + static_cast<uint32_t>(i0 & ((1ull << log2_block) - 1u)) * r.pw);
    }
    Cx step(uint64_t i0) const { return Cx{of(i0).step_re, of(i0).step_im}; }
};

// frame 0 of iq is absolute frame `base`: the phase and the runs of 8 are the absolute axis's
template <int FMT, class Phase>
void run(const Design &d, uint64_t base, const uint8_t *iq, size_t n_frames, float *audio, const Phase &phase)
{
    const size_t n_out = out_len(d, n_frames);
    if (!n_out) return;
    const size_t T = d.T, D = d.D, m_count = n_out + 1;
    const size_t used = (m_count - 1) * D + T;  // frames any window reads
    std::vector<Cx> u(used);
    const int a = d.swap ? 1 : 0;
    const size_t cb = component_bytes(FMT);
    const uint64_t end = base + used;
    const bool mix = phase.mix();
    for (uint64_t i0 = base - base % kRun; i0 < end; i0 += kRun) {
        Cx ph = mix ? phase.first(i0) : Cx{1.f, 0.f};
        const Cx step = mix ? phase.step(i0) : Cx{1.f, 0.f};
        for (uint64_t j = i0; j < i0 + kRun && j < end; ++j) {
            if (j >= base) {
                const size_t i = static_cast<size_t>(j - base);
                uint32_t raw[2];
                for (int k = 0; k < 2; ++k) {
                    raw[k] = 0;
                    std::memcpy(&raw[k], iq + (2 * i + static_cast<size_t>(k)) * cb, cb);  // little endian
                }
                const Cx x{component<FMT>(raw[a]), component<FMT>(raw[1 - a])};
                u[i] = mix ? cmul(x, ph) : x;
            }
            if (mix) ph = cmul(ph, step);
        }
    }
    Cx prev{};
    for (size_t m = 0; m < m_count; ++m) {
        float re = 0.f, im = 0.f;
        const Cx *w = u.data() + m * D;
        for (size_t j = 0; j < T; ++j) {
            re += d.taps_rev[j] * w[j].re;
            im += d.taps_rev[j] * w[j].im;
        }
        const Cx v{re, im};
        if (m) audio[m - 1] = discriminate(prev, v, d.gain);
        prev = v;
    }
}
}  // namespace

Design design_of(const aptgpu_fm_settings *s)
{
    if (!s) refuse("settings are required");
    if (s->struct_size < sizeof(aptgpu_fm_settings)) refuse("struct_size not set");
    if (s->format < APTGPU_IQ_U8 || s->format > APTGPU_IQ_F32) refuse("format is not an APTGPU_IQ_* value");
    if (s->flags & ~APTGPU_FM_SWAP_IQ) refuse("flags has an unknown bit");
    if (s->sample_rate_hz == 0) refuse("sample_rate_hz must be positive");
    if (s->decimation == 0 || s->decimation > kMaxDecimation) refuse("decimation must be 1 ... 4096");
    if (s->sample_rate_hz % s->decimation != 0)
        refuse("sample_rate_hz is not a multiple of decimation (the output rate must be a whole number of Hz)");
    if (!positive(s->channel_cutout_hz)) refuse("channel_cutout_hz must be finite and positive");
    if (!positive(s->channel_delta_hz)) refuse("channel_delta_hz must be finite and positive");
    if (!positive(s->deviation_hz)) refuse("deviation_hz must be finite and positive");
    if (!std::isfinite(s->channel_atten) || !(s->channel_atten > 8.f)) refuse("channel_atten must be finite and above 8 dB");
    const double fs = static_cast<double>(s->sample_rate_hz);
    if (!std::isfinite(s->shift_hz) || std::fabs(s->shift_hz) > fs / 2.) refuse("shift_hz must be finite and within fs / 2");
    Design d;
    d.format = s->format;
    d.swap = (s->flags & APTGPU_FM_SWAP_IQ) != 0;
    d.fs = s->sample_rate_hz;
    d.D = s->decimation;
    d.fs_out = d.fs / d.D;
    if (static_cast<double>(s->channel_cutout_hz) + static_cast<double>(s->channel_delta_hz) / 2. >
        static_cast<double>(d.fs_out) / 2.)
        refuse("channel_cutout_hz + channel_delta_hz / 2 is above half the output rate (the filter would alias)");
    const Freq cutout = Freq::hz(s->channel_cutout_hz, Rate::hz(s->sample_rate_hz));
    const Freq delta = Freq::hz(s->channel_delta_hz, Rate::hz(s->sample_rate_hz));
    // the window's length before it is built (kaiser(), apt_host.cpp): a transition this narrow would allocate it first
    const double est = (static_cast<double>(s->channel_atten) - 8.) / (2.285 * static_cast<double>(delta.get_rad()));
    if (!(est <= static_cast<double>(kMaxTaps) + 2.)) refuse("channel_delta_hz and channel_atten need more than 4096 taps");
    d.taps = Lowpass(cutout, s->channel_atten, delta).design();
    if (d.taps.empty() || d.taps.size() > kMaxTaps) refuse("channel_delta_hz and channel_atten need more than 4096 taps");
    d.T = static_cast<uint32_t>(d.taps.size());
    d.taps_rev.assign(d.taps.rbegin(), d.taps.rend());
    d.pw = static_cast<uint32_t>(static_cast<int64_t>(std::llround(s->shift_hz / fs * 4294967296.)));
    d.shift_used = static_cast<double>(static_cast<int32_t>(d.pw)) * fs / 4294967296.;
    const double t1 = static_cast<double>(static_cast<int32_t>(d.pw)) * (3.14159265358979323846 / 2147483648.);
    d.step = Cx{static_cast<float>(std::cos(t1)), static_cast<float>(-std::sin(t1))};
    d.deviation_hz = s->deviation_hz;
    d.gain = static_cast<float>(static_cast<double>(d.fs_out) /
                                (2. * 3.14159265358979323846 * static_cast<double>(s->deviation_hz)));
    return d;
}

void run_host_based(const Design &d, uint64_t base, const void *iq, size_t n_frames, float *audio)
{
    const uint8_t *p = static_cast<const uint8_t *>(iq);
    const UniformPhase ph{d};
    switch (d.format) {
    case APTGPU_IQ_U8: return run<APTGPU_IQ_U8>(d, base, p, n_frames, audio, ph);
    case APTGPU_IQ_S8: return run<APTGPU_IQ_S8>(d, base, p, n_frames, audio, ph);
    case APTGPU_IQ_S16: return run<APTGPU_IQ_S16>(d, base, p, n_frames, audio, ph);
    default: return run<APTGPU_IQ_F32>(d, base, p, n_frames, audio, ph);
    }
}

void run_host_tracked(const Design &d, const void *iq, size_t n_frames, const aptgpu_afc_record *table,
                      uint32_t log2_block, float *audio)
{
    const uint8_t *p = static_cast<const uint8_t *>(iq);
    const TablePhase ph{table, log2_block};
    switch (d.format) {
    case APTGPU_IQ_U8: return run<APTGPU_IQ_U8>(d, 0, p, n_frames, audio, ph);
    case APTGPU_IQ_S8: return run<APTGPU_IQ_S8>(d, 0, p, n_frames, audio, ph);
    case APTGPU_IQ_S16: return run<APTGPU_IQ_S16>(d, 0, p, n_frames, audio, ph);
    default: return run<APTGPU_IQ_F32>(d, 0, p, n_frames, audio, ph);
    }
}

void run_host(const Design &d, const void *iq, size_t n_frames, float *audio) { run_host_based(d, 0, iq, n_frames, audio); }

}  // namespace apt::fm
