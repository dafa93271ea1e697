// apt_fm_stream.cpp — the streaming FM demodulator on the CPU: the checks every entry point shares and the twin
// (apt_kernels_fm_stream.hpp), which a stand-alone program can call without a GPU (tools/sanitize/fm_stream_host_main.cpp).
#include "apt_kernels_fm_stream.hpp"

#include <algorithm>

namespace apt::fm {

StreamDesign design_stream(const aptgpu_fm_settings *fm, const aptgpu_fm_stream_settings *ss)
{
    StreamDesign d;
    d.fm = design_of(fm);  // everything the one-shot refuses
    if (ss) {
        if (ss->struct_size < sizeof(aptgpu_fm_stream_settings))
            throw Error{ErrorKind::Invalid, "aptgpu_fm_stream_settings: struct_size not set"};
        if (ss->max_push_frames == 0 || ss->max_push_frames > (1u << 28))
            throw Error{ErrorKind::Invalid, "aptgpu_fm_stream_settings: max_push_frames must be 1 ... 2^28"};
        d.max_push_frames = ss->max_push_frames;
        d.first_frame = ss->first_frame;
    }
    return d;
}

void check_push(const StreamDesign &d, uint64_t n_pushed, const void *iq, size_t n_frames, const void *audio, size_t audio_cap,
                const char *iq_name, const char *audio_name)
{
    const uint64_t n_out = stream_out_len(d.fm, n_pushed + n_frames) - stream_out_len(d.fm, n_pushed);
    const std::string in = iq_name, out = audio_name ? audio_name : "";
    if (n_frames && !iq) throw Error{ErrorKind::Invalid, "fm stream: " + in + " is null"};
    if (n_frames && reinterpret_cast<uintptr_t>(iq) % component_bytes(d.fm.format) != 0)
        throw Error{ErrorKind::Invalid, "fm stream: " + in + " is not aligned to one component"};
    if (!audio_name) return;  // (the coupling: the audio goes to a scratch of its own)
    if (n_out && !audio) throw Error{ErrorKind::Invalid, "fm stream: " + out + " is null"};
    if (n_out && reinterpret_cast<uintptr_t>(audio) % sizeof(float) != 0)
        throw Error{ErrorKind::Invalid, "fm stream: " + out + " is not aligned to a float"};
    if (audio_cap < n_out) throw Error{ErrorKind::Invalid, "fm stream: audio_cap is below the output length"};
}

size_t HostFmStream::push(const void *iq, size_t n_frames, float *audio)
{
    const Design &d = d_.fm;
    const size_t fb = 2u * component_bytes(d.format);
    const uint8_t *src = static_cast<const uint8_t *>(iq);
    size_t done = 0, written = 0;
    while (done < n_frames) {
        const size_t seg = std::min<size_t>(n_frames - done, d_.max_push_frames);
        const uint64_t n0 = n_, n1 = n_ + seg;
        const uint64_t c0 = stream_carry_start(d, n0), c1 = stream_carry_start(d, n1);
        const size_t n_carry = static_cast<size_t>(n0 - c0);
        // the virtual recording carry ++ chunk: its frame 0 is stream frame c0
        work_.resize((n_carry + seg) * fb);
        if (n_carry) std::memcpy(work_.data(), carry_.data(), n_carry * fb);
        std::memcpy(work_.data() + n_carry * fb, src + done * fb, seg * fb);
        run_host_based(d, d_.first_frame + c0, work_.data(), n_carry + seg, audio + written);
        written += static_cast<size_t>(stream_out_len(d, n1) - stream_out_len(d, n0));
        const uint8_t *keep = work_.data() + static_cast<size_t>(c1 - c0) * fb;
        carry_.assign(keep, keep + static_cast<size_t>(n1 - c1) * fb);
        n_ = n1;
        done += seg;
    }
    return written;
}

}  // namespace apt::fm
