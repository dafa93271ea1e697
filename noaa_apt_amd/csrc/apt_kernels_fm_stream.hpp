// apt_kernels_fm_stream.hpp — the FM demodulator in streaming form (include/aptgpu.h §4b'): frames in
// by pushes of any size, exactly the one-shot's outputs out, each as soon as its last frame is in.
//
// The state is raw frames only.  With n frames pushed, M(n) = (n - T) / D + 1 (0 below T) and
// out_len(n) = max(M(n) - 1, 0), the carry holds the frames [c0(n), n), c0(n) = out_len(n) * D: fewer than T + D.
// A push from n0 to n1 runs the one-shot's tile over the virtual recording carry ++ chunk, whose frame 0 is stream
// frame c0(n0) (absolute frame first_frame + c0(n0): the phase and the run grid are the absolute axis's), and returns
// its out_len(n1) - out_len(n0) outputs; the v it shares with the previous push is computed again from the same frames.
// Everything below is host arithmetic on n alone (apt_kernels_fm_stream.hip: the kernel, apt_fm_stream.cpp: the twin).
#pragma once

#include "apt_kernels_fm.hpp"

namespace apt::fm {

constexpr uint32_t kDefaultMaxPushFrames = 1u << 20;

inline uint64_t stream_out_len(const Design &d, uint64_t n)
{
    return n < d.T ? 0 : (n - d.T) / d.D;  // M(n) - 1
}
inline uint64_t stream_carry_start(const Design &d, uint64_t n) { return stream_out_len(d, n) * d.D; }  // c0(n)
// frames of room a carry buffer needs: fewer than T + D frames behind up to 7 slots of lead
inline size_t stream_carry_slots(const Design &d) { return static_cast<size_t>(d.T) + d.D + kRun; }

// What the settings of a stream come to; throws Error{Invalid} naming the field.
struct StreamDesign {
    Design fm;
    uint32_t max_push_frames = kDefaultMaxPushFrames;
    uint64_t first_frame = 0;
};
StreamDesign design_stream(const aptgpu_fm_settings *fm, const aptgpu_fm_stream_settings *ss);
// the pointer checks of a push, before anything is enqueued or computed; the names go into the refusal's text
// ("iq" / "d_iq", "audio" / "d_audio"); audio_name null: the input's checks only
void check_push(const StreamDesign &d, uint64_t n_pushed, const void *iq, size_t n_frames, const void *audio, size_t audio_cap,
                const char *iq_name, const char *audio_name);

// run_host over a recording whose frame 0 is absolute frame `base` (run_host itself: base 0)
void run_host_based(const Design &d, uint64_t base, const void *iq, size_t n_frames, float *audio);

// The twin: plain C++, the same indexing.
class HostFmStream {
public:
    explicit HostFmStream(const StreamDesign &d) : d_(d) {}
    const StreamDesign &design() const { return d_; }
    uint64_t frames() const { return n_; }
    uint64_t outputs() const { return stream_out_len(d_.fm, n_); }
    uint32_t carry_frames() const { return static_cast<uint32_t>(n_ - stream_carry_start(d_.fm, n_)); }
    size_t bytes() const { return carry_.capacity() + work_.capacity(); }
    void reset()
    {
        n_ = 0;
        carry_.clear();
    }
    // n_frames more frames; audio receives stream_out_len(n + n_frames) - stream_out_len(n) floats; returns that count
    size_t push(const void *iq, size_t n_frames, float *audio);

private:
    StreamDesign d_;
    uint64_t n_ = 0;
    std::vector<uint8_t> carry_, work_;  // the frames [c0(n), n); carry ++ chunk of one launch
};

}  // namespace apt::fm

#if defined(__HIPCC__)
namespace apt::gpu {

// One launch: the virtual recording carry ++ chunk (apt_kernels_fm_body.hpp, TwoSegment) and where its outputs go.
struct FmStreamPush {
    const uint8_t *carry, *chunk;
    float *audio;
    uint64_t first;    // absolute index of the virtual recording's frame 0
    uint64_t n_total;  // n_carry + the chunk's frames
    uint32_t n_carry;
};
void fm_stream_prepare(int format, bool mix, const apt::fm::Tile &tile);
// tiles = ceil(outputs / (nv - 1)); nothing is launched for 0
void fm_stream_launch(hipStream_t stream, int format, bool mix, const apt::fm::Tile &tile, const FmStreamPush &push,
                      uint32_t tiles, const FmParams &p);

}  // namespace apt::gpu
#endif
