// apt_capi_fm_stream.hip — extern "C" surface of include/aptgpu.h §4b': the FM demodulator in streaming form
// (aptgpu_fm_stream_*) and its coupling to the live decode on one HIP stream (aptgpu_iq_live_*).  DESIGN.md §23.
// The host mirrors the frame count and nothing else: launch sizes, output counts and carry lengths are arithmetic on it.
#include <algorithm>
#include <memory>
#include <vector>

#include "apt_capi_stream_parts.hpp"
#include "apt_capi_util.hpp"
#include "apt_kernels_fm_stream.hpp"
#include "apt_kernels_stream_track.hpp"

namespace fms = apt::fm;
namespace parts = apt::capi::stream_parts;

struct aptgpu_fm_stream {
    bool host = false;
    fms::StreamDesign d;
    std::unique_ptr<fms::HostFmStream> twin;
    // ---- the device form
    fms::Tile tile{};
    int device = 0;
    hipStream_t stream = nullptr;
    apt::DeviceBuffer<float> d_taps_rev;
    apt::DeviceBuffer<uint32_t> d_offsets;
    apt::DeviceBuffer<uint8_t> carry[2];  // used in turn; slot 0 of the current one is absolute frame a - a % 8, a = first_frame + c0(n)
    int cur = 0;
    apt::DeviceBuffer<uint8_t> stage_iq;  // the host-fed form's staging: max_push_frames frames and their outputs
    apt::DeviceBuffer<float> stage_audio;
    uint64_t n = 0;  // frames pushed

    ~aptgpu_fm_stream()
    {
        if (!host) {
            (void)hipSetDevice(device);
            (void)hipStreamSynchronize(stream);  // the buffers may still be read
        }
    }
};

struct aptgpu_iq_live {
    bool host = false;
    aptgpu_fm_stream *fm = nullptr;
    aptgpu_stream *dec = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    size_t audio_cap = 0;  // outputs of one piece of max_push_frames frames
    apt::DeviceBuffer<float> d_audio;
    std::vector<float> h_audio;

    ~aptgpu_iq_live()
    {
        aptgpu_stream_destroy(dec);
        delete fm;
        if (own_stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

using namespace apt::capi;

size_t frame_bytes(const aptgpu_fm_stream *s) { return 2u * fms::component_bytes(s->d.fm.format); }
// frames pushed so far, and the outputs n_frames more would return: the one place that knows where the count lives
uint64_t frames(const aptgpu_fm_stream *s) { return s->host ? s->twin->frames() : s->n; }
size_t out_len_after(const aptgpu_fm_stream *s, size_t n_frames)
{
    const uint64_t n = frames(s);
    return static_cast<size_t>(fms::stream_out_len(s->d.fm, n + n_frames) - fms::stream_out_len(s->d.fm, n));
}
// outputs one piece of at most max_push_frames frames can return
size_t piece_outputs(const fms::StreamDesign &d) { return d.max_push_frames / d.fm.D + 2u; }

void create_device(aptgpu_fm_stream *s, int device, hipStream_t stream)
{
    const fms::Design &d = s->d.fm;
    s->tile = fms::tile_of(d.D, d.T);
    s->device = device;
    s->stream = stream;
    apt::hip_check(hipSetDevice(device), "hipSetDevice");
    s->d_taps_rev.alloc(d.T + 16);
    apt::hip_check(hipMemcpyAsync(s->d_taps_rev.ptr, d.taps_rev.data(), d.T * sizeof(float), hipMemcpyHostToDevice, stream),
                   "hipMemcpyAsync H2D");
    const std::vector<uint32_t> offsets = fms::tap_offsets(d.D, d.T, s->tile.R);
    s->d_offsets.alloc(d.T + 16);
    apt::hip_check(hipMemcpyAsync(s->d_offsets.ptr, offsets.data(), offsets.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream),
                   "hipMemcpyAsync H2D");
    const size_t fb = frame_bytes(s);
    for (auto &c : s->carry) {
        c.alloc(fms::stream_carry_slots(d) * fb);
        apt::hip_check(hipMemsetAsync(c.ptr, 0, c.count, stream), "hipMemsetAsync");
    }
    s->stage_iq.alloc(static_cast<size_t>(s->d.max_push_frames) * fb + 16);
    s->stage_audio.alloc(piece_outputs(s->d));
    apt::hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");  // (offsets leaves scope)
    apt::gpu::fm_stream_prepare(d.format, d.pw != 0, s->tile);
}

// One piece (seg <= max_push_frames frames in device memory, read in place): the launch and the carry's refresh.
// Returns the outputs written to d_audio.  Nothing waits.
size_t enqueue_piece(aptgpu_fm_stream *s, const uint8_t *d_chunk, size_t seg, float *d_audio)
{
    const fms::Design &d = s->d.fm;
    const size_t fb = frame_bytes(s);
    const uint64_t n0 = s->n, n1 = n0 + seg;
    const uint64_t c0 = fms::stream_carry_start(d, n0), c1 = fms::stream_carry_start(d, n1);
    const uint32_t n_carry = static_cast<uint32_t>(n0 - c0);
    const size_t n_out = static_cast<size_t>(fms::stream_out_len(d, n1) - fms::stream_out_len(d, n0));
    const uint64_t a0 = s->d.first_frame + c0, a1 = s->d.first_frame + c1;  // absolute frame of the carry's first frame
    const size_t lead0 = static_cast<size_t>(a0 & 7u), lead1 = static_cast<size_t>(a1 & 7u);
    uint8_t *now = s->carry[s->cur].ptr;
    if (n_out) {
        const apt::gpu::FmStreamPush push{now, d_chunk, d_audio, a0, n_carry + seg, n_carry};
        const apt::gpu::FmParams p{s->d_taps_rev.ptr, s->d_offsets.ptr, d.T, d.D, s->tile.R, s->tile.nv, d.pw, d.swap ? 1u : 0u,
                                   d.step.re, d.step.im, d.gain};
        const size_t tiles = (n_out + s->tile.nv - 2) / (s->tile.nv - 1);
        apt::gpu::fm_stream_launch(s->stream, d.format, d.pw != 0, s->tile, push, static_cast<uint32_t>(tiles), p);
        apt::hip_check(hipGetLastError(), "kernel launch (k_fm_stream)");
    }
    // the frames [c1, n1) stay: n1 - c1 < T + D of them
    if (c1 == c0) {  // no output passed: the chunk goes behind what is held
        if (seg)
            apt::hip_check(hipMemcpyAsync(now + (lead0 + n_carry) * fb, d_chunk, seg * fb, hipMemcpyDeviceToDevice, s->stream),
                           "hipMemcpyAsync D2D");
    } else {
        uint8_t *next = s->carry[1 - s->cur].ptr;
        const uint64_t from_chunk = std::max(c1, n0);  // first stream frame taken from the chunk
        if (c1 < n0)
            apt::hip_check(hipMemcpyAsync(next + lead1 * fb, now + (lead0 + static_cast<size_t>(c1 - c0)) * fb,
                                          static_cast<size_t>(n0 - c1) * fb, hipMemcpyDeviceToDevice, s->stream),
                           "hipMemcpyAsync D2D");
        if (from_chunk < n1)
            apt::hip_check(hipMemcpyAsync(next + (lead1 + static_cast<size_t>(from_chunk - c1)) * fb,
                                          d_chunk + static_cast<size_t>(from_chunk - n0) * fb,
                                          static_cast<size_t>(n1 - from_chunk) * fb, hipMemcpyDeviceToDevice, s->stream),
                           "hipMemcpyAsync D2D");
        s->cur = 1 - s->cur;
    }
    s->n = n1;
    return n_out;
}

// one piece from host memory through the staging
size_t enqueue_piece_from_host(aptgpu_fm_stream *s, const uint8_t *iq, size_t seg, float *d_audio)
{
    if (seg)
        apt::hip_check(hipMemcpyAsync(s->stage_iq.ptr, iq, seg * frame_bytes(s), hipMemcpyHostToDevice, s->stream),
                       "hipMemcpyAsync H2D");
    return enqueue_piece(s, s->stage_iq.ptr, seg, d_audio);
}

void fill_info(const aptgpu_fm_stream *s, aptgpu_fm_stream_info *info)
{
    const fms::Design &d = s->d.fm;
    const uint32_t size = info->struct_size;
    *info = aptgpu_fm_stream_info{};
    info->struct_size = size;
    info->fs_out = d.fs_out;
    info->n_taps = d.T;
    info->decimation = d.D;
    info->pw = d.pw;
    const uint64_t n = frames(s);
    info->carry_frames = static_cast<uint32_t>(n - fms::stream_carry_start(d, n));
    info->shift_hz_used = d.shift_used;
    info->taps = d.taps.data();
    info->frames = n;
    info->outputs = fms::stream_out_len(d, n);
    info->first_frame = s->d.first_frame;
    info->device_bytes = s->host ? s->twin->bytes()
                                 : s->d_taps_rev.count * 4 + s->d_offsets.count * 4 + s->carry[0].count + s->carry[1].count +
                                       s->stage_iq.count + s->stage_audio.count * 4;
    info->max_push_frames = s->d.max_push_frames;
}

std::unique_ptr<aptgpu_fm_stream> make_fm_stream(const aptgpu_fm_settings *settings, const aptgpu_fm_stream_settings *ss, bool host,
                                                 int device, hipStream_t stream)
{
    auto s = std::make_unique<aptgpu_fm_stream>();
    s->host = host;
    s->d = fms::design_stream(settings, ss);  // every refusal, before a device is touched
    if (host) s->twin = std::make_unique<fms::HostFmStream>(s->d);
    else create_device(s.get(), device, stream);
    return s;
}

void reset_fm(aptgpu_fm_stream *s)
{
    if (s->host) s->twin->reset();
    s->n = 0;
    s->cur = 0;
}

// the host-fed push of an FM stream alone
size_t push_fm_host_fed(aptgpu_fm_stream *s, const void *iq, size_t n_frames, float *audio)
{
    if (s->host) return s->twin->push(iq, n_frames, audio);
    apt::hip_check(hipSetDevice(s->device), "hipSetDevice");
    const uint8_t *src = static_cast<const uint8_t *>(iq);
    const size_t fb = frame_bytes(s);
    size_t done = 0, written = 0;
    while (done < n_frames) {
        const size_t seg = std::min<size_t>(n_frames - done, s->d.max_push_frames);
        const size_t k = enqueue_piece_from_host(s, src + done * fb, seg, s->stage_audio.ptr);
        if (k)
            apt::hip_check(hipMemcpyAsync(audio + written, s->stage_audio.ptr, k * sizeof(float), hipMemcpyDeviceToHost, s->stream),
                           "hipMemcpyAsync D2H");
        written += k;
        done += seg;
    }
    apt::hip_check(hipStreamSynchronize(s->stream), "hipStreamSynchronize");
    return written;
}

// ---- the coupling
int create_live(const aptgpu_context *ctx, const aptgpu_settings *decode_settings, const aptgpu_fm_settings *fm_settings,
                const aptgpu_iq_live_settings *ls, bool tracked, const aptgpu_live_track_settings *track, bool host,
                aptgpu_iq_live **out, char *err, size_t err_cap)
{
    if (!out) return null_argument(err, err_cap, "iq live");
    *out = nullptr;
    return guarded(err, err_cap, [&] {
        if (!ls || ls->struct_size < sizeof(aptgpu_iq_live_settings))
            throw Error{ErrorKind::Invalid, "aptgpu_iq_live_settings: struct_size not set"};
        aptgpu_fm_stream_settings fss{};
        fss.struct_size = sizeof fss;
        fss.max_push_frames = ls->max_push_frames ? ls->max_push_frames : fms::kDefaultMaxPushFrames;
        fss.first_frame = ls->first_frame;
        const fms::StreamDesign checked = fms::design_stream(fm_settings, &fss);  // the refusals, before a device is touched
        auto live = std::make_unique<aptgpu_iq_live>();
        live->host = host;
        aptgpu_context c{};
        if (ctx) c = *ctx;
        live->device = c.device;
        aptgpu_stream_settings ss{};
        ss.struct_size = sizeof ss;
        ss.input_rate_hz = checked.fm.fs_out;
        ss.sync = ls->sync;
        ss.format = APTGPU_STREAM_F32;
        ss.max_push = ls->max_push;
        // (a tracked coupling: the tracker's and the decode stream's refusals, before a device is touched)
        if (tracked) (void)apt::stream_track::design_tracked(decode_settings, &ss, track, c.mode, apt::gpu::read_plan_switches().fast_mfma == '1');
        if (!host) {
            apt::hip_check(hipSetDevice(c.device), "hipSetDevice");
            if (!c.stream) {
                apt::hip_check(hipStreamCreateWithFlags(&live->stream, hipStreamNonBlocking), "hipStreamCreate");
                live->own_stream = true;
                c.stream = live->stream;
            } else {
                live->stream = static_cast<hipStream_t>(c.stream);
            }
        }
        char text[1024] = "";
        // (a tracked coupling: the same handle with the flywheel tracker in the picker's place, include/aptgpu.h §4e)
        const int rc = parts::create(&c, decode_settings, &ss, tracked, track, host, &live->dec, text, sizeof text);
        if (rc != APTGPU_OK) throw Error{static_cast<ErrorKind>(rc), text};
        live->fm = make_fm_stream(fm_settings, &fss, host, c.device, live->stream).release();
        live->audio_cap = piece_outputs(live->fm->d);
        if (host) live->h_audio.resize(live->audio_cap);
        else live->d_audio.alloc(live->audio_cap);
        *out = live.release();
        return APTGPU_OK;
    });
}

// the pieces of one push: FM into the scratch, the scratch into the decode stream
void live_pieces(aptgpu_iq_live *s, const void *iq, size_t n_frames, bool iq_on_host, const parts::Target &t)
{
    aptgpu_fm_stream *fm = s->fm;
    const uint8_t *src = static_cast<const uint8_t *>(iq);
    const size_t fb = frame_bytes(fm);
    size_t done = 0;
    bool first = true;
    do {
        const size_t seg = std::min<size_t>(n_frames - done, fm->d.max_push_frames);
        size_t k;
        const float *audio;
        if (s->host) {
            k = fm->twin->push(src + done * fb, seg, s->h_audio.data());
            audio = s->h_audio.data();
        } else {
            k = iq_on_host ? enqueue_piece_from_host(fm, src + done * fb, seg, s->d_audio.ptr)
                           : enqueue_piece(fm, src + done * fb, seg, s->d_audio.ptr);
            audio = s->d_audio.ptr;
        }
        parts::piece(s->dec, audio, k, first, false, t);
        first = false;
        done += seg;
    } while (done < n_frames);
}

void check_live_push(const aptgpu_iq_live *s, const void *iq, size_t n_frames, size_t rows_cap, const aptgpu_stream_result *result,
                     bool want_result, const char *iq_name)
{
    fms::check_push(s->fm->d, frames(s->fm), iq, n_frames, nullptr, 0, iq_name, nullptr);
    parts::check(s->dec, out_len_after(s->fm, n_frames), rows_cap, result, want_result);
}

}  // namespace

extern "C" {

int aptgpu_fm_stream_create(const aptgpu_context *ctx, const aptgpu_fm_settings *settings,
                            const aptgpu_fm_stream_settings *stream_settings, aptgpu_fm_stream **out, char *err, size_t err_cap)
{
    if (!out) return null_argument(err, err_cap, "fm stream");
    *out = nullptr;
    return guarded(err, err_cap, [&] {
        *out = make_fm_stream(settings, stream_settings, false, ctx ? ctx->device : 0,
                              ctx ? static_cast<hipStream_t>(ctx->stream) : nullptr)
                   .release();
        return APTGPU_OK;
    });
}

int aptgpu_fm_stream_create_host(const aptgpu_fm_settings *settings, const aptgpu_fm_stream_settings *stream_settings,
                                 aptgpu_fm_stream **out, char *err, size_t err_cap)
{
    if (!out) return null_argument(err, err_cap, "fm stream");
    *out = nullptr;
    return guarded(err, err_cap, [&] {
        *out = make_fm_stream(settings, stream_settings, true, 0, nullptr).release();
        return APTGPU_OK;
    });
}

void aptgpu_fm_stream_destroy(aptgpu_fm_stream *s) { delete s; }

int aptgpu_fm_stream_reset(aptgpu_fm_stream *s, char *err, size_t err_cap)
{
    if (!s) return null_argument(err, err_cap, "fm stream");
    reset_fm(s);
    return APTGPU_OK;
}

int aptgpu_fm_stream_get_info(const aptgpu_fm_stream *s, aptgpu_fm_stream_info *info)
{
    if (!s || !info || info->struct_size < sizeof(aptgpu_fm_stream_info)) return APTGPU_ERR_INVALID;
    fill_info(s, info);
    return APTGPU_OK;
}

size_t aptgpu_fm_stream_out_len(const aptgpu_fm_stream *s, size_t n_frames)
{
    return s ? out_len_after(s, n_frames) : 0;
}

int aptgpu_fm_stream_push(aptgpu_fm_stream *s, const void *iq, size_t n_frames, float *audio, size_t audio_cap, size_t *n_out,
                          char *err, size_t err_cap)
{
    if (!s || !n_out) return null_argument(err, err_cap, "fm stream");
    *n_out = 0;
    return guarded(err, err_cap, [&] {
        fms::check_push(s->d, frames(s), iq, n_frames, audio, audio_cap, "iq", "audio");
        *n_out = push_fm_host_fed(s, iq, n_frames, audio);
        return APTGPU_OK;
    });
}

int aptgpu_fm_stream_push_device(aptgpu_fm_stream *s, const void *d_iq, size_t n_frames, float *d_audio, size_t audio_cap,
                                 size_t *n_out, char *err, size_t err_cap)
{
    if (!s || !n_out) return null_argument(err, err_cap, "fm stream");
    *n_out = 0;
    return guarded(err, err_cap, [&] {
        if (s->host) throw Error{ErrorKind::Invalid, "fm stream: a host handle has no device entry points"};
        fms::check_push(s->d, s->n, d_iq, n_frames, d_audio, audio_cap, "d_iq", "d_audio");
        apt::hip_check(hipSetDevice(s->device), "hipSetDevice");
        const uint8_t *src = static_cast<const uint8_t *>(d_iq);
        const size_t fb = frame_bytes(s);
        size_t done = 0, written = 0;
        while (done < n_frames) {  // pairs of launch and refresh back to back, no read-back
            const size_t seg = std::min<size_t>(n_frames - done, s->d.max_push_frames);
            written += enqueue_piece(s, src + done * fb, seg, d_audio + written);
            done += seg;
        }
        *n_out = written;
        return APTGPU_OK;
    });
}

// ---------------------------------------------------------------- live decode from IQ
int aptgpu_iq_live_create(const aptgpu_context *ctx, const aptgpu_settings *decode_settings, const aptgpu_fm_settings *fm_settings,
                          const aptgpu_iq_live_settings *live_settings, aptgpu_iq_live **out, char *err, size_t err_cap)
{
    return create_live(ctx, decode_settings, fm_settings, live_settings, false, nullptr, false, out, err, err_cap);
}

int aptgpu_iq_live_create_host(const aptgpu_context *ctx, const aptgpu_settings *decode_settings,
                               const aptgpu_fm_settings *fm_settings, const aptgpu_iq_live_settings *live_settings,
                               aptgpu_iq_live **out, char *err, size_t err_cap)
{
    return create_live(ctx, decode_settings, fm_settings, live_settings, false, nullptr, true, out, err, err_cap);
}

int aptgpu_iq_live_create_tracked(const aptgpu_context *ctx, const aptgpu_settings *decode_settings,
                                  const aptgpu_fm_settings *fm_settings, const aptgpu_iq_live_settings *live_settings,
                                  const aptgpu_live_track_settings *track, aptgpu_iq_live **out, char *err, size_t err_cap)
{
    return create_live(ctx, decode_settings, fm_settings, live_settings, true, track, false, out, err, err_cap);
}

int aptgpu_iq_live_create_tracked_host(const aptgpu_context *ctx, const aptgpu_settings *decode_settings,
                                       const aptgpu_fm_settings *fm_settings, const aptgpu_iq_live_settings *live_settings,
                                       const aptgpu_live_track_settings *track, aptgpu_iq_live **out, char *err, size_t err_cap)
{
    return create_live(ctx, decode_settings, fm_settings, live_settings, true, track, true, out, err, err_cap);
}

int aptgpu_iq_live_track_scores(aptgpu_iq_live *s, float *scores, size_t cap, size_t *n, char *err, size_t err_cap)
{
    if (!s) return null_argument(err, err_cap, "iq live");
    return aptgpu_stream_track_scores(s->dec, scores, cap, n, err, err_cap);
}

int aptgpu_iq_live_track_scores_device(aptgpu_iq_live *s, float *d_scores, char *err, size_t err_cap)
{
    if (!s) return null_argument(err, err_cap, "iq live");
    return aptgpu_stream_track_scores_device(s->dec, d_scores, err, err_cap);
}

int aptgpu_iq_live_track_results(aptgpu_iq_live *s, aptgpu_stream_track_result *result, char *err, size_t err_cap)
{
    if (!s) return null_argument(err, err_cap, "iq live");
    return aptgpu_stream_track_results(s->dec, result, err, err_cap);
}

void aptgpu_iq_live_destroy(aptgpu_iq_live *s)
{
    if (!s) return;
    if (!s->host) {
        (void)hipSetDevice(s->device);
        (void)hipStreamSynchronize(s->stream);  // the scratch may still be read
    }
    delete s;
}

int aptgpu_iq_live_reset(aptgpu_iq_live *s, char *err, size_t err_cap)
{
    if (!s) return null_argument(err, err_cap, "iq live");
    const int rc = aptgpu_stream_reset(s->dec, err, err_cap);
    if (rc == APTGPU_OK) reset_fm(s->fm);
    return rc;
}

int aptgpu_iq_live_get_info(const aptgpu_iq_live *s, aptgpu_fm_stream_info *fm_info, aptgpu_stream_info *stream_info)
{
    if (!s) return APTGPU_ERR_INVALID;
    if (fm_info) {
        const int rc = aptgpu_fm_stream_get_info(s->fm, fm_info);
        if (rc != APTGPU_OK) return rc;
        if (!s->host) fm_info->device_bytes += s->d_audio.count * sizeof(float);
    }
    return stream_info ? aptgpu_stream_get_info(s->dec, stream_info) : APTGPU_OK;
}

size_t aptgpu_iq_live_rows_bound(const aptgpu_iq_live *s, size_t n_frames)
{
    return s ? aptgpu_stream_rows_bound(s->dec, out_len_after(s->fm, n_frames)) : 0;
}

int aptgpu_iq_live_push(aptgpu_iq_live *s, const void *iq, size_t n_frames, float *rows, uint64_t *positions, size_t rows_cap,
                        aptgpu_stream_result *result, char *err, size_t err_cap)
{
    if (!s || !rows || !positions || !result) return null_argument(err, err_cap, "iq live");
    return guarded(err, err_cap, [&] {
        check_live_push(s, iq, n_frames, rows_cap, result, true, "iq");
        if (!s->host) apt::hip_check(hipSetDevice(s->device), "hipSetDevice");
        const parts::Target t = parts::begin(s->dec, out_len_after(s->fm, n_frames), rows, positions, rows_cap);
        live_pieces(s, iq, n_frames, true, t);
        parts::end(s->dec, t, rows, positions, result);
        return APTGPU_OK;
    });
}

int aptgpu_iq_live_finish(aptgpu_iq_live *s, float *rows, uint64_t *positions, size_t rows_cap, aptgpu_stream_result *result,
                          char *err, size_t err_cap)
{
    if (!s) return null_argument(err, err_cap, "iq live");
    return aptgpu_stream_finish(s->dec, rows, positions, rows_cap, result, err, err_cap);
}

int aptgpu_iq_live_push_device(aptgpu_iq_live *s, const void *d_iq, size_t n_frames, float *d_rows, uint64_t *d_positions,
                               size_t rows_cap, char *err, size_t err_cap)
{
    if (!s || !d_rows || !d_positions) return null_argument(err, err_cap, "iq live");
    return guarded(err, err_cap, [&] {
        if (s->host) throw Error{ErrorKind::Invalid, "iq live: a host handle has no device entry points"};
        check_live_push(s, d_iq, n_frames, rows_cap, nullptr, false, "d_iq");
        apt::hip_check(hipSetDevice(s->device), "hipSetDevice");
        const parts::Target t = parts::device_target(s->dec, d_rows, d_positions, rows_cap);
        live_pieces(s, d_iq, n_frames, false, t);
        return APTGPU_OK;
    });
}

int aptgpu_iq_live_finish_device(aptgpu_iq_live *s, float *d_rows, uint64_t *d_positions, size_t rows_cap, char *err, size_t err_cap)
{
    if (!s) return null_argument(err, err_cap, "iq live");
    return aptgpu_stream_finish_device(s->dec, d_rows, d_positions, rows_cap, err, err_cap);
}

int aptgpu_iq_live_results(aptgpu_iq_live *s, aptgpu_stream_result *result, char *err, size_t err_cap)
{
    if (!s) return null_argument(err, err_cap, "iq live");
    return aptgpu_stream_results(s->dec, result, err, err_cap);
}

}  // extern "C"
