// apt_capi_fm.hip — extern "C" surface of include/aptgpu.h §4b: FM demodulation of IQ recordings in front of decode().
#include "apt_capi_fm_handle.hpp"
#include "apt_capi_util.hpp"
#include "apt_wav.hpp"

namespace {

using namespace apt::capi;

void fill_info(const apt::fm::Design &d, aptgpu_fm_info *info, const float *taps)
{
    info->fs_out = d.fs_out;
    info->n_taps = d.T;
    info->decimation = d.D;
    info->pw = d.pw;
    info->reserved = 0;
    info->shift_hz_used = d.shift_used;
    info->taps = taps;
}

}  // namespace

namespace apt::capi {
// the demodulator's state on `stream` of `device`; the taps are on the device when this returns
void fm_setup(aptgpu_fm &fm, const aptgpu_fm_settings *settings, int device, hipStream_t stream)
{
    fm.design = apt::fm::design_of(settings);  // every refusal, before a device is touched
    fm.tile = apt::fm::tile_of(fm.design.D, fm.design.T);
    fm.device = device;
    fm.stream = stream;
    apt::hip_check(hipSetDevice(device), "hipSetDevice");
    fm.d_taps_rev.alloc(fm.design.T + 16);
    apt::hip_check(hipMemcpyAsync(fm.d_taps_rev.ptr, fm.design.taps_rev.data(), fm.design.T * sizeof(float),
                                  hipMemcpyHostToDevice, stream),
                   "hipMemcpyAsync H2D");
    const std::vector<uint32_t> offsets = apt::fm::tap_offsets(fm.design.D, fm.design.T, fm.tile.R);
    fm.d_offsets.alloc(fm.design.T + 16);
    apt::hip_check(hipMemcpyAsync(fm.d_offsets.ptr, offsets.data(), offsets.size() * sizeof(uint32_t),
                                  hipMemcpyHostToDevice, stream),
                   "hipMemcpyAsync H2D");
    apt::hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
    apt::gpu::fm_prepare(fm.design.format, fm.design.pw != 0, fm.tile);
}

FmLaunch fm_launch_checks(const aptgpu_fm &fm, int count, const void *const *d_iq, const size_t *n_frames,
                          float *const *d_audio, const size_t *audio_cap)
{
    if (count > apt::fm::kMaxBatch) throw Error{ErrorKind::Invalid, "fm: more than APTGPU_FM_MAX_BATCH recordings"};
    const apt::fm::Design &d = fm.design;
    const uintptr_t align = apt::fm::component_bytes(d.format);
    FmLaunch t;
    uint64_t max_tiles = 0;
    for (int i = 0; i < count; ++i) {
        const size_t n_out = apt::fm::out_len(d, n_frames[i]);
        if (n_out && (!d_iq[i] || !d_audio[i])) throw Error{ErrorKind::Invalid, "fm: a null device pointer"};
        if (reinterpret_cast<uintptr_t>(d_iq[i]) % align != 0)
            throw Error{ErrorKind::Invalid, "fm: d_iq is not aligned to one component"};
        if (reinterpret_cast<uintptr_t>(d_audio[i]) % sizeof(float) != 0)
            throw Error{ErrorKind::Invalid, "fm: d_audio is not aligned to a float"};
        if (audio_cap[i] < n_out) throw Error{ErrorKind::Invalid, "fm: audio_cap is below the output length"};
        t.batch.r[i] = apt::gpu::FmRecording{static_cast<const uint8_t *>(d_iq[i]), d_audio[i], n_frames[i]};
        const uint64_t tiles = (n_out + fm.tile.nv - 2) / (fm.tile.nv - 1);
        max_tiles = tiles > max_tiles ? tiles : max_tiles;
    }
    if (max_tiles > 0x7FFFFFFFull) throw Error{ErrorKind::Invalid, "fm: n_frames is too long for one launch"};
    t.max_tiles = static_cast<uint32_t>(max_tiles);
    return t;
}
}  // namespace apt::capi

namespace {

// checks, then one launch; nothing is enqueued when a check fails
void enqueue(aptgpu_fm &fm, int count, const void *const *d_iq, const size_t *n_frames, float *const *d_audio,
             const size_t *audio_cap)
{
    const FmLaunch t = fm_launch_checks(fm, count, d_iq, n_frames, d_audio, audio_cap);
    const apt::fm::Design &d = fm.design;
    apt::hip_check(hipSetDevice(fm.device), "hipSetDevice");
    const apt::gpu::FmParams p{fm.d_taps_rev.ptr, fm.d_offsets.ptr, d.T, d.D, fm.tile.R, fm.tile.nv, d.pw, d.swap ? 1u : 0u,
                               d.step.re, d.step.im, d.gain};
    apt::gpu::fm_demodulate(fm.stream, d.format, d.pw != 0, fm.tile, t.batch, count, t.max_tiles, p);
    apt::hip_check(hipGetLastError(), "kernel launch (k_fm)");
}

int demodulate_host_array(const aptgpu_context *ctx, const aptgpu_fm_settings *settings, const void *iq, size_t n_frames,
                          float **audio, size_t *n_out, uint32_t *rate_hz)
{
    // the refusals first: Scratch touches the device
    const apt::fm::Design checked = apt::fm::design_of(settings);
    if (!iq && apt::fm::out_len(checked, n_frames)) throw Error{ErrorKind::Invalid, "fm: iq is null"};
    Scratch sc(ctx);
    aptgpu_fm fm;
    fm_setup(fm, settings, sc.device, sc.stream);
    const size_t out = apt::fm::out_len(fm.design, n_frames);
    const size_t bytes = n_frames * 2u * apt::fm::component_bytes(fm.design.format);
    apt::DeviceBuffer<uint8_t> d_iq;
    apt::DeviceBuffer<float> d_audio;
    d_iq.alloc(bytes + 16);
    d_audio.alloc(out + 16);
    if (bytes && out)
        apt::hip_check(hipMemcpyAsync(d_iq.ptr, iq, bytes, hipMemcpyHostToDevice, sc.stream), "hipMemcpyAsync H2D");
    const void *in = d_iq.ptr;
    float *dst = d_audio.ptr;
    enqueue(fm, 1, &in, &n_frames, &dst, &out);
    *audio = sc.download_malloc(d_audio.ptr, out);
    if (!out) apt::hip_check(hipStreamSynchronize(sc.stream), "hipStreamSynchronize");
    *n_out = out;
    if (rate_hz) *rate_hz = fm.design.fs_out;
    return APTGPU_OK;
}

}  // namespace

extern "C" {

void aptgpu_fm_default_settings(aptgpu_fm_settings *s)
{
    if (!s) return;
    *s = aptgpu_fm_settings{};
    s->struct_size = sizeof(aptgpu_fm_settings);
    s->format = APTGPU_IQ_U8;
    s->decimation = 1;
    s->channel_cutout_hz = 18000.f;
    s->channel_atten = 40.f;
    s->channel_delta_hz = 8000.f;
    s->deviation_hz = 17000.f;
}

int aptgpu_fm_design(const aptgpu_fm_settings *settings, aptgpu_fm_info *info, float **taps, char *err, size_t err_cap)
{
    if (!info || info->struct_size < sizeof(aptgpu_fm_info)) {
        put_err(err, err_cap, "aptgpu_fm_info: struct_size not set");
        return APTGPU_ERR_INVALID;
    }
    if (taps) *taps = nullptr;
    return guarded(err, err_cap, [&] {
        const apt::fm::Design d = apt::fm::design_of(settings);
        fill_info(d, info, nullptr);
        if (taps) {
            float *p = host_alloc<float>(d.taps.size());
            std::memcpy(p, d.taps.data(), d.taps.size() * sizeof(float));
            *taps = p;
        }
        return APTGPU_OK;
    });
}

int aptgpu_fm_create(const aptgpu_context *ctx, const aptgpu_fm_settings *settings, aptgpu_fm **out, char *err,
                     size_t err_cap)
{
    if (!out) return APTGPU_ERR_INVALID;
    *out = nullptr;
    return guarded(err, err_cap, [&] {
        auto fm = std::make_unique<aptgpu_fm>();
        fm_setup(*fm, settings, ctx ? ctx->device : 0, ctx ? static_cast<hipStream_t>(ctx->stream) : nullptr);
        *out = fm.release();
        return APTGPU_OK;
    });
}

void aptgpu_fm_destroy(aptgpu_fm *fm)
{
    if (!fm) return;
    (void)hipSetDevice(fm->device);
    (void)hipStreamSynchronize(fm->stream);  // the taps may still be read
    delete fm;
}

int aptgpu_fm_get_info(const aptgpu_fm *fm, aptgpu_fm_info *info)
{
    if (!fm || !info || info->struct_size < sizeof(aptgpu_fm_info)) return APTGPU_ERR_INVALID;
    fill_info(fm->design, info, fm->design.taps.data());
    return APTGPU_OK;
}

size_t aptgpu_fm_out_len(const aptgpu_fm *fm, size_t n_frames) { return fm ? apt::fm::out_len(fm->design, n_frames) : 0; }

int aptgpu_fm_demodulate(const aptgpu_context *ctx, const aptgpu_fm_settings *settings, const void *iq, size_t n_frames,
                         float **audio, size_t *n_out, uint32_t *rate_hz, char *err, size_t err_cap)
{
    if (!audio || !n_out) return APTGPU_ERR_INVALID;
    *audio = nullptr;
    *n_out = 0;
    return guarded(err, err_cap, [&] { return demodulate_host_array(ctx, settings, iq, n_frames, audio, n_out, rate_hz); });
}

int aptgpu_fm_demodulate_host(const aptgpu_fm_settings *settings, const void *iq, size_t n_frames, float **audio,
                              size_t *n_out, uint32_t *rate_hz, char *err, size_t err_cap)
{
    if (!audio || !n_out) return APTGPU_ERR_INVALID;
    *audio = nullptr;
    *n_out = 0;
    return guarded(err, err_cap, [&] {
        const apt::fm::Design d = apt::fm::design_of(settings);
        const size_t out = apt::fm::out_len(d, n_frames);
        if (!iq && out) throw Error{ErrorKind::Invalid, "fm: iq is null"};
        float *p = host_alloc<float>(out);
        try {
            apt::fm::run_host(d, iq, n_frames, p);
        } catch (...) {
            std::free(p);
            throw;
        }
        *audio = p;
        *n_out = out;
        if (rate_hz) *rate_hz = d.fs_out;
        return APTGPU_OK;
    });
}

int aptgpu_fm_demodulate_device(aptgpu_fm *fm, int count, const void *const *d_iq, const size_t *n_frames,
                                float *const *d_audio, const size_t *audio_cap, char *err, size_t err_cap)
{
    if (!fm || count < 0 || (count && (!d_iq || !n_frames || !d_audio || !audio_cap))) {
        put_err(err, err_cap, "fm: null argument");
        return APTGPU_ERR_INVALID;
    }
    return guarded(err, err_cap, [&] {
        enqueue(*fm, count, d_iq, n_frames, d_audio, audio_cap);
        return APTGPU_OK;
    });
}

int aptgpu_fm_demodulate_wav(const aptgpu_context *ctx, const aptgpu_fm_settings *settings, const void *file_bytes,
                             size_t n, float **audio, size_t *n_out, uint32_t *rate_hz, char *err, size_t err_cap)
{
    if (!audio || !n_out || !file_bytes) return APTGPU_ERR_INVALID;
    *audio = nullptr;
    *n_out = 0;
    return guarded(err, err_cap, [&] {
        if (!settings || settings->struct_size < sizeof(aptgpu_fm_settings))
            throw Error{ErrorKind::Invalid, "aptgpu_fm_settings: struct_size not set"};
        const uint8_t *bytes = static_cast<const uint8_t *>(file_bytes);
        const apt::WavInfo w = apt::parse_wav(bytes, n);
        if (w.channels != 2 || (w.codec != apt::WavCodec::I16 && w.codec != apt::WavCodec::F32))
            throw Error{ErrorKind::Unsupported,
                        "fm: an IQ WAV has two channels of 16-bit integer or 32-bit float samples"};
        aptgpu_fm_settings s = *settings;
        s.struct_size = sizeof s;
        s.format = w.codec == apt::WavCodec::I16 ? APTGPU_IQ_S16 : APTGPU_IQ_F32;
        s.sample_rate_hz = w.sample_rate;
        return demodulate_host_array(ctx, &s, bytes + w.data_offset, w.n_frames, audio, n_out, rate_hz);
    });
}

}  // extern "C"
