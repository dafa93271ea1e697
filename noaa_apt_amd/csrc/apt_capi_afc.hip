// apt_capi_afc.hip — extern "C" surface of include/aptgpu.h §4b': AFC in front of the FM demodulator (block sums, the
// table, tracked demodulation), on host arrays, on the CPU (the twin of apt_afc.cpp) and device-resident.
#include "apt_capi_fm_handle.hpp"
#include "apt_capi_util.hpp"
#include "apt_kernels_afc.hpp"

struct aptgpu_fm_afc {
    aptgpu_fm *fm = nullptr;
    int device = 0;                // the demodulator's, kept here so that destroy() does not need it alive
    hipStream_t stream = nullptr;
    apt::afc::Design design;
    size_t max_frames = 0;
    uint64_t max_blocks = 0;  // of one recording
    // the work space: APTGPU_FM_MAX_BATCH slots of max_blocks entries
    apt::DeviceBuffer<double> d_sums;
    apt::DeviceBuffer<apt::afc::Record> d_table;
    apt::DeviceBuffer<float> d_coherence;
    apt::DeviceBuffer<uint8_t> d_good;
};

namespace {

using namespace apt::capi;
using apt::afc::Record;

struct Designs {
    apt::fm::Design fm;
    apt::afc::Design afc;
};
// every refusal of both settings, on the host
Designs designs_of(const aptgpu_fm_settings *fs, const aptgpu_afc_settings *as)
{
    Designs d;
    d.fm = apt::fm::design_of(fs);
    d.afc = apt::afc::design_of(d.fm, d.fm.deviation_hz, as);
    return d;
}

void check_table_len(const apt::afc::Design &d, size_t n_frames, size_t n_blocks)
{
    if (n_blocks != apt::afc::checked_blocks(d, n_frames))
        throw Error{ErrorKind::Invalid, "afc: n_blocks is not ceil(n_frames / block_frames)"};
}

template <typename T>
T *download(const T *d, size_t n, hipStream_t s)
{
    HostPtr<T> p(host_alloc<T>(n));
    if (n) {
        apt::hip_check(hipMemcpyAsync(p.get(), d, n * sizeof(T), hipMemcpyDeviceToHost, s), "hipMemcpyAsync D2H");
        apt::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
    }
    return p.release();
}
template <typename T>
apt::DeviceBuffer<T> upload(const T *h, size_t n, hipStream_t s)
{
    apt::DeviceBuffer<T> d;
    d.alloc(n + 16);
    if (n) apt::hip_check(hipMemcpyAsync(d.ptr, h, n * sizeof(T), hipMemcpyHostToDevice, s), "hipMemcpyAsync H2D");
    return d;
}

// stages A and B of a batch whose every pointer is set; nothing is checked here
void enqueue_estimate(hipStream_t stream, const apt::fm::Design &fm, const apt::afc::Design &d,
                      const apt::gpu::AfcBatch &batch, int count, bool sums, bool table)
{
    uint64_t max_blocks = 0;
    for (int i = 0; i < count; ++i) {
        const uint64_t nb = apt::afc::blocks_of(batch.r[i].n_frames, d.log2_B);
        max_blocks = nb > max_blocks ? nb : max_blocks;
    }
    if (sums) {
        apt::gpu::afc_sums(stream, fm.format, fm.swap, d, batch, count, static_cast<uint32_t>(max_blocks));
        apt::hip_check(hipGetLastError(), "kernel launch (k_afc_sums)");
    }
    if (table && max_blocks) {
        apt::gpu::afc_table(stream, d, batch, count);
        apt::hip_check(hipGetLastError(), "kernel launch (k_afc_table)");
    }
}

// stage C's launch after fm_launch_checks (apt_capi_fm.hip: aptgpu_fm_demodulate_device's checks)
void enqueue_tracked(const aptgpu_fm &fm, const apt::afc::Design &ad, const FmLaunch &t, int count,
                     const apt::gpu::AfcTables &tables)
{
    const apt::fm::Design &d = fm.design;
    const apt::gpu::FmParams p{fm.d_taps_rev.ptr, fm.d_offsets.ptr, d.T, d.D, fm.tile.R, fm.tile.nv, ad.pw_base,
                               d.swap ? 1u : 0u, d.step.re, d.step.im, d.gain};
    apt::gpu::fm_demodulate_tracked(fm.stream, d.format, fm.tile, t.batch, tables, count, t.max_tiles, p);
    apt::hip_check(hipGetLastError(), "kernel launch (k_fm_tracked)");
}

// the stage-B outputs a one-shot call hands out: released into the (nullable) out-parameters last
struct TableOut {
    HostPtr<Record> table;
    HostPtr<float> coherence;
    HostPtr<uint8_t> good;
    void give(aptgpu_afc_record **t, float **c, uint8_t **g)
    {
        if (t) *t = table.release();
        if (c) *c = coherence.release();
        if (g) *g = good.release();
    }
};

// the refusals every one-shot form shares -> nb.  tracked: stages A and B are skipped, the table is the caller's
uint64_t one_shot_checks(const Designs &d, const void *iq, size_t n_frames, bool tracked, const Record *table_in,
                         size_t n_blocks_in)
{
    const uint64_t nb = apt::afc::checked_blocks(d.afc, n_frames);
    if (tracked) {
        check_table_len(d.afc, n_frames, n_blocks_in);
        if (nb && !table_in) throw Error{ErrorKind::Invalid, "afc: table is null"};
    }
    if (!iq && n_frames) throw Error{ErrorKind::Invalid, "fm: iq is null"};
    return nb;
}

// one recording on host arrays through all three stages, or (tracked) through stage C with the caller's table
int one_shot(const aptgpu_context *ctx, const aptgpu_fm_settings *fs, const aptgpu_afc_settings *as, const void *iq,
             size_t n_frames, bool tracked, const Record *table_in, size_t n_blocks_in, float **audio, size_t *n_out,
             uint32_t *rate_hz,
             aptgpu_afc_record **table, float **coherence, uint8_t **good, size_t *n_blocks)
{
    const Designs checked = designs_of(fs, as);  // the refusals first: Scratch touches the device
    const uint64_t nb = one_shot_checks(checked, iq, n_frames, tracked, table_in, n_blocks_in);
    Scratch sc(ctx);
    aptgpu_fm fm;
    fm_setup(fm, fs, sc.device, sc.stream);
    apt::gpu::fm_tracked_prepare(fm.design.format, fm.tile);
    const size_t out = apt::fm::out_len(fm.design, n_frames);
    const size_t bytes = n_frames * 2u * apt::fm::component_bytes(fm.design.format);
    auto d_iq = upload(static_cast<const uint8_t *>(iq), bytes, sc.stream);
    apt::DeviceBuffer<float> d_audio, d_coh;
    apt::DeviceBuffer<double> d_sums;
    apt::DeviceBuffer<Record> d_table;
    apt::DeviceBuffer<uint8_t> d_good;
    d_audio.alloc(out + 16);
    if (tracked) {
        d_table = upload(table_in, nb, sc.stream);
    } else {
        d_sums.alloc(3 * nb + 16);
        d_table.alloc(nb + 16);
        d_coh.alloc(nb + 16);
        d_good.alloc(nb + 16);
        apt::gpu::AfcBatch batch{};
        batch.r[0] = apt::gpu::AfcRecording{d_iq.ptr, n_frames, d_sums.ptr, d_table.ptr, d_coh.ptr, d_good.ptr};
        enqueue_estimate(sc.stream, fm.design, checked.afc, batch, 1, true, true);
    }
    const void *in = d_iq.ptr;
    float *dst = d_audio.ptr;
    const FmLaunch t = fm_launch_checks(fm, 1, &in, &n_frames, &dst, &out);
    apt::gpu::AfcTables tables{};
    tables.table[0] = d_table.ptr;
    tables.log2_B = checked.afc.log2_B;
    enqueue_tracked(fm, checked.afc, t, 1, tables);
    HostSignal a(download(d_audio.ptr, out, sc.stream));
    TableOut to;
    if (!tracked) {
        if (table) to.table.reset(download(d_table.ptr, nb, sc.stream));
        if (coherence) to.coherence.reset(download(d_coh.ptr, nb, sc.stream));
        if (good) to.good.reset(download(d_good.ptr, nb, sc.stream));
    }
    apt::hip_check(hipStreamSynchronize(sc.stream), "hipStreamSynchronize");
    to.give(table, coherence, good);
    if (n_blocks) *n_blocks = nb;
    *audio = a.release();
    *n_out = out;
    if (rate_hz) *rate_hz = fm.design.fs_out;
    return APTGPU_OK;
}

int one_shot_host(const aptgpu_fm_settings *fs, const aptgpu_afc_settings *as, const void *iq, size_t n_frames,
                  bool tracked, const Record *table_in, size_t n_blocks_in, float **audio, size_t *n_out,
                  uint32_t *rate_hz,
                  aptgpu_afc_record **table, float **coherence, uint8_t **good, size_t *n_blocks)
{
    const Designs d = designs_of(fs, as);
    const uint64_t nb = one_shot_checks(d, iq, n_frames, tracked, table_in, n_blocks_in);
    const size_t out = apt::fm::out_len(d.fm, n_frames);
    TableOut to;
    const Record *use = table_in;
    if (!tracked) {
        std::vector<double> sums(3 * nb);
        apt::afc::sums_host(d.fm, d.afc, iq, n_frames, sums.data());
        to.table.reset(host_alloc<Record>(nb));
        to.coherence.reset(host_alloc<float>(nb));
        to.good.reset(host_alloc<uint8_t>(nb));
        apt::afc::table_host(d.afc, sums.data(), nb, to.table.get(), to.coherence.get(), to.good.get());
        use = to.table.get();
    }
    HostSignal a(host_alloc<float>(out));
    apt::afc::tracked_host(d.fm, d.afc, iq, n_frames, use, a.get());
    to.give(table, coherence, good);
    if (n_blocks) *n_blocks = nb;
    *audio = a.release();
    *n_out = out;
    if (rate_hz) *rate_hz = d.fm.fs_out;
    return APTGPU_OK;
}

void clear_outputs(float **audio, size_t *n_out, aptgpu_afc_record **table, float **coherence, uint8_t **good,
                   size_t *n_blocks)
{
    if (audio) *audio = nullptr;
    if (n_out) *n_out = 0;
    if (table) *table = nullptr;
    if (coherence) *coherence = nullptr;
    if (good) *good = nullptr;
    if (n_blocks) *n_blocks = 0;
}

}  // namespace

extern "C" {

void aptgpu_fm_afc_default_settings(aptgpu_afc_settings *s)
{
    if (s) apt::afc::default_settings(s);
}

int aptgpu_fm_afc_design(const aptgpu_fm_settings *fs, const aptgpu_afc_settings *as, aptgpu_afc_info *info, char *err,
                         size_t err_cap)
{
    if (!info || info->struct_size < sizeof(aptgpu_afc_info)) {
        put_err(err, err_cap, "aptgpu_afc_info: struct_size not set");
        return APTGPU_ERR_INVALID;
    }
    return guarded(err, err_cap, [&] {
        const Designs d = designs_of(fs, as);
        info->block_frames = d.afc.B;
        info->lag = d.afc.L;
        info->smooth_blocks = d.afc.W;
        info->pw_base = d.afc.pw_base;
        info->sample_rate_hz = d.afc.fs;
        info->max_offset_hz = d.afc.max_offset_hz;
        info->min_coherence = d.afc.min_coherence;
        return APTGPU_OK;
    });
}

int aptgpu_fm_afc_sums(const aptgpu_context *ctx, const aptgpu_fm_settings *fs, const aptgpu_afc_settings *as,
                       const void *iq, size_t n_frames, double **sums, size_t *n_blocks, char *err, size_t err_cap)
{
    if (!sums || !n_blocks) return APTGPU_ERR_INVALID;
    *sums = nullptr;
    *n_blocks = 0;
    return guarded(err, err_cap, [&] {
        const Designs d = designs_of(fs, as);
        const uint64_t nb = apt::afc::checked_blocks(d.afc, n_frames);
        if (!iq && n_frames) throw Error{ErrorKind::Invalid, "fm: iq is null"};
        Scratch sc(ctx);
        const size_t bytes = n_frames * 2u * apt::fm::component_bytes(d.fm.format);
        auto d_iq = upload(static_cast<const uint8_t *>(iq), bytes, sc.stream);
        apt::DeviceBuffer<double> d_sums;
        d_sums.alloc(3 * nb + 16);
        apt::gpu::AfcBatch batch{};
        batch.r[0] = apt::gpu::AfcRecording{d_iq.ptr, n_frames, d_sums.ptr, nullptr, nullptr, nullptr};
        enqueue_estimate(sc.stream, d.fm, d.afc, batch, 1, true, false);
        *sums = download(d_sums.ptr, 3 * nb, sc.stream);
        apt::hip_check(hipStreamSynchronize(sc.stream), "hipStreamSynchronize");
        *n_blocks = nb;
        return APTGPU_OK;
    });
}

int aptgpu_fm_afc_sums_host(const aptgpu_fm_settings *fs, const aptgpu_afc_settings *as, const void *iq, size_t n_frames,
                            double **sums, size_t *n_blocks, char *err, size_t err_cap)
{
    if (!sums || !n_blocks) return APTGPU_ERR_INVALID;
    *sums = nullptr;
    *n_blocks = 0;
    return guarded(err, err_cap, [&] {
        const Designs d = designs_of(fs, as);
        const uint64_t nb = apt::afc::checked_blocks(d.afc, n_frames);
        if (!iq && n_frames) throw Error{ErrorKind::Invalid, "fm: iq is null"};
        HostPtr<double> p(host_alloc<double>(3 * nb));
        apt::afc::sums_host(d.fm, d.afc, iq, n_frames, p.get());
        *sums = p.release();
        *n_blocks = nb;
        return APTGPU_OK;
    });
}

int aptgpu_fm_afc_estimate(const aptgpu_context *ctx, const aptgpu_fm_settings *fs, const aptgpu_afc_settings *as,
                           const double *sums, size_t n_blocks, aptgpu_afc_record **table, float **coherence,
                           uint8_t **good, char *err, size_t err_cap)
{
    if (!table) return APTGPU_ERR_INVALID;
    clear_outputs(nullptr, nullptr, table, coherence, good, nullptr);
    return guarded(err, err_cap, [&] {
        const Designs d = designs_of(fs, as);
        if (n_blocks > apt::afc::kMaxBlocks) throw Error{ErrorKind::Invalid, "afc: n_blocks is above 2^20"};
        if (!sums && n_blocks) throw Error{ErrorKind::Invalid, "afc: sums is null"};
        Scratch sc(ctx);
        auto d_sums = upload(sums, 3 * n_blocks, sc.stream);
        apt::DeviceBuffer<Record> d_table;
        apt::DeviceBuffer<float> d_coh;
        apt::DeviceBuffer<uint8_t> d_good;
        d_table.alloc(n_blocks + 16);
        d_coh.alloc(n_blocks + 16);
        d_good.alloc(n_blocks + 16);
        apt::gpu::AfcBatch batch{};
        // (stage B reads the block count from the frame count: any n with ceil(n / B) == n_blocks)
        batch.r[0] = apt::gpu::AfcRecording{nullptr, static_cast<uint64_t>(n_blocks) << d.afc.log2_B, d_sums.ptr,
                                            d_table.ptr, d_coh.ptr, d_good.ptr};
        enqueue_estimate(sc.stream, d.fm, d.afc, batch, 1, false, true);
        TableOut to;
        to.table.reset(download(d_table.ptr, n_blocks, sc.stream));
        if (coherence) to.coherence.reset(download(d_coh.ptr, n_blocks, sc.stream));
        if (good) to.good.reset(download(d_good.ptr, n_blocks, sc.stream));
        apt::hip_check(hipStreamSynchronize(sc.stream), "hipStreamSynchronize");
        to.give(table, coherence, good);
        return APTGPU_OK;
    });
}

int aptgpu_fm_afc_estimate_host(const aptgpu_fm_settings *fs, const aptgpu_afc_settings *as, const double *sums,
                                size_t n_blocks, aptgpu_afc_record **table, float **coherence, uint8_t **good, char *err,
                                size_t err_cap)
{
    if (!table) return APTGPU_ERR_INVALID;
    clear_outputs(nullptr, nullptr, table, coherence, good, nullptr);
    return guarded(err, err_cap, [&] {
        const Designs d = designs_of(fs, as);
        if (n_blocks > apt::afc::kMaxBlocks) throw Error{ErrorKind::Invalid, "afc: n_blocks is above 2^20"};
        if (!sums && n_blocks) throw Error{ErrorKind::Invalid, "afc: sums is null"};
        TableOut to;
        to.table.reset(host_alloc<Record>(n_blocks));
        to.coherence.reset(host_alloc<float>(n_blocks));
        to.good.reset(host_alloc<uint8_t>(n_blocks));
        apt::afc::table_host(d.afc, sums, n_blocks, to.table.get(), to.coherence.get(), to.good.get());
        to.give(table, coherence, good);
        return APTGPU_OK;
    });
}

int aptgpu_fm_demodulate_tracked(const aptgpu_context *ctx, const aptgpu_fm_settings *fs, const aptgpu_afc_settings *as,
                                 const void *iq, size_t n_frames, const aptgpu_afc_record *table, size_t n_blocks,
                                 float **audio, size_t *n_out, uint32_t *rate_hz, char *err, size_t err_cap)
{
    if (!audio || !n_out) return APTGPU_ERR_INVALID;
    clear_outputs(audio, n_out, nullptr, nullptr, nullptr, nullptr);
    return guarded(err, err_cap, [&] {
        return one_shot(ctx, fs, as, iq, n_frames, true, table, n_blocks, audio, n_out, rate_hz, nullptr, nullptr,
                        nullptr, nullptr);
    });
}

int aptgpu_fm_demodulate_tracked_host(const aptgpu_fm_settings *fs, const aptgpu_afc_settings *as, const void *iq,
                                      size_t n_frames, const aptgpu_afc_record *table, size_t n_blocks, float **audio,
                                      size_t *n_out, uint32_t *rate_hz, char *err, size_t err_cap)
{
    if (!audio || !n_out) return APTGPU_ERR_INVALID;
    clear_outputs(audio, n_out, nullptr, nullptr, nullptr, nullptr);
    return guarded(err, err_cap, [&] {
        return one_shot_host(fs, as, iq, n_frames, true, table, n_blocks, audio, n_out, rate_hz, nullptr, nullptr,
                             nullptr, nullptr);
    });
}

int aptgpu_fm_demodulate_afc(const aptgpu_context *ctx, const aptgpu_fm_settings *fs, const aptgpu_afc_settings *as,
                             const void *iq, size_t n_frames, float **audio, size_t *n_out, uint32_t *rate_hz,
                             aptgpu_afc_record **table, float **coherence, uint8_t **good, size_t *n_blocks, char *err,
                             size_t err_cap)
{
    if (!audio || !n_out) return APTGPU_ERR_INVALID;
    clear_outputs(audio, n_out, table, coherence, good, n_blocks);
    return guarded(err, err_cap, [&] {
        return one_shot(ctx, fs, as, iq, n_frames, false, nullptr, 0, audio, n_out, rate_hz, table, coherence, good, n_blocks);
    });
}

int aptgpu_fm_demodulate_afc_host(const aptgpu_fm_settings *fs, const aptgpu_afc_settings *as, const void *iq,
                                  size_t n_frames, float **audio, size_t *n_out, uint32_t *rate_hz,
                                  aptgpu_afc_record **table, float **coherence, uint8_t **good, size_t *n_blocks, char *err,
                                  size_t err_cap)
{
    if (!audio || !n_out) return APTGPU_ERR_INVALID;
    clear_outputs(audio, n_out, table, coherence, good, n_blocks);
    return guarded(err, err_cap, [&] {
        return one_shot_host(fs, as, iq, n_frames, false, nullptr, 0, audio, n_out, rate_hz, table, coherence, good, n_blocks);
    });
}

int aptgpu_fm_afc_create(aptgpu_fm *fm, const aptgpu_afc_settings *as, size_t max_frames, aptgpu_fm_afc **out, char *err,
                         size_t err_cap)
{
    if (!out) return APTGPU_ERR_INVALID;
    *out = nullptr;
    if (!fm) {
        put_err(err, err_cap, "afc: null argument");
        return APTGPU_ERR_INVALID;
    }
    return guarded(err, err_cap, [&] {
        auto afc = std::make_unique<aptgpu_fm_afc>();
        afc->fm = fm;
        afc->device = fm->device;
        afc->stream = fm->stream;
        afc->design = apt::afc::design_of(fm->design, fm->design.deviation_hz, as);  // before a device is touched
        afc->max_frames = max_frames;
        afc->max_blocks = apt::afc::checked_blocks(afc->design, max_frames);
        apt::hip_check(hipSetDevice(fm->device), "hipSetDevice");
        const size_t slots = static_cast<size_t>(apt::fm::kMaxBatch) * afc->max_blocks;
        afc->d_sums.alloc(3 * slots + 16);
        afc->d_table.alloc(slots + 16);
        afc->d_coherence.alloc(slots + 16);
        afc->d_good.alloc(slots + 16);
        apt::gpu::fm_tracked_prepare(fm->design.format, fm->tile);
        *out = afc.release();
        return APTGPU_OK;
    });
}

void aptgpu_fm_afc_destroy(aptgpu_fm_afc *afc)
{
    if (!afc) return;
    (void)hipSetDevice(afc->device);
    (void)hipStreamSynchronize(afc->stream);  // the work space may still be in use
    delete afc;
}

int aptgpu_fm_afc_demodulate_device(aptgpu_fm_afc *afc, int count, const void *const *d_iq, const size_t *n_frames,
                                    float *const *d_audio, const size_t *audio_cap, double *const *d_sums,
                                    aptgpu_afc_record *const *d_table, float *const *d_coherence, uint8_t *const *d_good,
                                    char *err, size_t err_cap)
{
    if (!afc || count < 0 || (count && (!d_iq || !n_frames || !d_audio || !audio_cap))) {
        put_err(err, err_cap, "afc: null argument");
        return APTGPU_ERR_INVALID;
    }
    return guarded(err, err_cap, [&] {
        aptgpu_fm &fm = *afc->fm;
        const FmLaunch t = fm_launch_checks(fm, count, d_iq, n_frames, d_audio, audio_cap);
        apt::gpu::AfcBatch batch{};
        apt::gpu::AfcTables tables{};
        tables.log2_B = afc->design.log2_B;
        for (int i = 0; i < count; ++i) {
            if (n_frames[i] > afc->max_frames) throw Error{ErrorKind::Invalid, "afc: n_frames is above max_frames"};
            if (n_frames[i] && !d_iq[i])  // (stage A reads the frames even where stage C has no output)
                throw Error{ErrorKind::Invalid, "fm: a null device pointer"};
            const size_t slot = static_cast<size_t>(i) * afc->max_blocks;
            double *su = d_sums && d_sums[i] ? d_sums[i] : afc->d_sums.ptr + 3 * slot;
            Record *tb = d_table && d_table[i] ? d_table[i] : afc->d_table.ptr + slot;
            float *co = d_coherence && d_coherence[i] ? d_coherence[i] : afc->d_coherence.ptr + slot;
            uint8_t *gd = d_good && d_good[i] ? d_good[i] : afc->d_good.ptr + slot;
            if (reinterpret_cast<uintptr_t>(su) % sizeof(double) != 0)
                throw Error{ErrorKind::Invalid, "afc: d_sums is not aligned to a double"};
            if (reinterpret_cast<uintptr_t>(tb) % sizeof(Record) != 0)
                throw Error{ErrorKind::Invalid, "afc: d_table is not aligned to 16 bytes"};
            if (reinterpret_cast<uintptr_t>(co) % sizeof(float) != 0)
                throw Error{ErrorKind::Invalid, "afc: d_coherence is not aligned to a float"};
            batch.r[i] = apt::gpu::AfcRecording{static_cast<const uint8_t *>(d_iq[i]), n_frames[i],
                                                su, tb, co, gd};
            tables.table[i] = tb;
        }
        apt::hip_check(hipSetDevice(fm.device), "hipSetDevice");
        enqueue_estimate(fm.stream, fm.design, afc->design, batch, count, true, true);
        enqueue_tracked(fm, afc->design, t, count, tables);
        return APTGPU_OK;
    });
}

}  // extern "C"
