// apt_plan.hpp — the decode() plan: designed taps, HBM workspace, stream, pipeline.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/aptgpu.h"
#include "apt_host.hpp"
#include "apt_image_request.hpp"
#include "apt_kernels.hpp"
#include "apt_kernels_color.hpp"
#include "apt_kernels_despeckle.hpp"
#include "apt_kernels_thermal.hpp"
#include "apt_kernels_geoloc.hpp"
#include "apt_kernels_eqfloat.hpp"
#include "apt_kernels_map.hpp"
#include "apt_kernels_png.hpp"
#include "apt_kernels_project.hpp"
#include "apt_wav.hpp"

namespace apt {

// Throws apt::Error on failure.
void hip_check(hipError_t e, const char *what);

template <typename T>
struct DeviceBuffer {
    T *ptr = nullptr;
    size_t count = 0;
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    DeviceBuffer(DeviceBuffer &&o) noexcept : ptr(o.ptr), count(o.count) { o.ptr = nullptr; o.count = 0; }
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept
    {
        if (this != &o) {
            release();
            ptr = o.ptr;
            count = o.count;
            o.ptr = nullptr;
            o.count = 0;
        }
        return *this;
    }
    ~DeviceBuffer() { release(); }
    void alloc(size_t n)
    {
        release();
        count = n;
        if (n) hip_check(hipMalloc(reinterpret_cast<void **>(&ptr), n * sizeof(T)), "hipMalloc");
    }
    void release()
    {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        count = 0;
    }
};

// Event-pair timing of kernel launches on the plan's stream.
class KernelTimer {
public:
    ~KernelTimer();
    // 0 = off, 1 = every 8th launch flagged `dominant`, 2 = every launch
    void enable(int mode);
    int mode() const { return mode_; }
    void begin(hipStream_t s, const char *name, bool dominant);
    void end(hipStream_t s);
    // synchronises the stream, folds all recorded pairs into per-name averages
    std::vector<aptgpu_kernel_time> collect(hipStream_t s);

private:
    struct Pair {
        const char *name;
        hipEvent_t a, b;
    };
    int mode_ = 0;
    bool open_ = false;
    uint64_t sampled_ = 0;
    std::vector<Pair> pairs_;
    std::vector<hipEvent_t> pool_;
    hipEvent_t take();
};

}  // namespace apt

namespace apt {
// fast_resampling (dsp.rs:186-289) evaluated at t = off + d0 + k*step of the interpolated axis, k < w (apt_plan.hip):
// the export_resample_filtered branch (dsp.rs:265-273) — d0 = ResampleGeom::d0 and step = m for the output, d0 = 0 and
// step = 1 for the expanded signal
void resample_at(hipStream_t s, const float *x, uint64_t n, const float *coeff, uint32_t ntaps, uint32_t l, uint64_t d0,
                 uint32_t step, float *out, uint64_t w);

// One resample_with_filter stage (dsp.rs:62-126) on the device: its geometry, its taps in HBM and the fp16-taps option.
// decode()'s first resample, its final resample to 4160 Hz (NoFilter: one tap) and the WAV tool's are each one of these.
struct ResampleStage {
    ResampleGeom g;
    const float *d_taps = nullptr;
    const uint16_t *d_taps_f16 = nullptr;  // APTGPU_MODE_FP16_TAPS tables (apt::gpu::f16taps_pack), else null
    float f16_unscale = 1.f;
    // the name of enqueue()'s kernel in a plan's timing (aptgpu_plan_collect_timing): of decode()'s first stage, or of
    // its final one
    const char *label(bool final_stage) const;
    // the stage's output: the first w <= g.out_len(n) samples into d_out
    void enqueue(hipStream_t s, const float *d_x, uint64_t n, float *d_out, uint64_t w) const;
    // the signal of the stage's "resample_filtered" step, g.expanded_len(n) samples into d_out: the expanded signal
    // (l > 1: dsp.rs:269,281-285) or the filtered one before its decimation (l == 1: dsp.rs:108-114)
    void enqueue_filtered(hipStream_t s, const float *d_x, uint64_t n, float *d_out) const;

private:
    enum Kernel { kResampleAt, kResampleF16Taps, kResampleGeneric, kFirDecimate };
    Kernel kernel() const;
};
}  // namespace apt

// The opaque C-ABI plan: the host-side design of decode() (apt::PlanDesign: l, m, the taps, the sync geometry ...) and
// what runs it on the device.
struct aptgpu_plan : apt::PlanDesign {
    int device = 0;
    int mode = APTGPU_MODE_STRICT;
    // Pipeline over consecutive calls: the recordings of ONE decode_device call go through ONE launch
    // per stage (front end -> k_sync_words -> k_sync_slots -> k_sync_orbit -> k_gather_rows; blockIdx.y / .x picks
    // the recording, per-recording arguments travel by value in the kernel arguments), in order on
    // one of `depth` streams; consecutive calls go round-robin over the streams, so the front end
    // of call j+1 overlaps the latency-bound picker of call j.  Stream k owns the workspace slots
    // [k*max_batch, (k+1)*max_batch): a slot is only ever reused by a later call on its own stream
    // (in-order => no hazards, no cross-stream events, nothing for the host to wait on).
    std::vector<hipStream_t> streams;
    hipStream_t stream = nullptr;       // = streams[0] (host-API helpers, plan-creation uploads)
    // Batched plans serialise the fused front ends of consecutive calls: the front end of call j+1 (on its own
    // stream) waits for an event recorded behind the front end of call j (on another), so front ends run one
    // after the other, each with the whole GPU, and the picker / gather of call j overlap the front end of
    // call j+1.  Left alone, the front ends of `depth` consecutive calls start together, share the GPU,
    // finish together — and their latency-bound chains then run with nothing to overlap (a kernel trace showed
    // three calls marching in step: 2.4 ms of front ends, then 0.8 ms of chains).  Worth 7 % in a 20-step run
    // (477 against 445 Gsamples/s), nothing in a long one (the chains cost their own time either way).  The front
    // ends stay on the calls' own streams: on one stream of their own every chain starts an event hand-over later
    // (0.0588 against 0.053 ms per recording, profiles/r04_sweeps.txt).
    // Chosen from what the plan can see: max_batch >= 4, more than one stream, no user stream (create_streams).
    bool front_serial = false;
    std::vector<hipEvent_t> ev_front;   // [depth]: behind the front end of the latest call on that stream
    int prev_front = -1;                // stream index whose ev_front the next front end waits for
    hipStream_t user_stream = nullptr;  // ctx.stream: inputs are ordered after it (may be null)
    hipEvent_t ev_user = nullptr;
    uint64_t calls = 0;             // calls enqueued so far (stream = calls % depth)
    int last_stream = 0;            // stream index of the most recent call
    std::vector<int> last_slots;    // slot of recording i of the most recent decode_device call

    aptgpu_settings settings{};
    uint32_t input_rate = 0;
    bool sync = true;

    size_t max_samples = 0;
    uint64_t max_work_len = 0;
    uint32_t max_rows = 0;
    int max_batch = 1;
    // strict: RN(1/sinphi) if the exactly rounded fast divide verified for it, else 0 (apt_envelope.hpp);
    // fast mode: RN(1/sinphi)
    float inv_sinphi = 0.f;
    apt::gpu::FrontEnd fe{};  // the front end of the plan's calls, chosen once (apt::gpu::select_front_end)
    int fused() const { return static_cast<int>(fe.kind); }  // (stats.fused, aptgpu_plan_info.fused)
    apt::gpu::LaunchSwitches sw{};  // the A/B switches of the launch wrappers as the environment had them at plan creation
    apt::gpu::PlanSwitches psw{};   // ... and the switches of the plan's shape
    bool force_walk = false;  // APTGPU_FORCE_WALK=1: the picker's sequential fallback for every recording

    apt::DeviceBuffer<float> d_taps_resample, d_taps_lowpass, d_one, d_taps_branch, d_taps_lowpass_pairs, d_taps_any, d_taps_lowpass_pad;
    apt::DeviceBuffer<uint16_t> d_taps_f16;  // APTGPU_MODE_FP16_TAPS
    float f16_unscale = 1.f;
    struct Slot {
        apt::DeviceBuffer<float> resampled, demodulated, filtered;
        apt::DeviceBuffer<float> correlation;  // unfused kernels / step export only (the fused front ends never write it)
        apt::DeviceBuffer<uint64_t> bits;     // 64-bit terminal words (generic-mode picker)
        apt::DeviceBuffer<uint32_t> peaks;
        apt::DeviceBuffer<apt::gpu::GroupMax> gm;  // per-group maxima of the correlation
        apt::DeviceBuffer<uint64_t> words;    // 52-bit terminal words
        apt::DeviceBuffer<uint64_t> nanw;     // 52-bit words of NaN correlation positions
        apt::DeviceBuffer<uint32_t> slot_nt, slot_cnt, flags, orbit_ws;
        apt::DeviceBuffer<char> image_ws;  // scratch of the image stage, allocated on first use
        apt::DeviceBuffer<char> color_ws;  // histograms, tables and palette of the colour stage, on first use
        uint64_t palette_gen = 0;          // generation of the palette color_ws holds (0 = none)
        apt::DeviceBuffer<char> lab_ws;    // Lab tables + per-call RGBA table, on first use of the Lab path
        uint64_t lab_gen = 0;              // generation of the palette whose Lab tables lab_ws holds (0 = none)
        apt::DeviceBuffer<char> eqfloat_ws;  // counters, select records and thresholds of HISTOGRAM_FLOAT, on first use
        apt::DeviceBuffer<char> despeckle_ws;  // record + limits record of the despeckle stage, on first use
        apt::DeviceBuffer<char> thermal_ws;    // record, pixel parameters, telemetry record and row means of the thermal stage, on first use
        apt::DeviceBuffer<char> geoloc_ws;     // record, frame, height record and per-row sun vectors of the geolocation stage, on first use
        size_t geoloc_rows = 0;                // rows geoloc_ws has room for
        std::shared_ptr<void> landmask;        // the land mask stage's table, record and scratch (apt_capi_landmask.hip), on first use
        apt::DeviceBuffer<char> track_ws;      // scores, back-pointers, position lists and record of the flywheel sync stage, on first use
        std::unique_ptr<apt::map::Device> map;  // the map overlay's layer set, lists and track, on first use
        std::unique_ptr<apt::project::Device> project;  // the reprojection's graticule, record and PNG scratch, on first use
        apt::DeviceBuffer<char> png_ws;    // the PNG encoder's filtered stream, staging and chunk records, on first use
        apt::DeviceBuffer<float> ingest;   // WAV -> f32 staging when the fused PCM16 path does not apply
        // the k_fused instantiation the slot's last front-end launch ran: row of apt_kernels_fused_variants.hpp (-1:
        // k_fused_any or the unfused kernels) and whether it was the 16-bit PCM one (read_internal "fused_variant")
        int fused_variant = -1;
        bool fused_variant_i16 = false;
        // layout of `filtered` as the slot's last call left it (apt::gpu::f_index): 0 contiguous, else the plane length —
        // the k_fused instantiations write pixel-phase planes; k_fused_any, the unfused kernels and every step export do not
        uint32_t f_stride = 0;
    };
    std::vector<Slot> slots;
    apt::DeviceBuffer<apt::gpu::SlotPtrs> d_slots;  // the slots' pointers, for the per-call launches
    apt::DeviceBuffer<apt::gpu::FusedParams> d_fused_params;  // parameters of the specialised front end
    bool writes_planes() const { return fe.writes_planes(); }  // F in pixel-phase planes (apt::gpu::f_index)
    uint32_t plane_stride = 0;  // plane length of such a plan (f_plane_stride of max_work_len), else 0
    void upload_slot_table();                       // (re)writes d_slots + d_fused_params; synchronises plan->stream
    apt::DeviceBuffer<apt::gpu::Result> d_results;
    apt::DeviceBuffer<apt::gpu::ImageResult> d_image_results;  // one per slot, on first use
    // image stage (contrast limits -> u8, telemetry) of recording i of the last call, enqueued
    // behind its decode on the same stream
    void enqueue_image(int i, const float *d_rows, uint64_t rows_cap_floats, int contrast, float percent,
                       bool rotate, uint8_t *d_image);
    hipStream_t stream_of(int) { return streams[static_cast<size_t>(last_stream)]; }
    struct ImageTarget {
        Slot &slot;
        hipStream_t stream;
        uint64_t cap;  // floats of the rows buffer the image stage may read
        void *ws;
        apt::gpu::ImageResult *out;
        const apt::gpu::Result *res;
    };
    ImageTarget image_target(int i, uint64_t rows_cap_floats);  // allocates the slot's scratch on first use
    static apt::ImageJob image_job(const ImageTarget &t, const float *d_rows)  // (the scratch pointers stay null)
    {
        return apt::ImageJob{t.stream, d_rows, t.res, 0, t.cap, t.ws, t.out};
    }
    template <typename Fn>
    void timed(hipStream_t s, const char *name, Fn &&launch)
    {
        timer.begin(s, name, false);
        launch();
        timer.end(s);
    }
    // The image stage under a request (the aptgpu_plan_process_device_image* entry points) of the first `count`
    // recordings of the last call, behind their decode on the same stream: one ImageJob per recording from its slot,
    // whose scratch is allocated on first use and whose palette / Lab tables are uploaded once per generation
    // (set_palette first), then the launches of apt_image_request.hpp.
    void enqueue_images(const apt::ImageRequest &q, int count, const float *const *d_rows, const size_t *rows_cap);
    // The composite (aptgpu_plan_composite_device_images) of the finished images of the first `count` recordings of
    // the last call: one ImageJob per pass from its slot (heights[i] rows of capacity; the height is the slot's
    // record's), the plan's composite device as the request's, then the launches of apt_image_request.hpp.  The
    // composite's record is the one past the passes' in aptgpu_plan_image_results.
    void enqueue_composite(apt::ImageRequest &q, int count, const uint32_t *heights);
    // per stream (calls in flight never share one): pass table, graticule, record and PNG scratch, on first use
    std::vector<std::unique_ptr<apt::composite::Device>> composite;
    int composite_count = -1;  // passes of the latest composite (-1: none since the last decode call)
    // The row stages of recording i, behind its decode on the same stream: the slot's scratch on first use, the
    // recording's job (image_job: the decode's record, the capacity), then the stage's launches of
    // apt_image_request.hpp, which the one-shot entry points go through too.  The record stays in the slot.
    // Despeckle: the limits go into the slot's image scratch, which the image stage behind it rewrites, and their
    // record beside the stage's own; d_out has d_rows' capacity and does not overlap it.
    void enqueue_despeckle(int i, const float *d_rows, uint64_t rows_cap_floats, int radius, float threshold,
                           float *d_out);
    // Thermal: launch.x / kelvin / image are the recording's buffers; the telemetry launches use the slot's image
    // scratch likewise.
    void enqueue_thermal(int i, uint64_t rows_cap_floats, const apt::gpu::ThermalLaunch &launch,
                         const apt::gpu::ThermalCoeffs &coeffs, const apt::gpu::ThermalTable &table);
    // Geolocation: launch.x and the output planes are the recording's buffers; the track goes into the slot's map
    // device, whose track and x offsets a later overlay or reprojection rewrites.
    void enqueue_geoloc(int i, uint64_t rows_cap_floats, const apt::gpu::GeolocLaunch &launch);
    // The false-colour palette (256*256*3 RGB).  The plan keeps a host copy; bytes that differ from it start a new
    // generation, which every slot uploads on its own stream the next time it colours an image.  lab: also the
    // palette's Lab tables (apt_lab.hpp), computed once per generation and uploaded per slot likewise.
    void set_palette(const uint8_t *rgb, bool lab = false);
    void new_palette(const uint8_t *rgb);  // (set_palette: the bytes differ)
    struct Palette {
        std::vector<uint8_t> rgb;   // the host copy the next call compares against
        uint32_t *pinned = nullptr; // packed RGBA of the current generation, the source of the slots' uploads
        std::vector<hipEvent_t> uploaded;  // per stream: behind its latest upload from `pinned` (null: none yet)
        uint64_t gen = 0;
        apt::lab::Tables *lab_pinned = nullptr;  // Lab tables of generation lab_gen
        std::vector<hipEvent_t> lab_uploaded;    // per stream: behind its latest upload from `lab_pinned`
        uint64_t lab_gen = 0;
        Palette() = default;
        Palette(const Palette &) = delete;
        Palette &operator=(const Palette &) = delete;
        ~Palette();
    } palette;

    apt::KernelTimer timer;

    // Settings.export_resample_filtered (config.rs:83 -> context.rs:113): fast_resampling then walks every t of the
    // interpolated axis and decimates at (t + 1) % m == 0 (dsp.rs:265-273) — another phase than the t = off + k*m of
    // the normal branch, whether or not anything is exported.  Such a plan runs the unfused kernels.
    bool export_filtered = false;
    // decode()'s two resample_with_filter stages: input rate -> work_rate, and (no-sync: decode.rs:158-159) the whole
    // rows at work_rate -> 4160 Hz with NoFilter
    apt::ResampleStage first_stage() const
    {
        return {{l, m, taps_resample.size(), export_filtered}, d_taps_resample.ptr, d_taps_f16.ptr, f16_unscale};
    }
    apt::ResampleStage final_stage() const { return {{l2, m2, 1, export_filtered}, d_one.ptr, nullptr, 1.f}; }

    // geometry for an n-sample recording
    uint64_t work_len_for(uint64_t n) const { return first_stage().g.out_len(n); }
    uint64_t whole_rows(uint64_t work_len) const { return spr ? work_len / spr * spr : 0; }  // decode.rs:142-147
    uint64_t out_len_nosync(uint64_t work_len) const { return final_stage().g.out_len(whole_rows(work_len)); }
    // floats the rows of an n-sample recording can take (what a rows buffer for it holds)
    uint64_t rows_bound(uint64_t n) const
    {
        const uint64_t w = work_len_for(n);
        return sync ? (spr ? w / spr + 2 : 2) * 2080u : out_len_nosync(w) + 16;
    }

    // what a recording looks like in HBM: the f32 Signal (codec < 0), or the payload of a WAV
    // data chunk (codec = apt::WavCodec) that is converted on the device — inside the fused
    // front end for mono PCM16, through the slot's staging buffer otherwise
    struct Input {
        const void *ptr = nullptr;
        uint64_t n = 0;  // samples of the Signal == WAV frames
        uint32_t channels = 1, bytes_per_sample = 4;
        int codec = -1;
        // from what describes a WAV payload: apt::WavInfo, or the C ABI's aptgpu_wav_spec
        template <typename Wav>
        static Input wav(const void *data, uint64_t n_frames, const Wav &w)
        {
            return {data, n_frames, w.channels, w.bytes_per_sample, static_cast<int>(w.codec)};
        }
    };
    // enqueue the whole decode() of the `count` device-resident recordings of one call (count <=
    // max_batch) on the next stream; never synchronises with the host.  keep_steps: unfused kernels,
    // every intermediate stays in the slot (Context::step export).
    void run_call(int count, const Input *ins, float *const *d_rows, const uint64_t *rows_cap_floats,
                  bool keep_steps);
    void sync_all();                // waits for every internal stream
    Slot &slot_of(int i) { return slots[static_cast<size_t>(last_slots[static_cast<size_t>(i)])]; }
    apt::gpu::Result *result_of(int i) { return d_results.ptr + last_slots[static_cast<size_t>(i)]; }
};

namespace apt {

// Builds a plan; throws apt::Error with the reference's messages.
aptgpu_plan *plan_create(const aptgpu_context *ctx, const aptgpu_settings &settings,
                         uint32_t input_rate, bool sync, size_t max_samples, int max_batch,
                         int depth = 0 /* calls in flight; 0 = default (APTGPU_STREAMS overrides) */);

}  // namespace apt
