// apt_capi_fm_handle.hpp — the aptgpu_fm handle of include/aptgpu.h §4b, shared by apt_capi_fm.hip (which creates it)
// and apt_capi_afc.hip (§4b': the tracked demodulator runs on its taps, device and stream).
#pragma once

#include "apt_kernels_fm.hpp"
#include "apt_plan.hpp"

struct aptgpu_fm {
    apt::fm::Design design;
    apt::fm::Tile tile{};
    int device = 0;
    hipStream_t stream = nullptr;
    apt::DeviceBuffer<float> d_taps_rev;
    apt::DeviceBuffer<uint32_t> d_offsets;
};

namespace apt::capi {
// What one launch over `count` recordings takes, after the checks of aptgpu_fm_demodulate_device (a null or misaligned
// pointer, audio_cap below the output length, more than APTGPU_FM_MAX_BATCH recordings, too many tiles): k_fm's and
// k_fm_tracked's.  Throws Error{Invalid}; nothing is enqueued here.
struct FmLaunch {
    apt::gpu::FmBatch batch{};
    uint32_t max_tiles = 0;
};
FmLaunch fm_launch_checks(const aptgpu_fm &fm, int count, const void *const *d_iq, const size_t *n_frames,
                          float *const *d_audio, const size_t *audio_cap);
// the demodulator's state on `stream` of `device`; the taps are on the device when this returns (apt_capi_fm.hip)
void fm_setup(aptgpu_fm &fm, const aptgpu_fm_settings *settings, int device, hipStream_t stream);
}  // namespace apt::capi
