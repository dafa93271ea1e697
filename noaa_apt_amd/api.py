"""ctypes binding of include/aptgpu.h with the reference's names (see package docstring)."""
import ctypes as C
import itertools
import os
import sys
import subprocess
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence

import numpy as np

FINAL_RATE = 4160    # decode.rs:14
PX_PER_ROW = 2080    # decode.rs:35
CARRIER_FREQ = 2400  # decode.rs:38

MODE_STRICT = 0
MODE_GENERIC = 1
MODE_FP16_TAPS = 2
MODE_FAST = 3

_HERE = os.path.dirname(os.path.abspath(__file__))
# The product library, in-tree.  No environment variable redirects this module to another shared object; timing tools
# that want the probe build (`make -C noaa_apt_amd/csrc probe-lib`) say so in code, through use_library().
_LIB = os.path.join(_HERE, "libaptgpu.so")
_f32p = C.POINTER(C.c_float)
_u64p = C.POINTER(C.c_uint64)
_i8p = C.POINTER(C.c_int8)
_u8p = C.POINTER(C.c_uint8)
_f64p = C.POINTER(C.c_double)
_u32p = C.POINTER(C.c_uint32)
_ERRCAP = 1024


# ------------------------------------------------------------------ errors (err.rs:9-44)
class AptError(Exception):
    code = -1


class InternalError(AptError):       # err::Error::Internal
    code = 1


class RateOverflowError(AptError):   # err::Error::RateOverflow
    code = 2


class HipError(AptError):            # device/runtime failure
    code = 3


class InvalidError(AptError):        # FFI misuse
    code = 4


class WavOpenError(AptError):        # err::Error::WavOpen
    code = 6


class IoError(AptError):             # err::Error::Io
    code = 7


class UnsupportedError(AptError):
    code = 5


class InvalidInputError(AptError):   # err::Error::InvalidInput (a palette that cannot be used)
    code = 8


_ERRORS = {c.code: c for c in (InternalError, RateOverflowError, HipError, InvalidError,
                               UnsupportedError, WavOpenError, IoError, InvalidInputError)}


def _check(rc, err=None):
    if rc != 0:
        msg = err.value.decode("utf-8", "replace") if err is not None else ""
        raise _ERRORS.get(rc, AptError)(msg or f"aptgpu status {rc}")


# ------------------------------------------------------------------ C structs
class _CFilter(C.Structure):
    _fields_ = [("kind", C.c_int32), ("cutout_pi_rad", C.c_float), ("atten", C.c_float),
                ("delta_w_pi_rad", C.c_float)]


class _CSettings(C.Structure):
    _fields_ = [("work_rate", C.c_uint32), ("resample_atten", C.c_float),
                ("resample_delta_freq", C.c_float), ("resample_cutout", C.c_float),
                ("demodulation_atten", C.c_float), ("export_wav", C.c_int32),
                ("export_resample_filtered", C.c_int32)]


_STATUS_FN = C.CFUNCTYPE(None, C.c_float, C.c_char_p, C.c_void_p)
_STEP_FN = C.CFUNCTYPE(C.c_int, C.c_char_p, C.c_int, _f32p, C.c_size_t, C.c_uint32, C.c_void_p)


class _CContext(C.Structure):
    _fields_ = [("status", _STATUS_FN), ("step", _STEP_FN), ("user", C.c_void_p),
                ("device", C.c_int32), ("mode", C.c_int32), ("stream", C.c_void_p)]


class Stats(C.Structure):
    _fields_ = [("work_len", C.c_uint64), ("n_sync", C.c_uint64), ("n_rows", C.c_uint64),
                ("l", C.c_uint32), ("m", C.c_uint32), ("n_resample_taps", C.c_uint32),
                ("n_lowpass_taps", C.c_uint32), ("fused", C.c_int32), ("orbit_path", C.c_int32)]


class PlanInfo(C.Structure):
    _fields_ = [("l", C.c_uint32), ("m", C.c_uint32), ("n_resample_taps", C.c_uint32),
                ("n_lowpass_taps", C.c_uint32), ("n_sync_taps", C.c_uint32),
                ("samples_per_work_row", C.c_uint32), ("min_distance", C.c_uint32),
                ("max_samples", C.c_uint64), ("max_work_len", C.c_uint64),
                ("max_rows", C.c_uint64), ("fused", C.c_int32), ("max_batch", C.c_int32)]


class Result(C.Structure):
    _fields_ = [("status", C.c_int32), ("reason", C.c_int32), ("n_rows", C.c_uint32),
                ("n_sync", C.c_uint32), ("work_len", C.c_uint64), ("n_out", C.c_uint64)]


class ImageResult(C.Structure):
    """aptgpu_image_result: contrast limits, image height and the telemetry values."""
    _fields_ = [("status", C.c_int32), ("reason", C.c_int32), ("height", C.c_uint32),
                ("telemetry_row", C.c_uint32), ("low", C.c_float), ("high", C.c_float),
                ("telemetry_quality", C.c_float), ("channel_a", C.c_int32), ("channel_b", C.c_int32),
                ("png_bytes", C.c_uint32), ("n_px", C.c_uint64), ("values_a", C.c_float * 16),
                ("values_b", C.c_float * 16)]

    @property
    def reserved(self):  # the field's name before the PNG entry points used it
        return self.png_bytes


class _CColorSettings(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("palette_rgb", _u8p),
                ("ch_a_tune_start", C.c_float), ("ch_a_tune_end", C.c_float),
                ("ch_b_tune_start", C.c_float), ("ch_b_tune_end", C.c_float)]


class _CPngSettings(C.Structure):
    """aptgpu_png_settings"""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32)]


class _COrbitSettings(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("sat_name", C.c_char_p), ("tle", C.c_char_p),
                ("ref_kind", C.c_int32), ("reserved", C.c_int32), ("ref_unix_ms", C.c_int64),
                ("draw_map", C.c_void_p)]


class _CMapSettings(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("yaw", C.c_double),
                ("hscale", C.c_double), ("vscale", C.c_double)]


class _CProjectionSettings(C.Structure):
    """aptgpu_projection_settings"""
    _fields_ = [("struct_size", C.c_uint32), ("kind", C.c_int32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("lat_north", C.c_double), ("lon_west", C.c_double), ("step", C.c_double), ("channel", C.c_int32),
                ("sampling", C.c_int32), ("grid_deg", C.c_double), ("grid_color", C.c_uint8 * 4),
                ("reserved", C.c_uint32)]


class _CCompositeSettings(C.Structure):
    """aptgpu_composite_settings"""
    _fields_ = [("struct_size", C.c_uint32), ("blend", C.c_int32), ("reserved", C.c_uint32)]


class _CDespeckleSettings(C.Structure):
    """aptgpu_despeckle_settings"""
    _fields_ = [("struct_size", C.c_uint32), ("radius", C.c_int32), ("threshold", C.c_float)]


class DespeckleResult(C.Structure):
    """aptgpu_despeckle_result: rows filtered, samples replaced, the 98 % limits and t = threshold * (high - low)."""
    _fields_ = [("status", C.c_int32), ("reason", C.c_int32), ("height", C.c_uint32), ("reserved", C.c_uint32),
                ("replaced", C.c_uint64), ("low", C.c_float), ("high", C.c_float), ("t", C.c_float),
                ("reserved2", C.c_uint32)]


class _CTrackSettings(C.Structure):
    """aptgpu_track_settings"""
    _fields_ = [("struct_size", C.c_uint32), ("max_jitter", C.c_uint32), ("penalty", C.c_float), ("reserved", C.c_uint32)]


class TrackResult(C.Structure):
    """aptgpu_track_result: positions and rows of the flywheel sync stage, the path's last position and its total."""
    _fields_ = [("struct_size", C.c_uint32), ("status", C.c_int32), ("reason", C.c_int32), ("n_positions", C.c_uint32),
                ("n_rows", C.c_uint32), ("end", C.c_uint32), ("n", C.c_uint64), ("total", C.c_float),
                ("reserved", C.c_uint32)]


class _CStreamSettings(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("input_rate_hz", C.c_uint32), ("sync", C.c_int32), ("format", C.c_int32),
                ("max_push", C.c_uint32), ("reserved", C.c_uint32)]


class StreamInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("work_rate", C.c_uint32), ("pw", C.c_uint32),
                ("samples_per_row", C.c_uint32), ("l", C.c_uint32), ("m", C.c_uint32),
                ("n_resample_taps", C.c_uint32), ("n_lowpass_taps", C.c_uint32), ("max_push", C.c_uint32),
                ("cap_in", C.c_uint32), ("cap_f", C.c_uint32), ("cap_corr", C.c_uint32), ("device_bytes", C.c_uint64)]


class StreamResult(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("status", C.c_int32), ("reason", C.c_int32), ("n_rows", C.c_uint32),
                ("rows_total", C.c_uint64), ("n_sync", C.c_uint64), ("n_in", C.c_uint64), ("work_len", C.c_uint64),
                ("scan_pos", C.c_uint64)]


class _CLiveTrackSettings(C.Structure):
    """aptgpu_live_track_settings"""
    _fields_ = [("struct_size", C.c_uint32), ("lag_rows", C.c_uint32), ("max_jitter", C.c_uint32), ("penalty", C.c_float)]


class StreamTrackResult(C.Structure):
    """aptgpu_stream_track_result: the live tracker's record."""
    _fields_ = [("struct_size", C.c_uint32), ("n_relocks", C.c_uint32), ("n_positions", C.c_uint64), ("m", C.c_uint64),
                ("next_checkpoint", C.c_uint64), ("last_position", C.c_uint64), ("has_position", C.c_int32),
                ("reserved", C.c_uint32), ("cap_best", C.c_uint32), ("cap_bp", C.c_uint32)]


class _CThermalCoeffs(C.Structure):
    """aptgpu_thermal_coeffs"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("prt", (C.c_double * 3) * 4),
                ("channel", (C.c_double * 7) * 3)]


class _CThermalSettings(C.Structure):
    """aptgpu_thermal_settings"""
    _fields_ = [("struct_size", C.c_uint32), ("channel", C.c_int32), ("channel_id", C.c_int32),
                ("image_channels", C.c_int32), ("flags", C.c_uint32), ("t_low", C.c_float), ("t_high", C.c_float),
                ("reserved", C.c_uint32), ("palette", C.c_void_p)]


class ThermalResult(C.Structure):
    """aptgpu_thermal_result: the frame and identity used, the f64 scalars of the calibration and what the Kelvin
    plane holds (n_nan, t_min, t_max)."""
    _fields_ = [("status", C.c_int32), ("reason", C.c_int32), ("height", C.c_uint32), ("telemetry_row", C.c_uint32),
                ("channel_id", C.c_int32), ("reserved", C.c_uint32), ("n_nan", C.c_uint64), ("slope", C.c_double),
                ("icpt", C.c_double), ("space", C.c_double), ("c_space", C.c_double), ("c_bb", C.c_double),
                ("t_bb", C.c_double), ("n_bb", C.c_double), ("t_min", C.c_float), ("t_max", C.c_float)]


class _CGeolocSettings(C.Structure):
    """aptgpu_geoloc_settings"""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("channel", C.c_int32), ("time_kind", C.c_int32),
                ("unix_ms", C.c_int64), ("black_level", C.c_float), ("max_zenith_deg", C.c_float)]


class GeolocResult(C.Structure):
    """aptgpu_geoloc_result: the height, the pixels beyond the geometry's limit (n_outside), those whose cos_sun is
    below the cap (n_capped) and the extremes of cos_sun over the valid pixels."""
    _fields_ = [("struct_size", C.c_uint32), ("status", C.c_int32), ("reason", C.c_int32), ("height", C.c_uint32),
                ("n_outside", C.c_uint64), ("n_capped", C.c_uint64), ("cos_min", C.c_float), ("cos_max", C.c_float)]


class _CLandMaskSettings(C.Structure):
    """aptgpu_land_mask_settings"""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("n_bands", C.c_int32), ("reserved", C.c_int32)]


class LandMaskResult(C.Structure):
    """aptgpu_land_mask_result: the height (0 in the plane forms), the points of each class and the size of the
    acceleration table (non-horizontal edges of countries and lakes, band entries of both)."""
    _fields_ = [("struct_size", C.c_uint32), ("status", C.c_int32), ("reason", C.c_int32), ("height", C.c_uint32),
                ("n_sea", C.c_uint64), ("n_land", C.c_uint64), ("n_lake", C.c_uint64), ("n_invalid", C.c_uint64),
                ("n_edges", C.c_uint32 * 2), ("n_band_entries", C.c_uint64)]


class _CFitSettings(C.Structure):
    """aptgpu_fit_settings"""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("channel", C.c_int32), ("layer_mask", C.c_uint32),
                ("margin_rows", C.c_int32), ("rounds", C.c_int32), ("radius", C.c_int32), ("min_points", C.c_int32),
                ("shift_step", C.c_int32), ("n_shift", C.c_int32), ("n_yaw", C.c_int32), ("n_hscale", C.c_int32),
                ("n_vscale", C.c_int32), ("timing", C.c_int32), ("yaw_step", C.c_double), ("hscale_step", C.c_double),
                ("vscale_step", C.c_double), ("spacing_deg", C.c_double)]


class FitRound(C.Structure):
    """aptgpu_fit_round: the centre a round started from, its winner and the winner's sums."""
    _fields_ = [("c_yaw", C.c_double), ("c_hscale", C.c_double), ("c_vscale", C.c_double), ("w_yaw", C.c_double),
                ("w_hscale", C.c_double), ("w_vscale", C.c_double), ("q", C.c_double), ("c_shift", C.c_int32),
                ("w_shift", C.c_int32), ("count", C.c_uint32), ("index", C.c_uint32), ("score", C.c_uint64)]


class FitResult(C.Structure):
    """aptgpu_fit_result"""
    _fields_ = [("struct_size", C.c_uint32), ("status", C.c_int32), ("reason", C.c_int32), ("height", C.c_uint32),
                ("n_rounds", C.c_uint32), ("n_points", C.c_uint32), ("n_candidates", C.c_uint32),
                ("shift_rows", C.c_int32), ("time_offset_ms", C.c_int64), ("yaw", C.c_double), ("hscale", C.c_double),
                ("vscale", C.c_double), ("q", C.c_double), ("count", C.c_uint32), ("done", C.c_uint32),
                ("ms_edge", C.c_float), ("ms_angles", C.c_float), ("ms_score", C.c_float), ("ms_pick", C.c_float),
                ("round", FitRound * 8)]


class _CFmSettings(C.Structure):
    """aptgpu_fm_settings"""
    _fields_ = [("struct_size", C.c_uint32), ("format", C.c_int32), ("sample_rate_hz", C.c_uint32),
                ("decimation", C.c_uint32), ("shift_hz", C.c_double), ("channel_cutout_hz", C.c_float),
                ("channel_atten", C.c_float), ("channel_delta_hz", C.c_float), ("deviation_hz", C.c_float),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class _CFmInfo(C.Structure):
    """aptgpu_fm_info"""
    _fields_ = [("struct_size", C.c_uint32), ("fs_out", C.c_uint32), ("n_taps", C.c_uint32), ("decimation", C.c_uint32),
                ("pw", C.c_uint32), ("reserved", C.c_uint32), ("shift_hz_used", C.c_double), ("taps", _f32p)]


class _CAfcSettings(C.Structure):
    """aptgpu_afc_settings"""
    _fields_ = [("struct_size", C.c_uint32), ("block_frames", C.c_uint32), ("lag", C.c_uint32),
                ("smooth_blocks", C.c_uint32), ("max_offset_hz", C.c_float), ("min_coherence", C.c_float)]


class _CAfcInfo(C.Structure):
    """aptgpu_afc_info"""
    _fields_ = [("struct_size", C.c_uint32), ("block_frames", C.c_uint32), ("lag", C.c_uint32),
                ("smooth_blocks", C.c_uint32), ("pw_base", C.c_uint32), ("sample_rate_hz", C.c_uint32),
                ("max_offset_hz", C.c_double), ("min_coherence", C.c_double)]


class _CFmStreamSettings(C.Structure):
    """aptgpu_fm_stream_settings"""
    _fields_ = [("struct_size", C.c_uint32), ("max_push_frames", C.c_uint32), ("first_frame", C.c_uint64),
                ("reserved", C.c_uint64)]


class FmStreamInfo(C.Structure):
    """aptgpu_fm_stream_info: the aptgpu_fm_info fields, the frames pushed and the outputs returned so far, the frames
    held (carry_frames) and what the stream holds on the device."""
    _fields_ = [("struct_size", C.c_uint32), ("fs_out", C.c_uint32), ("n_taps", C.c_uint32), ("decimation", C.c_uint32),
                ("pw", C.c_uint32), ("carry_frames", C.c_uint32), ("shift_hz_used", C.c_double), ("taps", _f32p),
                ("frames", C.c_uint64), ("outputs", C.c_uint64), ("first_frame", C.c_uint64),
                ("device_bytes", C.c_uint64), ("max_push_frames", C.c_uint32), ("reserved", C.c_uint32)]


class _CIqLiveSettings(C.Structure):
    """aptgpu_iq_live_settings"""
    _fields_ = [("struct_size", C.c_uint32), ("sync", C.c_int32), ("max_push_frames", C.c_uint32),
                ("max_push", C.c_uint32), ("first_frame", C.c_uint64)]


class WavSpec(C.Structure):
    """aptgpu_wav_spec: hound::WavSpec plus where the samples are."""
    _fields_ = [("channels", C.c_uint16), ("bits_per_sample", C.c_uint16),
                ("bytes_per_sample", C.c_uint16), ("sample_format", C.c_uint16),
                ("sample_rate", C.c_uint32), ("codec", C.c_int32), ("data_offset", C.c_uint64),
                ("data_len", C.c_uint64), ("n_samples", C.c_uint64), ("n_frames", C.c_uint64)]


class BatchStats(C.Structure):
    """aptgpu_batch_stats: what a host-fed batch moved and how long it took."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32),
                ("seconds", C.c_double), ("samples", C.c_uint64), ("h2d_bytes", C.c_uint64),
                ("d2h_bytes", C.c_uint64), ("h2d_seconds", C.c_double), ("d2h_seconds", C.c_double),
                ("workers", C.c_int32), ("recordings_per_call", C.c_int32),
                ("gate_wait_seconds", C.c_double), ("setup_seconds", C.c_double),
                ("sessions_created", C.c_int32), ("workers_pinned", C.c_int32)]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("avg_ms", C.c_double), ("launches", C.c_uint64)]


# ------------------------------------------------------------------ library loading
_lib = None


def lib_path():
    return _LIB


def use_library(path):
    """tools/ only: load `path` (the probe build, libaptgpu_probe.so — same ABI, APTGPU_DEBUG_* switches that leave
    kernels out, so its rows can be garbage) instead of the product library.  Must be called before the first lib();
    says so on stderr."""
    global _LIB
    if _lib is not None:
        raise RuntimeError("use_library() after the library was loaded")
    _LIB = os.path.abspath(path)
    sys.stderr.write(f"aptgpu: loading {_LIB} instead of the product library (timing experiments only)\n")


def build():
    """Compile libaptgpu.so in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "-s", "-j8", "all"])


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm bundles its own libamdhip64.so whose SONAME
    (libamdhip64.so.7) equals /opt/rocm's; whichever is loaded first satisfies the other's
    NEEDED entry only in one direction (torch asks for "libamdhip64.so").  Loading torch's
    copy first makes libaptgpu.so and torch share it, so torch tensors' device pointers and
    streams are valid in our launches regardless of import order.  Without torch installed,
    libaptgpu.so's RUNPATH finds /opt/rocm's runtime as usual."""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def lib():
    """The loaded libaptgpu.so.  Raises if it has not been built — there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    _preload_hip_runtime()
    if not os.path.exists(_LIB):
        raise ImportError(f"{_LIB} is missing: run `python -c 'import __graft_entry__ as g; "
                          f"g.build()'` (or `make -C noaa_apt_amd/csrc`) first")
    L = C.CDLL(_LIB)
    vp, sz, u32, i32 = C.c_void_p, C.c_size_t, C.c_uint32, C.c_int
    L.aptgpu_version.restype = C.c_char_p
    L.aptgpu_abi_version.restype = C.c_int
    L.aptgpu_device_count.restype = i32
    L.aptgpu_free.argtypes = [vp]
    L.aptgpu_free.restype = None
    L.aptgpu_cache_clear.argtypes = []
    L.aptgpu_cache_clear.restype = None
    L.aptgpu_cache_info.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]
    L.aptgpu_cache_info.restype = None
    L.aptgpu_decode.argtypes = [C.POINTER(_CContext), C.POINTER(_CSettings), _f32p, sz, u32, i32,
                                C.POINTER(_f32p), C.POINTER(sz), C.POINTER(Stats), C.c_char_p, sz]
    L.aptgpu_plan_create.argtypes = [C.POINTER(_CContext), C.POINTER(_CSettings), u32, i32, sz,
                                     i32, C.POINTER(vp), C.c_char_p, sz]
    L.aptgpu_plan_destroy.argtypes = [vp]
    L.aptgpu_plan_destroy.restype = None
    L.aptgpu_plan_get_info.argtypes = [vp, C.POINTER(PlanInfo)]
    L.aptgpu_plan_decode_device.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp),
                                            C.POINTER(sz), C.c_char_p, sz]
    L.aptgpu_plan_results.argtypes = [vp, i32, C.POINTER(Result)]
    L.aptgpu_plan_sync_positions.argtypes = [vp, i32, _u64p, sz, C.POINTER(sz)]
    L.aptgpu_plan_synchronize.argtypes = [vp]
    L.aptgpu_plan_join.argtypes = [vp]
    L.aptgpu_plan_read_internal.argtypes = [vp, i32, C.c_char_p, vp, sz, C.POINTER(sz)]
    L.aptgpu_plan_enable_timing.argtypes = [vp, i32]
    L.aptgpu_plan_collect_timing.argtypes = [vp, C.POINTER(KernelTime), sz, C.POINTER(sz)]
    L.aptgpu_filter_design.argtypes = [C.POINTER(_CFilter), C.POINTER(_f32p), C.POINTER(sz)]
    L.aptgpu_filter_resample.argtypes = [C.POINTER(_CFilter), u32, u32]
    L.aptgpu_lab_from_rgb.argtypes = [_u8p, sz, _f32p]
    L.aptgpu_lab_to_rgb.argtypes = [_f32p, sz, _u8p]
    L.aptgpu_filter_resample.restype = None
    L.aptgpu_generate_sync_frame.argtypes = [u32, C.POINTER(_i8p), C.POINTER(sz), C.c_char_p, sz]
    L.aptgpu_resample_with_filter.argtypes = [C.POINTER(_CContext), _f32p, sz, u32, u32, _CFilter,
                                              C.POINTER(_f32p), C.POINTER(sz), C.c_char_p, sz]
    L.aptgpu_resample.argtypes = [C.POINTER(_CContext), _f32p, sz, u32, u32, C.c_float, C.c_float,
                                  C.POINTER(_f32p), C.POINTER(sz), C.c_char_p, sz]
    L.aptgpu_demodulate.argtypes = [C.POINTER(_CContext), _f32p, sz, C.c_float, C.POINTER(_f32p),
                                    C.c_char_p, sz]
    L.aptgpu_filter_signal.argtypes = [C.POINTER(_CContext), _f32p, sz, _CFilter, C.POINTER(_f32p),
                                       C.c_char_p, sz]
    L.aptgpu_find_sync.argtypes = [C.POINTER(_CContext), _f32p, sz, u32, C.POINTER(_u64p),
                                   C.POINTER(sz), C.POINTER(_f32p), C.POINTER(sz), C.c_char_p, sz]
    cp, f = C.POINTER(_CContext), C.c_float
    wsp = C.POINTER(WavSpec)
    L.aptgpu_wav_parse.argtypes = [C.c_char_p, sz, wsp, C.c_char_p, sz]
    L.aptgpu_load_wav.argtypes = [cp, C.c_char_p, sz, C.POINTER(_f32p), C.POINTER(sz), C.POINTER(u32),
                                  wsp, C.c_char_p, sz]
    L.aptgpu_load_wav_file.argtypes = [cp, C.c_char_p, C.POINTER(_f32p), C.POINTER(sz), C.POINTER(u32),
                                       wsp, C.c_char_p, sz]
    L.aptgpu_decode_wav.argtypes = [cp, C.POINTER(_CSettings), C.c_char_p, sz, i32, C.POINTER(_f32p),
                                    C.POINTER(sz), C.POINTER(Stats), C.POINTER(u32), C.c_char_p, sz]
    L.aptgpu_write_wav_i16.argtypes = [cp, _f32p, sz, u32, C.POINTER(vp), C.POINTER(sz), C.c_char_p, sz]
    L.aptgpu_resample_wav.argtypes = [cp, C.c_char_p, sz, u32, f, f, C.c_char_p, C.POINTER(vp),
                                      C.POINTER(sz), C.c_char_p, sz]
    L.aptgpu_resample_wav_file.argtypes = [cp, C.c_char_p, C.c_char_p, u32, f, f, C.c_char_p, sz]
    L.aptgpu_resample_wav_ex.argtypes = [cp, C.c_char_p, sz, u32, f, f, i32, C.c_char_p, C.POINTER(vp),
                                         C.POINTER(sz), C.c_char_p, sz]
    L.aptgpu_resample_wav_file_ex.argtypes = [cp, C.c_char_p, C.c_char_p, u32, f, f, i32, C.c_char_p, sz]
    L.aptgpu_plan_decode_device_wav.argtypes = [vp, i32, C.POINTER(vp), wsp, C.POINTER(vp),
                                                C.POINTER(sz), C.c_char_p, sz]
    i32p = C.POINTER(C.c_int32)
    for name in ("aptgpu_decode_batch", "aptgpu_decode_batch_wav"):
        getattr(L, name).argtypes = [cp, C.POINTER(_CSettings), u32, i32, i32, C.POINTER(vp), C.POINTER(sz), i32p, i32,
                                     i32, C.POINTER(_f32p), C.POINTER(sz), i32p, C.POINTER(Result),
                                     C.POINTER(BatchStats), C.c_char_p, sz]
    L.aptgpu_host_alloc.argtypes = [sz]
    L.aptgpu_host_alloc.restype = vp
    L.aptgpu_host_free.argtypes = [vp]
    L.aptgpu_host_free.restype = None
    L.aptgpu_host_affinity.argtypes = [i32, C.c_char_p, C.POINTER(C.c_int32), C.c_char_p, sz]
    L.aptgpu_host_affinity_from_sysfs.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_int32), C.c_char_p, sz]
    L.aptgpu_get_min.argtypes = [cp, _f32p, sz, _f32p, C.c_char_p, sz]
    L.aptgpu_get_max.argtypes = [cp, _f32p, sz, _f32p, C.c_char_p, sz]
    L.aptgpu_percent.argtypes = [cp, _f32p, sz, f, _f32p, _f32p, C.c_char_p, sz]
    L.aptgpu_map_signal_u8.argtypes = [cp, _f32p, sz, f, f, C.POINTER(_u8p), C.c_char_p, sz]
    L.aptgpu_read_telemetry.argtypes = [cp, _f32p, sz, C.POINTER(ImageResult), C.c_char_p, sz]
    L.aptgpu_channel_name.argtypes = [i32]
    L.aptgpu_channel_name.restype = C.c_char_p
    L.aptgpu_process_gray.argtypes = [cp, _f32p, sz, i32, f, i32, C.POINTER(_u8p), C.POINTER(sz),
                                      C.POINTER(ImageResult), C.c_char_p, sz]
    L.aptgpu_plan_process_device.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(sz), i32, f, i32,
                                             C.POINTER(vp), C.c_char_p, sz]
    L.aptgpu_plan_image_results.argtypes = [vp, i32, C.POINTER(ImageResult)]
    ccs = C.POINTER(_CColorSettings)
    L.aptgpu_process_image.argtypes = [cp, _f32p, sz, i32, f, i32, ccs, i32, C.POINTER(_u8p), C.POINTER(sz),
                                       C.POINTER(ImageResult), C.c_char_p, sz]
    L.aptgpu_plan_process_device_image.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(sz), i32, f, i32, ccs, i32,
                                                   C.POINTER(vp), C.c_char_p, sz]
    cms = C.POINTER(_CMapSettings)
    L.aptgpu_map_layers_create.argtypes = [C.POINTER(vp)]
    L.aptgpu_map_layers_destroy.argtypes = [vp]
    L.aptgpu_map_layers_destroy.restype = None
    L.aptgpu_map_layers_load_dir.argtypes = [vp, C.c_char_p, C.c_char_p, sz]
    L.aptgpu_map_layers_set.argtypes = [vp, i32, _f64p, sz, _u32p, sz, C.c_char_p, sz]
    L.aptgpu_map_layers_set_color.argtypes = [vp, i32, _u8p]
    L.aptgpu_map_read_shapefile.argtypes = [C.c_char_p, i32, C.POINTER(_f64p), C.POINTER(sz), C.POINTER(_u32p),
                                            C.POINTER(sz), C.c_char_p, sz]
    L.aptgpu_process_image_map.argtypes = [cp, _f32p, sz, i32, f, i32, ccs, i32, cms, vp, _f64p, C.POINTER(_u8p),
                                           C.POINTER(sz), C.POINTER(ImageResult), C.c_char_p, sz]
    L.aptgpu_plan_process_device_image_map.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(sz), i32, f, i32, ccs, i32,
                                                       cms, vp, C.POINTER(_f64p), C.POINTER(sz), C.POINTER(vp),
                                                       C.c_char_p, sz]
    cps = C.POINTER(_CPngSettings)
    cos = C.POINTER(_COrbitSettings)
    L.aptgpu_sat_track.argtypes = [cp, cos, u32, _f64p, C.c_char_p, sz]
    L.aptgpu_sat_track_host.argtypes = [cos, u32, _f64p, C.c_char_p, sz]
    L.aptgpu_south_to_north_pass.argtypes = [cos, C.POINTER(C.c_int), C.c_char_p, sz]
    L.aptgpu_process_image_orbit.argtypes = [cp, _f32p, sz, i32, f, i32, ccs, i32, cos, vp, i32, cps,
                                             C.POINTER(_u8p), C.POINTER(sz), C.POINTER(ImageResult), C.c_char_p, sz]
    L.aptgpu_plan_process_device_image_orbit.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(sz), i32, f, i32, ccs, i32,
                                                         C.POINTER(cos), vp, C.POINTER(vp), cps, C.POINTER(vp),
                                                         C.POINTER(sz), C.c_char_p, sz]
    L.aptgpu_png_bound.argtypes = [u32, u32, i32]
    L.aptgpu_png_bound.restype = sz
    L.aptgpu_encode_png.argtypes = [cp, _u8p, u32, u32, i32, cps, C.POINTER(_u8p), C.POINTER(sz), C.c_char_p, sz]
    L.aptgpu_process_image_png.argtypes = [cp, _f32p, sz, i32, f, i32, ccs, i32, cms, vp, _f64p, cps, C.POINTER(_u8p),
                                           C.POINTER(sz), C.POINTER(ImageResult), C.c_char_p, sz]
    L.aptgpu_plan_process_device_image_png.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(sz), i32, f, i32, ccs, i32,
                                                       cms, vp, C.POINTER(_f64p), C.POINTER(sz), C.POINTER(vp), cps,
                                                       C.POINTER(vp), C.POINTER(sz), C.c_char_p, sz]
    cpr = C.POINTER(_CProjectionSettings)
    L.aptgpu_projection_fit.argtypes = [_f64p, sz, C.c_double, i32, C.c_double, u32, cpr, C.c_char_p, sz]
    L.aptgpu_project_image.argtypes = [cp, _u8p, u32, i32, _f64p, sz, cms, cpr, i32, cps, C.POINTER(_u8p),
                                       C.POINTER(sz), C.c_char_p, sz]
    L.aptgpu_process_image_project.argtypes = [cp, _f32p, sz, i32, f, i32, ccs, i32, cms, vp, _f64p, cos, cpr, i32, cps,
                                               C.POINTER(_u8p), C.POINTER(sz), C.POINTER(ImageResult), C.c_char_p, sz]
    L.aptgpu_plan_process_device_image_project.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(sz), i32, f, i32, ccs, i32,
                                                           cms, vp, C.POINTER(_f64p), C.POINTER(sz), C.POINTER(cos),
                                                           C.POINTER(vp), cpr, C.POINTER(vp), C.POINTER(sz), cps,
                                                           C.POINTER(vp), C.POINTER(sz), C.c_char_p, sz]
    cco = C.POINTER(_CCompositeSettings)
    L.aptgpu_projection_fit_many.argtypes = [C.POINTER(_f64p), C.POINTER(sz), sz, C.c_double, i32, C.c_double, u32, cpr,
                                             C.c_char_p, sz]
    L.aptgpu_composite_images.argtypes = [cp, i32, C.POINTER(_u8p), _u32p, i32p, C.POINTER(_f64p), C.POINTER(sz),
                                          C.POINTER(cms), cpr, cco, i32, cps, C.POINTER(_u8p), C.POINTER(sz),
                                          C.POINTER(_u8p), C.c_char_p, sz]
    L.aptgpu_plan_composite_device_images.argtypes = [vp, i32, C.POINTER(vp), _u32p, i32p, C.POINTER(_f64p),
                                                      C.POINTER(sz), C.POINTER(cos), C.POINTER(cms), cpr, cco, vp, sz,
                                                      vp, cps, vp, sz, C.c_char_p, sz]
    cds = C.POINTER(_CDespeckleSettings)
    L.aptgpu_despeckle.argtypes = [cp, _f32p, sz, cds, C.POINTER(_f32p), C.POINTER(DespeckleResult), C.c_char_p, sz]
    L.aptgpu_despeckle_host.argtypes = [_f32p, sz, cds, C.POINTER(_f32p), C.POINTER(DespeckleResult), C.c_char_p, sz]
    L.aptgpu_plan_despeckle_device.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(sz), cds, C.POINTER(vp), C.c_char_p, sz]
    L.aptgpu_plan_despeckle_results.argtypes = [vp, i32, C.POINTER(DespeckleResult)]
    cth = (C.POINTER(_CThermalCoeffs), C.POINTER(_CThermalSettings))
    L.aptgpu_calibrate_thermal.argtypes = [cp, _f32p, sz, *cth, C.POINTER(_f32p), C.POINTER(_u8p),
                                           C.POINTER(ThermalResult), C.c_char_p, sz]
    L.aptgpu_calibrate_thermal_host.argtypes = [_f32p, sz, *cth, C.POINTER(_f32p), C.POINTER(_u8p),
                                                C.POINTER(ThermalResult), C.c_char_p, sz]
    L.aptgpu_plan_calibrate_thermal_device.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(sz), *cth, C.POINTER(vp),
                                                       C.POINTER(vp), C.c_char_p, sz]
    L.aptgpu_plan_thermal_results.argtypes = [vp, i32, C.POINTER(ThermalResult)]
    geo = (_f64p, sz, C.POINTER(_COrbitSettings), C.POINTER(_CMapSettings), C.POINTER(_CGeolocSettings),
           C.POINTER(_f64p), C.POINTER(_f32p), C.POINTER(_f32p), C.POINTER(GeolocResult), C.c_char_p, sz)
    L.aptgpu_geolocate.argtypes = [cp, _f32p, sz, *geo]
    L.aptgpu_geolocate_host.argtypes = [_f32p, sz, *geo]
    L.aptgpu_sun_position.argtypes = [C.c_int64, _f64p]
    L.aptgpu_plan_geolocate_device.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(sz), C.POINTER(_f64p), C.POINTER(sz),
                                               C.POINTER(C.POINTER(_COrbitSettings)), C.POINTER(_CMapSettings),
                                               C.POINTER(_CGeolocSettings), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                               C.c_char_p, sz]
    L.aptgpu_plan_geoloc_results.argtypes = [vp, i32, C.POINTER(GeolocResult)]
    fit = (_f64p, sz, C.POINTER(_COrbitSettings), vp, C.POINTER(_CMapSettings), C.POINTER(_CFitSettings),
           C.POINTER(FitResult), C.POINTER(vp), C.POINTER(sz), C.c_char_p, sz)
    L.aptgpu_fit_default_settings.argtypes = [C.POINTER(_CFitSettings)]
    L.aptgpu_fit_default_settings.restype = None
    L.aptgpu_fit_overlay.argtypes = [cp, _u8p, sz, *fit]
    L.aptgpu_fit_overlay_device.argtypes = [cp, vp, sz, vp, *fit]
    L.aptgpu_fit_overlay_host.argtypes = [_u8p, sz, *fit]
    L.aptgpu_fit_sample_points.argtypes = [vp, C.c_uint32, C.c_double, C.POINTER(_f64p), C.POINTER(sz), C.c_char_p, sz]
    clm, rlm = C.POINTER(_CLandMaskSettings), C.POINTER(LandMaskResult)
    land = (sz, _f64p, sz, C.POINTER(_COrbitSettings), C.POINTER(_CMapSettings), vp, clm, C.POINTER(_u8p), rlm,
            C.c_char_p, sz)
    L.aptgpu_land_mask.argtypes = [cp, *land]
    L.aptgpu_land_mask_host.argtypes = [*land]
    L.aptgpu_land_mask_plane.argtypes = [cp, vp, sz, vp, clm, C.POINTER(_u8p), rlm, C.c_char_p, sz]
    L.aptgpu_land_mask_plane_host.argtypes = [vp, sz, vp, clm, C.POINTER(_u8p), rlm, C.c_char_p, sz]
    L.aptgpu_plan_land_mask_device.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(sz), C.POINTER(_f64p), C.POINTER(sz),
                                               C.POINTER(C.POINTER(_COrbitSettings)), C.POINTER(_CMapSettings), vp, clm,
                                               C.POINTER(vp), C.c_char_p, sz]
    L.aptgpu_plan_land_mask_results.argtypes = [vp, i32, rlm]
    fcm = (_u8p, sz, _u8p, sz, C.POINTER(vp), C.POINTER(sz), _f32p, C.POINTER(_u8p), C.c_char_p, sz)
    L.aptgpu_false_color_masked.argtypes = [cp, *fcm]
    L.aptgpu_false_color_masked_host.argtypes = [*fcm]
    cfm = C.POINTER(_CFmSettings)
    fm_out = (C.POINTER(_f32p), C.POINTER(sz), _u32p, C.c_char_p, sz)
    L.aptgpu_fm_default_settings.argtypes = [cfm]
    L.aptgpu_fm_default_settings.restype = None
    L.aptgpu_fm_design.argtypes = [cfm, C.POINTER(_CFmInfo), C.POINTER(_f32p), C.c_char_p, sz]
    L.aptgpu_fm_create.argtypes = [cp, cfm, C.POINTER(vp), C.c_char_p, sz]
    L.aptgpu_fm_destroy.argtypes = [vp]
    L.aptgpu_fm_destroy.restype = None
    L.aptgpu_fm_get_info.argtypes = [vp, C.POINTER(_CFmInfo)]
    L.aptgpu_fm_out_len.argtypes = [vp, sz]
    L.aptgpu_fm_out_len.restype = sz
    L.aptgpu_fm_demodulate.argtypes = [cp, cfm, vp, sz, *fm_out]
    L.aptgpu_fm_demodulate_host.argtypes = [cfm, vp, sz, *fm_out]
    L.aptgpu_fm_demodulate_device.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz),
                                              C.c_char_p, sz]
    L.aptgpu_fm_demodulate_wav.argtypes = [cp, cfm, C.c_char_p, sz, *fm_out]
    cafc = C.POINTER(_CAfcSettings)
    f64p, u8p = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    afc_table_out = (C.POINTER(_u32p), C.POINTER(_f32p), C.POINTER(u8p))
    L.aptgpu_fm_afc_default_settings.argtypes = [cafc]
    L.aptgpu_fm_afc_default_settings.restype = None
    L.aptgpu_fm_afc_design.argtypes = [cfm, cafc, C.POINTER(_CAfcInfo), C.c_char_p, sz]
    L.aptgpu_fm_afc_sums.argtypes = [cp, cfm, cafc, vp, sz, C.POINTER(f64p), C.POINTER(sz), C.c_char_p, sz]
    L.aptgpu_fm_afc_sums_host.argtypes = [cfm, cafc, vp, sz, C.POINTER(f64p), C.POINTER(sz), C.c_char_p, sz]
    L.aptgpu_fm_afc_estimate.argtypes = [cp, cfm, cafc, vp, sz, *afc_table_out, C.c_char_p, sz]
    L.aptgpu_fm_afc_estimate_host.argtypes = [cfm, cafc, vp, sz, *afc_table_out, C.c_char_p, sz]
    L.aptgpu_fm_demodulate_tracked.argtypes = [cp, cfm, cafc, vp, sz, vp, sz, *fm_out]
    L.aptgpu_fm_demodulate_tracked_host.argtypes = [cfm, cafc, vp, sz, vp, sz, *fm_out]
    L.aptgpu_fm_demodulate_afc.argtypes = [cp, cfm, cafc, vp, sz, *fm_out[:3], *afc_table_out, C.POINTER(sz), C.c_char_p, sz]
    L.aptgpu_fm_demodulate_afc_host.argtypes = [cfm, cafc, vp, sz, *fm_out[:3], *afc_table_out, C.POINTER(sz), C.c_char_p, sz]
    L.aptgpu_fm_afc_create.argtypes = [vp, cafc, sz, C.POINTER(vp), C.c_char_p, sz]
    L.aptgpu_fm_afc_destroy.argtypes = [vp]
    L.aptgpu_fm_afc_destroy.restype = None
    L.aptgpu_fm_afc_demodulate_device.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz),
                                                  C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.c_char_p, sz]
    cts, ctr = C.POINTER(_CTrackSettings), C.POINTER(TrackResult)
    L.aptgpu_track_sync.argtypes = [cp, i32, C.POINTER(_f32p), C.POINTER(sz), u32, cts, C.POINTER(_u64p),
                                    C.POINTER(_f32p), C.POINTER(_f32p), ctr, C.c_char_p, sz]
    L.aptgpu_track_sync_host.argtypes = [_f32p, sz, u32, cts, C.POINTER(_u64p), C.POINTER(_f32p), C.POINTER(_f32p),
                                         C.POINTER(_f32p), ctr, C.c_char_p, sz]
    L.aptgpu_sync_score.argtypes = [cp, i32, C.POINTER(_f32p), C.POINTER(sz), u32, C.POINTER(_f32p), C.c_char_p, sz]
    L.aptgpu_plan_track_device.argtypes = [vp, i32, cts, C.POINTER(vp), C.POINTER(sz), C.c_char_p, sz]
    L.aptgpu_plan_track_results.argtypes = [vp, i32, ctr]
    L.aptgpu_plan_track_positions.argtypes = [vp, i32, _u64p, _f32p, sz, C.POINTER(sz)]
    L.aptgpu_decode_tracked.argtypes = [cp, C.POINTER(_CSettings), _f32p, sz, u32, cts, C.POINTER(_f32p), C.POINTER(sz),
                                        C.POINTER(_u64p), C.POINTER(_f32p), ctr, C.c_char_p, sz]
    css, csr = C.POINTER(_CStreamSettings), C.POINTER(StreamResult)
    for name in ("aptgpu_stream_create", "aptgpu_stream_create_host"):
        getattr(L, name).argtypes = [cp, C.POINTER(_CSettings), css, C.POINTER(vp), C.c_char_p, sz]
    L.aptgpu_stream_destroy.argtypes = [vp]
    L.aptgpu_stream_destroy.restype = None
    L.aptgpu_stream_get_info.argtypes = [vp, C.POINTER(StreamInfo)]
    L.aptgpu_stream_reset.argtypes = [vp, C.c_char_p, sz]
    L.aptgpu_stream_rows_bound.argtypes = [vp, sz]
    L.aptgpu_stream_rows_bound.restype = sz
    L.aptgpu_stream_push.argtypes = [vp, vp, sz, _f32p, _u64p, sz, csr, C.c_char_p, sz]
    L.aptgpu_stream_finish.argtypes = [vp, _f32p, _u64p, sz, csr, C.c_char_p, sz]
    L.aptgpu_stream_push_device.argtypes = [vp, vp, sz, vp, vp, sz, C.c_char_p, sz]
    L.aptgpu_stream_finish_device.argtypes = [vp, vp, vp, sz, C.c_char_p, sz]
    L.aptgpu_stream_results.argtypes = [vp, csr, C.c_char_p, sz]
    for name in ("aptgpu_stream_create_tracked", "aptgpu_stream_create_tracked_host"):
        getattr(L, name).argtypes = [cp, C.POINTER(_CSettings), css, C.POINTER(_CLiveTrackSettings), C.POINTER(vp),
                                     C.c_char_p, sz]
    L.aptgpu_stream_track_scores.argtypes = [vp, _f32p, sz, C.POINTER(sz), C.c_char_p, sz]
    L.aptgpu_stream_track_scores_device.argtypes = [vp, vp, C.c_char_p, sz]
    L.aptgpu_stream_track_results.argtypes = [vp, C.POINTER(StreamTrackResult), C.c_char_p, sz]
    cfss = C.POINTER(_CFmStreamSettings)
    L.aptgpu_fm_stream_create.argtypes = [cp, cfm, cfss, C.POINTER(vp), C.c_char_p, sz]
    L.aptgpu_fm_stream_create_host.argtypes = [cfm, cfss, C.POINTER(vp), C.c_char_p, sz]
    L.aptgpu_fm_stream_destroy.argtypes = [vp]
    L.aptgpu_fm_stream_destroy.restype = None
    L.aptgpu_fm_stream_reset.argtypes = [vp, C.c_char_p, sz]
    L.aptgpu_fm_stream_get_info.argtypes = [vp, C.POINTER(FmStreamInfo)]
    L.aptgpu_fm_stream_out_len.argtypes = [vp, sz]
    L.aptgpu_fm_stream_out_len.restype = sz
    L.aptgpu_fm_stream_push.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz), C.c_char_p, sz]
    L.aptgpu_fm_stream_push_device.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz), C.c_char_p, sz]
    for name in ("aptgpu_iq_live_create", "aptgpu_iq_live_create_host"):
        getattr(L, name).argtypes = [cp, C.POINTER(_CSettings), cfm, C.POINTER(_CIqLiveSettings), C.POINTER(vp),
                                     C.c_char_p, sz]
    L.aptgpu_iq_live_destroy.argtypes = [vp]
    L.aptgpu_iq_live_destroy.restype = None
    L.aptgpu_iq_live_reset.argtypes = [vp, C.c_char_p, sz]
    L.aptgpu_iq_live_get_info.argtypes = [vp, C.POINTER(FmStreamInfo), C.POINTER(StreamInfo)]
    L.aptgpu_iq_live_rows_bound.argtypes = [vp, sz]
    L.aptgpu_iq_live_rows_bound.restype = sz
    L.aptgpu_iq_live_push.argtypes = [vp, vp, sz, _f32p, _u64p, sz, csr, C.c_char_p, sz]
    L.aptgpu_iq_live_finish.argtypes = [vp, _f32p, _u64p, sz, csr, C.c_char_p, sz]
    L.aptgpu_iq_live_push_device.argtypes = [vp, vp, sz, vp, vp, sz, C.c_char_p, sz]
    L.aptgpu_iq_live_finish_device.argtypes = [vp, vp, vp, sz, C.c_char_p, sz]
    L.aptgpu_iq_live_results.argtypes = [vp, csr, C.c_char_p, sz]
    for name in ("aptgpu_iq_live_create_tracked", "aptgpu_iq_live_create_tracked_host"):
        getattr(L, name).argtypes = [cp, C.POINTER(_CSettings), cfm, C.POINTER(_CIqLiveSettings),
                                     C.POINTER(_CLiveTrackSettings), C.POINTER(vp), C.c_char_p, sz]
    L.aptgpu_iq_live_track_scores.argtypes = [vp, _f32p, sz, C.POINTER(sz), C.c_char_p, sz]
    L.aptgpu_iq_live_track_scores_device.argtypes = [vp, vp, C.c_char_p, sz]
    L.aptgpu_iq_live_track_results.argtypes = [vp, C.POINTER(StreamTrackResult), C.c_char_p, sz]
    _lib = L
    return L


def version():
    return lib().aptgpu_version().decode()


def abi_version():
    return int(lib().aptgpu_abi_version())


def device_count():
    return int(lib().aptgpu_device_count())


def cache_clear():
    """Releases every idle session (plan + device buffers) of the host-array entry points' cache."""
    lib().aptgpu_cache_clear()


def cache_info():
    """(idle sessions, device bytes they hold)."""
    e, b = C.c_int32(0), C.c_uint64(0)
    lib().aptgpu_cache_info(C.byref(e), C.byref(b))
    return int(e.value), int(b.value)


def host_affinity(device=0):
    """(PCI address, NUMA node, CPU list) a batch worker of `device` pins itself to; node -1 / '' when the
    platform does not say."""
    bdf, node, cpus = C.create_string_buffer(32), C.c_int32(-1), C.create_string_buffer(4096)
    lib().aptgpu_host_affinity(int(device), bdf, C.byref(node), cpus, 4096)
    return bdf.value.decode(), int(node.value), cpus.value.decode()


def host_affinity_from_sysfs(sysfs_root, pci_bdf):
    """The same lookup on a PCI address under a given sysfs root (no GPU needed): (NUMA node, CPU list)."""
    node, cpus = C.c_int32(-1), C.create_string_buffer(4096)
    rc = lib().aptgpu_host_affinity_from_sysfs(str(sysfs_root).encode(), str(pci_bdf).encode(), C.byref(node), cpus, 4096)
    if rc != 0:
        raise InvalidError("bad argument to aptgpu_host_affinity_from_sysfs")
    return int(node.value), cpus.value.decode()


class _Owned:
    """A buffer the library malloc'd, exposed to numpy without a copy (ten megabytes of rows per ten-minute recording:
    a copy costs as much as a fifth of the decode); aptgpu_free runs when the last array viewing it is gone."""
    __slots__ = ("addr", "free", "__array_interface__")

    def __init__(self, addr, n, dtype):
        self.addr = addr
        self.free = lib().aptgpu_free  # (bound now: module globals may be gone when the last array dies at exit)
        self.__array_interface__ = {"shape": (n,), "typestr": np.dtype(dtype).str, "data": (addr, False), "version": 3}

    def __del__(self):
        self.free(self.addr)


def _take(ptr, n, dtype=np.float32):
    n = int(n)
    addr = C.cast(ptr, C.c_void_p).value
    if n and addr and C.sizeof(ptr._type_) == np.dtype(dtype).itemsize:
        return np.asarray(_Owned(addr, n, dtype))
    out = np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True) if n else np.zeros(0, dtype)
    lib().aptgpu_free(C.cast(ptr, C.c_void_p))
    return out


def _as_f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(_f32p)


# ------------------------------------------------------------------ frequency.rs
@dataclass(frozen=True)
class Rate:
    """Sample rate in Hz (frequency.rs:98-117)."""
    hz_: int

    @staticmethod
    def hz(r):
        return Rate(int(r))

    def get_hz(self):
        return self.hz_


@dataclass(frozen=True)
class Freq:
    """Discrete-time frequency as a fraction of pi rad/sample, f32 (frequency.rs:30-88)."""
    pi_rad_: float

    @staticmethod
    def pi_rad(f):
        return Freq(float(np.float32(f)))

    @staticmethod
    def hz(f, rate: Rate):
        return Freq(float(np.float32(2.0) * np.float32(f) / np.float32(rate.get_hz())))

    def get_pi_rad(self):
        return self.pi_rad_

    def __truediv__(self, o):
        return Freq(float(np.float32(self.pi_rad_) / np.float32(o)))


# ------------------------------------------------------------------ config.rs / context.rs
@dataclass
class Settings:
    """The config::Settings fields decode() reads; defaults = the `standard` profile
    (/root/reference/src/default_settings.toml:108-116)."""
    work_rate: int = 12480
    resample_atten: float = 30.0
    resample_delta_freq: float = 1000.0
    resample_cutout: float = 4800.0
    demodulation_atten: float = 25.0
    export_wav: bool = False
    export_resample_filtered: bool = False
    # used only by the WAV->WAV resample tool (config.rs:100-106)
    wav_resample_atten: float = 40.0
    wav_resample_delta_freq: float = 0.1

    @staticmethod
    def profile(name):
        p = {"standard": dict(work_rate=12480, resample_atten=30.0, resample_delta_freq=1000.0,
                              resample_cutout=4800.0, demodulation_atten=25.0,
                              wav_resample_atten=40.0, wav_resample_delta_freq=0.1),
             "fast": dict(work_rate=16640, resample_atten=30.0, resample_delta_freq=3000.0,
                          resample_cutout=4800.0, demodulation_atten=23.0,
                          wav_resample_atten=30.0, wav_resample_delta_freq=0.2),
             "slow": dict(work_rate=20800, resample_atten=40.0, resample_delta_freq=500.0,
                          resample_cutout=4800.0, demodulation_atten=25.0,
                          wav_resample_atten=50.0, wav_resample_delta_freq=0.05)}[name]
        return Settings(**p)

    def _c(self):
        return _CSettings(self.work_rate, self.resample_atten, self.resample_delta_freq,
                          self.resample_cutout, self.demodulation_atten,
                          1 if self.export_wav else 0, 1 if self.export_resample_filtered else 0)


@dataclass
class Context:
    """context::Context: progress callback + step export (context.rs:100-211)."""
    ui_callback: Optional[Callable[[float, str], None]] = None
    step_callback: Optional[Callable[[str, int, np.ndarray, Optional[int]], None]] = None
    device: int = 0
    mode: int = MODE_STRICT
    stream: int = 0
    _keep: list = field(default_factory=list, repr=False)

    @staticmethod
    def decode(ui_callback=None, step_callback=None, device=0, mode=MODE_STRICT):
        return Context(ui_callback, step_callback, device, mode)

    def _c(self):
        def status(progress, text, _user):
            if self.ui_callback:
                self.ui_callback(float(progress), text.decode())

        def step(ident, variant, data, n, rate, _user):
            if self.step_callback:
                arr = (np.ctypeslib.as_array(data, shape=(int(n),)).copy() if n
                       else np.zeros(0, np.float32))
                try:
                    self.step_callback(ident.decode(), int(variant), arr, int(rate) or None)
                except Exception:  # propagate like `?`
                    return 1
            return 0

        s, t = _STATUS_FN(status), _STEP_FN(step)
        self._keep = [s, t]
        return _CContext(s, t, None, self.device, self.mode, self.stream or None)


# ------------------------------------------------------------------ filters.rs
@dataclass
class NoFilter:
    kind = 0

    def _c(self):
        return _CFilter(0, 0.0, 0.0, 0.0)

    def design(self):
        return _design(self._c())

    def resample(self, input_rate: Rate, output_rate: Rate):
        pass


@dataclass
class Lowpass:
    cutout: Freq
    atten: float
    delta_w: Freq
    kind = 1

    def _c(self):
        return _CFilter(self.kind, self.cutout.get_pi_rad(), self.atten, self.delta_w.get_pi_rad())

    def design(self):
        return _design(self._c())

    def resample(self, input_rate: Rate, output_rate: Rate):
        c = self._c()
        lib().aptgpu_filter_resample(C.byref(c), input_rate.get_hz(), output_rate.get_hz())
        self.cutout, self.delta_w = Freq(float(c.cutout_pi_rad)), Freq(float(c.delta_w_pi_rad))


@dataclass
class LowpassDcRemoval(Lowpass):
    kind = 2


def _design(cf):
    out, n = _f32p(), C.c_size_t()
    _check(lib().aptgpu_filter_design(C.byref(cf), C.byref(out), C.byref(n)))
    return _take(out, n.value)


# ------------------------------------------------------------------ decode.rs / dsp.rs
def decode(context: Optional[Context], settings: Settings, signal, input_rate: Rate, sync: bool,
           return_stats=False):
    """noaa_apt::decode — returns the raw image, line by line (flat f32, rows*2080)."""
    ctx = (context or Context())
    cctx, cs = ctx._c(), settings._c()
    x, xp = _as_f32(signal)
    out, n, st = _f32p(), C.c_size_t(), Stats()
    err = C.create_string_buffer(_ERRCAP)
    rc = lib().aptgpu_decode(C.byref(cctx), C.byref(cs), xp, x.size, input_rate.get_hz(),
                             1 if sync else 0, C.byref(out), C.byref(n), C.byref(st), err, _ERRCAP)
    _check(rc, err)
    rows = _take(out, n.value)
    return (rows, st) if return_stats else rows


def resample_with_filter(context, signal, input_rate: Rate, output_rate: Rate, filt):
    cctx = (context or Context())._c()
    x, xp = _as_f32(signal)
    out, n = _f32p(), C.c_size_t()
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_resample_with_filter(C.byref(cctx), xp, x.size, input_rate.get_hz(),
                                             output_rate.get_hz(), filt._c(), C.byref(out),
                                             C.byref(n), err, _ERRCAP), err)
    return _take(out, n.value)


def resample(context, signal, input_rate: Rate, output_rate: Rate, atten, delta_w: Freq):
    cctx = (context or Context())._c()
    x, xp = _as_f32(signal)
    out, n = _f32p(), C.c_size_t()
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_resample(C.byref(cctx), xp, x.size, input_rate.get_hz(),
                                 output_rate.get_hz(), atten, delta_w.get_pi_rad(), C.byref(out),
                                 C.byref(n), err, _ERRCAP), err)
    return _take(out, n.value)


def demodulate(context, signal, carrier_freq: Freq):
    cctx = (context or Context())._c()
    x, xp = _as_f32(signal)
    out = _f32p()
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_demodulate(C.byref(cctx), xp, x.size, carrier_freq.get_pi_rad(),
                                   C.byref(out), err, _ERRCAP), err)
    return _take(out, x.size)


def filter(context, signal, filt):  # noqa: A001 - the reference's name (dsp.rs:386)
    cctx = (context or Context())._c()
    x, xp = _as_f32(signal)
    out = _f32p()
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_filter_signal(C.byref(cctx), xp, x.size, filt._c(), C.byref(out), err,
                                      _ERRCAP), err)
    return _take(out, x.size)


def find_sync(context, signal, work_rate: Rate, return_correlation=False):
    cctx = (context or Context())._c()
    x, xp = _as_f32(signal)
    pos, npos, corr, ncorr = _u64p(), C.c_size_t(), _f32p(), C.c_size_t()
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_find_sync(C.byref(cctx), xp, x.size, work_rate.get_hz(), C.byref(pos),
                                  C.byref(npos), C.byref(corr) if return_correlation else None,
                                  C.byref(ncorr), err, _ERRCAP), err)
    p = _take(pos, npos.value, np.uint64)
    return (p, _take(corr, ncorr.value)) if return_correlation else p


def generate_sync_frame(work_rate: Rate):
    out, n = _i8p(), C.c_size_t()
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_generate_sync_frame(work_rate.get_hz(), C.byref(out), C.byref(n), err,
                                            _ERRCAP), err)
    return _take(out, n.value, np.int8)


# ------------------------------------------------------------------ WAV ingest
def wav_parse(file_bytes: bytes) -> WavSpec:
    """hound::WavReader::new(...).spec() on an in-memory file image (host only)."""
    spec = WavSpec()
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_wav_parse(file_bytes, len(file_bytes), C.byref(spec), err, _ERRCAP), err)
    return spec


def load(input_filename, context=None, return_spec=False):
    """noaa_apt::load (noaa_apt.rs:114-130): (Signal, Rate).  Also accepts the file's bytes."""
    cctx = (context or Context())._c()
    out, n, rate, spec = _f32p(), C.c_size_t(), C.c_uint32(), WavSpec()
    err = C.create_string_buffer(_ERRCAP)
    if isinstance(input_filename, (bytes, bytearray, memoryview)):
        data = bytes(input_filename)
        _check(lib().aptgpu_load_wav(C.byref(cctx), data, len(data), C.byref(out), C.byref(n),
                                     C.byref(rate), C.byref(spec), err, _ERRCAP), err)
    else:
        _check(lib().aptgpu_load_wav_file(C.byref(cctx), os.fsencode(input_filename), C.byref(out),
                                          C.byref(n), C.byref(rate), C.byref(spec), err, _ERRCAP), err)
    res = (_take(out, n.value), Rate.hz(rate.value))
    return res + (spec,) if return_spec else res


def decode_wav(context: Optional[Context], settings: Settings, file_bytes: bytes, sync: bool,
               return_stats=False):
    """load() + decode() without the host-side f32 detour: the data chunk goes to the GPU as it
    is and is converted there (inside the fused front end for mono PCM16)."""
    cctx = (context or Context())._c()
    cs = settings._c()
    out, n, st, rate = _f32p(), C.c_size_t(), Stats(), C.c_uint32()
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_decode_wav(C.byref(cctx), C.byref(cs), file_bytes, len(file_bytes), int(sync),
                                   C.byref(out), C.byref(n), C.byref(st), C.byref(rate), err, _ERRCAP), err)
    rows = _take(out, n.value)
    return (rows, st) if return_stats else rows


def _take_bytes(ptr, n):
    out = C.string_at(ptr, n) if n else b""
    lib().aptgpu_free(ptr)
    return out


def write_wav(signal, sample_rate: Rate, context=None) -> bytes:
    """wav::write_wav (wav.rs:59-98) with the {1 channel, 16 bit, Int} spec: the file image."""
    cctx = (context or Context())._c()
    x, xp = _as_f32(signal)
    out, n = C.c_void_p(), C.c_size_t()
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_write_wav_i16(C.byref(cctx), xp, x.size, sample_rate.get_hz(), C.byref(out),
                                      C.byref(n), err, _ERRCAP), err)
    return _take_bytes(out, n.value)


def resample_wav(context, settings, input_wav, output_filename, output_rate: int):
    """resample::resample (resample.rs:17-71).  `input_wav` / `output_filename` are paths (the
    result is written, modification time copied) — or pass the input file's bytes and get the
    output file's bytes back (output_filename then only labels the status text)."""
    cctx = (context or Context())._c()
    atten, delta = settings.wav_resample_atten, settings.wav_resample_delta_freq
    flag = 1 if settings.export_resample_filtered else 0  # main.rs:125-130 -> Context::resample
    err = C.create_string_buffer(_ERRCAP)
    if isinstance(input_wav, (bytes, bytearray, memoryview)):
        data = bytes(input_wav)
        out, n = C.c_void_p(), C.c_size_t()
        name = os.fsencode(output_filename) if output_filename else None
        _check(lib().aptgpu_resample_wav_ex(C.byref(cctx), data, len(data), output_rate, atten, delta, flag, name,
                                            C.byref(out), C.byref(n), err, _ERRCAP), err)
        return _take_bytes(out, n.value)
    _check(lib().aptgpu_resample_wav_file_ex(C.byref(cctx), os.fsencode(input_wav), os.fsencode(output_filename),
                                             output_rate, atten, delta, flag, err, _ERRCAP), err)
    return None


# ------------------------------------------------------------------ consumers of the rows
class Contrast:
    """noaa_apt::Contrast (noaa_apt.rs:25-37).  HISTOGRAM takes MinMax limits (noaa_apt.rs:158), then
    equalises the histogram of each channel half (processing.rs:83-101).  HISTOGRAM_FLOAT is not a reference
    variant: the equalisation on the f32 signal, before the pixel values become integers (the reference's
    docs/development.md:105-106; APTGPU_CONTRAST_HISTOGRAM_FLOAT in include/aptgpu.h has the definition).  Gray
    images only: with a ColorSettings it raises UnsupportedError."""
    TELEMETRY, MINMAX, HISTOGRAM = ("telemetry",), ("minmax",), ("histogram",)
    HISTOGRAM_FLOAT = ("histogram_float",)

    @staticmethod
    def Percent(p):  # noqa: N802 - the reference's variant name
        return ("percent", float(p))

    @staticmethod
    def _c(contrast):
        kind = contrast[0]
        return ({"telemetry": 0, "percent": 1, "minmax": 2, "histogram": 3, "histogram_float": 4}[kind],
                contrast[1] if kind == "percent" else 0.0)


class Rotate:
    """noaa_apt::Rotate (noaa_apt.rs:52-60).  ORBIT decides from the satellite's pass (south_to_north_pass) and
    needs process(orbit=OrbitSettings(...))."""
    NO, YES, ORBIT = 0, 1, 2


def _rust_debug_str(text):
    """`{:?}` of a path (Rust's Debug for str): quoted, with backslashes and quotes escaped."""
    out = []
    for ch in str(text):
        if ch in '"\\':
            out.append("\\" + ch)
        elif ch == "\n":
            out.append("\\n")
        elif ch == "\r":
            out.append("\\r")
        elif ch == "\t":
            out.append("\\t")
        else:
            out.append(ch)
    return '"' + "".join(out) + '"'


COLOR_EQUALIZE_LAB = 1 << 0  # aptgpu_color_settings.flags


def lab_from_rgb(rgb):
    """Lab::from_rgb of the lab crate 0.11.0 (CPU, aptgpu_lab_from_rgb): (..., 3) uint8 -> (..., 3) float32 L, a, b."""
    x = np.ascontiguousarray(rgb, np.uint8)
    if x.shape[-1:] != (3,):
        raise InvalidError("lab_from_rgb: the last axis must hold R, G, B")
    out = np.empty(x.shape, np.float32)
    _check(lib().aptgpu_lab_from_rgb(x.ctypes.data_as(_u8p), x.size // 3, out.ctypes.data_as(_f32p)))
    return out


def lab_to_rgb(lab):
    """Lab::to_rgb of the lab crate 0.11.0 (CPU, aptgpu_lab_to_rgb) as the GPU's Lab path computes it:
    (..., 3) float32 L, a, b -> (..., 3) uint8."""
    x = np.ascontiguousarray(lab, np.float32)
    if x.shape[-1:] != (3,):
        raise InvalidError("lab_to_rgb: the last axis must hold L, a, b")
    out = np.empty(x.shape, np.uint8)
    _check(lib().aptgpu_lab_to_rgb(x.ctypes.data_as(_f32p), x.size // 3, out.ctypes.data_as(_u8p)))
    return out


class ColorSettings:
    """noaa_apt::ColorSettings (noaa_apt.rs:63-71): the false-colour palette and the tune values of both channels.

    `palette` is a path, decoded here with PIL's convert("RGB") as processing::false_color decodes it with
    `image::open(..).into_rgb8()` (processing.rs:113-121: alpha dropped), or a (256, 256, 3) or (256, 256, 4) uint8
    array, indexed [b, a] (alpha dropped).  Errors are the reference's InvalidInput texts.

    `equalize_lab` (opt-in) lets Contrast.HISTOGRAM run with this colour: the reference's CIE Lab equalisation of
    channel A (APTGPU_COLOR_EQUALIZE_LAB; bit-exact against a restatement of the lab crate).
    Without it that combination raises UnsupportedError; with the other contrasts it changes nothing."""

    def __init__(self, palette, ch_a_tune_start=0.0, ch_a_tune_end=0.0, ch_b_tune_start=0.0, ch_b_tune_end=0.0,
                 equalize_lab=False):
        if isinstance(palette, (str, bytes, os.PathLike)):
            path = os.fsdecode(palette)
            try:
                from PIL import Image
                with Image.open(path) as im:
                    arr = np.asarray(im.convert("RGB"), dtype=np.uint8)
            except Exception:
                raise InvalidInputError(f"Could not load {_rust_debug_str(path)}") from None
        else:
            arr = np.asarray(palette)
            if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] not in (3, 4):
                raise InvalidInputError("Invalid palette image dimensions")
            arr = arr[:, :, :3]
        if arr.shape[:2] != (256, 256):
            raise InvalidInputError("Invalid palette image dimensions")
        self.palette = np.ascontiguousarray(arr)
        self.ch_a_tune_start, self.ch_a_tune_end = float(ch_a_tune_start), float(ch_a_tune_end)
        self.ch_b_tune_start, self.ch_b_tune_end = float(ch_b_tune_start), float(ch_b_tune_end)
        self.equalize_lab = bool(equalize_lab)

    def _c(self):
        flags = COLOR_EQUALIZE_LAB if self.equalize_lab else 0
        return _CColorSettings(C.sizeof(_CColorSettings), flags, self.palette.ctypes.data_as(_u8p),
                               self.ch_a_tune_start, self.ch_a_tune_end, self.ch_b_tune_start, self.ch_b_tune_end)


MAP_STATES, MAP_COUNTRIES, MAP_LAKES = 0, 1, 2  # aptgpu_map_layers layer indices (the reference's draw order)


def read_shapefile(path, shape_type):
    """The layer set's ESRI shapefile reader alone (aptgpu_map_read_shapefile, CPU): the parts of `path` read as
    shape_type 3 (Polyline) or 5 (Polygon), as a list of (n, 2) float64 arrays of (lon°, lat°)."""
    xy, n, parts, k = _f64p(), C.c_size_t(), _u32p(), C.c_size_t()
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_map_read_shapefile(os.fsencode(os.fspath(path)), int(shape_type), C.byref(xy), C.byref(n),
                                           C.byref(parts), C.byref(k), err, _ERRCAP), err)
    pts = _take(xy, 2 * n.value, np.float64).reshape(-1, 2)
    off = _take(parts, k.value + 1, np.uint32)
    return [pts[off[i]:off[i + 1]].copy() for i in range(k.value)]


class MapLayers:
    """The shapefile layers of the map overlay (aptgpu_map_layers): states (drawn as polylines), countries and lakes
    (polygons), in the reference's draw order (map.rs:133-198).  Each argument is None (layer left out) or a list of
    parts, each an (n, 2) array of (lon°, lat°).  Parsed and flattened once; a plan uploads it once per slot."""

    def __init__(self, states=None, countries=None, lakes=None):
        self._p = C.c_void_p()
        _check(lib().aptgpu_map_layers_create(C.byref(self._p)))
        for k, parts in ((MAP_STATES, states), (MAP_COUNTRIES, countries), (MAP_LAKES, lakes)):
            if parts is not None:
                self._set(k, parts)

    @staticmethod
    def load(directory):
        """map.rs's res/shapefiles: <directory>/states.shp, countries.shp and lakes.shp."""
        m = MapLayers()
        err = C.create_string_buffer(_ERRCAP)
        _check(lib().aptgpu_map_layers_load_dir(m._p, os.fsencode(os.fspath(directory)), err, _ERRCAP), err)
        return m

    def _set(self, k, parts):
        arrs = [np.ascontiguousarray(np.asarray(p, dtype=np.float64).reshape(-1, 2)) for p in parts]
        xy = np.ascontiguousarray(np.concatenate(arrs) if arrs else np.zeros((0, 2)), dtype=np.float64)
        off = np.zeros(len(arrs) + 1, np.uint32)
        off[1:] = np.cumsum([len(a) for a in arrs]) if arrs else []
        err = C.create_string_buffer(_ERRCAP)
        _check(lib().aptgpu_map_layers_set(self._p, k, xy.ctypes.data_as(_f64p), len(xy), off.ctypes.data_as(_u32p),
                                           len(arrs), err, _ERRCAP), err)

    def _colors(self, settings):
        for k, c in ((MAP_STATES, settings.states_color), (MAP_COUNTRIES, settings.countries_color),
                     (MAP_LAKES, settings.lakes_color)):
            rgba = (C.c_uint8 * 4)(*[int(v) for v in c])
            _check(lib().aptgpu_map_layers_set_color(self._p, k, rgba))

    def close(self):
        if self._p:
            lib().aptgpu_map_layers_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MapSettings:
    """noaa_apt::MapSettings (noaa_apt.rs:84-91) with the CLI's defaults (config.rs:646-648) and the colours of
    default_settings.toml:72-74."""

    def __init__(self, yaw=0.0, hscale=1.0, vscale=1.0, countries_color=(255, 255, 0, 255),
                 states_color=(255, 255, 0, 150), lakes_color=(50, 200, 200, 255)):
        self.yaw, self.hscale, self.vscale = float(yaw), float(hscale), float(vscale)
        self.countries_color, self.states_color, self.lakes_color = (tuple(countries_color), tuple(states_color),
                                                                     tuple(lakes_color))
        for c in (self.countries_color, self.states_color, self.lakes_color):
            if len(c) != 4 or not all(0 <= int(v) <= 255 for v in c):
                raise InvalidError("map colours are (r, g, b, a) tuples of u8")

    def _c(self):
        return _CMapSettings(C.sizeof(_CMapSettings), 0, self.yaw, self.hscale, self.vscale)


class MapOverlay:
    """What process() needs to draw the map from a track the caller has (the `orbit` argument): the satellite's
    (lat, lon) in radians for every image row, as map.rs:41-58 computes them with SGP4 (sat_track_host() does; an
    OrbitSettings leaves it to the GPU), the settings and the layers."""

    def __init__(self, sat_positions, settings=None, layers=None):
        self.sat_positions = np.ascontiguousarray(np.asarray(sat_positions, dtype=np.float64).reshape(-1, 2))
        self.settings = settings if settings is not None else MapSettings()
        if not isinstance(layers, MapLayers):
            raise InvalidError("MapOverlay needs a MapLayers")
        self.layers = layers


class SatName:
    """noaa_apt::SatName with its to_string() (noaa_apt.rs:95-108)."""
    NOAA15, NOAA18, NOAA19 = "NOAA 15", "NOAA 18", "NOAA 19"


class RefTime:
    """noaa_apt::RefTime (noaa_apt.rs:58-61): the time of the image's first row (Start) or of the row after its last
    (End: the start is 500 ms * height earlier, map.rs:45).  `t`: a timezone-aware datetime (truncated to
    milliseconds) or integer Unix milliseconds."""
    START, END = 0, 1

    def __init__(self, kind, t):
        if kind not in (RefTime.START, RefTime.END):
            raise InvalidError("RefTime: kind is RefTime.START or RefTime.END")
        if hasattr(t, "utcoffset"):
            import datetime as _dt
            if t.utcoffset() is None:
                raise InvalidError("RefTime: the datetime must be timezone-aware")
            d = t - _dt.datetime(1970, 1, 1, tzinfo=_dt.timezone.utc)
            t = (d.days * 86400 + d.seconds) * 1000 + d.microseconds // 1000
        elif not isinstance(t, (int, np.integer)):
            raise InvalidError("RefTime: a timezone-aware datetime or integer Unix milliseconds")
        self.kind, self.unix_ms = kind, int(t)

    @staticmethod
    def Start(t):  # noqa: N802 - the reference's variant name
        return RefTime(RefTime.START, t)

    @staticmethod
    def End(t):  # noqa: N802
        return RefTime(RefTime.END, t)


class OrbitSettings:
    """noaa_apt::OrbitSettings (noaa_apt.rs:75-82): satellite, TLE text, reference time and, to draw the map, a
    MapSettings.  custom_tle=None raises UnsupportedError (the reference downloads the current TLE then)."""

    def __init__(self, sat_name, custom_tle, ref_time, draw_map=None):
        if not isinstance(ref_time, RefTime):
            raise InvalidError("OrbitSettings: ref_time is RefTime.Start(t) or RefTime.End(t)")
        if draw_map is not None and not isinstance(draw_map, MapSettings):
            raise InvalidError("OrbitSettings: draw_map is a MapSettings or None")
        self.sat_name, self.custom_tle, self.ref_time, self.draw_map = str(sat_name), custom_tle, ref_time, draw_map

    def _c(self):
        """(struct, keepalive): the struct points into the keepalive objects"""
        name = self.sat_name.encode()
        tle = self.custom_tle.encode() if isinstance(self.custom_tle, str) else self.custom_tle
        cms = self.draw_map._c() if self.draw_map is not None else None
        c = _COrbitSettings(C.sizeof(_COrbitSettings), 0, name, tle, self.ref_time.kind, 0, self.ref_time.unix_ms,
                            C.cast(C.pointer(cms), C.c_void_p) if cms is not None else None)
        return c, (name, tle, cms)


def sat_track(orbit: OrbitSettings, height, context=None):
    """The (lat, lon) in radians of the satellite for each of `height` image rows (map.rs:41-58), computed by the
    GPU kernel: a height x 2 f64 array."""
    out = np.empty((int(height), 2), np.float64)
    c, _keep = orbit._c()
    cctx = (context or Context())._c()
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_sat_track(C.byref(cctx), C.byref(c), int(height), out.ctypes.data_as(_f64p), err, _ERRCAP), err)
    return out


def sat_track_host(orbit: OrbitSettings, height):
    """sat_track on the CPU, with the same source text (no GPU needed)."""
    out = np.empty((int(height), 2), np.float64)
    c, _keep = orbit._c()
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_sat_track_host(C.byref(c), int(height), out.ctypes.data_as(_f64p), err, _ERRCAP), err)
    return out


def south_to_north_pass(orbit: OrbitSettings) -> bool:
    """processing::south_to_north_pass (processing.rs:40-81), CPU: whether Rotate.ORBIT rotates the image.  True when
    the sub-point's heading over the 2 s after the reference time is northward (|azimuth| < pi/2); the reference's
    own comparison is true for southbound NOAA passes too."""
    c, _keep = orbit._c()
    out = C.c_int(0)
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_south_to_north_pass(C.byref(c), C.byref(out), err, _ERRCAP), err)
    return bool(out.value)


class Telemetry:
    """telemetry::Telemetry (telemetry.rs:19-121): wedge values of both bands."""

    def __init__(self, values_a, values_b, row=0, quality=0.0, channels=(-1, -1)):
        self.values_a = np.asarray(values_a, np.float32)
        self.values_b = np.asarray(values_b, np.float32)
        self.row, self.quality, self._channels = int(row), np.float32(quality), channels

    @staticmethod
    def _from(r: ImageResult):
        return Telemetry(list(r.values_a), list(r.values_b), r.telemetry_row, r.telemetry_quality,
                         (r.channel_a, r.channel_b))

    def get_wedge_value(self, wedge, channel=None):
        if channel == "A":
            return self.values_a[wedge - 1]
        if channel == "B":
            return self.values_b[wedge - 1]
        return np.float32((self.values_a[wedge - 1] + self.values_b[wedge - 1]) / np.float32(2.))

    def get_channel_name(self, channel):
        i = self._channels[{"A": 0, "B": 1}[channel]]
        if i < 0:
            raise InternalError("Can't compare values")
        return lib().aptgpu_channel_name(i).decode()


def _reduce(fn, context, signal):
    cctx = (context or Context())._c()
    x, xp = _as_f32(signal)
    out = C.c_float()
    err = C.create_string_buffer(_ERRCAP)
    _check(fn(C.byref(cctx), xp, x.size, C.byref(out), err, _ERRCAP), err)
    return np.float32(out.value)


def get_min(signal, context=None):   # dsp.rs:38
    return _reduce(lib().aptgpu_get_min, context, signal)


def get_max(signal, context=None):   # dsp.rs:20
    return _reduce(lib().aptgpu_get_max, context, signal)


def percent(signal, percent_value, context=None):  # misc.rs:119
    cctx = (context or Context())._c()
    x, xp = _as_f32(signal)
    lo, hi = C.c_float(), C.c_float()
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_percent(C.byref(cctx), xp, x.size, percent_value, C.byref(lo), C.byref(hi),
                                err, _ERRCAP), err)
    return np.float32(lo.value), np.float32(hi.value)


def map_signal_u8(signal, low, high, context=None):  # noaa_apt.rs:249
    cctx = (context or Context())._c()
    x, xp = _as_f32(signal)
    out = _u8p()
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_map_signal_u8(C.byref(cctx), xp, x.size, low, high, C.byref(out), err,
                                      _ERRCAP), err)
    return _take(out, x.size, np.uint8)


def read_telemetry(context, signal):  # telemetry.rs:125
    cctx = (context or Context())._c()
    x, xp = _as_f32(signal)
    r = ImageResult()
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_read_telemetry(C.byref(cctx), xp, x.size, C.byref(r), err, _ERRCAP), err)
    return Telemetry._from(r)


SAT_REASON_SGP4 = 10  # ImageResult.reason: SGP4 failed for a row of the image; no overlay was drawn
PNG_REASON_CAPACITY = 9  # ImageResult.reason: the PNG buffer is smaller than the file (png_bytes = its length)


def png_bound(width, height, channels):
    """aptgpu_png_bound: the largest file the encoder can emit for such an image (host arithmetic)."""
    n = lib().aptgpu_png_bound(int(width), int(height), int(channels))
    if n == 0:
        raise InvalidError("png_bound: width and height >= 1, channels 1 or 4, below 2^31 bytes")
    return int(n)


def encode_png(image, context=None) -> bytes:
    """aptgpu_encode_png: a (height, width) or (height, width, 1) uint8 image as a gray PNG, a (height, width, 4) one
    as RGBA, encoded on the GPU.  Decoding the file gives the array back exactly."""
    x = np.ascontiguousarray(image)
    if x.dtype != np.uint8 or x.ndim not in (2, 3):
        raise InvalidError("encode_png: a uint8 array of (height, width) or (height, width, channels)")
    height, width = x.shape[:2]
    channels = x.shape[2] if x.ndim == 3 else 1
    cctx = (context or Context())._c()
    cps = _CPngSettings(C.sizeof(_CPngSettings), 0)
    out, n = _u8p(), C.c_size_t()
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_encode_png(C.byref(cctx), x.ctypes.data_as(_u8p), width, height, channels, C.byref(cps),
                                   C.byref(out), C.byref(n), err, _ERRCAP), err)
    return _take(out, n.value, np.uint8).tobytes()


PROJECT_REASON_CAPACITY = 11  # ImageResult.reason: the projection's output buffer is below width * height * 4 bytes


class Projection:
    """The map grids of the reprojection (aptgpu_projection_settings.kind), its source channel and its sampling."""
    EQUIRECTANGULAR, MERCATOR = 0, 1
    CHANNEL_A, CHANNEL_B = 0, 1
    NEAREST, BILINEAR = 0, 1


class ProjectionSettings:
    """aptgpu_projection_settings: a north-up grid of width x height pixels whose pixel (i, j) has its centre at
    longitude lon_west + j * step and latitude lat_north - i * step (equirectangular) or
    atan(sinh(asinh(tan(lat_north)) - i * step)) (Mercator), all in degrees; this is the georeference of the output.
    channel: the half of the swath that is sampled; sampling: NEAREST or BILINEAR; grid_deg > 0 draws a graticule
    in grid_color over every multiple of it.  geometry: the MapSettings whose yaw / hscale / vscale place the swath
    when no overlay is drawn (with an overlay, the overlay's settings do)."""

    def __init__(self, kind, width, height, lat_north, lon_west, step, channel=Projection.CHANNEL_A,
                 sampling=Projection.NEAREST, grid_deg=0.0, grid_color=(255, 255, 255, 255), geometry=None):
        self.kind, self.width, self.height = int(kind), int(width), int(height)
        self.lat_north, self.lon_west, self.step = float(lat_north), float(lon_west), float(step)
        self.channel, self.sampling, self.grid_deg = int(channel), int(sampling), float(grid_deg)
        self.grid_color = tuple(int(v) for v in grid_color)
        if len(self.grid_color) != 4 or not all(0 <= v <= 255 for v in self.grid_color):
            raise InvalidError("grid_color is an (r, g, b, a) tuple of u8")
        if geometry is not None and not isinstance(geometry, MapSettings):
            raise InvalidError("geometry is a MapSettings or None")
        self.geometry = geometry
        if not (0 <= self.width < 1 << 32 and 0 <= self.height < 1 << 32):
            raise InvalidError("aptgpu_projection_settings: width and height must be at least 1")

    def _c(self):
        return _CProjectionSettings(C.sizeof(_CProjectionSettings), self.kind, self.width, self.height, self.lat_north,
                                    self.lon_west, self.step, self.channel, self.sampling, self.grid_deg,
                                    (C.c_uint8 * 4)(*self.grid_color), 0)

    @property
    def shape(self):
        return (self.height, self.width, 4)


def projection_fit(sat_positions, kind=Projection.EQUIRECTANGULAR, step=None, max_width=None, hscale=1.0):
    """aptgpu_projection_fit (host only): a ProjectionSettings whose grid covers the swath of a track of (lat, lon)
    rows in radians, with `step` degrees per pixel or, without it, `max_width` columns.  Conservative, not tight:
    the track's bounding box grown by the swath's half angle.  A list of tracks gives the grid of their union
    (aptgpu_projection_fit_many), with longitudes unwrapped relative to the first track."""
    out = _CProjectionSettings()
    err = C.create_string_buffer(_ERRCAP)
    if isinstance(sat_positions, (list, tuple)) and len(sat_positions) and np.ndim(sat_positions[0]) == 2:
        # several tracks (aptgpu_projection_fit_many): the union box, longitudes unwrapped from the first track
        tracks, pos, npos = _track_arrays(sat_positions)
        _check(lib().aptgpu_projection_fit_many(pos, npos, len(tracks), float(hscale),
                                                int(kind), float(step) if step is not None else 0.0,
                                                int(max_width) if max_width is not None else 0, C.byref(out), err,
                                                _ERRCAP), err)
        return ProjectionSettings(out.kind, out.width, out.height, out.lat_north, out.lon_west, out.step, out.channel,
                                  out.sampling, out.grid_deg)
    pos = np.ascontiguousarray(np.asarray(sat_positions, dtype=np.float64).reshape(-1, 2))
    _check(lib().aptgpu_projection_fit(pos.ctypes.data_as(_f64p), len(pos), float(hscale), int(kind),
                                       float(step) if step is not None else 0.0,
                                       int(max_width) if max_width is not None else 0, C.byref(out), err, _ERRCAP), err)
    return ProjectionSettings(out.kind, out.width, out.height, out.lat_north, out.lon_west, out.step, out.channel,
                              out.sampling, out.grid_deg)


def _one_per(x, cls, k, name, noun, per):
    """x as a list of k `cls`: the one object that serves all of them, or one per recording (or pass)."""
    xs = [x] * k if isinstance(x, cls) else list(x)
    if len(xs) != k or not all(isinstance(v, cls) for v in xs):
        raise InvalidError(f"{name}: {noun} or one per {per}")
    return xs


def _orbit_pointers(orbits):
    """(the array of pointers to the OrbitSettings' structs, what those structs point into)"""
    keep = [o._c() for o in orbits]
    return (C.POINTER(_COrbitSettings) * len(keep))(*[C.pointer(c) for c, _ in keep]), keep


def _track_arrays(tracks):
    """sat_positions arrays as (contiguous (rows, 2) f64 arrays, the array of their pointers, their row counts)"""
    tr = [np.ascontiguousarray(np.asarray(t, dtype=np.float64).reshape(-1, 2)) for t in tracks]
    return tr, (_f64p * len(tr))(*[t.ctypes.data_as(_f64p) for t in tr]), (C.c_size_t * len(tr))(*[len(t) for t in tr])


def _ref(struct):
    return C.byref(struct) if struct is not None else None


def project_image(image, sat_positions, projection, settings=None, png=False, context=None):
    """aptgpu_project_image: an unrotated (height, 2080) gray or (height, 2080, 4) RGBA uint8 image with its track
    (height rows of lat, lon in radians) onto the grid of `projection`: the (grid height, grid width, 4) RGBA array,
    or with png=True the PNG file's bytes.  settings: the MapSettings of the geometry (yaw, hscale, vscale)."""
    x = np.ascontiguousarray(image)
    if x.dtype != np.uint8 or x.ndim not in (2, 3) or x.shape[1] != PX_PER_ROW or (x.ndim == 3 and x.shape[2] != 4):
        raise InvalidError("project_image: a uint8 array of (height, 2080) or (height, 2080, 4)")
    if not isinstance(projection, ProjectionSettings):
        raise InvalidError("projection must be a ProjectionSettings")
    _keep, pos, npos = _track_arrays([sat_positions])
    cctx = (context or Context())._c()
    cms = (settings or projection.geometry or MapSettings())._c()
    cpr, cps = projection._c(), _CPngSettings(C.sizeof(_CPngSettings), 0)
    out, n = _u8p(), C.c_size_t()
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_project_image(C.byref(cctx), x.ctypes.data_as(_u8p), x.shape[0], 4 if x.ndim == 3 else 1,
                                      pos[0], npos[0], C.byref(cms), C.byref(cpr), 1 if png else 0,
                                      C.byref(cps), C.byref(out), C.byref(n), err, _ERRCAP), err)
    data = _take(out, n.value, np.uint8)
    return data.tobytes() if png else data.reshape(projection.shape)


COMPOSITE_REASON_PASS = 12  # ImageResult.reason of a composite's record: one of its passes failed
COMPOSITE_MAX_PASSES = 16


class Composite:
    """How a composite chooses among the passes that cover a pixel (aptgpu_composite_settings.blend): the FIRST in
    list order, the one nearest to its NADIR (smallest off-nadir distance |x|), or all of them FEATHERed with the
    weights 456 - |x|."""
    FIRST, NADIR, FEATHER = 0, 1, 2


def _composite_passes(images):
    """The images of a composite's passes as checked contiguous arrays."""
    xs = []
    for im in images:
        x = np.ascontiguousarray(im)
        if x.dtype != np.uint8 or x.ndim not in (2, 3) or x.shape[1] != PX_PER_ROW or (x.ndim == 3 and x.shape[2] != 4):
            raise InvalidError("composite: every image is a uint8 array of (height, 2080) or (height, 2080, 4)")
        xs.append(x)
    return xs


def _composite_maps(settings, projection, k):
    ms = [settings] * k if settings is None or isinstance(settings, MapSettings) else list(settings)
    if len(ms) != k or not all(m is None or isinstance(m, MapSettings) for m in ms):
        raise InvalidError("settings: a MapSettings, or one (or None) per pass")
    keep = [(m or projection.geometry or MapSettings())._c() for m in ms]
    return (C.POINTER(_CMapSettings) * k)(*[C.pointer(c) for c in keep]), keep


def composite_images(images, tracks, projection, blend=Composite.NADIR, settings=None, png=False,
                     return_coverage=False, context=None):
    """aptgpu_composite_images: up to 16 passes on one map grid.  images: unrotated (height, 2080) gray
    or (height, 2080, 4) RGBA uint8 arrays, each of its own height; tracks: per image its (height, 2) positions (lat,
    lon in radians); projection: the shared grid's ProjectionSettings (projection_fit accepts the list of tracks);
    blend: a Composite value; settings: a MapSettings for every pass or a list of one per pass.  Returns the
    (grid height, grid width, 4) RGBA array, or with png=True the PNG file's bytes; with return_coverage also the
    (grid height, grid width) uint8 count of the passes that cover each pixel."""
    if not isinstance(projection, ProjectionSettings):
        raise InvalidError("projection must be a ProjectionSettings")
    k = len(images)
    if len(tracks) != k:
        raise InvalidError("composite: one track per image")
    xs = _composite_passes(images)
    keep_tracks, pos, npos = _track_arrays(tracks)
    maps, keep = _composite_maps(settings, projection, k)
    cctx = (context or Context())._c()
    cpr, cps = projection._c(), _CPngSettings(C.sizeof(_CPngSettings), 0)
    cco = _CCompositeSettings(C.sizeof(_CCompositeSettings), int(blend), 0)
    out, n, cov = _u8p(), C.c_size_t(), _u8p()
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_composite_images(
        C.byref(cctx), k, (_u8p * k)(*[x.ctypes.data_as(_u8p) for x in xs]),
        (C.c_uint32 * k)(*[x.shape[0] for x in xs]), (C.c_int32 * k)(*[4 if x.ndim == 3 else 1 for x in xs]),
        pos, npos, maps, C.byref(cpr), C.byref(cco), 1 if png else 0, C.byref(cps), C.byref(out), C.byref(n),
        C.byref(cov) if return_coverage else None, err, _ERRCAP), err)
    del keep, keep_tracks
    data = _take(out, n.value, np.uint8)
    data = data.tobytes() if png else data.reshape(projection.shape)
    if return_coverage:
        return data, _take(cov, projection.width * projection.height, np.uint8).reshape(projection.shape[:2])
    return data


class _ImageRequest:
    """What one call of process() or of Plan.process_device_image asks of the image entry points of include/aptgpu.h,
    turned into their arguments once.  The constructor takes what every entry point has (`head`); resolve() takes the
    rest and leaves the track source as one of four: none, MapOverlays (positions and a drawn map), OrbitSettings (a
    drawn map with draw_map) or, under a projection, plain sat_positions.  The two callers make the checks of their
    own before, between and after the two; tests/test_image_request_py_cpu.py holds the order of all of them."""

    def __init__(self, contrast, rotate, color, channels):
        if color is not None and not isinstance(color, ColorSettings):
            raise UnsupportedError("color must be a ColorSettings")
        self.contrast, self.percent = Contrast._c(contrast)
        self.rotate, self.channels = int(rotate), channels
        self.color = color._c() if color is not None else None

    def resolve(self, k, map, orbit, layers, png, grids):  # noqa: A002
        """map: a MapOverlay or k of them or, under a projection, k sat_positions arrays; orbit: an OrbitSettings or k
        of them; at most one of the two.  png: whether the PNG file is asked for; grids: k ProjectionSettings or None.
        `keep` is what the pointers in the arguments point into."""
        self.map = self.layers = self.positions = self.counts = self.orbits = self.cgrids = self.keep = None
        if orbit is not None:
            orbits = _one_per(orbit, OrbitSettings, k, "orbit", "an OrbitSettings", "recording")
            if orbits and orbits[0].draw_map is not None:
                if not isinstance(layers, MapLayers):
                    raise InvalidError("OrbitSettings.draw_map needs layers=MapLayers")
                self.map, self.layers = orbits[0].draw_map, layers
            self.orbits, self.keep = _orbit_pointers(orbits)
        elif map is not None:
            tracks = map
            if grids is None or isinstance(map, MapOverlay) or all(isinstance(m, MapOverlay) for m in map):
                maps = _one_per(map, MapOverlay, k, "map", "a MapOverlay", "recording")
                if any(m.layers is not maps[0].layers or vars(m.settings) != vars(maps[0].settings) for m in maps):
                    raise InvalidError("map: every recording's MapOverlay must share settings and layers")
                self.map, self.layers = maps[0].settings, maps[0].layers
                tracks = [m.sat_positions for m in maps]
            self.keep, self.positions, self.counts = _track_arrays(tracks)
            if len(self.keep) != k:
                raise InvalidError("map: one sat_positions array per recording")
        if self.layers is not None:
            self.layers._colors(self.map)
        if self.channels is None:
            self.channels = 4 if self.color is not None or self.layers is not None else 1
        if grids is not None:  # (the geometry that places the swath is the drawn map's, else the first grid's)
            self.map = self.map or grids[0].geometry or MapSettings()
            self.cgrids = (_CProjectionSettings * k)(*[g._c() for g in grids])
        self.cmap = self.map._c() if self.map is not None else None
        self.cpng = _CPngSettings(C.sizeof(_CPngSettings), 0)
        self.layers_p = self.layers._p if self.layers is not None else None
        self.head = self.contrast, self.percent, self.rotate, _ref(self.color), int(self.channels)
        # the entry point that serves the request, as what its name ends in
        self.entry = "_project" if grids is not None else "_orbit" if orbit is not None else "_png" if png else \
            "_map" if map is not None else ""


class DespeckleSettings:
    """aptgpu_despeckle_settings: the band-aware median in front of process().  radius 1 (3 x 3) or 2
    (5 x 5); threshold >= 0 is a fraction of the signal's 98 % range: a sample is replaced by its window's median only
    where it differs from it by more than that (0: the plain median)."""

    def __init__(self, radius=1, threshold=0.0):
        self.radius, self.threshold = radius, threshold

    def _c(self, struct_size=None):
        return _CDespeckleSettings(C.sizeof(_CDespeckleSettings) if struct_size is None else int(struct_size),
                                   int(self.radius), float(self.threshold))


def _despeckle_c(settings):
    if settings is None:
        return None
    if not isinstance(settings, DespeckleSettings):
        raise InvalidError("despeckle: settings must be a DespeckleSettings")
    try:
        return settings._c()
    except (TypeError, ValueError, OverflowError) as e:
        raise InvalidError(f"despeckle: {e}") from None


def despeckle(signal, settings=None, context=None, return_info=False):
    """The despeckle stage on the GPU: f32 samples in, as many f32 samples out.  Every whole row of 2080 samples is
    filtered with a (2 * radius + 1)^2 median that never leaves the pixel's column band (sync, space, video,
    telemetry of either channel); a partial last row is copied.  With return_info also the DespeckleResult (height,
    replaced, low, high, t)."""
    cs = _despeckle_c(settings)
    cctx = (context or Context())._c()
    x, xp = _as_f32(signal)
    out, info = _f32p(), DespeckleResult()
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_despeckle(C.byref(cctx), xp, x.size, C.byref(cs) if cs is not None else None, C.byref(out),
                                  C.byref(info), err, _ERRCAP), err)
    y = _take(out, x.size)
    return (y, info) if return_info else y


_despeckle = despeckle  # (process() has a parameter of that name)


def despeckle_host(signal, settings=None, return_info=False):
    """despeckle() on the CPU, in plain C++ (no GPU needed): the same bits."""
    cs = _despeckle_c(settings)
    x, xp = _as_f32(signal)
    out, info = _f32p(), DespeckleResult()
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_despeckle_host(xp, x.size, C.byref(cs) if cs is not None else None, C.byref(out),
                                       C.byref(info), err, _ERRCAP), err)
    y = _take(out, x.size)
    return (y, info) if return_info else y


TRACK_MAX_JITTER = 64


class TrackSettings:
    """aptgpu_track_settings: the flywheel sync stage.  max_jitter: how many work samples (0..64) a row
    start may move against the one before it; penalty (finite, >= 0): what one sample of such a move costs, in units
    of the normalised sync score."""

    def __init__(self, max_jitter=8, penalty=0.1):
        self.max_jitter, self.penalty = max_jitter, penalty

    def _c(self, struct_size=None):
        return _CTrackSettings(C.sizeof(_CTrackSettings) if struct_size is None else int(struct_size),
                               int(self.max_jitter), float(self.penalty), 0)


def _track_c(settings):
    if settings is None:
        return None
    if isinstance(settings, _CTrackSettings):  # (tests: a struct_size of their own)
        return settings
    if not isinstance(settings, TrackSettings):
        raise InvalidError("track: settings must be a TrackSettings")
    try:
        return settings._c()
    except (TypeError, ValueError, OverflowError) as e:
        raise InvalidError(f"track: {e}") from None


def _track_result(struct_size=None):
    r = TrackResult()
    r.struct_size = C.sizeof(TrackResult) if struct_size is None else int(struct_size)
    return r


def _track_signals(signal):
    many = isinstance(signal, (list, tuple))
    xs = [_as_f32(x) for x in (signal if many else [signal])]
    k = len(xs)
    ptrs = (_f32p * k)(*[p for _, p in xs])
    ns = (C.c_size_t * k)(*[x.size for x, _ in xs])
    return many, xs, k, ptrs, ns


def track_sync(signal, work_rate: "Rate", settings=None, context=None, rows=True, return_info=False):
    """The flywheel sync stage on the GPU.  signal: the low-passed envelope at the work rate (decode()'s
    "filter_result" step), or a list of such signals, which then share one launch per kernel.  Returns (positions
    u64, scores f32, rows f32 [n_rows, 2080] or None) — with return_info also the TrackResult — per signal."""
    cs = _track_c(settings)
    cctx = (context or Context())._c()
    many, xs, k, ptrs, ns = _track_signals(signal)
    pos, sc, rw = (_u64p * k)(), (_f32p * k)(), (_f32p * k)()
    info = (TrackResult * k)()
    for r in info:
        r.struct_size = C.sizeof(TrackResult)
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_track_sync(C.byref(cctx), k, ptrs, ns, work_rate.get_hz(), C.byref(cs) if cs is not None else None,
                                   pos, sc, rw if rows else None, info, err, _ERRCAP), err)
    out = []
    for i in range(k):
        r = info[i]
        item = (_take(pos[i], r.n_positions, np.uint64), _take(sc[i], r.n_positions),
                _take(rw[i], r.n_rows * PX_PER_ROW).reshape(-1, PX_PER_ROW) if rows else None)
        out.append(item + (r,) if return_info else item)
    return out if many else out[0]


def track_sync_host(signal, work_rate: "Rate", settings=None, rows=True, return_score=False, return_info=False,
                    result_struct_size=None):
    """track_sync() for one signal on the CPU, in plain C++ (no GPU needed): the same bits.  return_score: also s, the
    score of every position."""
    cs = _track_c(settings)
    x, xp = _as_f32(signal)
    pos, sc, rw, s = _u64p(), _f32p(), _f32p(), _f32p()
    info = _track_result(result_struct_size)
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_track_sync_host(xp, x.size, work_rate.get_hz(), C.byref(cs) if cs is not None else None,
                                        C.byref(pos), C.byref(sc), C.byref(rw) if rows else None,
                                        C.byref(s) if return_score else None, C.byref(info), err, _ERRCAP), err)
    out = (_take(pos, info.n_positions, np.uint64), _take(sc, info.n_positions),
           _take(rw, info.n_rows * PX_PER_ROW).reshape(-1, PX_PER_ROW) if rows else None)
    if return_score:
        pw = work_rate.get_hz() // FINAL_RATE
        out += (_take(s, x.size - 38 * pw),)
    return out + (info,) if return_info else out


def sync_score(signal, work_rate: "Rate", context=None):
    """s alone, on the GPU: the zero-mean normalised correlation of the signal (or of every signal of a list, in one
    launch) with the sync template at every position, 0 where a window holds no evidence."""
    cctx = (context or Context())._c()
    many, xs, k, ptrs, ns = _track_signals(signal)
    sc = (_f32p * k)()
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_sync_score(C.byref(cctx), k, ptrs, ns, work_rate.get_hz(), sc, err, _ERRCAP), err)
    pw = work_rate.get_hz() // FINAL_RATE
    out = [_take(sc[i], xs[i][0].size - 38 * pw) for i in range(k)]
    return out if many else out[0]


def decode_tracked(context: Optional["Context"], settings: "Settings", signal, input_rate: "Rate", track=None,
                   return_info=False):
    """decode() with the flywheel sync stage in place of find_sync: the front end of a sync = 0 plan, then the stage.
    Returns the rows (flat f32, rows * 2080, the filtered samples' own bits) — with return_info also (positions,
    scores, TrackResult).  Holds where decode() raises "less than 5 sync frames"; keeps its "less than 10 rows"."""
    cs = _track_c(track)
    cctx = (context or Context())._c()
    c_settings = settings._c()
    x, xp = _as_f32(signal)
    rw, n_out, pos, sc = _f32p(), C.c_size_t(0), _u64p(), _f32p()
    info = _track_result()
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_decode_tracked(C.byref(cctx), C.byref(c_settings), xp, x.size, input_rate.get_hz(),
                                       C.byref(cs) if cs is not None else None, C.byref(rw), C.byref(n_out),
                                       C.byref(pos), C.byref(sc), C.byref(info), err, _ERRCAP), err)
    rows = _take(rw, n_out.value)
    p, q = _take(pos, info.n_positions, np.uint64), _take(sc, info.n_positions)
    return (rows, p, q, info) if return_info else rows


class LiveTrackSettings:
    """aptgpu_live_track_settings: live flywheel sync.  lag_rows (0..64): how many rows behind the best
    survivor a row start is committed — 8 is four seconds behind real time, 0 is greedy; max_jitter and penalty are
    TrackSettings'."""

    def __init__(self, lag_rows=8, max_jitter=8, penalty=0.1):
        self.lag_rows, self.max_jitter, self.penalty = lag_rows, max_jitter, penalty

    def _c(self, struct_size=None):
        return _CLiveTrackSettings(C.sizeof(_CLiveTrackSettings) if struct_size is None else int(struct_size),
                                   int(self.lag_rows), int(self.max_jitter), float(self.penalty))


def _live_track_c(settings):
    if isinstance(settings, _CLiveTrackSettings):  # (tests: a struct_size of their own)
        return settings
    if not isinstance(settings, LiveTrackSettings):
        raise InvalidError("stream: track must be a LiveTrackSettings")
    try:
        return settings._c()
    except (TypeError, ValueError, OverflowError) as e:
        raise InvalidError(f"stream: {e}") from None


class _LiveBase:
    """What LiveDecoder and LiveIqDecoder share: the handle, the calls and the records.  _PREFIX names the C functions
    (<prefix>_create[_tracked][_host], _push, _finish, ...); a subclass adds its constructor's argument handling,
    get_info and the conversion of a chunk to (pointer, count)."""
    _PREFIX = None

    def _fn(self, name):
        return getattr(lib(), f"{self._PREFIX}_{name}")

    def _create(self, host, track, *head):
        """head: the structures in front of the track settings in the create call"""
        self._p = C.c_void_p()
        self.host = bool(host)
        err = C.create_string_buffer(_ERRCAP)
        self.tracked = track is not None
        self.scores, self.track_result = None, None
        args = [C.byref(a) for a in head]
        if self.tracked:
            ct = _live_track_c(track)
            args.append(C.byref(ct))
        fn = self._fn("create" + ("_tracked" if self.tracked else "") + ("_host" if host else ""))
        _check(fn(*args, C.byref(self._p), err, _ERRCAP), err)
        if self.tracked:
            self.scores = np.zeros(0, np.float32)
        self.result = StreamResult(struct_size=C.sizeof(StreamResult))

    def close(self):
        if self._p:
            self._fn("destroy")(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def reset(self):
        err = C.create_string_buffer(_ERRCAP)
        _check(self._fn("reset")(self._p, err, _ERRCAP), err)
        self.result = StreamResult(struct_size=C.sizeof(StreamResult))

    def _call(self, ptr, n, rows_cap, finish=False):
        cap = self.rows_bound(n) if rows_cap is None else int(rows_cap)
        rows = np.empty((max(cap, 1), PX_PER_ROW), np.float32)
        pos = np.empty(max(cap, 1), np.uint64)
        res = StreamResult(struct_size=C.sizeof(StreamResult))
        err = C.create_string_buffer(_ERRCAP)
        rp, pp = rows.ctypes.data_as(_f32p), pos.ctypes.data_as(_u64p)
        if finish:
            rc = self._fn("finish")(self._p, rp, pp, cap, C.byref(res), err, _ERRCAP)
        else:
            rc = self._fn("push")(self._p, ptr, n, rp, pp, cap, C.byref(res), err, _ERRCAP)
        if rc in (0, 1):  # (an end-of-signal error fills the record; a refused call leaves it alone)
            self.result = res
            if self.tracked:
                self._read_track(0 if rc else int(res.n_rows))
        _check(rc, err)
        k = int(res.n_rows)
        return rows[:k].copy(), pos[:k].copy()

    def _read_track(self, k):
        sc, n = np.zeros(max(k, 1), np.float32), C.c_size_t(0)
        err = C.create_string_buffer(_ERRCAP)
        _check(self._fn("track_scores")(self._p, sc.ctypes.data_as(_f32p), k, C.byref(n), err, _ERRCAP), err)
        self.scores = sc[:min(k, int(n.value))].copy()
        self.track_results()

    def track_results(self):
        """Waits like results() and returns the tracker's record (a tracked stream or coupling only)."""
        res = StreamTrackResult(struct_size=C.sizeof(StreamTrackResult))
        err = C.create_string_buffer(_ERRCAP)
        _check(self._fn("track_results")(self._p, C.byref(res), err, _ERRCAP), err)
        self.track_result = res
        return res

    def scores_device(self, d_scores):
        """Where the device-resident calls that follow write the lock indicators of their rows (a device pointer to
        rows_cap floats; None: the stream keeps them)."""
        err = C.create_string_buffer(_ERRCAP)
        _check(self._fn("track_scores_device")(self._p, d_scores, err, _ERRCAP), err)

    def finish(self, rows_cap=None):
        """The end of the recording: the remaining rows, or the error decode() would raise."""
        return self._call(None, 0, rows_cap, finish=True)

    def _push_device(self, d_in, n, d_rows, d_positions, rows_cap):
        err = C.create_string_buffer(_ERRCAP)
        _check(self._fn("push_device")(self._p, d_in, int(n), d_rows, d_positions, int(rows_cap), err, _ERRCAP), err)

    def finish_device(self, d_rows, d_positions, rows_cap):
        err = C.create_string_buffer(_ERRCAP)
        _check(self._fn("finish_device")(self._p, d_rows, d_positions, int(rows_cap), err, _ERRCAP), err)

    def results(self):
        """Waits for the device-resident calls and returns the record of the last one (raising its error)."""
        res = StreamResult(struct_size=C.sizeof(StreamResult))
        err = C.create_string_buffer(_ERRCAP)
        rc = self._fn("results")(self._p, C.byref(res), err, _ERRCAP)
        if rc in (0, 1):
            self.result = res
        _check(rc, err)
        return res


def _collect_live(dec, chunks, return_info):
    """What decode_live and decode_live_iq do with an open decoder: every chunk pushed, then the finish."""
    out, pos, sc = [], [], []
    with dec:
        def take(call):
            out.append(call[0])
            pos.append(call[1])
            if dec.tracked:
                sc.append(dec.scores)

        for chunk in chunks:
            take(dec.push(chunk))
        take(dec.finish())
        info = dec.track_result
    rows = np.concatenate(out).reshape(-1)
    if return_info and dec.tracked:
        return rows, np.concatenate(pos), np.concatenate(sc), info
    return rows


class LiveDecoder(_LiveBase):
    """aptgpu_stream: live decode.  Push the recording in chunks of any size; every push returns the
    image rows that are final — bit-identical to what strict decode() of the complete recording holds at that place,
    whatever is pushed later — and their work-rate positions.  finish() releases the rest and raises what decode()
    would raise ("less than 10 rows", "less than 5 sync frames"); rows handed out before stay handed out.  dtype:
    np.float32 or np.int16 (mono PCM16, the value as f32).  host=True: the plain C++ twin on the CPU (same bits, no GPU).
    `result` is the record of the last call, `info` the stream's geometry and ring capacities.
    track: a LiveTrackSettings finds the rows with the flywheel tracker in place of the reference's picker (DESIGN.md
    §24; `sync` is then not read): rows are the filtered samples' own bits, committed lag_rows behind real time;
    `scores` holds the lock indicators of the last call's rows and `track_result` the tracker's record."""
    _PREFIX = "aptgpu_stream"

    def __init__(self, settings, input_rate, sync=True, context=None, dtype=np.float32, max_push=None, host=False,
                 track=None):
        self._dtype = np.dtype(dtype)
        fmt = {np.dtype(np.float32): 0, np.dtype(np.int16): 1}.get(self._dtype)
        if fmt is None:
            raise InvalidError("stream: dtype must be float32 or int16")
        self._ctx = context or Context()
        cctx, cs = self._ctx._c(), settings._c()
        css = _CStreamSettings(C.sizeof(_CStreamSettings), int(input_rate.get_hz()), 1 if sync else 0, fmt, int(max_push or 0), 0)
        self._create(host, track, cctx, cs, css)
        self.info = self.get_info()

    def get_info(self):
        info = StreamInfo(struct_size=C.sizeof(StreamInfo))
        _check(lib().aptgpu_stream_get_info(self._p, C.byref(info)))
        return info

    def rows_bound(self, n=0):
        """Upper bound of the rows a push of n more samples (0: a finish) can release now: from the work signal's length
        after it and the rows known to be out (one event of the picker can push any number of peaks)."""
        return int(lib().aptgpu_stream_rows_bound(self._p, int(n)))

    def push(self, chunk, rows_cap=None):
        """chunk: 1-D samples of the stream's dtype -> (rows [n, 2080] f32, positions [n] u64) that became final."""
        chunk = np.ascontiguousarray(chunk, dtype=self._dtype).reshape(-1)
        return self._call(chunk.ctypes.data_as(C.c_void_p), chunk.size, rows_cap)

    def push_device(self, d_samples, n, d_rows, d_positions, rows_cap):
        """Device pointers (ints); asynchronous on the context's stream.  rows_cap >= rows_bound(n)."""
        self._push_device(d_samples, n, d_rows, d_positions, rows_cap)


def decode_live(context: Optional["Context"], settings: "Settings", chunks, input_rate: "Rate", sync: bool, host=False,
                max_push=None, track=None, return_info=False):
    """decode() over an iterable of chunks through a LiveDecoder: returns what decode() returns for their
    concatenation (flat f32, rows * 2080) and raises what it raises.  The chunks' dtype (float32 or int16) is the
    first chunk's.  track: a LiveTrackSettings; return_info then gives (rows, positions, scores,
    StreamTrackResult)."""
    it = iter(chunks)
    first = next(it, None)
    dtype = np.int16 if first is not None and np.asarray(first).dtype == np.int16 else np.float32
    rest = it if first is None else itertools.chain([first], it)
    return _collect_live(LiveDecoder(settings, input_rate, sync, context, dtype, max_push, host, track), rest, return_info)


THERMAL_COLD_WHITE = 1
THERMAL_REASON_CHANNEL = 13
THERMAL_REASON_DEGENERATE = 14
THERMAL_PX = 909
_THERMAL_IDS = {"4": 3, "5": 4, "3b": 5}


class ThermalCoefficients:
    """aptgpu_thermal_coeffs: the caller's calibration coefficients (NOAA KLM User's Guide, Appendix D; no presets are
    shipped).  prt: 4 x 3, T_i = prt[i][0] + prt[i][1] * C + prt[i][2] * C^2 of the four black-body thermometers;
    ch3b, ch4, ch5: (nu, A, B, N_s, b0, b1, b2) of each infrared channel."""

    def __init__(self, prt, ch3b, ch4, ch5):
        self.prt = np.asarray(prt, dtype=np.float64)
        self.channel = np.asarray([ch3b, ch4, ch5], dtype=np.float64)
        if self.prt.shape != (4, 3) or self.channel.shape != (3, 7):
            raise InvalidError("thermal: prt must be 4 x 3 and every channel set 7 values")

    def _c(self, struct_size=None):
        c = _CThermalCoeffs()
        c.struct_size = C.sizeof(_CThermalCoeffs) if struct_size is None else int(struct_size)
        for i in range(4):
            for k in range(3):
                c.prt[i][k] = self.prt[i, k]
        for i in range(3):
            for k in range(7):
                c.channel[i][k] = self.channel[i, k]
        return c


class ThermalSettings:
    """aptgpu_thermal_settings.  channel: "A" / "B" (or 0 / 1), the half of the row image to calibrate.  channel_id:
    None takes the identity from the telemetry (wedge 16); "4", "5", "3b" (or an index of the channel-name table)
    forces it.  t_low / t_high: Kelvin at levels 0 and 255 of the scale image; cold_white: 255 - level.  palette: 256 x 3
    RGB bytes by level (RGBA image only).  image_channels: 0 no scale image, 1 gray, 4 RGBA (default: 4 with a palette,
    else 0)."""

    def __init__(self, channel, channel_id=None, *, t_low, t_high, cold_white=True, palette=None, image_channels=None,
                 flags=None):
        self.channel, self.channel_id, self.t_low, self.t_high = channel, channel_id, t_low, t_high
        self.cold_white, self.palette, self.flags = cold_white, palette, flags
        self.image_channels = (4 if palette is not None else 0) if image_channels is None else image_channels

    def _c(self, struct_size=None):
        """-> (struct, the object that keeps the palette's bytes alive)"""
        ch = {"A": 0, "B": 1}.get(self.channel, self.channel)
        cid = -1 if self.channel_id is None else _THERMAL_IDS.get(self.channel_id, self.channel_id)
        if isinstance(cid, str):
            raise InvalidError(f"thermal: unknown channel identity {self.channel_id!r}")
        flags = (THERMAL_COLD_WHITE if self.cold_white else 0) if self.flags is None else int(self.flags)
        pal = None
        if self.palette is not None:
            pal = np.ascontiguousarray(self.palette, dtype=np.uint8)
            if pal.shape != (256, 3):
                raise InvalidError("thermal: the palette must be 256 x 3 bytes")
        c = _CThermalSettings(C.sizeof(_CThermalSettings) if struct_size is None else int(struct_size), int(ch),
                              int(cid), int(self.image_channels), flags, float(self.t_low), float(self.t_high), 0,
                              pal.ctypes.data if pal is not None else None)
        return c, pal


def _thermal_c(coeffs, settings):
    if not isinstance(coeffs, ThermalCoefficients) or not isinstance(settings, ThermalSettings):
        raise InvalidError("thermal: coeffs must be a ThermalCoefficients and settings a ThermalSettings")
    try:
        return (coeffs._c(),) + settings._c()
    except (TypeError, ValueError, OverflowError) as e:
        raise InvalidError(f"thermal: {e}") from None


def _thermal_call(fn, head, signal, coeffs, settings):
    cc, cs, keep = _thermal_c(coeffs, settings)
    x, xp = _as_f32(signal)
    kelvin, image, info = _f32p(), _u8p(), ThermalResult()
    err = C.create_string_buffer(_ERRCAP)
    ch = int(cs.image_channels)
    try:
        _check(fn(*head, xp, x.size, C.byref(cc), C.byref(cs), C.byref(kelvin), C.byref(image) if ch else None,
                  C.byref(info), err, _ERRCAP), err)
    except AptError as e:
        e.info = info  # (the record of a failed calibration: status, reason, the scalars so far)
        raise
    del keep
    h = x.size // PX_PER_ROW
    k = _take(kelvin, h * THERMAL_PX).reshape(h, THERMAL_PX)
    img = None
    if ch:
        img = _take(image, h * PX_PER_ROW * ch, np.uint8)
        img = img.reshape(h, PX_PER_ROW) if ch == 1 else img.reshape(h, PX_PER_ROW, 4)
    return k, img, info


def calibrate_thermal(signal, coeffs, settings, context=None):
    """Brightness temperature of an infrared channel of decoded rows, on the GPU: the telemetry
    frame gives the count scale, the black body's thermometers and its view, the space columns the space view; every
    video pixel of the channel becomes a temperature.  Returns (kelvin, image, info): the height x 909 f32 Kelvin
    plane, the height x 2080 (x 4) u8 scale image in the standard row layout (None with image_channels 0) and the
    ThermalResult.  A failed calibration (too short, not a thermal channel, degenerate) raises InternalError whose
    `info` attribute is the record."""
    cctx = (context or Context())._c()
    return _thermal_call(lib().aptgpu_calibrate_thermal, (C.byref(cctx),), signal, coeffs, settings)


def calibrate_thermal_host(signal, coeffs, settings):
    """calibrate_thermal() on the CPU, in plain C++ (no GPU needed): the same scalars, the same f32 pixel
    arithmetic up to the C library's logf."""
    return _thermal_call(lib().aptgpu_calibrate_thermal_host, (), signal, coeffs, settings)


# ------------------------------------------------------------------ FM demodulation of IQ recordings
GEOLOC_PX = 909
GEOLOC_REASON_HEIGHT = 15
GEOLOC_REASON_DECODE = 16


class GeolocSettings:
    """aptgpu_geoloc_settings.  channel: "A" / "B" (or 0 / 1), the half of the row image normalize_sun() rewrites.
    ref_time: RefTime.Start(t) / RefTime.End(t) of the image, used for the sun when the track is an array (an
    OrbitSettings brings its own).  black: the zero level in row units.  max_zenith_deg: the normalisation divides by
    max(cos_sun, cos(max_zenith_deg)); in (0, 90)."""

    def __init__(self, channel="A", ref_time=None, black=0.0, max_zenith_deg=80.0, flags=0):
        self.channel, self.ref_time, self.black, self.max_zenith_deg = channel, ref_time, black, max_zenith_deg
        self.flags = flags

    def _c(self, struct_size=None):
        ch = {"A": 0, "B": 1}.get(self.channel, self.channel)
        rt = self.ref_time if self.ref_time is not None else RefTime.Start(0)
        if not isinstance(rt, RefTime):
            raise InvalidError("geoloc: ref_time is RefTime.Start(t) or RefTime.End(t)")
        return _CGeolocSettings(C.sizeof(_CGeolocSettings) if struct_size is None else int(struct_size), int(self.flags),
                                int(ch), rt.kind, rt.unix_ms, float(self.black), float(self.max_zenith_deg))


def _geoloc_c(track_or_orbit, map_settings, settings):
    """(positions pointer, count, orbit pointer, map pointer, settings, keepalive)"""
    settings = settings if settings is not None else GeolocSettings()
    if not isinstance(settings, GeolocSettings):
        raise InvalidError("geoloc: settings must be a GeolocSettings")
    if map_settings is not None and not isinstance(map_settings, MapSettings):
        raise InvalidError("geoloc: map_settings must be a MapSettings or None")
    try:
        cs = settings._c()
    except (TypeError, ValueError, OverflowError) as e:
        raise InvalidError(f"geoloc: {e}") from None
    cms = map_settings._c() if map_settings is not None else None
    if isinstance(track_or_orbit, OrbitSettings):
        co, keep = track_or_orbit._c()
        return None, 0, C.byref(co), (C.byref(cms) if cms is not None else None), cs, (co, keep, cms)
    if track_or_orbit is None:
        return None, 0, None, (C.byref(cms) if cms is not None else None), cs, (cms,)
    track = np.ascontiguousarray(np.asarray(track_or_orbit, dtype=np.float64).reshape(-1, 2))
    return (track.ctypes.data_as(_f64p), track.shape[0], None, (C.byref(cms) if cms is not None else None), cs,
            (track, cms))


def _geoloc_call(fn, head, signal_or_height, track_or_orbit, map_settings, settings, latlon, sun, rows):
    if isinstance(signal_or_height, (int, np.integer)):
        if rows:
            raise InvalidError("geoloc: normalised rows need the signal")
        xp, n = None, int(signal_or_height) * PX_PER_ROW
    else:
        x, xp = _as_f32(signal_or_height)
        n = x.size
    pos, count, co, cms, cs, keep = _geoloc_c(track_or_orbit, map_settings, settings)
    p_ll, p_cos, p_rows, info = _f64p(), _f32p(), _f32p(), GeolocResult()
    info.struct_size = C.sizeof(GeolocResult)
    err = C.create_string_buffer(_ERRCAP)
    try:
        _check(fn(*head, xp, n, pos, count, co, cms, C.byref(cs), C.byref(p_ll) if latlon else None,
                  C.byref(p_cos) if sun else None, C.byref(p_rows) if rows else None, C.byref(info), err, _ERRCAP), err)
    except AptError as e:
        e.info = info  # (the record of a failed call: status, reason, height)
        raise
    del keep
    h = n // PX_PER_ROW
    out_ll = _take(p_ll, h * GEOLOC_PX * 2, np.float64).reshape(h, GEOLOC_PX, 2) if latlon else None
    out_cos = _take(p_cos, h * GEOLOC_PX).reshape(h, GEOLOC_PX) if sun else None
    out_rows = _take(p_rows, n) if rows else None
    return out_ll, out_cos, out_rows, info


def geolocate(signal_or_height, track_or_orbit, map_settings=None, settings=None, latlon=True, sun=False, context=None):
    """Where on the Earth every video pixel of the swath lies, on the GPU: the inverse of the map
    overlay's projection.  signal_or_height: decoded rows, or just their number.  track_or_orbit: the satellite's
    (lat, lon) in radians per row, or an OrbitSettings (SGP4 then runs on the GPU).  Returns (latlon, cos_sun, info):
    the height x 909 x 2 f64 plane of (lat, lon) in radians, the height x 909 f32 cosine of the solar zenith angle
    (each None unless asked for) and the GeolocResult.  Pixels beyond 60 degrees of arc from the track's start are NaN.
    A failed call (fewer than two rows, a track of another length, SGP4) raises InternalError whose `info` attribute
    is the record."""
    cctx = (context or Context())._c()
    ll, cs, _, info = _geoloc_call(lib().aptgpu_geolocate, (C.byref(cctx),), signal_or_height, track_or_orbit,
                                   map_settings, settings, latlon, sun, False)
    return ll, cs, info


def geolocate_host(signal_or_height, track_or_orbit, map_settings=None, settings=None, latlon=True, sun=False,
                   rows=False):
    """geolocate() on the CPU, in plain C++ (no GPU needed): the same source text per pixel with the C library's f64
    functions.  With rows=True the fourth value is the sun-normalised signal (normalize_sun's)."""
    ll, cs, r, info = _geoloc_call(lib().aptgpu_geolocate_host, (), signal_or_height, track_or_orbit, map_settings,
                                   settings, latlon, sun, rows)
    return (ll, cs, r, info) if rows else (ll, cs, info)


def sun_position(unix_ms):
    """(declination, sub-solar longitude) in radians at a Unix time in milliseconds: the Astronomical Almanac's
    low-precision series the stage uses (CPU)."""
    out = (C.c_double * 2)()
    _check(lib().aptgpu_sun_position(int(unix_ms), out))
    return float(out[0]), float(out[1])


def normalize_sun(signal, track_or_orbit, channel, black=None, ref_time=None, max_zenith_deg=80.0, map_settings=None,
                  context=None, return_info=False):
    """The visible channel's video divided by the cosine of the solar zenith angle, in front of process() (DESIGN.md
    §25): out = black + (x - black) / max(cos_sun, cos(max_zenith_deg)) on the channel's 909 video columns, every other
    sample unchanged.  black=None takes wedge 9 of read_telemetry(), the zero-modulation wedge of that channel.
    ref_time: the image's RefTime when the track is an array."""
    if black is None:
        ch = {0: "A", 1: "B"}.get(channel, channel)
        black = float(read_telemetry(context, signal).get_wedge_value(9, ch))
    st = GeolocSettings(channel=channel, ref_time=ref_time, black=black, max_zenith_deg=max_zenith_deg)
    cctx = (context or Context())._c()
    _, _, rows, info = _geoloc_call(lib().aptgpu_geolocate, (C.byref(cctx),), signal, track_or_orbit, map_settings, st,
                                    False, False, True)
    return (rows, info) if return_info else rows


LAND_SEA, LAND_LAND, LAND_LAKE, LAND_INVALID = 0, 1, 2, 255


class LandMaskSettings:
    """aptgpu_land_mask_settings.  n_bands: the latitude bands of the acceleration table, 1 .. 7200; the mask does not
    depend on it."""

    def __init__(self, n_bands=720, flags=0):
        self.n_bands, self.flags = n_bands, flags

    def _c(self, struct_size=None):
        return _CLandMaskSettings(C.sizeof(_CLandMaskSettings) if struct_size is None else int(struct_size),
                                  int(self.flags), int(self.n_bands), 0)


def _land_c(layers, settings):
    settings = settings if settings is not None else LandMaskSettings()
    if not isinstance(settings, LandMaskSettings):
        raise InvalidError("land mask: settings must be a LandMaskSettings")
    if not isinstance(layers, MapLayers):
        raise InvalidError("land mask: layers must be a MapLayers")
    try:
        return settings._c()
    except (TypeError, ValueError, OverflowError) as e:
        raise InvalidError(f"land mask: {e}") from None


def _land_info():
    info = LandMaskResult()
    info.struct_size = C.sizeof(LandMaskResult)
    return info


def _land_call(fn, head, height_or_signal, track_or_orbit, layers, map_settings, settings):
    if isinstance(height_or_signal, (int, np.integer)):
        h = int(height_or_signal)
    else:
        h = np.asarray(height_or_signal).size // PX_PER_ROW
    if h < 0:
        raise InvalidError("land mask: the height is negative")
    cs = _land_c(layers, settings)
    if map_settings is not None and not isinstance(map_settings, MapSettings):
        raise InvalidError("land mask: map_settings must be a MapSettings or None")
    cms = map_settings._c() if map_settings is not None else None
    pos, count, co, keep = None, 0, None, None
    if isinstance(track_or_orbit, OrbitSettings):
        c_orbit, keep = track_or_orbit._c()
        co = C.byref(c_orbit)
    elif track_or_orbit is not None:
        keep = np.ascontiguousarray(np.asarray(track_or_orbit, dtype=np.float64).reshape(-1, 2))
        pos, count = keep.ctypes.data_as(_f64p), keep.shape[0]
    p_mask, info = _u8p(), _land_info()
    err = C.create_string_buffer(_ERRCAP)
    try:
        _check(fn(*head, h, pos, count, co, C.byref(cms) if cms is not None else None, layers._p, C.byref(cs),
                  C.byref(p_mask), C.byref(info), err, _ERRCAP), err)
    except AptError as e:
        e.info = info  # (the record of a failed call: status, reason, height)
        raise
    del keep
    return _take(p_mask, h * GEOLOC_PX, np.uint8).reshape(h, GEOLOC_PX), info


def land_mask(height_or_signal, track_or_orbit, layers, map_settings=None, settings=None, context=None):
    """Whether every video pixel of the swath shows sea, land or a lake, on the GPU: the even-odd rule
    against the polygons of the layer set's countries and lakes at the geolocation stage's points, which are computed
    in the kernel (the lat / lon plane is never written).  height_or_signal: the number of rows, or the decoded rows.
    track_or_orbit: the satellite's (lat, lon) in radians per row, or an OrbitSettings (SGP4 then runs on the GPU).
    Returns (mask, info): the height x 909 uint8 classes LAND_SEA, LAND_LAND, LAND_LAKE, LAND_INVALID (beyond 60 degrees
    of arc from the track's start) and the LandMaskResult.  A failed call (fewer than two rows, a track of another
    length, SGP4) raises InternalError whose `info` attribute is the record."""
    cctx = (context or Context())._c()
    return _land_call(lib().aptgpu_land_mask, (C.byref(cctx),), height_or_signal, track_or_orbit, layers, map_settings,
                      settings)


def land_mask_host(height_or_signal, track_or_orbit, layers, map_settings=None, settings=None):
    """land_mask() on the CPU, in plain C++ (no GPU needed): geolocate_host()'s points, the same source text per edge."""
    return _land_call(lib().aptgpu_land_mask_host, (), height_or_signal, track_or_orbit, layers, map_settings, settings)


def _land_plane_call(fn, head, latlon, layers, settings):
    cs = _land_c(layers, settings)
    ll = np.asarray(latlon)
    if ll.dtype != np.float64 or not ll.flags.c_contiguous:
        ll = np.ascontiguousarray(ll, dtype=np.float64)
    if ll.ndim < 1 or ll.shape[-1] != 2:
        raise InvalidError("land mask: the last axis of the plane holds (lat, lon)")
    n = ll.size // 2
    p_mask, info = _u8p(), _land_info()
    err = C.create_string_buffer(_ERRCAP)
    _check(fn(*head, C.c_void_p(ll.ctypes.data), n, layers._p, C.byref(cs), C.byref(p_mask), C.byref(info), err,
              _ERRCAP), err)
    return _take(p_mask, n, np.uint8).reshape(ll.shape[:-1]), info


def land_mask_plane(latlon, layers, settings=None, context=None):
    """The classes of arbitrary points, on the GPU: latlon is a (..., 2) float64 array of (lat, lon) in radians, such as
    geolocate()'s plane or the lat / lon of a map grid; a NaN in either is LAND_INVALID.  Returns (mask, info), the mask
    of latlon's shape without its last axis."""
    cctx = (context or Context())._c()
    return _land_plane_call(lib().aptgpu_land_mask_plane, (C.byref(cctx),), latlon, layers, settings)


def land_mask_plane_host(latlon, layers, settings=None):
    """land_mask_plane() on the CPU, in plain C++ (no GPU needed)."""
    return _land_plane_call(lib().aptgpu_land_mask_plane_host, (), latlon, layers, settings)


def _masked_color_call(fn, head, image, mask, palettes, tunes):
    image = np.ascontiguousarray(image, dtype=np.uint8)
    if image.ndim != 2 or image.shape[1] != PX_PER_ROW:
        raise InvalidError("false_color_masked: the image is an unrotated (height, 2080) uint8 array")
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    if mask.ndim != 2 or mask.shape[1] != GEOLOC_PX:
        raise InvalidError("false_color_masked: the mask is a (height, 909) uint8 array")
    pals = [np.ascontiguousarray(p, dtype=np.uint8) for p in palettes]
    if len(pals) != 3:
        raise InvalidError("false_color_masked: three palettes (sea, land, lake)")
    tn = np.ascontiguousarray(tunes, dtype=np.float32)
    if tn.shape != (4,):
        raise InvalidError("false_color_masked: tunes are (ch_a_start, ch_a_end, ch_b_start, ch_b_end)")
    h = image.shape[0]
    out = _u8p()
    err = C.create_string_buffer(_ERRCAP)
    _check(fn(*head, image.ctypes.data_as(_u8p), h, mask.ctypes.data_as(_u8p), mask.shape[0],
              (C.c_void_p * 3)(*[p.ctypes.data for p in pals]), (C.c_size_t * 3)(*[p.nbytes for p in pals]),
              tn.ctypes.data_as(_f32p), C.byref(out), err, _ERRCAP), err)
    return _take(out, h * PX_PER_ROW * 4, np.uint8).reshape(h, PX_PER_ROW, 4)


def false_color_masked(image, mask, palettes, tunes=(0.0, 0.0, 0.0, 0.0), context=None):
    """Map-coloured false colour, on the GPU: the unrotated gray image of process(rotate=Rotate.NO),
    (height, 2080) uint8, coloured over channel A's video columns by the palette of each pixel's class.  mask: the
    (height, 909) mask of land_mask(); palettes: three (256, 256, 3) uint8 arrays indexed [b, a], for sea, land and
    lake; tunes: ColorSettings' four tune values.  Returns (height, 2080, 4) RGBA; LAND_INVALID pixels and everything
    outside the video columns stay gray.  Rotate afterwards if the pass needs it."""
    cctx = (context or Context())._c()
    return _masked_color_call(lib().aptgpu_false_color_masked, (C.byref(cctx),), image, mask, palettes, tunes)


def false_color_masked_host(image, mask, palettes, tunes=(0.0, 0.0, 0.0, 0.0)):
    """false_color_masked() on the CPU, in plain C++ (no GPU needed)."""
    return _masked_color_call(lib().aptgpu_false_color_masked_host, (), image, mask, palettes, tunes)


FIT_REASON_NO_CANDIDATE = 17
FIT_REASON_FLAT = 18
FIT_SCORE_DTYPE = np.dtype([("score", np.uint64), ("count", np.uint32), ("zero", np.uint32)])


class FitSettings:
    """aptgpu_fit_settings with the suggested defaults, which have not been tried on a real pass.
    channel: "A" / "B" (or 0 / 1).  layers: an iterable of MAP_* layer indices, None: countries and lakes.  Round p
    of `rounds` searches centre + i * step / 2^p, i in [-n, n], on each axis (shift_step >> p rows, at least 1) and
    scores against the gradient summed over a box of radius << (rounds - 1 - p)."""

    def __init__(self, channel="A", layers=None, margin_rows=120, shift_step=8, n_shift=15, yaw_step=0.02, n_yaw=3,
                 hscale_step=0.04, n_hscale=3, vscale_step=0.04, n_vscale=3, rounds=4, radius=2, spacing_deg=0.05,
                 min_points=64, timing=False, flags=0):
        self.channel, self.layers, self.margin_rows = channel, layers, margin_rows
        self.shift_step, self.n_shift, self.yaw_step, self.n_yaw = shift_step, n_shift, yaw_step, n_yaw
        self.hscale_step, self.n_hscale, self.vscale_step, self.n_vscale = hscale_step, n_hscale, vscale_step, n_vscale
        self.rounds, self.radius, self.spacing_deg, self.min_points = rounds, radius, spacing_deg, min_points
        self.timing, self.flags = timing, flags

    def _mask(self):
        if self.layers is None:
            return 0
        mask = 0
        for k in self.layers:
            mask |= 1 << int(k)
        return mask

    def _c(self, struct_size=None):
        ch = {"A": 0, "B": 1}.get(self.channel, self.channel)
        return _CFitSettings(C.sizeof(_CFitSettings) if struct_size is None else int(struct_size), int(self.flags),
                             int(ch), self._mask(), int(self.margin_rows), int(self.rounds), int(self.radius),
                             int(self.min_points), int(self.shift_step), int(self.n_shift), int(self.n_yaw),
                             int(self.n_hscale), int(self.n_vscale), int(bool(self.timing)), float(self.yaw_step),
                             float(self.hscale_step), float(self.vscale_step), float(self.spacing_deg))


class OverlayFit:
    """What fit_overlay() found, ready to hand on: map_settings (the initial colours kept), shift_rows and
    time_offset_ms = 500 * shift_rows, the h-row `track` when a track was passed or `orbit`, the OrbitSettings with its
    reference time moved and the fitted settings as draw_map; rounds (the FitRound entries that ran), q and count of
    the winner, `info` (the FitResult) and, when asked for, `scores`: (rounds, candidates) records of score and count."""

    def __init__(self, info, map_settings, track, orbit, scores):
        self.info, self.map_settings, self.track, self.orbit, self.scores = info, map_settings, track, orbit, scores
        self.shift_rows, self.time_offset_ms = int(info.shift_rows), int(info.time_offset_ms)
        self.q, self.count, self.reason = float(info.q), int(info.count), int(info.reason)
        self.rounds = [info.round[i] for i in range(int(info.n_rounds))]


def margin_track(orbit: "OrbitSettings", height, margin_rows):
    """The long track fit_overlay() takes, on the CPU: height + 2 * margin_rows (lat, lon) pairs in radians, row r at
    start + 500 ms * (r - margin_rows), where start is the time of image row 0 under `orbit`."""
    height, m = int(height), int(margin_rows)
    start = orbit.ref_time.unix_ms - (500 * height if orbit.ref_time.kind == RefTime.END else 0)
    return sat_track_host(OrbitSettings(orbit.sat_name, orbit.custom_tle, RefTime.Start(start - 500 * m)), height + 2 * m)


def fit_sample_points(layers: "MapLayers", layer_ids=None, spacing_deg=0.05):
    """The fit's sample points (aptgpu_fit_sample_points, CPU): an (n, 2) array of (lon, lat) in degrees."""
    if not isinstance(layers, MapLayers):
        raise InvalidError("fit: layers must be a MapLayers")
    xy, n = _f64p(), C.c_size_t()
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_fit_sample_points(layers._p, FitSettings(layers=layer_ids)._mask(), float(spacing_deg),
                                          C.byref(xy), C.byref(n), err, _ERRCAP), err)
    return _take(xy, 2 * n.value, np.float64).reshape(-1, 2)


def _fit_call(fn, head, image, height, track_or_orbit, layers, map_settings, settings, return_scores):
    settings = settings if settings is not None else FitSettings()
    if not isinstance(settings, FitSettings):
        raise InvalidError("fit: settings must be a FitSettings")
    if map_settings is not None and not isinstance(map_settings, MapSettings):
        raise InvalidError("fit: map_settings must be a MapSettings or None")
    if not isinstance(layers, MapLayers):
        raise InvalidError("fit: layers must be a MapLayers")
    try:
        cs = settings._c()
    except (TypeError, ValueError, OverflowError) as e:
        raise InvalidError(f"fit: {e}") from None
    cms = map_settings._c() if map_settings is not None else None
    pos, count, co, keep, track = None, 0, None, None, None
    if isinstance(track_or_orbit, OrbitSettings):
        c_orbit, keep = track_or_orbit._c()
        co = C.byref(c_orbit)
    elif track_or_orbit is not None:
        track = np.ascontiguousarray(np.asarray(track_or_orbit, dtype=np.float64).reshape(-1, 2))
        pos, count = track.ctypes.data_as(_f64p), track.shape[0]
    info = FitResult()
    info.struct_size = C.sizeof(FitResult)
    p_scores, n_scores = C.c_void_p(), C.c_size_t()
    err = C.create_string_buffer(_ERRCAP)
    try:
        _check(fn(*head, image, height, pos, count, co, layers._p, C.byref(cms) if cms is not None else None,
                  C.byref(cs), C.byref(info), C.byref(p_scores) if return_scores else None,
                  C.byref(n_scores) if return_scores else None, err, _ERRCAP), err)
    except AptError as e:
        e.info = info  # (the record of a failed call: status, reason, the rounds that ran)
        raise
    del keep
    scores = None
    if return_scores:
        raw = C.string_at(p_scores, n_scores.value * FIT_SCORE_DTYPE.itemsize)
        lib().aptgpu_free(p_scores)
        scores = np.frombuffer(raw, FIT_SCORE_DTYPE).reshape(int(cs.rounds), -1)
    base = map_settings if map_settings is not None else MapSettings()
    fitted = MapSettings(info.yaw, info.hscale, info.vscale, base.countries_color, base.states_color, base.lakes_color)
    out_track, out_orbit = None, None
    if track is not None:
        m = int(cs.margin_rows) + int(info.shift_rows)
        out_track = track[m:m + int(height)].copy()
    else:
        rt = track_or_orbit.ref_time
        out_orbit = OrbitSettings(track_or_orbit.sat_name, track_or_orbit.custom_tle,
                                  RefTime(rt.kind, rt.unix_ms + int(info.time_offset_ms)), fitted)
    return OverlayFit(info, fitted, out_track, out_orbit, scores)


def _fit_image(image):
    image = np.ascontiguousarray(image, dtype=np.uint8)
    if image.ndim != 2 or image.shape[1] != PX_PER_ROW:
        raise InvalidError("fit: the image is an unrotated (height, 2080) uint8 array")
    return image


def fit_overlay(image, track_or_orbit, layers, map_settings=None, settings=None, context=None, return_scores=False):
    """Fits the map overlay to the image on the GPU: the yaw, hscale and vscale and the shift of the
    track, in rows of 500 ms, under which the layers' lines lie on the image's edges.  image: the unrotated gray image
    of process(rotate=Rotate.NO), (height, 2080) uint8.  track_or_orbit: a long track of height + 2 * margin_rows
    (lat, lon) pairs in radians (margin_track() makes one), or an OrbitSettings (SGP4 then runs on the GPU).  Returns
    an OverlayFit.  A failed call (a track of another length, SGP4, no candidate with min_points points inside)
    raises InternalError whose `info` attribute is the record; a flat image returns the initial settings with
    reason FIT_REASON_FLAT."""
    image = _fit_image(image)
    cctx = (context or Context())._c()
    return _fit_call(lib().aptgpu_fit_overlay, (C.byref(cctx),), image.ctypes.data_as(_u8p), image.shape[0],
                     track_or_orbit, layers, map_settings, settings, return_scores)


def fit_overlay_host(image, track_or_orbit, layers, map_settings=None, settings=None, return_scores=False):
    """fit_overlay() on the CPU, in plain C++ (no GPU needed): the same source text per point and candidate with the C
    library's f64 functions."""
    image = _fit_image(image)
    return _fit_call(lib().aptgpu_fit_overlay_host, (), image.ctypes.data_as(_u8p), image.shape[0], track_or_orbit,
                     layers, map_settings, settings, return_scores)


def fit_overlay_device(d_image, height, track_or_orbit, layers, map_settings=None, settings=None, context=None,
                       stream=None, return_scores=False):
    """fit_overlay() for an image already in the memory of the context's device: d_image is the device address of
    height rows of 2080 bytes, stream a hipStream_t as an integer (None: the default stream).  Returns once the record
    has been read."""
    cctx = (context or Context())._c()
    c_stream = C.c_void_p(int(stream)) if stream is not None else None

    def call(ctx, img, h, *rest):
        return lib().aptgpu_fit_overlay_device(ctx, img, h, c_stream, *rest)
    return _fit_call(call, (C.byref(cctx),), C.c_void_p(int(d_image)), int(height), track_or_orbit, layers,
                     map_settings, settings, return_scores)


class IqFormat:
    """aptgpu_fm_settings.format: how one component of a frame is stored (interleaved I then Q, never scaled)."""
    U8 = 0   # v - 127.5, the rtl_sdr convention
    S8 = 1
    S16 = 2  # little endian
    F32 = 3
    _DTYPES = {0: np.uint8, 1: np.int8, 2: np.dtype("<i2"), 3: np.dtype("<f4")}

    @staticmethod
    def dtype(fmt):
        try:
            return np.dtype(IqFormat._DTYPES[int(fmt)])
        except (KeyError, TypeError, ValueError):
            raise InvalidError(f"aptgpu_fm_settings: format is not an IqFormat value: {fmt!r}") from None


FM_SWAP_IQ = 1
FM_MAX_BATCH = 64


@dataclass
class FmSettings:
    """aptgpu_fm_settings.  format: an IqFormat; sample_rate: complex frames per second (fs); decimation: D, the audio
    comes out at fs / D; shift_hz: the signal's offset from the recording's centre; channel_*: the Kaiser low-pass in
    front of the discriminator; deviation_hz: the deviation that maps to +-1; swap_iq: exchange I and Q."""
    format: int
    sample_rate: int
    decimation: int = 1
    shift_hz: float = 0.0
    channel_cutout_hz: float = 18000.0
    channel_atten: float = 40.0
    channel_delta_hz: float = 8000.0
    deviation_hz: float = 17000.0
    swap_iq: bool = False
    flags: Optional[int] = None  # overrides swap_iq (raw aptgpu_fm_settings.flags)

    def _c(self, struct_size=None):
        try:
            rate = self.sample_rate.get_hz() if isinstance(self.sample_rate, Rate) else self.sample_rate
            flags = (FM_SWAP_IQ if self.swap_iq else 0) if self.flags is None else int(self.flags)
            return _CFmSettings(C.sizeof(_CFmSettings) if struct_size is None else int(struct_size), int(self.format),
                                int(rate), int(self.decimation), float(self.shift_hz), float(self.channel_cutout_hz),
                                float(self.channel_atten), float(self.channel_delta_hz), float(self.deviation_hz),
                                flags, 0)
        except (TypeError, ValueError, OverflowError) as e:
            raise InvalidError(f"aptgpu_fm_settings: {e}") from None


@dataclass(frozen=True)
class FmInfo:
    """aptgpu_fm_info: the output rate, the taps h (T of them), D, the phase increment per frame (2^32 = one turn)
    and the shift it stands for."""
    rate: Rate
    taps: np.ndarray
    decimation: int
    pw: int
    shift_hz_used: float

    @property
    def n_taps(self):
        return int(self.taps.size)


def _fm_settings_c(settings, struct_size=None):
    if not isinstance(settings, FmSettings):
        raise InvalidError("fm: settings must be an FmSettings")
    return settings._c(struct_size)


def fm_design(settings, struct_size=None) -> FmInfo:
    """The checks and the design of an FmSettings alone, on the host (no GPU): every refusal raises InvalidError with
    the field's name."""
    cs = _fm_settings_c(settings, struct_size)
    info, taps = _CFmInfo(struct_size=C.sizeof(_CFmInfo)), _f32p()
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_fm_design(C.byref(cs), C.byref(info), C.byref(taps), err, _ERRCAP), err)
    return FmInfo(Rate.hz(info.fs_out), _take(taps, info.n_taps), int(info.decimation), int(info.pw),
                  float(info.shift_hz_used))


def _fm_iq(iq, cs):
    """-> (contiguous array of the format's components, frames)"""
    dt = IqFormat.dtype(cs.format)
    if isinstance(iq, (bytes, bytearray, memoryview)):
        a = np.frombuffer(iq, dtype=np.uint8)
        a = a[:a.size - a.size % (2 * dt.itemsize)].view(dt)
    else:
        a = np.asarray(iq)
        if a.dtype == np.complex64 and dt == np.dtype("<f4"):
            a = np.ascontiguousarray(a).view(np.float32)
        if a.dtype != dt:
            raise InvalidError(f"fm: iq has dtype {a.dtype}, the format's is {dt}")
        a = np.ascontiguousarray(a).reshape(-1)
    return a, a.size // 2


def _fm_call(fn, head, iq, settings):
    cs = _fm_settings_c(settings)
    a, frames = _fm_iq(iq, cs)
    out, n, rate = _f32p(), C.c_size_t(), C.c_uint32()
    err = C.create_string_buffer(_ERRCAP)
    _check(fn(*head, C.byref(cs), a.ctypes.data if a.size else None, frames, C.byref(out), C.byref(n), C.byref(rate),
              err, _ERRCAP), err)
    return _take(out, n.value), Rate.hz(rate.value)


def fm_demodulate(iq, settings, context=None):
    """FM-demodulate an IQ recording on the GPU: convert, mix by settings.shift_hz, low-pass and
    decimate by settings.decimation, discriminate.  iq: interleaved I, Q components in the format's dtype (or bytes;
    complex64 for F32).  Returns (audio, Rate): f32 at sample_rate / decimation, for decode() at that rate."""
    cctx = (context or Context())._c()
    return _fm_call(lib().aptgpu_fm_demodulate, (C.byref(cctx),), iq, settings)


def fm_demodulate_host(iq, settings):
    """fm_demodulate() on the CPU, in plain C++ (no GPU needed): the same f32 arithmetic up to sincos and atan2."""
    return _fm_call(lib().aptgpu_fm_demodulate_host, (), iq, settings)


def fm_demodulate_wav(file_bytes, settings, context=None):
    """fm_demodulate() of a two-channel WAV (16-bit integer or 32-bit float): the format and the rate come from the
    header and overrule the settings' fields."""
    cctx, cs = (context or Context())._c(), _fm_settings_c(settings)
    data = bytes(file_bytes)
    out, n, rate = _f32p(), C.c_size_t(), C.c_uint32()
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_fm_demodulate_wav(C.byref(cctx), C.byref(cs), data, len(data), C.byref(out), C.byref(n),
                                          C.byref(rate), err, _ERRCAP), err)
    return _take(out, n.value), Rate.hz(rate.value)


def load_iq(path, fmt=None, sample_rate=None):
    """An IQ recording from a file: (iq, IqFormat value, Rate), iq being the interleaved components in the format's
    dtype.  A two-channel WAV (16-bit integer or 32-bit float) is read through its header; with both `fmt` and
    `sample_rate` given the file is raw frames (a trailing partial frame is dropped).  Also accepts the file's bytes."""
    if isinstance(path, (bytes, bytearray, memoryview)):
        data = bytes(path)
    else:
        with open(path, "rb") as f:
            data = f.read()
    if (fmt is None) != (sample_rate is None):
        raise InvalidError("load_iq: a raw file needs both fmt and sample_rate")
    if fmt is not None:
        dt = IqFormat.dtype(fmt)
        rate = sample_rate if isinstance(sample_rate, Rate) else Rate.hz(sample_rate)
        n = len(data) - len(data) % (2 * dt.itemsize)
        return np.frombuffer(data, dtype=dt, count=n // dt.itemsize), int(fmt), rate
    spec = wav_parse(data)
    if spec.channels != 2 or spec.codec not in (1, 5):
        raise UnsupportedError("fm: an IQ WAV has two channels of 16-bit integer or 32-bit float samples")
    fmt = IqFormat.S16 if spec.codec == 1 else IqFormat.F32
    dt = IqFormat.dtype(fmt)
    iq = np.frombuffer(data, dtype=dt, count=int(spec.n_frames) * 2, offset=int(spec.data_offset))
    return iq, fmt, Rate.hz(spec.sample_rate)


class FmDemodulator:
    """aptgpu_fm: the taps of one FmSettings on the device, for recordings already in HBM.  Runs on `stream` (0: the
    null stream) of `device`; a Plan created on the same stream orders its decode behind demodulate_device()."""

    def __init__(self, settings, device=0, stream=0):
        cs = _fm_settings_c(settings)
        self._ctx = Context(device=device, stream=stream)
        cctx = self._ctx._c()
        self._p = C.c_void_p()
        err = C.create_string_buffer(_ERRCAP)
        _check(lib().aptgpu_fm_create(C.byref(cctx), C.byref(cs), C.byref(self._p), err, _ERRCAP), err)
        info = _CFmInfo(struct_size=C.sizeof(_CFmInfo))
        _check(lib().aptgpu_fm_get_info(self._p, C.byref(info)))
        taps = np.ctypeslib.as_array(info.taps, shape=(int(info.n_taps),)).copy()
        self.info = FmInfo(Rate.hz(info.fs_out), taps, int(info.decimation), int(info.pw), float(info.shift_hz_used))

    def close(self):
        if self._p:
            lib().aptgpu_fm_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def out_len(self, n_frames):
        return int(lib().aptgpu_fm_out_len(self._p, int(n_frames)))

    def demodulate_device(self, d_iq: Sequence[int], n_frames: Sequence[int], d_audio: Sequence[int],
                          audio_cap: Sequence[int]):
        """Up to FM_MAX_BATCH recordings in one launch, asynchronous on the demodulator's stream: d_iq[i] holds
        n_frames[i] frames (aligned to one component), d_audio[i] receives out_len(n_frames[i]) floats and must hold
        audio_cap[i] >= that."""
        k = len(d_iq)
        err = C.create_string_buffer(_ERRCAP)
        _check(lib().aptgpu_fm_demodulate_device(self._p, k, (C.c_void_p * k)(*d_iq), (C.c_size_t * k)(*n_frames),
                                                 (C.c_void_p * k)(*d_audio), (C.c_size_t * k)(*audio_cap), err,
                                                 _ERRCAP), err)


# aptgpu_afc_record: one block of the tracked demodulator's table
AFC_RECORD_DTYPE = np.dtype([("pw", "<u4"), ("phase0", "<u4"), ("step_re", "<f4"), ("step_im", "<f4")])


@dataclass
class AfcSettings:
    """aptgpu_afc_settings.  block_frames: B, a power of two in 64 ... 2^20; lag: L in 1 ... 64, 0 = auto;
    smooth_blocks: W, odd, 1 ... 1023; max_offset_hz: estimates further from shift_hz are not believed; min_coherence:
    in [0, 1), below it a block holds its neighbour's estimate."""
    block_frames: int = 4096
    lag: int = 0
    smooth_blocks: int = 15
    max_offset_hz: float = 15000.0
    min_coherence: float = 0.05

    def _c(self, struct_size=None):
        try:
            return _CAfcSettings(C.sizeof(_CAfcSettings) if struct_size is None else int(struct_size),
                                 int(self.block_frames), int(self.lag), int(self.smooth_blocks),
                                 float(self.max_offset_hz), float(self.min_coherence))
        except (TypeError, ValueError, OverflowError) as e:
            raise InvalidError(f"aptgpu_afc_settings: {e}") from None


@dataclass(frozen=True)
class AfcInfo:
    """aptgpu_afc_info: the settings as they are used (lag: the auto value where it was 0), the phase increment of
    shift_hz and the rate."""
    block_frames: int
    lag: int
    smooth_blocks: int
    pw_base: int
    sample_rate: int
    max_offset_hz: float
    min_coherence: float


@dataclass(frozen=True)
class AfcTable:
    """Stage B's outputs: records (AFC_RECORD_DTYPE: pw, phase0, step_re, step_im per block), coherence (f32) and good
    (bool), with the info they were made under."""
    records: np.ndarray
    coherence: Optional[np.ndarray]
    good: Optional[np.ndarray]
    info: AfcInfo

    @property
    def offset_hz(self):
        """the carrier's offset from the recording's centre that every block's pw stands for, in Hz"""
        return self.records["pw"].astype(np.int32).astype(np.float64) * self.info.sample_rate / 4294967296.0


def _afc_settings_c(afc, struct_size=None):
    afc = AfcSettings() if afc is None else afc
    if not isinstance(afc, AfcSettings):
        raise InvalidError("afc: afc_settings must be an AfcSettings")
    return afc._c(struct_size)


def fm_afc_design(settings, afc=None, struct_size=None) -> AfcInfo:
    """The checks of an FmSettings and an AfcSettings alone, on the host (no GPU): every refusal raises InvalidError
    with the field's name."""
    cs, ca = _fm_settings_c(settings), _afc_settings_c(afc, struct_size)
    info = _CAfcInfo(struct_size=C.sizeof(_CAfcInfo))
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_fm_afc_design(C.byref(cs), C.byref(ca), C.byref(info), err, _ERRCAP), err)
    return AfcInfo(int(info.block_frames), int(info.lag), int(info.smooth_blocks), int(info.pw_base),
                   int(info.sample_rate_hz), float(info.max_offset_hz), float(info.min_coherence))


def _afc_table(table, coh, good, n, info):
    records = _take(table, 4 * n, np.uint32).view(AFC_RECORD_DTYPE)
    return AfcTable(records, _take(coh, n), _take(good, n, np.uint8).astype(bool), info)


def _afc_records(table):
    a = table.records if isinstance(table, AfcTable) else np.asarray(table)
    if a.dtype != AFC_RECORD_DTYPE:
        raise InvalidError(f"afc: the table has dtype {a.dtype}, not AFC_RECORD_DTYPE")
    return np.ascontiguousarray(a).reshape(-1)


def _afc_sums_call(fn, head, iq, settings, afc):
    cs, ca = _fm_settings_c(settings), _afc_settings_c(afc)
    a, frames = _fm_iq(iq, cs)
    out, n = C.POINTER(C.c_double)(), C.c_size_t()
    err = C.create_string_buffer(_ERRCAP)
    _check(fn(*head, C.byref(cs), C.byref(ca), a.ctypes.data if a.size else None, frames, C.byref(out), C.byref(n), err,
              _ERRCAP), err)
    return _take(out, 3 * n.value, np.float64).reshape(-1, 3)


def fm_afc_sums(iq, settings, afc=None, context=None):
    """Stage A of the AFC on the GPU: the block sums of an IQ recording, an (nb, 3) f64 array of {re, im, en}: the lag-L
    autocorrelation and the energy of every block of block_frames frames (exact for the integer formats)."""
    cctx = (context or Context())._c()
    return _afc_sums_call(lib().aptgpu_fm_afc_sums, (C.byref(cctx),), iq, settings, afc)


def fm_afc_sums_host(iq, settings, afc=None):
    """fm_afc_sums() on the CPU, in plain C++ (no GPU needed)."""
    return _afc_sums_call(lib().aptgpu_fm_afc_sums_host, (), iq, settings, afc)


def _afc_estimate_call(fn, head, sums, settings, afc):
    cs, ca = _fm_settings_c(settings), _afc_settings_c(afc)
    s = np.ascontiguousarray(sums, dtype=np.float64)
    if s.ndim != 2 or s.shape[1] != 3:
        raise InvalidError("afc: sums must have shape (blocks, 3)")
    nb = s.shape[0]
    table, coh, good = _u32p(), _f32p(), C.POINTER(C.c_uint8)()
    err = C.create_string_buffer(_ERRCAP)
    _check(fn(*head, C.byref(cs), C.byref(ca), s.ctypes.data if nb else None, nb, C.byref(table), C.byref(coh),
              C.byref(good), err, _ERRCAP), err)
    return _afc_table(table, coh, good, nb, fm_afc_design(settings, afc))


def fm_afc_estimate(sums, settings, afc=None, context=None) -> AfcTable:
    """Stage B of the AFC on the GPU: the table of one record per block from the block sums of fm_afc_sums()."""
    cctx = (context or Context())._c()
    return _afc_estimate_call(lib().aptgpu_fm_afc_estimate, (C.byref(cctx),), sums, settings, afc)


def fm_afc_estimate_host(sums, settings, afc=None) -> AfcTable:
    """fm_afc_estimate() on the CPU, in plain C++ (no GPU needed): the same f64 arithmetic up to atan2, cos and sin."""
    return _afc_estimate_call(lib().aptgpu_fm_afc_estimate_host, (), sums, settings, afc)


def _afc_tracked_call(fn, head, iq, table, settings, afc):
    cs, ca = _fm_settings_c(settings), _afc_settings_c(afc)
    a, frames = _fm_iq(iq, cs)
    t = _afc_records(table)
    out, n, rate = _f32p(), C.c_size_t(), C.c_uint32()
    err = C.create_string_buffer(_ERRCAP)
    _check(fn(*head, C.byref(cs), C.byref(ca), a.ctypes.data if a.size else None, frames, t.ctypes.data if t.size else None,
              t.size, C.byref(out), C.byref(n), C.byref(rate), err, _ERRCAP), err)
    return _take(out, n.value), Rate.hz(rate.value)


def fm_demodulate_tracked(iq, table, settings, afc=None, context=None):
    """Stage C of the AFC on the GPU: fm_demodulate() with the phase of every frame taken from `table` (an AfcTable or an
    AFC_RECORD_DTYPE array of ceil(frames / block_frames) records).  Returns (audio, Rate)."""
    cctx = (context or Context())._c()
    return _afc_tracked_call(lib().aptgpu_fm_demodulate_tracked, (C.byref(cctx),), iq, table, settings, afc)


def fm_demodulate_tracked_host(iq, table, settings, afc=None):
    """fm_demodulate_tracked() on the CPU, in plain C++ (no GPU needed)."""
    return _afc_tracked_call(lib().aptgpu_fm_demodulate_tracked_host, (), iq, table, settings, afc)


def _afc_call(fn, head, iq, settings, afc):
    cs, ca = _fm_settings_c(settings), _afc_settings_c(afc)
    a, frames = _fm_iq(iq, cs)
    out, n, rate = _f32p(), C.c_size_t(), C.c_uint32()
    table, coh, good, nb = _u32p(), _f32p(), C.POINTER(C.c_uint8)(), C.c_size_t()
    err = C.create_string_buffer(_ERRCAP)
    _check(fn(*head, C.byref(cs), C.byref(ca), a.ctypes.data if a.size else None, frames, C.byref(out), C.byref(n),
              C.byref(rate), C.byref(table), C.byref(coh), C.byref(good), C.byref(nb), err, _ERRCAP), err)
    return (_take(out, n.value), Rate.hz(rate.value),
            _afc_table(table, coh, good, nb.value, fm_afc_design(settings, afc)))


def fm_demodulate_afc(iq, settings, afc=None, context=None):
    """FM-demodulate an IQ recording whose carrier is not where settings.shift_hz says, on the GPU:
    estimate the carrier block by block from the raw frames, then demodulate with an NCO that follows the estimates.
    Returns (audio, Rate, AfcTable): the audio for decode(), and the table with its offset_hz per block."""
    cctx = (context or Context())._c()
    return _afc_call(lib().aptgpu_fm_demodulate_afc, (C.byref(cctx),), iq, settings, afc)


def fm_demodulate_afc_host(iq, settings, afc=None):
    """fm_demodulate_afc() on the CPU, in plain C++ (no GPU needed)."""
    return _afc_call(lib().aptgpu_fm_demodulate_afc_host, (), iq, settings, afc)


class FmAfc:
    """aptgpu_fm_afc: the AFC behind an FmDemodulator, for recordings already in HBM of up to max_frames frames each.
    Runs on the demodulator's stream; the demodulator must stay open while this is."""

    def __init__(self, demodulator: "FmDemodulator", afc=None, max_frames=1 << 24):
        if not isinstance(demodulator, FmDemodulator) or not demodulator._p:
            raise InvalidError("afc: demodulator must be an open FmDemodulator")
        ca = _afc_settings_c(afc)
        self._fmd = demodulator
        self._p = C.c_void_p()
        err = C.create_string_buffer(_ERRCAP)
        _check(lib().aptgpu_fm_afc_create(demodulator._p, C.byref(ca), int(max_frames), C.byref(self._p), err, _ERRCAP),
               err)
        self.block_frames = int(ca.block_frames)

    def close(self):
        if self._p:
            lib().aptgpu_fm_afc_destroy(self._p)  # (does not need the demodulator alive)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def n_blocks(self, n_frames):
        return -(-int(n_frames) // self.block_frames)

    def demodulate_device(self, d_iq: Sequence[int], n_frames: Sequence[int], d_audio: Sequence[int],
                          audio_cap: Sequence[int], d_table: Optional[Sequence[int]] = None,
                          d_coherence: Optional[Sequence[int]] = None, d_good: Optional[Sequence[int]] = None,
                          d_sums: Optional[Sequence[int]] = None):
        """Up to FM_MAX_BATCH recordings through the three stages: three launches, asynchronous on the demodulator's
        stream.  d_iq, n_frames, d_audio, audio_cap as FmDemodulator.demodulate_device; d_table / d_coherence / d_good /
        d_sums: optional device pointers (0: none) that receive recording i's n_blocks(n_frames[i]) records (16 bytes
        each), f32 coherences, u8 good flags and f64 {re, im, en} sums."""
        if not self._p or not self._fmd._p:
            raise InvalidError("afc: the FmAfc or its FmDemodulator is closed")
        k = len(d_iq)

        def ptrs(v):
            return None if v is None else (C.c_void_p * k)(*[int(x) or None for x in v])
        err = C.create_string_buffer(_ERRCAP)
        _check(lib().aptgpu_fm_afc_demodulate_device(self._p, k, (C.c_void_p * k)(*d_iq), (C.c_size_t * k)(*n_frames),
                                                     (C.c_void_p * k)(*d_audio), (C.c_size_t * k)(*audio_cap),
                                                     ptrs(d_sums), ptrs(d_table), ptrs(d_coherence), ptrs(d_good), err,
                                                     _ERRCAP), err)


FM_STREAM_MAX_PUSH_FRAMES = 1 << 20


class FmStream:
    """aptgpu_fm_stream: fm_demodulate() in streaming form.  Push the frames in chunks of any size;
    every push returns the outputs that became final, with the bits fm_demodulate() of the whole recording gives them
    (host=True: fm_demodulate_host(), in plain C++ on the CPU).  A push that takes the frame count from n0 to n1 returns
    exactly a[out_len(n0) .. out_len(n1)).  first_frame: the absolute index of the first frame (the phase uses its low
    32 bits).  There is no finish: nothing is held back."""

    def __init__(self, settings, context=None, max_push_frames=None, first_frame=0, host=False, struct_size=None):
        cs = _fm_settings_c(settings)
        self._ctx = context or Context()
        self._cs = cs
        try:
            css = _CFmStreamSettings(C.sizeof(_CFmStreamSettings) if struct_size is None else int(struct_size),
                                     FM_STREAM_MAX_PUSH_FRAMES if max_push_frames is None else int(max_push_frames),
                                     int(first_frame), 0)
        except (TypeError, ValueError, OverflowError) as e:
            raise InvalidError(f"aptgpu_fm_stream_settings: {e}") from None
        self._p = C.c_void_p()
        self.host = bool(host)
        err = C.create_string_buffer(_ERRCAP)
        if host:
            rc = lib().aptgpu_fm_stream_create_host(C.byref(cs), C.byref(css), C.byref(self._p), err, _ERRCAP)
        else:
            cctx = self._ctx._c()
            rc = lib().aptgpu_fm_stream_create(C.byref(cctx), C.byref(cs), C.byref(css), C.byref(self._p), err, _ERRCAP)
        _check(rc, err)
        self.info = self.get_info()
        self.rate = Rate.hz(self.info.fs_out)

    def close(self):
        if self._p:
            lib().aptgpu_fm_stream_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def get_info(self):
        info = FmStreamInfo(struct_size=C.sizeof(FmStreamInfo))
        _check(lib().aptgpu_fm_stream_get_info(self._p, C.byref(info)))
        return info

    def out_len(self, n_frames):
        """The outputs a push of n_frames more frames returns now."""
        return int(lib().aptgpu_fm_stream_out_len(self._p, int(n_frames)))

    def reset(self):
        err = C.create_string_buffer(_ERRCAP)
        _check(lib().aptgpu_fm_stream_reset(self._p, err, _ERRCAP), err)

    def push(self, iq, audio_cap=None):
        """iq: interleaved components of the format's dtype (or bytes; complex64 for F32) -> the f32 outputs that
        became final."""
        a, frames = _fm_iq(iq, self._cs)
        cap = self.out_len(frames) if audio_cap is None else int(audio_cap)
        out = np.empty(max(cap, 1), np.float32)
        n = C.c_size_t()
        err = C.create_string_buffer(_ERRCAP)
        _check(lib().aptgpu_fm_stream_push(self._p, a.ctypes.data if a.size else None, frames, out.ctypes.data, cap,
                                           C.byref(n), err, _ERRCAP), err)
        return out[:n.value].copy()

    def push_device(self, d_iq, n_frames, d_audio, audio_cap):
        """Device pointers (ints); asynchronous on the context's stream.  Returns the outputs the push writes."""
        n = C.c_size_t()
        err = C.create_string_buffer(_ERRCAP)
        _check(lib().aptgpu_fm_stream_push_device(self._p, d_iq or None, int(n_frames), d_audio or None, int(audio_cap),
                                                  C.byref(n), err, _ERRCAP), err)
        return int(n.value)


class LiveIqDecoder(_LiveBase):
    """aptgpu_iq_live: live decode from IQ frames: an FmStream in front of a LiveDecoder on one HIP
    stream, the audio staying on the device.  The surface is LiveDecoder's, with frames for samples: push() returns
    the rows that became final and their positions, finish() the rest or decode()'s error.  `fm_info` and `info` are
    the two stages' infos, `result` the record of the last call.  track: a LiveTrackSettings, as for LiveDecoder
    (DESIGN.md §24): `scores` and `track_result` then hold the lock indicators of the last call's rows and the
    tracker's record."""
    _PREFIX = "aptgpu_iq_live"

    def __init__(self, settings, fm_settings, sync=True, context=None, max_push_frames=None, max_push=None, first_frame=0,
                 host=False, track=None):
        self._cfm = _fm_settings_c(fm_settings)
        self._ctx = context or Context()
        cctx, cs = self._ctx._c(), settings._c()
        cls = _CIqLiveSettings(C.sizeof(_CIqLiveSettings), 1 if sync else 0, int(max_push_frames or 0), int(max_push or 0),
                               int(first_frame))
        self._create(host, track, cctx, cs, self._cfm, cls)
        self.fm_info, self.info = self.get_info()

    def get_info(self):
        """-> (FmStreamInfo, StreamInfo)"""
        fi, si = FmStreamInfo(struct_size=C.sizeof(FmStreamInfo)), StreamInfo(struct_size=C.sizeof(StreamInfo))
        _check(lib().aptgpu_iq_live_get_info(self._p, C.byref(fi), C.byref(si)))
        return fi, si

    def rows_bound(self, n_frames=0):
        """Upper bound of the rows a push of n_frames more frames (0: a finish) can release now."""
        return int(lib().aptgpu_iq_live_rows_bound(self._p, int(n_frames)))

    def push(self, iq, rows_cap=None):
        """iq: interleaved components of the format's dtype -> (rows [n, 2080] f32, positions [n] u64) that became
        final."""
        a, frames = _fm_iq(iq, self._cfm)
        return self._call(a.ctypes.data if a.size else None, frames, rows_cap)

    def push_device(self, d_iq, n_frames, d_rows, d_positions, rows_cap):
        """Device pointers (ints); asynchronous on the context's stream.  rows_cap >= rows_bound(n_frames)."""
        self._push_device(d_iq or None, n_frames, d_rows, d_positions, rows_cap)


def decode_live_iq(context: Optional["Context"], settings: "Settings", fm_settings: "FmSettings", chunks, sync: bool,
                   host=False, max_push_frames=None, track=None, return_info=False):
    """decode(fm_demodulate(...)) over an iterable of IQ chunks through a LiveIqDecoder: returns the rows of the
    chunks' concatenation (flat f32, rows * 2080) and raises what decode() raises.  track: a LiveTrackSettings
    (DESIGN.md §24); return_info then gives (rows, positions, scores, StreamTrackResult)."""
    dec = LiveIqDecoder(settings, fm_settings, sync, context, max_push_frames, host=host, track=track)
    return _collect_live(dec, chunks, return_info)


def process(context, signal, contrast_adjustment, rotate=Rotate.NO, color=None, orbit=None,
            return_info=False, png=False, layers=None, projection=None, despeckle=None):  # noqa: A002
    """noaa_apt::process (noaa_apt.rs:132-235).  Returns the height x 2080 u8
    gray image, or with `color` (a ColorSettings) the height x 2080 x 4 RGBA image of the reference's
    false colour (A = 255).  Contrast.HISTOGRAM equalises each channel half of the gray image; together with
    false colour it needs ColorSettings(equalize_lab=True) (the reference equalises channel A in CIE Lab then).
    Contrast.HISTOGRAM_FLOAT equalises each half on the f32 samples themselves (exact ranks, all 256 levels in use);
    it takes no colour (UnsupportedError) and chains into the overlay, PNG, orbit and projection like HISTOGRAM.
    `orbit` may be a MapOverlay: the map is drawn over the RGBA image (height x 2080 x 4, also without colour).
    png=True: the image is also encoded on the GPU and the PNG file's bytes are returned instead of the pixels
    (what `img.save()` writes in main.rs; gray without colour and map, RGBA with).
    `orbit` may also be the reference's OrbitSettings: the track is then computed on the GPU with SGP4; with
    draw_map set the map is drawn (`layers`, a MapLayers, is required then: the reference finds its shapefiles
    itself), and Rotate.ORBIT rotates south-to-north passes.
    Unsupported: any other `orbit`, Rotate.ORBIT without an OrbitSettings (the reference only warns and does not
    rotate; with a MapOverlay too: a bare track carries no time to decide with), and HISTOGRAM with colour without
    equalize_lab.
    projection (a ProjectionSettings): the finished image is reprojected on the GPU onto a north-up map grid and the
    (grid height, grid width, 4) RGBA array is returned (or its PNG file).  The track comes from `orbit`: a
    MapOverlay or an OrbitSettings with draw_map (the map is drawn on the swath first), an OrbitSettings without, or
    plain sat_positions (no map).  It reads the unrotated image and north is up by construction: any rotate but
    Rotate.NO raises InvalidError.
    despeckle (a DespeckleSettings): the signal goes through despeckle() first and the filtered rows are handed to
    whichever path the other arguments select.  These are two library calls (the rows cross to the host in between);
    the device-resident composition is Plan.despeckle_device followed by Plan.process_device_image."""
    if despeckle is not None:
        if not isinstance(despeckle, DespeckleSettings):
            raise InvalidError("despeckle must be a DespeckleSettings")
        signal = _despeckle(signal, despeckle, context)
        return process(context, signal, contrast_adjustment, rotate, color, orbit, return_info, png, layers, projection)
    if projection is not None or orbit is not None or png or color is not None or \
            contrast_adjustment in (Contrast.HISTOGRAM, Contrast.HISTOGRAM_FLOAT):
        return _process_image(context, signal, contrast_adjustment, rotate, color, return_info, orbit, None, png, layers,
                              projection)
    cctx = (context or Context())._c()
    x, xp = _as_f32(signal)
    kind, p = Contrast._c(contrast_adjustment)
    img, n, info = _u8p(), C.c_size_t(), ImageResult()
    err = C.create_string_buffer(_ERRCAP)
    _check(lib().aptgpu_process_gray(C.byref(cctx), xp, x.size, kind, p, int(rotate), C.byref(img),
                                     C.byref(n), C.byref(info), err, _ERRCAP), err)
    out = _take(img, n.value, np.uint8).reshape(-1, PX_PER_ROW)
    return (out, info) if return_info else out


def _process_image(context, signal, contrast_adjustment, rotate, color, return_info, orbit=None, channels=None,
                   png=False, layers=None, projection=None):
    """process() through the image entry points, rows and image on the host (channels: 1 or 4, process() leaves it
    to the request)."""
    if projection is not None and not isinstance(projection, ProjectionSettings):
        raise InvalidError("projection must be a ProjectionSettings")
    if projection is None and orbit is not None and not isinstance(orbit, (MapOverlay, OrbitSettings)):
        raise UnsupportedError("orbit: only a MapOverlay (the map overlay) is served on the GPU path")
    req = _ImageRequest(contrast_adjustment, rotate, color, channels)
    if projection is not None and orbit is None:
        raise InvalidError("a projection needs the track: orbit = a MapOverlay, an OrbitSettings or the sat_positions")
    grids = [projection] if projection is not None else None
    if isinstance(orbit, OrbitSettings):
        req.resolve(1, None, orbit, layers, png, grids)
    else:  # (nothing, a MapOverlay or, under a projection, the sat_positions)
        req.resolve(1, orbit if orbit is None or isinstance(orbit, MapOverlay) else [orbit], None, layers, png, grids)
    cctx = (context or Context())._c()
    x, xp = _as_f32(signal)
    if req.counts is not None and req.counts[0] != x.size // PX_PER_ROW:  # (the plan leaves this to the record)
        raise InvalidError(f"{'MapOverlay' if projection is None else 'projection'}: {req.counts[0]} positions for "
                           f"{x.size // PX_PER_ROW} rows")
    pos = req.positions[0] if req.positions is not None else None
    orb = req.orbits[0] if req.orbits is not None else None
    cmap, lay, output, cpng = _ref(req.cmap), req.layers_p, 1 if png else 0, C.byref(req.cpng)
    tail = {"_project": (cmap, lay, pos, orb, req.cgrids, output, cpng), "_orbit": (orb, lay, output, cpng),
            "_png": (cmap, lay, pos, cpng), "_map": (cmap, lay, pos), "": ()}[req.entry]
    img, n, info = _u8p(), C.c_size_t(), ImageResult()
    err = C.create_string_buffer(_ERRCAP)
    _check(getattr(lib(), "aptgpu_process_image" + req.entry)(
        C.byref(cctx), xp, x.size, *req.head, *tail, C.byref(img), C.byref(n), C.byref(info), err, _ERRCAP), err)
    out = _take(img, n.value, np.uint8)
    if png:
        out = out.tobytes()
    elif projection is not None:
        out = out.reshape(projection.shape)
    else:
        out = out.reshape(-1, PX_PER_ROW, 4) if req.channels == 4 else out.reshape(-1, PX_PER_ROW)
    return (out, info) if return_info else out


# ------------------------------------------------------------------ host-fed batch over GPUs
def decode_batch(context: Optional[Context], settings: Settings, inputs, input_rate: Rate, sync: bool,
                 devices: Sequence[int] = (), recordings_per_call: int = 0, return_stats=False):
    """aptgpu_decode_batch / aptgpu_decode_batch_wav: independent recordings — f32 Signals (numpy arrays) or
    WAV file images (bytes) — decoded on `devices` (ordinals, repeats allowed; empty = the context's
    device), no collectives.  Returns a list with one entry per recording: the rows (flat f32 array), or
    the AptError decode() would have raised for it; optionally also the result records and BatchStats."""
    cctx = (context or Context())._c()
    cs = settings._c()
    k = len(inputs)
    wav = k > 0 and isinstance(inputs[0], (bytes, bytearray, memoryview))
    keep, ptrs, sizes = [], (C.c_void_p * max(k, 1))(), (C.c_size_t * max(k, 1))()
    for i, x in enumerate(inputs):
        if wav:
            b = bytes(x)
            keep.append(b)
            ptrs[i] = C.cast(C.c_char_p(b), C.c_void_p)
            sizes[i] = len(b)
        else:
            a, ap = _as_f32(x)
            keep.append(a)
            ptrs[i] = C.cast(ap, C.c_void_p)
            sizes[i] = a.size
    devs = (C.c_int32 * max(len(devices), 1))(*devices)
    rows = (_f32p * max(k, 1))()
    n_out = (C.c_size_t * max(k, 1))()
    status = (C.c_int32 * max(k, 1))()
    results = (Result * max(k, 1))()
    stats = BatchStats()
    stats.struct_size = C.sizeof(BatchStats)
    err = C.create_string_buffer(_ERRCAP)
    fn = lib().aptgpu_decode_batch_wav if wav else lib().aptgpu_decode_batch
    rc = fn(C.byref(cctx), C.byref(cs), input_rate.get_hz(), int(sync), k, ptrs, sizes, devs, len(devices),
            int(recordings_per_call), rows, n_out, status, results, C.byref(stats), err, _ERRCAP)
    if rc != 0:
        # a worker-level failure (HIP error, bad argument): nothing of what finished before it is leaked
        for i in range(k):
            if rows[i]:
                lib().aptgpu_free(C.cast(rows[i], C.c_void_p))
        _check(rc, err)
    out = []
    for i in range(k):
        if status[i] == 0:
            out.append(_take(rows[i], n_out[i]))
            continue
        reason = {1: "Got less than 10 rows of samples, audio file is too short",
                  2: "Found less than 5 sync frames, audio file is too short or too noisy",
                  3: "work_rate is not multiple of FINAL_RATE"}.get(results[i].reason, "")
        if not reason and wav:
            # rejected before it reached a worker: the reference's message for this file (wav.rs / err.rs:72-83),
            # or the one thing a batch adds — every recording of a batch has the batch's input rate
            try:
                spec = wav_parse(keep[i])
                if spec.sample_rate != input_rate.get_hz():
                    reason = (f"recording {i}: WAV sample rate {spec.sample_rate} Hz differs from the batch's "
                              f"input rate {input_rate.get_hz()} Hz")
            except AptError as e:
                reason = str(e)
        elif not reason and sizes[i] and not ptrs[i]:
            reason = f"recording {i}: null input"
        out.append(_ERRORS.get(status[i], AptError)(reason or f"recording {i}: status {status[i]}"))
    return (out, list(results)[:k], stats) if return_stats else out


def host_alloc_f32(n: int) -> np.ndarray:
    """A pinned (hipHostMalloc) f32 buffer of n samples as a numpy array; free with host_free(array)."""
    p = lib().aptgpu_host_alloc(int(n) * 4)
    if not p:
        raise HipError("aptgpu_host_alloc failed")
    arr = np.ctypeslib.as_array(C.cast(p, _f32p), shape=(int(n),))
    _PINNED[arr.ctypes.data] = p
    return arr


def host_free(arr: np.ndarray):
    p = _PINNED.pop(arr.ctypes.data, None)
    if p:
        lib().aptgpu_host_free(p)


_PINNED = {}


# ------------------------------------------------------------------ plans (device-resident)
class Plan:
    """aptgpu_plan: device-resident / batched decode().  Device pointers are plain ints
    (e.g. torch.Tensor.data_ptr()); torch is only the allocator, never on the compute path."""

    def __init__(self, settings: Settings, input_rate: Rate, sync=True, max_samples=0, max_batch=1,
                 device=0, mode=MODE_STRICT, stream=0):
        self._ctx = Context(device=device, mode=mode, stream=stream)
        cctx, cs = self._ctx._c(), settings._c()
        self._p = C.c_void_p()
        err = C.create_string_buffer(_ERRCAP)
        _check(lib().aptgpu_plan_create(C.byref(cctx), C.byref(cs), input_rate.get_hz(),
                                        1 if sync else 0, int(max_samples), int(max_batch),
                                        C.byref(self._p), err, _ERRCAP), err)
        self.info = PlanInfo()
        _check(lib().aptgpu_plan_get_info(self._p, C.byref(self.info)))

    def close(self):
        if self._p:
            lib().aptgpu_plan_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def decode_device(self, d_signals: Sequence[int], n: Sequence[int], d_rows: Sequence[int],
                      rows_cap: Sequence[int]):
        k = len(d_signals)
        sig = (C.c_void_p * k)(*d_signals)
        rows = (C.c_void_p * k)(*d_rows)
        nn = (C.c_size_t * k)(*n)
        cap = (C.c_size_t * k)(*rows_cap)
        err = C.create_string_buffer(_ERRCAP)
        _check(lib().aptgpu_plan_decode_device(self._p, k, sig, nn, rows, cap, err, _ERRCAP), err)

    def decode_device_wav(self, d_data: Sequence[int], specs: Sequence[WavSpec], d_rows: Sequence[int],
                          rows_cap: Sequence[int]):
        """As decode_device, but every recording is the payload of a WAV data chunk in HBM."""
        k = len(d_data)
        err = C.create_string_buffer(_ERRCAP)
        _check(lib().aptgpu_plan_decode_device_wav(self._p, k, (C.c_void_p * k)(*d_data),
                                                   (WavSpec * k)(*specs), (C.c_void_p * k)(*d_rows),
                                                   (C.c_size_t * k)(*rows_cap), err, _ERRCAP), err)

    def process_device(self, d_rows: Sequence[int], rows_cap: Sequence[int], contrast_adjustment,
                       d_images: Sequence[int], rotate=Rotate.NO):
        """Contrast limits -> u8 image (and telemetry) of the recordings of the last
        decode_device call, chained on the device behind their decode."""
        k = len(d_rows)
        kind, p = Contrast._c(contrast_adjustment)
        err = C.create_string_buffer(_ERRCAP)
        _check(lib().aptgpu_plan_process_device(self._p, k, (C.c_void_p * k)(*d_rows),
                                                (C.c_size_t * k)(*rows_cap), kind, p, int(rotate),
                                                (C.c_void_p * k)(*d_images), err, _ERRCAP), err)

    def despeckle_device(self, d_rows: Sequence[int], rows_cap: Sequence[int], d_out: Sequence[int], settings=None):
        """The despeckle stage of the recordings of the last decode_device call, chained on the device behind their
        decode.  d_out[i] holds rows_cap[i] * 2080 floats and must not overlap d_rows; it can then be passed as d_rows
        to process_device / process_device_image.  Records through despeckle_results()."""
        k = len(d_rows)
        cs = _despeckle_c(settings)
        err = C.create_string_buffer(_ERRCAP)
        _check(lib().aptgpu_plan_despeckle_device(self._p, k, (C.c_void_p * k)(*d_rows), (C.c_size_t * k)(*rows_cap),
                                                  C.byref(cs) if cs is not None else None, (C.c_void_p * k)(*d_out),
                                                  err, _ERRCAP), err)

    def despeckle_results(self, count=1) -> List["DespeckleResult"]:
        arr = (DespeckleResult * count)()
        _check(lib().aptgpu_plan_despeckle_results(self._p, count, arr))
        return list(arr)

    def track_device(self, d_rows: Sequence[int], rows_cap: Sequence[int], settings=None):
        """The flywheel sync stage of the recordings of the last decode_device call, chained on the device behind their
        decode: re-aligns each from its slot's filtered signal into d_rows[i] (rows_cap[i] rows of 2080 floats).
        Records through track_results(), positions through track_positions()."""
        k = len(d_rows)
        cs = _track_c(settings)
        err = C.create_string_buffer(_ERRCAP)
        _check(lib().aptgpu_plan_track_device(self._p, k, C.byref(cs) if cs is not None else None,
                                              (C.c_void_p * k)(*d_rows), (C.c_size_t * k)(*rows_cap), err, _ERRCAP), err)

    def track_results(self, count=1) -> List["TrackResult"]:
        arr = (TrackResult * count)()
        for r in arr:
            r.struct_size = C.sizeof(TrackResult)
        _check(lib().aptgpu_plan_track_results(self._p, count, arr))
        return list(arr)

    def track_positions(self, i=0, cap=1 << 16):
        """(positions u64, scores f32) of recording i of the last track_device call"""
        pos, sc, n = np.zeros(cap, np.uint64), np.zeros(cap, np.float32), C.c_size_t(0)
        _check(lib().aptgpu_plan_track_positions(self._p, i, pos.ctypes.data_as(_u64p), sc.ctypes.data_as(_f32p), cap,
                                                 C.byref(n)))
        k = min(int(n.value), cap)
        return pos[:k].copy(), sc[:k].copy()

    def calibrate_thermal_device(self, d_rows: Sequence[int], rows_cap: Sequence[int], d_kelvin: Sequence[int],
                                 coeffs, settings, d_images: Optional[Sequence[int]] = None):
        """The thermal calibration of the recordings of the last decode_device call, chained on the device behind their
        decode.  d_kelvin[i] holds rows_cap[i] * 909 floats, d_images[i] (with settings.image_channels) rows_cap[i] *
        2080 * image_channels bytes; neither may overlap d_rows.  Records through thermal_results()."""
        k = len(d_rows)
        cc, cs, keep = _thermal_c(coeffs, settings)
        err = C.create_string_buffer(_ERRCAP)
        _check(lib().aptgpu_plan_calibrate_thermal_device(
            self._p, k, (C.c_void_p * k)(*d_rows), (C.c_size_t * k)(*rows_cap), C.byref(cc), C.byref(cs),
            (C.c_void_p * k)(*d_kelvin), (C.c_void_p * k)(*d_images) if d_images is not None else None, err, _ERRCAP),
            err)
        del keep

    def geolocate_device(self, d_rows: Sequence[int], rows_cap: Sequence[int], tracks_or_orbits, settings=None,
                         map_settings=None, d_latlon: Optional[Sequence[int]] = None,
                         d_cos: Optional[Sequence[int]] = None, d_out: Optional[Sequence[int]] = None):
        """The geolocation stage of the recordings of the last decode_device call, chained on the device behind their
        decode.  tracks_or_orbits: per recording a (rows, 2) track in radians, or per recording an OrbitSettings.
        d_latlon[i] holds rows_cap[i] * 909 * 2 doubles (16-byte aligned), d_cos[i] rows_cap[i] * 909 floats, d_out[i]
        rows_cap[i] * 2080 floats (d_out[i] == d_rows[i]: in place); what is None is not computed.  Records through
        geoloc_results()."""
        k = len(d_rows)
        if len(tracks_or_orbits) != k:
            raise InvalidError("geoloc: one track or orbit per recording")
        orbits = [isinstance(t, OrbitSettings) for t in tracks_or_orbits]
        if any(orbits) and not all(orbits):
            raise InvalidError("geoloc: tracks or orbits, not both")
        _, _, _, cms, cs, keep = _geoloc_c(None, map_settings, settings)
        pos = cnt = orb = None
        if k and all(orbits):
            orb, cos_ = _orbit_pointers(tracks_or_orbits)
            keep = (keep, cos_)
        else:
            tr, pos, cnt = _track_arrays(tracks_or_orbits)
            keep = (keep, tr)

        def arr(v):
            return (C.c_void_p * k)(*v) if v is not None else None
        err = C.create_string_buffer(_ERRCAP)
        _check(lib().aptgpu_plan_geolocate_device(self._p, k, (C.c_void_p * k)(*d_rows), (C.c_size_t * k)(*rows_cap),
                                                  pos, cnt, orb, cms, C.byref(cs), arr(d_latlon), arr(d_cos), arr(d_out),
                                                  err, _ERRCAP), err)
        del keep

    def geoloc_results(self, count=1) -> List["GeolocResult"]:
        arr = (GeolocResult * count)()
        for r in arr:
            r.struct_size = C.sizeof(GeolocResult)
        _check(lib().aptgpu_plan_geoloc_results(self._p, count, arr))
        return list(arr)

    def land_mask_device(self, d_rows: Sequence[int], rows_cap: Sequence[int], tracks_or_orbits, layers,
                         d_mask: Sequence[int], settings=None, map_settings=None):
        """The land mask of the recordings of the last decode_device call, chained on the device behind their decode
        (the height comes from the decode record).  tracks_or_orbits as geolocate_device().  d_mask[i] holds
        rows_cap[i] * 909 bytes.  Records through land_mask_results()."""
        k = len(d_rows)
        if len(tracks_or_orbits) != k or len(d_mask) != k:
            raise InvalidError("land mask: one track or orbit and one mask per recording")
        orbits = [isinstance(t, OrbitSettings) for t in tracks_or_orbits]
        if any(orbits) and not all(orbits):
            raise InvalidError("land mask: tracks or orbits, not both")
        cs = _land_c(layers, settings)
        if map_settings is not None and not isinstance(map_settings, MapSettings):
            raise InvalidError("land mask: map_settings must be a MapSettings or None")
        cms = map_settings._c() if map_settings is not None else None
        pos = cnt = orb = None
        if k and all(orbits):
            orb, keep = _orbit_pointers(tracks_or_orbits)
        else:
            keep, pos, cnt = _track_arrays(tracks_or_orbits)
        err = C.create_string_buffer(_ERRCAP)
        _check(lib().aptgpu_plan_land_mask_device(self._p, k, (C.c_void_p * k)(*d_rows), (C.c_size_t * k)(*rows_cap),
                                                  pos, cnt, orb, C.byref(cms) if cms is not None else None, layers._p,
                                                  C.byref(cs), (C.c_void_p * k)(*d_mask), err, _ERRCAP), err)
        del keep

    def land_mask_results(self, count=1) -> List["LandMaskResult"]:
        arr = (LandMaskResult * count)()
        for r in arr:
            r.struct_size = C.sizeof(LandMaskResult)
        _check(lib().aptgpu_plan_land_mask_results(self._p, count, arr))
        return list(arr)

    def thermal_results(self, count=1) -> List["ThermalResult"]:
        arr = (ThermalResult * count)()
        _check(lib().aptgpu_plan_thermal_results(self._p, count, arr))
        return list(arr)

    def process_device_image(self, d_rows: Sequence[int], rows_cap: Sequence[int], contrast_adjustment,
                             d_images: Sequence[int], rotate=Rotate.NO, color=None, channels=None, map=None,  # noqa: A002
                             png=None, orbit=None, layers=None, projection=None):
        """process() with every contrast (HISTOGRAM and, without colour, HISTOGRAM_FLOAT too) and optional false
        colour (a ColorSettings) for the
        recordings of the last decode_device call, chained on the device behind their decode.  d_images[i]
        holds rows_cap[i] * 2080 * channels bytes; channels defaults to 4 (RGBA) with colour or map, 1 (gray)
        without.  map: a MapOverlay, or one per recording (all with the same settings and layers); a position count
        that differs from a recording's height is reported in image_results() (reason 7).
        png: (d_png, png_cap), device pointers and their capacities in bytes, one per recording: each image is then
        also encoded as a PNG file on its stream (png_bound(2080, rows_cap[i], channels) bytes always suffice); the
        lengths arrive through png_sizes().  A capacity below the file's length is reported in image_results()
        (reason PNG_REASON_CAPACITY, png_bytes = the length needed) and nothing is written.
        orbit (instead of map): an OrbitSettings, or one per recording; each recording's track is computed on its
        stream (RefTime.End from the height the device found) and Rotate.ORBIT is decided per recording.  draw_map
        must be set for all or none (`layers` required then); an SGP4 error in a row is reported in image_results()
        (reason SAT_REASON_SGP4) and that image comes back without the overlay.
        projection: (settings, d_out, out_cap): a ProjectionSettings, a device pointer and its capacity in bytes per
        recording.  Behind everything above, recording i's unrotated image is reprojected onto settings[i] into
        d_out[i] (width * height * 4 bytes of RGBA); `png` then holds the projected image's file.  The track is
        `map`'s (a MapOverlay: the map is drawn first), `orbit`'s, or map = a list of plain sat_positions arrays
        (no map).  A capacity that is too small is reported in image_results() (reason PROJECT_REASON_CAPACITY) and
        nothing is written; a position count that differs from the height as reason 7."""
        req = _ImageRequest(contrast_adjustment, rotate, color, channels)
        k = len(d_rows)
        grids, out = None, (None, None)
        if projection is not None:
            grids, d_out, out_cap = projection
            grids = [grids] * k if isinstance(grids, ProjectionSettings) else list(grids)
            if len(grids) != k or len(d_out) != k or len(out_cap) != k or \
                    not all(isinstance(g, ProjectionSettings) for g in grids):
                raise InvalidError("projection: (settings, d_out, out_cap) with one entry per recording")
            if (map is None) == (orbit is None):
                raise InvalidError("a projection needs the track: exactly one of map and orbit")
            out = (C.c_void_p * k)(*d_out), (C.c_size_t * k)(*[int(c) for c in out_cap])
        elif map is not None and orbit is not None:
            raise InvalidError("map and orbit exclude each other")
        if projection is None and orbit is None:
            self._png_arrays(png, k)  # (this form alone has always checked the pair before the map)
        req.resolve(k, map, orbit, layers, png is not None, grids)
        pngs = self._png_arrays(png, k)
        cmap, lay, cpng, images = _ref(req.cmap), req.layers_p, C.byref(req.cpng), (C.c_void_p * k)(*d_images)
        pos = req.positions, req.counts
        tail = {"_project": (cmap, lay, *pos, req.orbits, images, req.cgrids, *out, cpng, *pngs),
                "_orbit": (req.orbits, lay, images, cpng, *pngs), "_png": (cmap, lay, *pos, images, cpng, *pngs),
                "_map": (cmap, lay, *pos, images), "": (images,)}[req.entry]
        err = C.create_string_buffer(_ERRCAP)
        _check(getattr(lib(), "aptgpu_plan_process_device_image" + req.entry)(
            self._p, k, (C.c_void_p * k)(*d_rows), (C.c_size_t * k)(*rows_cap), *req.head, *tail, err, _ERRCAP), err)

    @staticmethod
    def _png_arrays(png, k):
        """process_device_image's png = (d_png, png_cap) as the two arrays; (None, None) without."""
        if png is None:
            return None, None
        d_png, png_cap = png
        if len(d_png) != k or len(png_cap) != k:
            raise InvalidError("png: (d_png, png_cap) with one entry per recording")
        return (C.c_void_p * k)(*d_png), (C.c_size_t * k)(*[int(c) for c in png_cap])

    def composite_device_images(self, d_images: Sequence[int], heights: Sequence[int], channels: Sequence[int],
                                projection, d_out: int, out_cap: int, tracks=None, orbit=None,
                                blend=Composite.NADIR, settings=None, d_coverage=None, png=None):
        """aptgpu_plan_composite_device_images: the composite (composite_images) of the images that
        process_device_image left on the device for the first len(d_images) recordings of the last decode_device
        call, chained on the device.  heights[i] is the row capacity of d_images[i] (the height itself is the
        recording's record's), channels[i] 1 or 4.  tracks: one (height, 2) array per pass, or orbit: an OrbitSettings
        or one per pass (exactly one of the two).  d_out holds out_cap bytes (width * height * 4 are needed), d_coverage
        (optional) width * height bytes, png = (d_png, png_cap) (optional) the PNG file of the grid.
        image_results(len(d_images) + 1) then returns the passes' records followed by the composite's: a pass that
        failed shows its own reason there and COMPOSITE_REASON_PASS on the composite's, and nothing is written."""
        if not isinstance(projection, ProjectionSettings):
            raise InvalidError("projection must be a ProjectionSettings")
        k = len(d_images)
        if len(heights) != k or len(channels) != k:
            raise InvalidError("composite: one height and one channel count per image")
        if (tracks is None) == (orbit is None):
            raise InvalidError("a composite needs the tracks: exactly one of tracks and orbit")
        pos = npos = ptrs = keep = None
        if orbit is not None:
            ptrs, keep = _orbit_pointers(_one_per(orbit, OrbitSettings, k, "orbit", "an OrbitSettings", "pass"))
        else:
            keep, pos, npos = _track_arrays(tracks)
            if len(keep) != k:
                raise InvalidError("tracks: one sat_positions array per pass")
        maps, keep_maps = _composite_maps(settings, projection, k)
        if settings is None and projection.geometry is None and orbit is not None:
            maps = None  # (each pass's geometry is then its orbit's draw_map, or 0, 1, 1)
        cpr, cps = projection._c(), _CPngSettings(C.sizeof(_CPngSettings), 0)
        cco = _CCompositeSettings(C.sizeof(_CCompositeSettings), int(blend), 0)
        d_png, png_cap = png if png is not None else (None, 0)
        err = C.create_string_buffer(_ERRCAP)
        _check(lib().aptgpu_plan_composite_device_images(
            self._p, k, (C.c_void_p * k)(*d_images), (C.c_uint32 * k)(*[int(h) for h in heights]),
            (C.c_int32 * k)(*[int(c) for c in channels]), pos, npos, ptrs, maps, C.byref(cpr), C.byref(cco),
            d_out, int(out_cap), d_coverage, C.byref(cps), d_png, int(png_cap), err, _ERRCAP), err)
        del keep, keep_maps

    def png_sizes(self, count=1) -> List[int]:
        """Lengths of the PNG files of the last process_device_image(..., png=...) call (waits for it).  Raises for a
        recording whose image stage or encoding failed; image_results() has the records."""
        out = []
        for i, r in enumerate(self.image_results(count)):
            if r.status != 0:
                raise InternalError(f"recording {i}: image stage failed (reason {r.reason}"
                                    + (f", the PNG needs {r.png_bytes} bytes)" if r.reason == PNG_REASON_CAPACITY else ")"))
            out.append(int(r.png_bytes))
        return out

    def image_results(self, count=1) -> List[ImageResult]:
        arr = (ImageResult * count)()
        _check(lib().aptgpu_plan_image_results(self._p, count, arr))
        return list(arr)

    def results(self, count=1) -> List[Result]:
        arr = (Result * count)()
        _check(lib().aptgpu_plan_results(self._p, count, arr))
        return list(arr)

    def sync_positions(self, i=0, cap=1 << 20):
        buf = (C.c_uint64 * cap)()
        n = C.c_size_t()
        _check(lib().aptgpu_plan_sync_positions(self._p, i, buf, cap, C.byref(n)))
        return np.array(buf[:min(cap, n.value)], dtype=np.uint64)

    def read_internal(self, name, dtype, count, i=0):
        """Download `count` elements of an internal HBM buffer (see aptgpu_plan_read_internal)."""
        out = np.zeros(int(count), dtype=dtype)
        size = C.c_size_t()
        _check(lib().aptgpu_plan_read_internal(self._p, i, name.encode(), out.ctypes.data_as(C.c_void_p),
                                               out.nbytes, C.byref(size)))
        return out

    def synchronize(self):
        _check(lib().aptgpu_plan_synchronize(self._p))

    def join(self):
        """Order the caller's stream (given at creation) after everything enqueued so far."""
        _check(lib().aptgpu_plan_join(self._p))

    def enable_timing(self, mode=2):
        """0/False off, 1 dominant kernel only, 2/True every kernel launch."""
        mode = 2 if mode is True else (0 if mode is False else int(mode))
        _check(lib().aptgpu_plan_enable_timing(self._p, mode))

    def collect_timing(self):
        arr = (KernelTime * 32)()
        n = C.c_size_t()
        _check(lib().aptgpu_plan_collect_timing(self._p, arr, 32, C.byref(n)))
        return {arr[i].name.decode(): (arr[i].avg_ms, int(arr[i].launches))
                for i in range(min(32, n.value))}
