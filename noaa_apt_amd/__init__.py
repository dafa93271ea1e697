"""noaa_apt_amd — MI355X (gfx950) implementation of noaa-apt's decode() hot path.

This package is a thin ctypes mirror of the reference's Rust interface for the path
(`noaa_apt::decode` and the dsp/filters functions under it) on top of the C ABI in
include/aptgpu.h (libaptgpu.so: hand-written HIP kernels + host-side FIR design).
Names, argument meaning and error behaviour follow the reference:

    decode(context, settings, signal, input_rate, sync)   /root/reference/src/decode.rs:43-49
    Context.status / Context.step                          /root/reference/src/context.rs:127-211
    Settings (the 5 fields decode() reads)                 /root/reference/src/config.rs:76-106
    Rate, Freq                                             /root/reference/src/frequency.rs:30-117
    Lowpass, LowpassDcRemoval, NoFilter                    /root/reference/src/filters.rs:22-138
    resample_with_filter, resample, demodulate, filter     /root/reference/src/dsp.rs:62,132,350,386
    find_sync, generate_sync_frame                         /root/reference/src/decode.rs:171,204
    load (WAV ingest), decode_wav                          /root/reference/src/noaa_apt.rs:114-130, wav.rs:11-57
    resample_wav (WAV->WAV tool), write_wav                /root/reference/src/resample.rs:17-71, wav.rs:59-98
    process (grayscale part), Contrast, Rotate             /root/reference/src/noaa_apt.rs:25-60,132-235
    process: Contrast.HISTOGRAM, ColorSettings (false      the reference's processing.rs:83-165, imageext.rs:21-45,
    colour)                                                noaa_apt.rs:63-71
    ColorSettings(equalize_lab=True), lab_from_rgb,        imageext.rs:50-143, the lab crate 0.11.0
    lab_to_rgb (Histogram + colour in CIE Lab)
    process(orbit=MapOverlay(...)): the map overlay,       map.rs:14-200 (from a track the caller passes),
    MapSettings, MapLayers, read_shapefile                 noaa_apt.rs:84-91
    process(orbit=OrbitSettings(...)), Rotate.ORBIT,       noaa_apt.rs:58-108, map.rs:28-58, processing.rs:40-81
    SatName, RefTime, sat_track, sat_track_host,           (SGP4 on the GPU, one thread per image row)
    south_to_north_pass
    process(png=True), encode_png, png_bound: the PNG      main.rs, the Decode arm: img.save(&output_filename)
    file of the image, encoded on the GPU
    process(projection=ProjectionSettings(...)),           the reference's to-do list, docs/development.md:112,99:
    project_image, projection_fit, Projection              the image on an equirectangular or Mercator grid
    composite_images, Composite,                           what every APT user does next with reprojected passes:
    Plan.composite_device_images                           several of them on one map grid
    despeckle, despeckle_host, DespeckleSettings,          the reference's to-do list, docs/development.md:139: a
    process(despeckle=...), Plan.despeckle_device          band-aware median of the f32 rows in front of process()
    calibrate_thermal, calibrate_thermal_host,             brightness temperature of an infrared channel from the
    ThermalCoefficients, ThermalSettings,                  telemetry frame (NOAA KLM User's Guide §7.1.2.4), DESIGN.md §19
    Plan.calibrate_thermal_device
    geolocate, geolocate_host, sun_position,               where on the Earth a swath pixel lies (the overlay's projection
    normalize_sun, GeolocSettings, Plan.geolocate_device   inverted), the sun's zenith angle there and the visible rows
                                                           normalised by it (the reference only advises daylight passes,
                                                           docs/usage.md:409-417), DESIGN.md §25
    fit_overlay, fit_overlay_host, fit_overlay_device,     the reference's to-do list, docs/development.md:90: yaw, scales
    fit_sample_points, margin_track, FitSettings,          and the time offset fitted to the image's edges, DESIGN.md §26
    OverlayFit
    land_mask, land_mask_plane (each with a _host form),   what every APT user knows from WXtoImg's map-coloured
    false_color_masked, LandMaskSettings,                  enhancements: land, sea or lake per swath pixel from the layer
    Plan.land_mask_device                                  set's polygons, and a palette per class, DESIGN.md §28
    fm_demodulate, fm_demodulate_host, fm_demodulate_wav,  FM demodulation of an IQ recording in front of decode()
    fm_design, load_iq, IqFormat, FmSettings,              (the reference takes audio only, docs/usage.md:87),
    FmDemodulator                                          DESIGN.md §20
    fm_demodulate_afc, fm_afc_sums, fm_afc_estimate,       AFC in front of it: the carrier followed block by block, the
    fm_demodulate_tracked (each with a _host form),        NCO reading a table (the reference has no IQ input at all),
    fm_afc_design, AfcSettings, AfcTable, FmAfc            DESIGN.md §27
    track_sync, track_sync_host, sync_score,               the reference's to-do list, docs/development.md:148: row
    decode_tracked, TrackSettings, Plan.track_device       starts tracked through noise and dropouts, DESIGN.md §21
    LiveTrackSettings, LiveDecoder(track=...),             live decode with the flywheel tracker's row starts, from audio
    LiveIqDecoder(track=...)                               and from IQ frames, DESIGN.md §24
    LiveDecoder, decode_live                               the reference's to-do list, docs/development.md:151: audio
                                                           pushed in chunks, finished rows handed back, DESIGN.md §22
    FmStream, LiveIqDecoder, decode_live_iq                the same from IQ frames: the FM demodulator in streaming form
                                                           and its coupling to the live decode, DESIGN.md §23
    percent, get_min, get_max, map_signal_u8               /root/reference/src/misc.rs:119, dsp.rs:20-54
    read_telemetry, Telemetry                              /root/reference/src/telemetry.rs:19-243

There is no CPU fallback: if libaptgpu.so is missing or no GPU is present the calls
raise.  (The CPU oracle lives in oracle/ and is test infrastructure only.)
"""
from .api import (  # noqa: F401
    FINAL_RATE, PX_PER_ROW, CARRIER_FREQ,
    AptError, InternalError, RateOverflowError, HipError, InvalidError, UnsupportedError,
    InvalidInputError, WavOpenError, IoError, WavSpec, wav_parse, load, decode_wav, write_wav, resample_wav,
    Rate, Freq, Settings, Context, Stats,
    NoFilter, Lowpass, LowpassDcRemoval,
    decode, resample_with_filter, resample, demodulate, filter, find_sync, generate_sync_frame,
    Contrast, Rotate, ColorSettings, Telemetry, ImageResult, MapSettings, MapLayers, MapOverlay, read_shapefile,
    MAP_STATES, MAP_COUNTRIES, MAP_LAKES,
    get_min, get_max, percent, map_signal_u8, read_telemetry, process, lab_from_rgb, lab_to_rgb,
    encode_png, png_bound, PNG_REASON_CAPACITY,
    DespeckleSettings, DespeckleResult, despeckle, despeckle_host,
    ThermalCoefficients, ThermalSettings, ThermalResult, calibrate_thermal, calibrate_thermal_host,
    THERMAL_COLD_WHITE, THERMAL_REASON_CHANNEL, THERMAL_REASON_DEGENERATE, THERMAL_PX,
    GeolocSettings, GeolocResult, geolocate, geolocate_host, sun_position, normalize_sun,
    GEOLOC_PX, GEOLOC_REASON_HEIGHT, GEOLOC_REASON_DECODE,
    FitSettings, FitResult, FitRound, OverlayFit, fit_overlay, fit_overlay_host, fit_overlay_device, fit_sample_points,
    margin_track, FIT_REASON_NO_CANDIDATE, FIT_REASON_FLAT, FIT_SCORE_DTYPE,
    LandMaskSettings, LandMaskResult, land_mask, land_mask_host, land_mask_plane, land_mask_plane_host,
    false_color_masked, false_color_masked_host, LAND_SEA, LAND_LAND, LAND_LAKE, LAND_INVALID,
    IqFormat, FmSettings, FmInfo, FmDemodulator, fm_demodulate, fm_demodulate_host, fm_demodulate_wav, fm_design, load_iq,
    FM_SWAP_IQ, FM_MAX_BATCH,
    AfcSettings, AfcInfo, AfcTable, FmAfc, AFC_RECORD_DTYPE, fm_afc_design, fm_afc_sums, fm_afc_sums_host,
    fm_afc_estimate, fm_afc_estimate_host, fm_demodulate_tracked, fm_demodulate_tracked_host, fm_demodulate_afc,
    fm_demodulate_afc_host,
    TrackSettings, TrackResult, track_sync, track_sync_host, sync_score, decode_tracked, TRACK_MAX_JITTER,
    LiveDecoder, decode_live, StreamInfo, StreamResult, LiveTrackSettings, StreamTrackResult,
    FmStream, FmStreamInfo, LiveIqDecoder, decode_live_iq, FM_STREAM_MAX_PUSH_FRAMES,
    Projection, ProjectionSettings, projection_fit, project_image, PROJECT_REASON_CAPACITY,
    Composite, composite_images, COMPOSITE_REASON_PASS, COMPOSITE_MAX_PASSES,
    SatName, RefTime, OrbitSettings, sat_track, sat_track_host, south_to_north_pass, SAT_REASON_SGP4,
    Plan, PlanInfo, Result, KernelTime, decode_batch, BatchStats, host_alloc_f32, host_free,
    lib, lib_path, use_library, build, device_count, version, abi_version, cache_clear, cache_info, host_affinity, host_affinity_from_sysfs,
    MODE_STRICT, MODE_GENERIC, MODE_FP16_TAPS, MODE_FAST,
)
