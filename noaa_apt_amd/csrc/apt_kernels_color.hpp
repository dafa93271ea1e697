// apt_kernels_color.hpp — histogram equalisation and palette false colour of process()'s image
// (apt_kernels_color.hip): the layer of noaa_apt::process between map_signal_u8 and the rotation
// (src/noaa_apt.rs:166-231, processing.rs:83-165, imageext.rs:21-45,121-145).
//
// They run behind the contrast-limit kernels of apt_kernels_image.hip (image_minmax / image_percent /
// image_telemetry), read the limits from that stage's workspace and, like those kernels, take the
// pixel count from the decode result record on the device when one is given.
#pragma once

#include "apt_color_tune.hpp"  // ColorTune, tune()
#include "apt_kernels.hpp"
#include "apt_lab.hpp"

namespace apt::gpu {

// Scratch of the colour stage: two 256-bin histograms (channel A, channel B), two 256-entry u8
// equalisation tables, the palette as 65536 packed RGBA words (A = 255).  color_ws_init zeroes the
// histograms once; the table kernel zeroes them again after reading them, so a workspace is ready
// for its next call without a memset per call.
size_t color_ws_bytes();
hipError_t color_ws_init(hipStream_t s, void *color_ws);
// 256*256*3 RGB bytes, pixel (a, b) at (b*256 + a)*3  ->  the packed form color_ws holds (host side)
void color_pack_palette(const uint8_t *rgb, uint32_t *packed);
uint32_t *color_ws_palette(void *color_ws);

// imageext::equalize_histogram_grayscale of both channel halves (columns 0..1040 and 1040..2080,
// whole rows only) of the u8 image map_signal_u8 makes from the limits in image_ws: histogram, then
// the two tables.  cap: as for image_map_u8.
void image_equalize(hipStream_t s, const float *x, const Result *res, uint64_t n, uint64_t cap,
                    void *image_ws, void *color_ws);

// Scratch of the Lab path (equalisation of a false-colour image), allocated only when that path runs:
// the host's lab::Tables of the palette at offset 0 (the caller uploads them), then the 101 equalised
// L values and the RGBA of every table index, both rewritten by each call.
size_t lab_ws_bytes();

// Histogram + false colour (processing.rs:87-101 with has_color): channel A (the false-colour image
// incl. its gray columns) equalised in CIE Lab, channel B as image_equalize.  Leaves the RGBA of every
// Lab table index in lab_ws and channel B's table in color_ws for image_color.  tune: as image_color's.
void image_equalize_lab(hipStream_t s, const float *x, const Result *res, uint64_t n, uint64_t cap,
                        void *image_ws, void *color_ws, void *lab_ws, const ColorTune &tune);

// The output pass: map_signal_u8, then the equalisation tables (equalize) or the palette over
// channel A's image columns (tune != nullptr), then the optional 180-degree rotation, written as
// `channels` bytes per pixel (1 = gray, 4 = RGBA, A = 255) for the height = n / 2080 whole rows.
// lab_ws (after image_equalize_lab, with tune, equalize and channels 4): channel A comes from its RGBA
// table instead.  Fills info's limits, height and n_px (= height * 2080) like image_map_u8.  out:
// 4-byte aligned for channels 1, 16-byte aligned for channels 4.
void image_color(hipStream_t s, const float *x, const Result *res, uint64_t n, uint64_t cap,
                 void *image_ws, const void *color_ws, bool equalize, const ColorTune *tune, int channels,
                 bool rotate, uint8_t *out, ImageResult *info, const void *lab_ws = nullptr);

}  // namespace apt::gpu
