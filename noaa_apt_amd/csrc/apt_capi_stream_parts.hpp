// apt_capi_stream_parts.hpp — one push of an aptgpu_stream (apt_capi_stream.hip) whose samples arrive in pieces: what
// the live decode from IQ (apt_capi_fm_stream.hip) needs, since its audio scratch holds one piece at a time.
//   create  any of the four decoders: picker or tracker (track: NULL = the defaults), device form or host twin
//   check   the refusals of a push of n samples in all (or, n == 0 and finish, of a finish)
//   begin   host-fed form: where the rows of the push go (a device handle: its staging, grown to the bound)
//   device_target  device-resident form: the caller's buffers (and, on a tracked stream, where its lock indicators go)
//   piece   the next samples; `first` opens the push (the record's row count restarts), `finish` closes the recording.
//           A device handle enqueues and returns; samples, rows and positions are device pointers.  A host handle takes
//           host pointers.
//   end     host-fed form: one record read back, the rows it counts copied out, its error raised
// aptgpu_stream_push is begin, one piece, end; aptgpu_stream_push_device is device_target and one piece.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/aptgpu.h"

namespace apt::capi::stream_parts {

struct Target {
    float *rows;
    uint64_t *positions;
    float *scores;  // a tracked stream's lock indicators, beside the rows (the picker: null)
    uint32_t cap;
};
int create(const aptgpu_context *ctx, const aptgpu_settings *settings, const aptgpu_stream_settings *ss, bool tracked,
           const aptgpu_live_track_settings *track, bool host, aptgpu_stream **out, char *err, size_t err_cap);
void check(const aptgpu_stream *s, size_t n, size_t rows_cap, const aptgpu_stream_result *result, bool want_result);
Target begin(aptgpu_stream *s, size_t n, float *rows, uint64_t *positions, size_t rows_cap);
Target device_target(aptgpu_stream *s, float *d_rows, uint64_t *d_positions, size_t rows_cap);
void piece(aptgpu_stream *s, const void *samples, size_t n, bool first, bool finish, const Target &t);
void end(aptgpu_stream *s, const Target &t, float *rows, uint64_t *positions, aptgpu_stream_result *result);

}  // namespace apt::capi::stream_parts
