// apt_capi_stream_parts.hpp — one push of an aptgpu_stream (apt_capi_stream.hip) whose samples arrive in pieces: what
// the live decode from IQ (apt_capi_fm_stream.hip) needs, since its audio scratch holds one piece at a time.
//   check   the refusals of a push of n samples in all (or, n == 0 and finish, of a finish)
//   begin   host-fed form: where the rows of the push go (a device handle: its staging, grown to the bound)
//   piece   the next samples; `first` opens the push (the record's row count restarts), `finish` closes the recording.
//           A device handle enqueues and returns; samples, rows and positions are device pointers.  A host handle takes
//           host pointers.
//   end     host-fed form: one record read back, the rows it counts copied out, its error raised
// aptgpu_stream_push is begin, one piece, end; aptgpu_stream_push_device is one piece.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/aptgpu.h"

namespace apt::capi::stream_parts {

struct Target {
    float *rows;
    uint64_t *positions;
    uint32_t cap;
};
bool is_host(const aptgpu_stream *s);
void check(const aptgpu_stream *s, size_t n, size_t rows_cap, const aptgpu_stream_result *result, bool want_result);
Target begin(aptgpu_stream *s, size_t n, float *rows, uint64_t *positions, size_t rows_cap);
void piece(aptgpu_stream *s, const void *samples, size_t n, bool first, bool finish, const Target &t);
void end(aptgpu_stream *s, const Target &t, float *rows, uint64_t *positions, aptgpu_stream_result *result);
// aptgpu_stream_create_tracked / _host (include/aptgpu.h §4e): the same handle with the tracker in the picker's place
int create_tracked(const aptgpu_context *ctx, const aptgpu_settings *settings, const aptgpu_stream_settings *ss,
                   const aptgpu_live_track_settings *track, bool host, aptgpu_stream **out, char *err, size_t err_cap);

}  // namespace apt::capi::stream_parts
