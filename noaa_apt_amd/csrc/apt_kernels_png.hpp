// apt_kernels_png.hpp — the gfx950 PNG encoder (apt_kernels_png.hip): process()'s u8 image to the bytes of
// `img.save()` (main.rs, the Decode arm) without a host round trip.  DESIGN.md §13.
//
// The file is signature, IHDR, one IDAT, IEND; 8 bits per sample, colour type 0 (channels 1) or 6 (channels 4).  The
// zlib stream inside IDAT is cut into chunks of kChunk bytes of the filtered scanlines.  Every chunk becomes deflate
// blocks of its own that end on a byte boundary (an empty stored block, as pigz), so the bytes are a function of the
// pixels alone: not of the batch, the slot, the stream or the run.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "apt_kernels.hpp"

namespace apt {
void hip_check(hipError_t e, const char *what);
}

namespace apt::png {

constexpr uint32_t kChunk = 16384;            // filtered bytes per chunk; matches never leave their chunk
constexpr uint32_t kChunkOutMax = kChunk + 5; // a chunk's deflate bytes never exceed its stored form
constexpr uint32_t kStageStride = kChunk + 8; // bytes of one chunk's staging area (4-byte aligned)
constexpr int kReasonCapacity = 9;            // aptgpu_image_result.reason: d_png too small (APTGPU_PNG_REASON_CAPACITY)
constexpr uint64_t kMaxStream = 1ull << 31;   // filtered bytes one image may have

// bytes of the filtered scanlines: a filter byte in front of every row
inline uint64_t stream_bytes(uint64_t width, uint64_t height, int channels)
{
    return height * (width * static_cast<uint64_t>(channels) + 1u);
}
inline uint64_t chunks_of(uint64_t stream) { return (stream + kChunk - 1) / kChunk; }
// The largest file encode() can emit for such an image: every chunk stored (5 bytes of block header each), the
// signature (8), IHDR (25), IDAT's length / type / CRC (12), the zlib header (2) and Adler-32 (4), IEND (12).
inline uint64_t bound(uint64_t width, uint64_t height, int channels)
{
    const uint64_t s = stream_bytes(width, height, channels);
    return 8 + 25 + 12 + 2 + s + 5 * chunks_of(s) + 4 + 12;
}

// Per-chunk record the deflate kernel leaves for the placement.
struct ChunkRec {
    uint32_t bytes;    // deflate bytes of the chunk in its staging area
    uint32_t adler_a;  // sum of the chunk's filtered bytes mod 65521
    uint32_t adler_b;  // sum of (bytes after it in the chunk + 1) * byte mod 65521
    uint32_t offset;   // byte offset of the chunk inside the zlib stream's deflate data (the scan)
};

// Scratch of one encode target (a one-shot call or a plan slot), sized for `stream_cap` filtered bytes.
size_t ws_bytes(uint64_t stream_cap);

// Encodes img (height rows of width px, `channels` bytes each) into d_png (png_cap bytes).  With `info` the height is
// info->height as the image stage left it on the device (`height` is then the capacity the launch grids cover) and
// nothing is encoded when info->status is set; the file's length lands in info->reserved (aptgpu_image_result:
// png_bytes).  Without `info` (a plain image) the length lands in *d_len.  A file longer than png_cap is not written
// at all: with `info`, status = 1 and reason = kReasonCapacity with the needed length in png_bytes; without, *d_len
// holds the needed length (> png_cap).  Enqueues on s, never synchronises.
void encode(hipStream_t s, const uint8_t *img, uint32_t width, uint32_t height, int channels, void *ws,
            uint64_t stream_cap, uint8_t *d_png, uint64_t png_cap, apt::gpu::ImageResult *info, uint64_t *d_len);
// The same in its three stages (a plan times them apart): scanline filter; per-chunk deflate; layout, placement and
// checksums.
void encode_filter(hipStream_t s, const uint8_t *img, uint32_t width, uint32_t height, int channels, void *ws,
                   uint64_t stream_cap, const apt::gpu::ImageResult *info);
void encode_deflate(hipStream_t s, uint32_t width, uint32_t height, int channels, void *ws, uint64_t stream_cap,
                    const apt::gpu::ImageResult *info);
void encode_place(hipStream_t s, uint32_t width, uint32_t height, int channels, void *ws, uint64_t stream_cap,
                  uint8_t *d_png, uint64_t png_cap, apt::gpu::ImageResult *info, uint64_t *d_len);

}  // namespace apt::png
