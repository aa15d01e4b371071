// rc2dgi_read.h -- a rectangle of a render texture as an image (rc2dgi_read / rc2dgi_read_device, include/rc2dgi.h):
// the texels through the decoder of the views (rc2dgi_texel.h), converted to RGBA32F, RGBA16F (round to nearest even)
// or RGBA8 (q8), into pitched rows.  See rc2dgi_read.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "rc2dgi_present.h"

namespace rc2dgi {

// The device memory rc2dgi_read stages an image in, at most: a larger rectangle goes through it in blocks of whole
// rows (one row where a row is longer).  Allocated at the first call, kept to the end.
constexpr size_t kReadChunkBytes = (size_t)8 << 20;

constexpr int kReadTexels = 4;  // texels a lane converts: 64 bytes of RGBA32F, 32 of RGBA16F, 16 of RGBA8

// bytes of a pixel of an rc2dgi_format (the three rc2dgi_read takes)
constexpr int read_pixel_bytes(int format) {
  return format == RC2DGI_FMT_RGBA32F ? 16 : (format == RC2DGI_FMT_RGBA16F ? 8 : 4);
}

// One launch: image rows [0, rows) of a rectangle w texels wide whose first column is x.  Image row j is texel row
// y0 + ystep * j (ystep -1 from the rectangle's top row: RC2DGI_READ_FLIP) and goes to dst + j * pitch.
struct ReadArgs {
  int x, w;
  int y0, ystep;
  int rows;
  unsigned char *dst;  // aligned to a pixel
  size_t pitch;        // bytes, a multiple of a pixel, at least w pixels
};

// Enqueues the launch on `st` (rows >= 1, w >= 1; the rectangle lies inside the texture).
hipError_t launch_read(const TexSource &t, const ReadArgs &a, int format, hipStream_t st);

}  // namespace rc2dgi
