// rc2dgi_write.h -- an image into a rectangle of an input texture (rc2dgi_write / rc2dgi_write_device,
// include/rc2dgi.h): pitched rows of RGBA32F, RGBA16F (widened exactly) or RGBA8 pixels become the float4 texels
// rc2dgi_upload would store, replacing the texels or blended over them.  See rc2dgi_write.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "rc2dgi_read.h"

namespace rc2dgi {

constexpr int kWriteRows = 4;  // rows a lane writes a texel of: 64 bytes of RGBA32F loaded, 64 bytes stored

// One launch: image rows [0, rows) of a rectangle w texels wide whose first column is x.  Image row j comes from
// src + j * pitch and goes to texel row y0 + ystep * j (ystep -1 from the rectangle's top row: RC2DGI_WRITE_FLIP).
struct WriteArgs {
  float4 *dst;  // the input texture (COLOR's input or EMISSIVE): float4 texels in every storage mode
  int dpitch;   // its pitch in texels
  int x, w;
  int y0, ystep;
  int rows;
  const unsigned char *src;  // aligned to a pixel
  size_t pitch;              // bytes, a multiple of a pixel, at least w pixels
};

// Enqueues the launch on `st` (rows >= 1, w >= 1; the rectangle lies inside the texture).  u8: the context stores
// RGBA8_COMPAT (texels are quantized, the blend is the 8-bit one); blend: RC2DGI_WRITE_BLEND.
hipError_t launch_write(const WriteArgs &a, int format, bool u8, bool blend, hipStream_t st);

}  // namespace rc2dgi
