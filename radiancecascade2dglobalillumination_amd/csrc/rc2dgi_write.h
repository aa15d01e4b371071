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

#ifdef __HIP__  // device units only (rc2dgi_write.hip, rc2dgi_sprites.hip): the one definition of a pixel's value
#include "rc2dgi_device.h"

namespace rc2dgi {

template <int FMT> struct WritePixel;
template <> struct WritePixel<RC2DGI_FMT_RGBA32F> { typedef uint4 T; };
template <> struct WritePixel<RC2DGI_FMT_RGBA16F> { typedef uint2 T; };
template <> struct WritePixel<RC2DGI_FMT_RGBA8> { typedef unsigned T; };

// the value a pixel becomes in a texture whose storage is RGBA8_COMPAT (U8) or float (include/rc2dgi.h)
template <bool U8, int FMT>
__device__ __forceinline__ float4 write_value(typename WritePixel<FMT>::T p) {
  if constexpr (FMT == RC2DGI_FMT_RGBA8) {
    const float r = (float)(p & 255u), g = (float)((p >> 8) & 255u), b = (float)((p >> 16) & 255u), a = (float)(p >> 24);
    return U8 ? make_float4(r * kInv255, g * kInv255, b * kInv255, a * kInv255)
              : make_float4(r / 255.0f, g / 255.0f, b / 255.0f, a / 255.0f);
  } else {
    float4 v;
    if constexpr (FMT == RC2DGI_FMT_RGBA16F) v = GiF16::unpack(p);
    else v = make_float4(__uint_as_float(p.x), __uint_as_float(p.y), __uint_as_float(p.z), __uint_as_float(p.w));
    return U8 ? GiU8::unpack(GiU8::pack(v)) : v;
  }
}

}  // namespace rc2dgi
#endif
