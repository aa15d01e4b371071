// rc2dgi_texel.h -- the one device-side decoder of the render textures' stored formats: a texel of a TexSource
// (rc2dgi_present.h) as the value rc2dgi_download returns for it, and texture(T, (u, v)) with the POINT / LINEAR +
// REPEAT semantics of rc2dgi_device.h.  k_present (rc2dgi_present.hip) fetches a view's texels through it and
// k_sample (rc2dgi_query.hip) a caller's points, so a point sample equals what a compose view fetches at that
// texcoord.
#pragma once

#include "rc2dgi_device.h"
#include "rc2dgi_present.h"

namespace rc2dgi {

// the value of texel (i, j), 0 <= i < nx, 0 <= j < ny, as rc2dgi_download returns it
__device__ __forceinline__ float4 present_texel(const TexSource &v, int i, int j) {
  const size_t o = (size_t)j * v.pitch + i;
  switch (v.kind) {
    case PK_F32: return static_cast<const float4 *>(v.src)[o];
    case PK_F16: return GiF16::ld(static_cast<const uint2 *>(v.src) + o);
    case PK_U8: return GiU8::ld(static_cast<const unsigned *>(v.src) + o);
    case PK_JUMP: {
      const unsigned s = static_cast<const unsigned *>(v.src)[o];
      if (s == 0x80008000u) return make_float4(0.0f, 0.0f, 0.0f, 1.0f);
      return make_float4(((float)(int)(s & 0xFFFFu) + 0.5f) / (float)v.nx, ((float)(int)(s >> 16) + 0.5f) / (float)v.ny,
                         0.0f, 1.0f);
    }
    case PK_JUMP8: {
      const unsigned s = static_cast<const unsigned *>(v.src)[o];
      return make_float4((float)(s & 0xFFFFu) * kInv255, (float)(s >> 16) * kInv255, 0.0f, 1.0f);
    }
    case PK_DIST:
    case PK_DIST8: {
      const unsigned d = static_cast<const unsigned short *>(v.src)[o];
      const float hi = (float)((d >> 8) & 255u), lo = (float)(d & 255u);
      return v.kind == PK_DIST8 ? make_float4(hi * kInv255, lo * kInv255, 0.0f, 1.0f)
                                : make_float4(hi / 255.0f, lo / 255.0f, 0.0f, 1.0f);
    }
    default: return make_float4(0.0f, 0.0f, 0.0f, 1.0f);
  }
}

// texture(T, (u, v)): POINT, or LINEAR with the bilerp of the texture's storage.  Every index below is masked or
// clamped into the texture (wrap_nearest / wrap_linear), whatever finite value u and v hold.
__device__ __forceinline__ float4 present_sample(const TexSource &v, float tu, float tv) {
  const Axis ax{v.nx, v.powx}, ay{v.ny, v.powy};
  if (!v.linear || v.kind == PK_CONST) return present_texel(v, wrap_nearest(tu, ax), wrap_nearest(tv, ay));
  int x0, x1, y0, y1;
  float wx, wy;
  wrap_linear(tu, ax, x0, x1, wx);
  wrap_linear(tv, ay, y0, y1, wy);
  const size_t r0 = (size_t)y0 * v.pitch, r1 = (size_t)y1 * v.pitch;
  if (v.kind == PK_U8) {
    const unsigned *T = static_cast<const unsigned *>(v.src);
    return GiU8::bilerp(T[r0 + x0], T[r0 + x1], T[r1 + x0], T[r1 + x1], wx, wy);
  }
  if (v.kind == PK_F16) {
    const uint2 *T = static_cast<const uint2 *>(v.src);
    return GiF32::bilerp(GiF16::ld(T + r0 + x0), GiF16::ld(T + r0 + x1), GiF16::ld(T + r1 + x0), GiF16::ld(T + r1 + x1),
                         wx, wy);
  }
  const float4 *T = static_cast<const float4 *>(v.src);  // PK_F32 (the host admits LINEAR on no other kind)
  return GiF32::bilerp(T[r0 + x0], T[r0 + x1], T[r1 + x0], T[r1 + x1], wx, wy);
}

}  // namespace rc2dgi
