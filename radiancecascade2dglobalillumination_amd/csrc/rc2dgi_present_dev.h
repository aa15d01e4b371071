// rc2dgi_present_dev.h -- the device helpers the two display kernels share: k_present (rc2dgi_present.hip) and
// k_present_tone (rc2dgi_tone.hip).  The 8-bit blend of a draw and the wave-uniform test for the plain blit.
#pragma once

#include "rc2dgi_device.h"
#include "rc2dgi_present.h"

namespace rc2dgi {

// one 8-bit draw: src over dst, both r | g << 8 | b << 16 | a << 24
__device__ __forceinline__ unsigned blend8(unsigned s, unsigned d) {
  const unsigned a8 = s >> 24, ia8 = 255u - a8;
  unsigned o = 0;
#pragma unroll
  for (int k = 0; k < 32; k += 8) {
    const unsigned v = mul8((s >> k) & 255u, a8) + mul8((d >> k) & 255u, ia8);
    o |= (v < 255u ? v : 255u) << k;
  }
  return o;
}

// The plain-blit test for pixels [x0, x1) of row py: exactly one view's clipped rectangle meets them, and they lie
// inside that view's blit rectangle.  Returns the view's source in `f` (k is uniform, so the view fields are scalar
// loads; x0 / x1 may be per lane).
struct PresentBlit {
  const void *src;
  int pitch, u8, x, y, h;
  int k;  // the view's index (its tone, rc2dgi_tone.hip)
};
__device__ __forceinline__ bool present_blit(const PresentArgs &a, int x0, int x1, int py, PresentBlit &f) {
  int hits = 0;
  bool inside = false;
  for (int k = 0; k < a.n; ++k) {
    const PresentView &v = a.v[k];
    if (py < v.cy0 || py >= v.cy1 || x1 <= v.cx0 || x0 >= v.cx1) continue;
    ++hits;
    inside = py >= v.fy0 && py < v.fy1 && x0 >= v.fx0 && x1 <= v.fx1;
    f.src = v.src;
    f.pitch = v.pitch;
    f.u8 = v.kind == PK_U8;
    f.x = v.x;
    f.y = v.y;
    f.h = v.h;
    f.k = k;
  }
  return hits == 1 && inside;
}

}  // namespace rc2dgi
