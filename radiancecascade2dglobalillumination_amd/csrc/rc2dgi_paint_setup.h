// rc2dgi_paint_setup.h -- the device-side primitive set-up the two list painters share (rc2dgi_paint_dev.hip,
// rc2dgi_shapes.hip): to_window and the 1/256-pixel snap, paint_prims' per-triangle loop (zero-area drop, CCW swap, the
// integer edge equations and the incl rule) and the pixel box of what was emitted, clipped to the target.  Every float
// operation is one IEEE single operation (__fmul_rn / __fadd_rn: nothing contracts).  Device units only.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>

#include "rc2dgi_gradient_interp.h"
#include "rc2dgi_paint_raster.h"

namespace rc2dgi {

constexpr int kPaintDevHead = 256;        // bytes of counters ahead of the records: word 0 counts refused primitives
constexpr int kPaintDevTris = 36;         // triangle slots a primitive (a circle's 18 quads)

struct PaintCircle {
  float c[37], s[37];
};

struct PaintXform {  // to_window's constants, computed on the host as to_window computes them
  float sx, sy, hw, hh;
  int W, H;
};

struct PaintSnap {
  long long x, y;
};

__device__ __forceinline__ PaintSnap paint_dev_window(float vx, float vy, const PaintXform &t) {
  const float xn = __fadd_rn(__fmul_rn(vx, t.sx), -1.0f);
  const float yn = __fadd_rn(__fmul_rn(vy, t.sy), 1.0f);
  const float xw = __fadd_rn(__fmul_rn(xn, t.hw), t.hw), yw = __fadd_rn(__fmul_rn(yn, t.hh), t.hh);
  return PaintSnap{(long long)rint((double)xw * 256.0), (long long)rint((double)yw * 256.0)};
}

__device__ __forceinline__ long long paint_dev_floor_div(long long a, long long b) {
  return a >= 0 ? a / b : -((-a + b - 1) / b);
}

struct PaintAcc {
  PaintTri *out;
  int nt;
  long long mnx, mny, mxx, mxy;
};

// one triangle of paint_prims' loop: dropped when its area is zero, made counter-clockwise, its three edges.  kTag
// (rc2dgi_gradients_device): q0, q1, q2 are the colours of s0, s1, s2 as the caller lists them; they go into the
// record's pad words in that order, with kGradSwapped in `incl` when the swap exchanged s1 and s2
// (grad_tag, rc2dgi_gradient_interp.h).  Without kTag the pad words are zero, as ever.
template <bool kTag>
__device__ __forceinline__ void paint_dev_emit_t(PaintAcc &A, PaintSnap s0, PaintSnap s1, PaintSnap s2, unsigned q0,
                                                 unsigned q1, unsigned q2) {
  const long long area = (s1.x - s0.x) * (s2.y - s0.y) - (s2.x - s0.x) * (s1.y - s0.y);
  if (area == 0) return;
  if (area < 0) {
    const PaintSnap t = s1;
    s1 = s2;
    s2 = t;
  }
  const PaintSnap s[3] = {s0, s1, s2};
  PaintTri tri{};
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const PaintSnap a = s[e], b = s[(e + 1) % 3];
    const long long dx = b.x - a.x, dy = b.y - a.y;
    tri.e[e].a = (int)(-dy);
    tri.e[e].b = (int)dx;
    tri.e[e].c = dy * a.x - dx * a.y;
    if (dy < 0 || (dy == 0 && dx > 0)) tri.incl |= 1u << e;
    A.mnx = min(A.mnx, a.x); A.mxx = max(A.mxx, a.x);
    A.mny = min(A.mny, a.y); A.mxy = max(A.mxy, a.y);
  }
  if (kTag) grad_tag(tri, area < 0, q0, q1, q2);
  A.out[A.nt++] = tri;
}

__device__ __forceinline__ void paint_dev_emit(PaintAcc &A, PaintSnap s0, PaintSnap s1, PaintSnap s2) {
  paint_dev_emit_t<false>(A, s0, s1, s2, 0u, 0u, 0u);
}

}  // namespace rc2dgi
