// rc2dgi_shapes_setup.h -- the set-up of one record of a shape list, the text k_shapes_setup (rc2dgi_shapes.hip, the
// 32-byte rc2dgi_shape) and k_gradients_setup (rc2dgi_gradients.hip, the 48-byte rc2dgi_gradient) share: the words the
// kind names, the refusal test of the kind, the kind's vertex list in the header's float operations, then
// paint_dev_window / paint_dev_emit (rc2dgi_paint_setup.h) into the PaintPrim / PaintTri records the rasters read, 36
// triangle slots a shape.  kWords is the record's length in 32-bit words; word 0 is the kind and words 1 .. 6 are v[]
// in both.  kGrad: words 7 .. 10 are the four vertex colours and word 11 the gain -- each triangle is emitted with the
// colours of its vertices as listed (the header's "Colours by kind"), a gain that fails fabsf(gain) <= 0x1p20f
// refuses the record, and the gain's bits go to PaintPrim::pad0.  Without kGrad word 7 is the shape's one colour.
// Device units only.
#pragma once

#include "rc2dgi_device.h"
#include "rc2dgi_paint_raster.h"
#include "rc2dgi_paint_setup.h"

namespace rc2dgi {

template <int kWords, bool kGrad>
__device__ __forceinline__ void shapes_setup_record(const unsigned *__restrict__ list, int n,
                                                    const int *__restrict__ count_dev, int base, int batch,
                                                    PaintPrim *__restrict__ prims, PaintTri *__restrict__ tris,
                                                    unsigned *__restrict__ counters, const PaintXform &xf,
                                                    const PaintCircle &tab) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  const int mb = paint_dev_batch(count_dev, n, base, batch);
  bool refused = false;
  if (k < mb) {  // (base + k < m <= n: inside the list)
    const unsigned *q = list + (size_t)(base + k) * kWords;
    const int kind = (int)q[0];
    const bool rect = kind == RC2DGI_SHAPE_RECT, circle = kind == RC2DGI_SHAPE_CIRCLE,
               tri = kind == RC2DGI_SHAPE_TRIANGLE, line = kind == RC2DGI_SHAPE_LINE,
               ellipse = kind == RC2DGI_SHAPE_ELLIPSE;
    // the words the kind names, no others: 4, 3, 6, 5, 4 of v[]; none for an unknown kind
    const int nv = rect || ellipse ? 4 : circle ? 3 : tri ? 6 : line ? 5 : 0;
    float v[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) v[i] = i < nv ? __uint_as_float(q[1 + i]) : 0.0f;
    bool ok = nv != 0;
    if (rect || circle) {  // rc2dgi_paint's test, term for term (k_paint_dev_setup)
      const float lim = 4194304.0f;  // 2^22 pixels
      ok = fabsf(v[0]) < lim && fabsf(v[1]) < lim && fabsf(v[2]) < lim;
      if (rect)
        ok = ok && fabsf(v[3]) < lim && fabsf(__fadd_rn(v[0], v[2])) < lim && fabsf(__fadd_rn(v[1], v[3])) < lim;
      else
        ok = ok && __fadd_rn(fabsf(v[0]), fabsf(v[2])) < lim && __fadd_rn(fabsf(v[1]), fabsf(v[2])) < lim;
    } else {  // every value read is below 2^20 in magnitude (false for a NaN and for an infinity)
#pragma unroll
      for (int i = 0; i < 6; ++i) ok = ok && (i >= nv || fabsf(v[i]) < 0x1p20f);
    }
    // the colours the kind names, no others: 4, 2, 3, 2, 2 of c[]; then the gain (false for a NaN and an infinity)
    unsigned c[4] = {0u, 0u, 0u, 0u};
    float gain = 1.0f;
    if (kGrad) {
      const int nc = rect ? 4 : tri ? 3 : nv != 0 ? 2 : 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) c[i] = i < nc ? q[7 + i] : 0u;
      gain = __uint_as_float(q[kWords - 1]);
      ok = ok && fabsf(gain) <= 0x1p20f;
    }
    refused = !ok;
    PaintPrim pp{};
    pp.tri0 = k * kPaintDevTris;
    PaintAcc A{tris + (size_t)k * kPaintDevTris, 0, LLONG_MAX, LLONG_MAX, LLONG_MIN, LLONG_MIN};
    if (ok && rect) {  // DrawRectanglePro (rotation 0): TL, BL, BR, TR as (0, 1, 2), (0, 2, 3)
      const float xr = __fadd_rn(v[0], v[2]), yb = __fadd_rn(v[1], v[3]);
      const PaintSnap tl = paint_dev_window(v[0], v[1], xf), tr = paint_dev_window(xr, v[1], xf),
                      bl = paint_dev_window(v[0], yb, xf), br = paint_dev_window(xr, yb, xf);
      paint_dev_emit_t<kGrad>(A, tl, bl, br, c[0], c[1], c[2]);
      paint_dev_emit_t<kGrad>(A, tl, br, tr, c[0], c[2], c[3]);
    } else if (ok && (circle || ellipse)) {
      // the fan (c, T(k + 1), T(k)), k = 0 .. 35, T(k) = (cx + c37[k] * rh, cy + s37[k] * rv), two triangles a step as
      // k_paint_dev_setup walks DrawCircleSector's 18 quads; a circle is rh = rv = radius, a radius <= 0 being 0.1
      const float rh = circle ? (v[2] <= 0.0f ? 0.1f : v[2]) : v[2], rv = circle ? rh : v[3];
      const PaintSnap ctr = paint_dev_window(v[0], v[1], xf);
      PaintSnap p0 =
          paint_dev_window(__fadd_rn(v[0], __fmul_rn(tab.c[0], rh)), __fadd_rn(v[1], __fmul_rn(tab.s[0], rv)), xf);
#pragma unroll 1
      for (int s = 0; s < 18; ++s) {
        const int a = 2 * s;
        const PaintSnap p1 = paint_dev_window(__fadd_rn(v[0], __fmul_rn(tab.c[a + 1], rh)),
                                              __fadd_rn(v[1], __fmul_rn(tab.s[a + 1], rv)), xf);
        const PaintSnap p2 = paint_dev_window(__fadd_rn(v[0], __fmul_rn(tab.c[a + 2], rh)),
                                              __fadd_rn(v[1], __fmul_rn(tab.s[a + 2], rv)), xf);
        paint_dev_emit_t<kGrad>(A, ctr, p2, p1, c[0], c[1], c[1]);
        paint_dev_emit_t<kGrad>(A, ctr, p1, p0, c[0], c[1], c[1]);
        p0 = p2;
      }
    } else if (ok && tri) {
      paint_dev_emit_t<kGrad>(A, paint_dev_window(v[0], v[1], xf), paint_dev_window(v[2], v[3], xf),
                              paint_dev_window(v[4], v[5], xf), c[0], c[1], c[2]);
    } else if (ok) {  // DrawLineEx: the quad s0, s1, s2, s3 around the segment, as {s0, s1, s2} and {s1, s2, s3}
      const float dx = __fadd_rn(v[2], -v[0]), dy = __fadd_rn(v[3], -v[1]), thick = v[4];
      const float len = sqrtf(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
      if (len > 0.0f && thick > 0.0f) {
        const float scale = thick / __fmul_rn(2.0f, len);
        const float rx = __fmul_rn(-scale, dy), ry = __fmul_rn(scale, dx);
        const PaintSnap s0 = paint_dev_window(__fadd_rn(v[0], -rx), __fadd_rn(v[1], -ry), xf),
                        s1 = paint_dev_window(__fadd_rn(v[0], rx), __fadd_rn(v[1], ry), xf),
                        s2 = paint_dev_window(__fadd_rn(v[2], -rx), __fadd_rn(v[3], -ry), xf),
                        s3 = paint_dev_window(__fadd_rn(v[2], rx), __fadd_rn(v[3], ry), xf);
        paint_dev_emit_t<kGrad>(A, s0, s1, s2, c[0], c[0], c[1]);
        paint_dev_emit_t<kGrad>(A, s1, s2, s3, c[0], c[1], c[1]);
      }
    }
    pp.ntri = A.nt;
    if (pp.ntri > 0) {  // pixels whose centre 256 i + 128 lies in [min, max], clipped to the target
      pp.x0 = (int)max(0LL, -paint_dev_floor_div(-(A.mnx - 128), 256));
      pp.x1 = (int)min((long long)xf.W - 1, paint_dev_floor_div(A.mxx - 128, 256));
      pp.y0 = (int)max(0LL, -paint_dev_floor_div(-(A.mny - 128), 256));
      pp.y1 = (int)min((long long)xf.H - 1, paint_dev_floor_div(A.mxy - 128, 256));
      if (pp.x0 > pp.x1 || pp.y0 > pp.y1) pp.ntri = 0;
    }
    if (kGrad) pp.pad0 = (int)__float_as_uint(gain);
    const unsigned rgba = q[7];
    pp.color = make_float4(__fmul_rn((float)(rgba & 255u), kInv255), __fmul_rn((float)((rgba >> 8) & 255u), kInv255),
                           __fmul_rn((float)((rgba >> 16) & 255u), kInv255), __fmul_rn((float)(rgba >> 24), kInv255));
    prims[k] = pp;
  }
  const unsigned long long b = __ballot(refused);  // integer adds: the sum is the same in any order
  if (b != 0 && (threadIdx.x & 63) == 0) atomicAdd(&counters[0], (unsigned)__popcll(b));
}

}  // namespace rc2dgi
