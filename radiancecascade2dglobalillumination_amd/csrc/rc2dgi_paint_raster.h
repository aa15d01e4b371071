// rc2dgi_paint_raster.h -- what the two painters share on the device (rc2dgi_paint.hip, whose primitives are set up on
// the host, and rc2dgi_paint_dev.hip, which sets them up on the device): the set-up records and the coverage test.
// rc2dgi_sprites.hip lays its set-up record over PaintPrim and shares the count clamp.  Device units only.
#pragma once

#include <hip/hip_runtime.h>

namespace rc2dgi {

struct PaintEdge {
  int a, b;     // E(X, Y) = a*X + b*Y + c over 1/256-pixel window coordinates
  long long c;
};

struct PaintTri {
  PaintEdge e[3];
  unsigned incl;  // bit k: pixel centres exactly on edge k are covered
  unsigned pad[3];
};

struct PaintPrim {
  int x0, y0, x1, y1;  // pixel bounding box (inclusive, GL rows), already clipped to the target
  int tri0, ntri;
  int pad0, pad1;
  float4 color;        // unorm8 * (1/255)
};

// rc2dgi_paint_device and rc2dgi_sprites_device: the number of records of the batch at `base` --
// m = min(max(*count_dev, 0), n) of the call, then this batch's share
__device__ __forceinline__ int paint_dev_total(const int *__restrict__ count_dev, int n) {
  if (!count_dev) return n;
  const int c = *count_dev;
  return min(max(c, 0), n);
}
__device__ __forceinline__ int paint_dev_batch(const int *__restrict__ count_dev, int n, int base, int batch) {
  return min(max(paint_dev_total(count_dev, n) - base, 0), batch);
}

// the centre (X, Y) = (256 i + 128, 256 j + 128) of a pixel inside p's bounding box is covered by one of p's triangles:
// every edge function E > 0, or E == 0 on an edge whose incl bit is set
__device__ __forceinline__ bool paint_covered(const PaintPrim &p, const PaintTri *__restrict__ tris, long long X,
                                              long long Y) {
  bool cov = false;
  for (int t = p.tri0; t < p.tri0 + p.ntri && !cov; ++t) {
    const PaintTri &tr = tris[t];
    bool ok = true;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const long long E = (long long)tr.e[e].a * X + (long long)tr.e[e].b * Y + tr.e[e].c;
      ok = ok && (E > 0 || (E == 0 && ((tr.incl >> e) & 1u)));
    }
    cov = ok;
  }
  return cov;
}

}  // namespace rc2dgi
