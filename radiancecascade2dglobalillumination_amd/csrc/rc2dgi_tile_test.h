// rc2dgi_tile_test.h -- the exact tile rejection of k_shapes_bin (rc2dgi_shapes.hip): can a triangle's
// edge equations cover any pixel centre of a rectangle of centres?  Plain C++ with no HIP include, so that a host
// program calls the very text the kernel runs (tests/shapes_tile_check.cpp).
//
// Tri is any record with e[3] of {int a, b; long long c} and an `incl` word, as PaintTri: edge k is
// E(X, Y) = a*X + b*Y + c over 1/256-pixel window coordinates, and a centre is covered when every E > 0, or E == 0 on
// an edge whose incl bit is set.  The centres of a rectangle are X0 <= X <= X1, Y0 <= Y <= Y1 (X = 256 i + 128).  E is
// linear, so its largest value over the rectangle lies at the corner the signs of a and b choose.  If that value fails
// the edge's test, every centre of the rectangle fails it and the triangle covers none of them: the triangle is "out".
// The converse does not hold (the three edges may pass at different corners), so a tile that is kept may still be
// empty; a tile that is rejected never holds a covered centre.
// Ranges: |a|, |b| < 2^31, |X|, |Y| < 2^23 (a 32768-pixel target), |c| < 2^61 (rc2dgi.h, rc2dgi_shapes_device):
// |a*X| + |b*Y| + |c| < 2^54 + 2^54 + 2^61 < 2^63.
#pragma once

#ifndef RC2DGI_TILE_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define RC2DGI_TILE_HD __host__ __device__
#else
#define RC2DGI_TILE_HD
#endif
#endif

namespace rc2dgi {

// the largest value of edge (a, b, c) over the rectangle of centres
RC2DGI_TILE_HD inline long long paint_edge_max(int a, int b, long long c, long long X0, long long Y0, long long X1,
                                               long long Y1) {
  return (long long)a * (a >= 0 ? X1 : X0) + (long long)b * (b >= 0 ? Y1 : Y0) + c;
}

// true: the triangle covers no centre of the rectangle
template <class Tri>
RC2DGI_TILE_HD inline bool paint_tri_out(const Tri &t, long long X0, long long Y0, long long X1, long long Y1) {
  bool out = false;
  for (int e = 0; e < 3; ++e) {
    const long long E = paint_edge_max(t.e[e].a, t.e[e].b, t.e[e].c, X0, Y0, X1, Y1);
    out = out || E < 0 || (E == 0 && !((t.incl >> e) & 1u));
  }
  return out;
}

}  // namespace rc2dgi
