// rc2dgi_gradient_interp.h -- what k_gradients_raster (rc2dgi_gradients.hip) does at a pixel centre:
// which triangle of a shape supplies the colour, and the interpolation of its three vertex colours.  Plain C++ with no
// HIP include, so that a host program compiles the very text the kernel runs (tests/gradients_interp_check.cpp).
//
// Tri is any record with e[3] of {int a, b; long long c}, an `incl` word and three `pad` words, as PaintTri.  The
// set-up (paint_dev_emit_t<true>, rc2dgi_paint_setup.h) leaves in pad[0 .. 2] the colours q0, q1, q2 of the triangle's
// vertices R0, R1, R2 IN THE ORDER THE HEADER LISTS THEM, four bytes r, g, b, a each, and sets kGradSwapped in `incl`
// when it exchanged R1 and R2 to make the triangle counter-clockwise.  Edge k of the record joins its vertices k and
// k + 1, so it is opposite to its vertex k + 2:
//   not swapped (record vertices R0, R1, R2):  E_0 = e[1], E_1 = e[2], E_2 = e[0]
//   swapped     (record vertices R0, R2, R1):  E_0 = e[1], E_1 = e[0], E_2 = e[2]
// where E_k is the edge function opposite to R_k.  Inside is positive either way, so the numbers do not depend on the
// swap; only their association with the colours does, which is why the colours are tagged before the swap.
// Ranges: |a|, |b| < 2^31, |X|, |Y| < 2^23, |c| < 2^61 (rc2dgi_tile_test.h): every |E| < 2^61 + 2^55, and the sum of
// three stays below 2^63.
// Every float operation is one IEEE single operation, rounded to nearest, never fused: the device unit spells them
// __fsub_rn / __fmul_rn / __fadd_rn / __fdiv_rn / __ll2float_rn, a host unit is built with -ffp-contract=off.
#pragma once

#ifndef RC2DGI_GRAD_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define RC2DGI_GRAD_HD __host__ __device__
#else
#define RC2DGI_GRAD_HD
#endif
#endif

namespace rc2dgi {

constexpr unsigned kGradSwapped = 1u << 8;  // in `incl`, above the three bits its other readers look at

#if defined(__HIP_DEVICE_COMPILE__)
#define RC2DGI_GRAD_SUB(x, y) __fsub_rn((x), (y))
#define RC2DGI_GRAD_MUL(x, y) __fmul_rn((x), (y))
#define RC2DGI_GRAD_ADD(x, y) __fadd_rn((x), (y))
#define RC2DGI_GRAD_DIV(x, y) __fdiv_rn((x), (y))
#define RC2DGI_GRAD_LL2F(x) __ll2float_rn(x)
#else
#define RC2DGI_GRAD_SUB(x, y) ((x) - (y))
#define RC2DGI_GRAD_MUL(x, y) ((x) * (y))
#define RC2DGI_GRAD_ADD(x, y) ((x) + (y))
#define RC2DGI_GRAD_DIV(x, y) ((x) / (y))
#define RC2DGI_GRAD_LL2F(x) ((float)(x))
#endif

// the set-up's half: the colours of the vertices as listed, and whether the swap exchanged the last two
template <class Tri>
RC2DGI_GRAD_HD inline void grad_tag(Tri &t, bool swapped, unsigned q0, unsigned q1, unsigned q2) {
  t.pad[0] = q0;
  t.pad[1] = q1;
  t.pad[2] = q2;
  if (swapped) t.incl |= kGradSwapped;
}

// one step of the walk: does `tr` cover the centre (X, Y)?  If so E[k] becomes the edge function opposite to the
// triangle's listed vertex k; otherwise E is left alone.
template <class Tri>
RC2DGI_GRAD_HD inline bool grad_covers(const Tri &tr, long long X, long long Y, long long E[3]) {
  long long e[3];
  bool ok = true;
  for (int k = 0; k < 3; ++k) {
    e[k] = (long long)tr.e[k].a * X + (long long)tr.e[k].b * Y + tr.e[k].c;
    ok = ok && (e[k] > 0 || (e[k] == 0 && ((tr.incl >> k) & 1u)));
  }
  if (ok) {
    const bool sw = (tr.incl & kGradSwapped) != 0;
    E[0] = e[1];
    E[1] = sw ? e[0] : e[2];
    E[2] = sw ? e[2] : e[0];
  }
  return ok;
}

// "Which triangle": the first of tris[0 .. ntri) that covers the centre (X, Y), in slot order -- the listed order with
// the dropped triangles skipped, the order paint_covered walks -- or -1.  (k_gradients_raster takes the same steps in
// the same order with a loop every lane of the wave stays in, so that the records come through scalar loads.)
template <class Tri>
RC2DGI_GRAD_HD inline int grad_first_covering(const Tri *tris, int ntri, long long X, long long Y, long long E[3]) {
  for (int t = 0; t < ntri; ++t)
    if (grad_covers(tris[t], X, Y, E)) return t;
  return -1;
}

// w1 = (float)E_1 / (float)A, w2 = (float)E_2 / (float)A with A = E_0 + E_1 + E_2, twice the area
RC2DGI_GRAD_HD inline void grad_weights(const long long E[3], float &w1, float &w2) {
  const float fa = RC2DGI_GRAD_LL2F(E[0] + E[1] + E[2]);
  w1 = RC2DGI_GRAD_DIV(RC2DGI_GRAD_LL2F(E[1]), fa);
  w2 = RC2DGI_GRAD_DIV(RC2DGI_GRAD_LL2F(E[2]), fa);
}

// a colour byte as a float: k * (1/255), one multiply (k_shapes_setup's conversion)
RC2DGI_GRAD_HD inline float grad_unorm(unsigned q, int ch) {
  return RC2DGI_GRAD_MUL((float)((q >> (8 * ch)) & 255u), 1.0f / 255.0f);
}

// (q0 + w1 * (q1 - q0)) + w2 * (q2 - q0): two differences, two products, two sums, in that order
RC2DGI_GRAD_HD inline float grad_channel(float q0, float q1, float q2, float w1, float w2) {
  const float d1 = RC2DGI_GRAD_SUB(q1, q0), d2 = RC2DGI_GRAD_SUB(q2, q0);
  const float p1 = RC2DGI_GRAD_MUL(w1, d1), p2 = RC2DGI_GRAD_MUL(w2, d2);
  return RC2DGI_GRAD_ADD(RC2DGI_GRAD_ADD(q0, p1), p2);
}

// src of the header's "Interpolation" paragraph: the four channels interpolated, then r, g, b times the gain.  q0, q1,
// q2 are the colours of the listed vertices (the record's pad words).
RC2DGI_GRAD_HD inline void grad_colour(unsigned q0, unsigned q1, unsigned q2, const long long E[3], float gain,
                                       float src[4]) {
  float w1, w2;
  grad_weights(E, w1, w2);
  for (int ch = 0; ch < 4; ++ch)
    src[ch] = grad_channel(grad_unorm(q0, ch), grad_unorm(q1, ch), grad_unorm(q2, ch), w1, w2);
  for (int ch = 0; ch < 3; ++ch) src[ch] = RC2DGI_GRAD_MUL(src[ch], gain);
}
template <class Tri>
RC2DGI_GRAD_HD inline void grad_colour(const Tri &tr, const long long E[3], float gain, float src[4]) {
  grad_colour(tr.pad[0], tr.pad[1], tr.pad[2], E, gain, src);
}

}  // namespace rc2dgi
