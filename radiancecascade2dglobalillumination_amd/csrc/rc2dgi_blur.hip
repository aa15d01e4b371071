// rc2dgi_blur.hip -- the blur and merge passes, each kernel with its launcher (gfx950).
//   k_blur          shaders/Blur.fs:11-37              (RC2DGI.cs:367-379)
//   k_blur_copyback default shader, blended            (RC2DGI.cs:381-386)
//   k_merge         shaders/merge.fs:10-15 + copy-back (RC2DGI.cs:389-404)
//   k_blur_fused, k_blur_rows: those passes in one kernel where the shapes allow; k_blur_exact: their redo
//   (k_blur_odd_rows: a row-strip shard's report that its rows need it)
//   giRT1/2: float4, RGBA16F (f16 mode) or RGBA8 bytes; cascadeBlurRT: float4 (RGBA8 mode: bytes)
#include "rc2dgi_device.h"
#include "rc2dgi_kernels.h"
#include "rc2dgi_launch.h"

#include <type_traits>

namespace rc2dgi {

// The storage of giRT1 / giRT2 as its policy type (GiU8 / GiF16 / GiF32, rc2dgi_device.h): f(GI{}).  U8 false:
// the kernels that are not built for RGBA8 (their launchers refuse c.gi_u8 before they get here).
template <bool U8 = true, class F>
static void with_gi(CascadeDims c, F &&f) {
  if constexpr (U8) {
    if (c.gi_u8) return f(GiU8{});
  }
  if (c.gi_f16) return f(GiF16{});
  f(GiF32{});
}
// a float4-typed texture pointer as the policy's texel type
template <class P, class V>
static auto tex(V *p) {
  return reinterpret_cast<std::conditional_t<std::is_const<V>::value, const typename P::T, typename P::T> *>(p);
}

// ---------------------------------------------------------------- Blur + copy-back
template <class GI>
__global__ __launch_bounds__(256) void k_blur(const typename GI::T *__restrict__ gi,
                                              typename GI::RT::T *__restrict__ blur_out, CascadeDims c, float radius,
                                              int row0, int row1) {
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  const int j = row0 + blockIdx.y * 4 + (threadIdx.x >> 6);
  if (i >= c.CW || j >= row1) return;
  const Axis ax{c.CW, c.powW}, ay{c.CH, c.powH};
  const float u = texcoord(i, ax), v = texcoord(j, ay);
  const float tsx = 1.0f / (float)c.CW, tsy = 1.0f / (float)c.CH;
  // Blur.fs:22-34 order: 4 corners, 4 edges, centre
  const float kx[8] = {-1.f, 1.f, -1.f, 1.f, 0.f, 0.f, -1.f, 1.f};
  const float ky[8] = {-1.f, -1.f, 1.f, 1.f, -1.f, 1.f, 0.f, 0.f};
  float4 res = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    float su = u, sv = v, w = 0.250f;
    if (k < 8) {
      su = u + (kx[k] * tsx) * radius;
      sv = v + (ky[k] * tsy) * radius;
      w = k < 4 ? 0.0625f : 0.125f;
    }
    const float4 t = sample_bilinear_gi<GI>(gi, c.pitch, ax, ay, su, sv);
    res.x = res.x + t.x * w;
    res.y = res.y + t.y * w;
    res.z = res.z + t.z * w;
    res.w = res.w + t.w * w;
  }
  GI::RT::st(&blur_out[(size_t)j * c.pitch + i], GI::RT::blend_black(res));  // cascadeBlurRT cleared to (0,0,0,1)
}

hipError_t launch_blur(const BlurArgs &a, CascadeDims c, hipStream_t st) {
  int row0 = a.row0, row1 = a.row1;
  clamp_rows(c.CH, row0, row1);
  if (row0 >= row1) return hipSuccess;
  with_gi(c, [&](auto gi) {
    using GI = decltype(gi);
    hipLaunchKernelGGL(k_blur<GI>, grid2d(c.CW, row1 - row0), dim3(256), 0, st, tex<GI>(a.gi_in),
                       tex<typename GI::RT>(a.blur_out), c, a.radius, row0, row1);
  });
  return hipGetLastError();
}

// The fused blur kernels below skip LINEAR taps of weight 0: fma(0, b - a, a) = a.  That holds for finite a, b whose
// difference is finite; the reference's lerp gives NaN when the neighbour is not finite (0 * inf).  A G_0 channel
// that is not finite, or 2^30 or more in magnitude, could break the identity in a lerp downstream; below that every
// value of the pass stays finite (the blur is a convex sum of G_0 values, so below 2^30 too; its blend over black
// and the copy-back multiply two such and add: below 2^62, then 2^124; the merge adds colour).  absmax4 is the
// largest magnitude of a texel as bits (NaN and inf compare above every finite value); a fused kernel that stages a
// texel at or above kOddBits writes the frame's epoch to *flag, and k_blur_exact then redoes the frame tap by tap
// (launch_blur_exact).  Every G_0 texel is staged by some workgroup of a whole frame.
constexpr unsigned kOddBits = 0x4E800000u;  // 2^30
__device__ __forceinline__ unsigned absmax4(float4 v) {
  return max(max(__float_as_uint(v.x) & 0x7FFFFFFFu, __float_as_uint(v.y) & 0x7FFFFFFFu),
             max(__float_as_uint(v.z) & 0x7FFFFFFFu, __float_as_uint(v.w) & 0x7FFFFFFFu));
}

// Blur.fs + its blended copy-back in one pass, for power-of-two cascade sizes.  There the
// copy-back's LINEAR sample of cascadeBlurRT at fragTexCoord lands exactly on the texel
// (x = (i+0.5)/n*n - 0.5 = i, weight 0: fma(0, b - a, a) = a), so each texel needs only its
// own blur value.  G_0 is staged in LDS: a 64 x 16 core plus an H-texel halo covers every
// bilinear tap of radius <= H - 2 (taps that ever fall outside are read from HBM).
template <int H, class GI>
__global__ __launch_bounds__(256) void k_blur_fused(const typename GI::T *__restrict__ gi_in,
                                                    float4 *__restrict__ blur_out, typename GI::T *__restrict__ gi_out,
                                                    CascadeDims c, float radius,
                                                    int tile0, unsigned *__restrict__ flag, unsigned epoch) {
  constexpr int TW = 64 + 2 * H, TH = 16 + 2 * H;
  __shared__ float4 tile[TH * TW];
  const int by = (int)blockIdx.y + tile0;  // 16-row tile
  const int x0 = blockIdx.x * 64 - H, y0 = by * 16 - H;
  unsigned odd = 0u;
  for (int k = threadIdx.x; k < TW * TH; k += 256) {
    const int ty = k / TW, tx = k - ty * TW;
    const int gx = (x0 + tx) & (c.CW - 1), gy = (y0 + ty) & (c.CH - 1);
    const float4 g = GI::ld(&gi_in[(size_t)gy * c.pitch + gx]);
    tile[k] = g;
    odd = max(odd, absmax4(g));
  }
  __syncthreads();
  const Axis ax{c.CW, 1}, ay{c.CH, 1};
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  const float u = texcoord(i, ax);
  const float tsx = 1.0f / (float)c.CW, tsy = 1.0f / (float)c.CH;
  // Blur.fs taps use only three distinct x coordinates (offset -1, 0, +1 texels * radius) and three
  // y coordinates; resolve each to (tap0, tap1, weight) once.  fragTexCoord + vec2(k, .) * texelSize *
  // _BlurRadius evaluates x as u + (k * tsx) * radius, the same float for every tap with that k.
  int xa[3], xb[3];
  float xw[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const float su = q == 1 ? u : u + ((float)(q - 1) * tsx) * radius;
    wrap_linear(su, ax, xa[q], xb[q], xw[q]);
    xa[q] = (xa[q] - x0) & (c.CW - 1);  // tile-local columns
    xb[q] = (xb[q] - x0) & (c.CW - 1);
  }
  const bool xin = xa[0] < TW && xb[0] < TW && xa[2] < TW && xb[2] < TW && xa[1] < TW && xb[1] < TW;
  // Blur.fs:22-34 order: (-1,-1) (1,-1) (-1,1) (1,1) (0,-1) (0,1) (-1,0) (1,0) (0,0); index 0..2 = -1,0,+1
  constexpr int KX[9] = {0, 2, 0, 2, 1, 1, 0, 2, 1};
  constexpr int KY[9] = {0, 0, 2, 2, 0, 2, 1, 1, 1};
  constexpr float KW[9] = {0.0625f, 0.0625f, 0.0625f, 0.0625f, 0.125f, 0.125f, 0.125f, 0.125f, 0.250f};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int j = by * 16 + (threadIdx.x >> 6) + 4 * t;
    if (i >= c.CW || j >= c.CH) continue;
    const float v = texcoord(j, ay);
    int ya[3], yb[3];
    float yw[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const float sv = q == 1 ? v : v + ((float)(q - 1) * tsy) * radius;
      wrap_linear(sv, ay, ya[q], yb[q], yw[q]);
      ya[q] = (ya[q] - y0) & (c.CH - 1);
      yb[q] = (yb[q] - y0) & (c.CH - 1);
    }
    const bool inside = xin && ya[0] < TH && yb[0] < TH && ya[1] < TH && yb[1] < TH && ya[2] < TH && yb[2] < TH;
    float4 res = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int qx = KX[k], qy = KY[k];
      float4 t00, t10, t01, t11;
      if (inside) {
        t00 = tile[ya[qy] * TW + xa[qx]];
        t10 = tile[ya[qy] * TW + xb[qx]];
        t01 = tile[yb[qy] * TW + xa[qx]];
        t11 = tile[yb[qy] * TW + xb[qx]];
      } else {  // a tap beyond the staged halo: global coordinates are tile-local + origin
        auto g = [&](int ly, int lx) {
          return GI::ldnt(&gi_in[(size_t)((ly + y0) & (c.CH - 1)) * c.pitch + ((lx + x0) & (c.CW - 1))]);
        };
        t00 = g(ya[qy], xa[qx]);
        t10 = g(ya[qy], xb[qx]);
        t01 = g(yb[qy], xa[qx]);
        t11 = g(yb[qy], xb[qx]);
      }
      const float4 tp = lerp_gl(lerp_gl(t00, t10, xw[qx]), lerp_gl(t01, t11, xw[qx]), yw[qy]);
      const float w = KW[k];
      res.x = res.x + tp.x * w;
      res.y = res.y + tp.y * w;
      res.z = res.z + tp.z * w;
      res.w = res.w + tp.w * w;
    }
    const float4 b = blend_over_black(res);  // cascadeBlurRT cleared to (0,0,0,1)
    const size_t o = (size_t)j * c.pitch + i;
    blur_out[o] = b;
    const float4 g = GI::round(blend(b, tile[(j - y0) * TW + (i - x0)]));  // copy-back onto finalGI, blended
    GI::st(&gi_out[o], g);
  }
  if (odd >= kOddBits && flag) *flag = epoch;
}

bool blur_fused_ok(CascadeDims c, float radius) {
  return !c.gi_u8 && c.powW && c.powH && c.CW >= 64 && c.CH >= 16 && radius <= 6.0f;
}

bool launch_blur_fused(const BlurArgs &a, CascadeDims c, hipStream_t st) {
  if (!blur_fused_ok(c, a.radius)) return false;
  int row0 = a.row0, row1 = a.row1;
  clamp_rows(c.CH, row0, row1);
  if (row0 >= row1) return true;
  const int t0 = row0 / 16, t1 = ceil_div(row1, 16);  // whole 16-row tiles
  const dim3 grid(ceil_div(c.CW, 64), t1 - t0);
  with_gi<false>(c, [&](auto gi) {
    using GI = decltype(gi);
    if (a.radius <= 2.0f)
      hipLaunchKernelGGL((k_blur_fused<4, GI>), grid, dim3(256), 0, st, tex<GI>(a.gi_in), a.blur_out,
                         tex<GI>(a.gi_out), c, a.radius, t0, a.flag, a.epoch);
    else  // (blur_fused_ok: radius <= 6)
      hipLaunchKernelGGL((k_blur_fused<8, GI>), grid, dim3(256), 0, st, tex<GI>(a.gi_in), a.blur_out,
                         tex<GI>(a.gi_out), c, a.radius, t0, a.flag, a.epoch);
  });
  return true;
}

// Blur.fs + blended copy-back (+ merge.fs and its copy-back when MERGE) for power-of-two cascades
// and a dyadic radius (radius * 256 integral, radius < F + 1, sizes <= 2^14).  Then every
// fragTexCoord + k * texelSize * radius is exact (a multiple of 2^-8 texels below 2^15 texels), so
// the LINEAR taps of texel i sit at the fixed columns i + a0, i + a0 + 1 (weight w0), i, i + 1
// (weight 0) and i + F, i + F + 1 (weight w2) -- the same for every texel, the same values the
// general path computes.  Rows follow the same pattern.  Each thread owns a column of 8
// consecutive rows: it lerps every input row horizontally once (3 samples per row) and reuses those
// along the column for the vertical lerps of all 8 outputs.  Weight-0 lerps are identities for
// finite values (fma(0, b - a, a) = a) and are skipped.  With MERGE (screen == cascade size) the
// merge's LINEAR sample of finalGI lands exactly on the texel as well (same argument), so
// merge.fs runs on the blended GI value held in registers.
#ifndef RC2DGI_BLUR_RPT
#define RC2DGI_BLUR_RPT 8  // output rows per thread (tiles of 4 x this many rows; A/B builds: 4)
#endif
template <int F, bool MERGE, class GI>
__global__ __launch_bounds__(256) void k_blur_rows(const typename GI::T *__restrict__ gi_in,
                                                   float4 *__restrict__ blur_out, typename GI::T *__restrict__ gi_out,
                                                   CascadeDims c, BlurTaps bt,
                                                   const float4 *__restrict__ color_in, float4 *__restrict__ temp,
                                                   float4 *__restrict__ color_out, int spitch, int tile0, int m0, int m1,
                                                   int g0, int gn, unsigned *__restrict__ flag, unsigned epoch) {
  constexpr int RPT = RC2DGI_BLUR_RPT, TR = 4 * RPT;  // rows per thread, rows per tile
  constexpr int HALO = F + 1, TW = 64 + 2 * HALO, TH = TR + 2 * HALO, NR = RPT + 2 * HALO;
  __shared__ float4 tile[TH * TW];
  const int by = (int)blockIdx.y + tile0;  // TR-row tile
  const int x0 = blockIdx.x * 64 - HALO, y0 = by * TR - HALO;
  unsigned odd = 0u;  // (absmax4: at kOddBits and above a skipped weight-0 tap is no identity)
  for (int k = threadIdx.x; k < TW * TH; k += 256) {
    const int ty = k / TW, tx = k - ty * TW;
    // gi_in holds rows [g0, g0 + gn) cyclically (a row-strip shard's banded level 0; else g0 0, gn CH): the band
    // row, rows past the band read its last row (only for texels the launch does not store)
    const int gx = (x0 + tx) & (c.CW - 1), gy = min((y0 + ty - g0) & (c.CH - 1), gn - 1);
    const float4 g = GI::ld(&gi_in[(size_t)gy * c.pitch + gx]);
    tile[k] = g;
    odd = max(odd, absmax4(g));
  }
  __syncthreads();
  const int lx = (threadIdx.x & 63) + HALO;  // tile column of this thread's texel
  const int r0 = (threadIdx.x >> 6) * RPT;   // first input row (tile-local) = first output row - HALO
  const bool lo = bt.a0 == -F - 1;           // a0 is -F-1 (fractional radius) or -F (integral radius)
  const float w0 = bt.w0, w2 = bt.w2;
  // h[k][q]: input row r0 + k lerped horizontally at column offset q (0: a0, 1: 0, 2: F)
  float4 h[NR][3];
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    const float4 *row = tile + (r0 + k) * TW + lx;
    const float4 a = row[bt.a0], b = row[bt.a0 + 1];
    h[k][0] = lerp_gl(a, b, w0);
    h[k][1] = row[0];
    h[k][2] = lerp_gl(row[F], row[F + 1], w2);
  }
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
#pragma unroll
  for (int t = 0; t < RPT; ++t) {
    const int m = t + HALO;  // this output's own row in h
    // row pairs of the y offsets: -1 -> (m + a0, m + a0 + 1) w0; 0 -> m (weight 0); +1 -> (m + F, m + F + 1) w2
    float4 s[3][3];  // s[qy][qx]
#pragma unroll
    for (int qx = 0; qx < 3; ++qx) {
      const float4 ra = lo ? h[m - F - 1][qx] : h[m - F][qx];
      const float4 rb = lo ? h[m - F][qx] : h[m - F + 1][qx];
      s[0][qx] = lerp_gl(ra, rb, w0);
      s[1][qx] = h[m][qx];
      s[2][qx] = lerp_gl(h[m + F][qx], h[m + F + 1][qx], w2);
    }
    // Blur.fs:22-34 order: (-1,-1) (1,-1) (-1,1) (1,1) (0,-1) (0,1) (-1,0) (1,0) (0,0)
    constexpr int KX[9] = {0, 2, 0, 2, 1, 1, 0, 2, 1};
    constexpr int KY[9] = {0, 0, 2, 2, 0, 2, 1, 1, 1};
    constexpr float KW[9] = {0.0625f, 0.0625f, 0.0625f, 0.0625f, 0.125f, 0.125f, 0.125f, 0.125f, 0.250f};
    float4 res = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const float4 tp = s[KY[k]][KX[k]];
      const float w = KW[k];
      res.x = res.x + tp.x * w;
      res.y = res.y + tp.y * w;
      res.z = res.z + tp.z * w;
      res.w = res.w + tp.w * w;
    }
    const float4 b = blend_over_black(res);  // cascadeBlurRT cleared to (0,0,0,1)
    const float4 g = GI::round(blend(b, h[m][1]));  // copy-back onto finalGI, blended (as stored)
    const int j = by * TR + r0 + t;
    if constexpr (!MERGE) {
      const size_t o = (size_t)j * c.pitch + i;
      blur_out[o] = b;
      GI::st(&gi_out[o], g);
    } else {  // merge.fs:10-15 + tempRT -> colorRT copy-back (RC2DGI.cs:389-404)
      // every output texture (cascadeBlurRT, the copied-back GI, temp, color_out; cascade == screen here, so one
      // pitch) holds rows [m0, m1) -- a shard's own rows -- and one guard row after them, which takes the rows
      // outside (unconditional stores: a branch around them doubled the kernel's registers)
      const int jr = (j >= m0 && j < m1) ? j - m0 : m1 - m0;
      const size_t so = (size_t)j * spitch + i, mo = (size_t)jr * spitch + i;
      blur_out[mo] = b;
      GI::st(&gi_out[mo], g);
      const float4 col = color_in[so];
      const float4 src =
          make_float4(fminf(col.x + g.x, 1.0f), fminf(col.y + g.y, 1.0f), fminf(col.z + g.z, 1.0f), col.w);
      const float4 tt = blend_over_black(src);
      temp[mo] = tt;
      color_out[mo] = blend(tt, col);
    }
  }
  if (odd >= kOddBits && flag) *flag = epoch;
}

int blur_rows_plan(CascadeDims c, float radius, BlurTaps *bt) {
  if (c.gi_u8 || !(c.powW && c.powH) || c.CW < 64 || c.CH < 32 || c.CW > 16384 || c.CH > 16384) return -1;
  if (!(radius > 0.0f) || !(radius < 3.0f) || radius * 256.0f != floorf(radius * 256.0f)) return -1;
  // x = i - radius and i + radius are exact: floor / fraction do not depend on i
  const float lo = -radius, hi = radius;
  bt->a0 = (int)floorf(lo);
  bt->w0 = lo - floorf(lo);
  bt->w2 = hi - floorf(hi);
  return (int)floorf(hi);  // F
}

bool launch_blur_rows(const BlurArgs &a, ScreenDims s, CascadeDims c, hipStream_t st) {
  BlurTaps bt;
  const int m1 = a.m1 < 0 ? s.H : a.m1;
  const int g0 = a.gn <= 0 ? 0 : a.g0, gn = a.gn <= 0 ? c.CH : a.gn;
  const int F = blur_rows_plan(c, a.radius, &bt);
  if (F < 0) return false;
  if (a.merge && !(s.W == c.CW && s.H == c.CH)) return false;
  int row0 = a.row0, row1 = a.row1;
  clamp_rows(c.CH, row0, row1);
  if (row0 >= row1) return true;
  constexpr int TR = 4 * RC2DGI_BLUR_RPT;
  const int t0 = row0 / TR, t1 = ceil_div(row1, TR);  // whole tiles
  const dim3 grid(c.CW / 64, t1 - t0);
  with_gi<false>(c, [&](auto gi) {
    using GI = decltype(gi);
#define RC2DGI_BLUR_ROWS(FV, MV)                                                                                  \
  hipLaunchKernelGGL((k_blur_rows<FV, MV, GI>), grid, dim3(256), 0, st, tex<GI>(a.gi_in), a.blur_out,            \
                     tex<GI>(a.gi_out), c, bt, a.color_in, a.temp, a.color_out, s.pitch, t0, a.m0, m1, g0, gn, \
                     a.flag, a.epoch)
    if (a.merge) {
      if (F == 0) RC2DGI_BLUR_ROWS(0, true); else if (F == 1) RC2DGI_BLUR_ROWS(1, true); else RC2DGI_BLUR_ROWS(2, true);
    } else {
      if (F == 0) RC2DGI_BLUR_ROWS(0, false); else if (F == 1) RC2DGI_BLUR_ROWS(1, false); else RC2DGI_BLUR_ROWS(2, false);
    }
#undef RC2DGI_BLUR_ROWS
  });
  return true;
}

template <class GI>
__global__ __launch_bounds__(256) void k_blur_copyback(const typename GI::RT::T *__restrict__ blur,
                                                       typename GI::T *__restrict__ gi, CascadeDims c, int row0,
                                                       int row1) {
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  const int j = row0 + blockIdx.y * 4 + (threadIdx.x >> 6);
  if (i >= c.CW || j >= row1) return;
  const float u = texcoord(i, Axis{c.CW, c.powW}), v = texcoord(j, Axis{c.CH, c.powH});
  const float4 s = sample_bilinear_gi<typename GI::RT>(blur, c.pitch, Axis{c.CW, c.powW}, Axis{c.CH, c.powH}, u, v);
  const size_t o = (size_t)j * c.pitch + i;
  GI::st(&gi[o], GI::blend(s, GI::ld(&gi[o])));
}

hipError_t launch_blur_copyback(const float4 *blur, float4 *gi, CascadeDims c, hipStream_t st, int row0, int row1) {
  clamp_rows(c.CH, row0, row1);
  if (row0 >= row1) return hipSuccess;
  with_gi(c, [&](auto p) {
    using GI = decltype(p);
    hipLaunchKernelGGL(k_blur_copyback<GI>, grid2d(c.CW, row1 - row0), dim3(256), 0, st, tex<typename GI::RT>(blur),
                       tex<GI>(gi), c, row0, row1);
  });
  return hipGetLastError();
}

// ---------------------------------------------------------------- Merge + copy-back
template <class GI>
__global__ __launch_bounds__(256) void k_merge(const float4 *__restrict__ color_in, const typename GI::T *__restrict__ gi,
                                               float4 *__restrict__ temp, float4 *__restrict__ color_out,
                                               ScreenDims s, CascadeDims c, int row0, int row1, int linux_merge,
                                               int m0) {
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  const int j = row0 + blockIdx.y * 4 + (threadIdx.x >> 6);
  if (i >= s.W || j >= row1) return;
  const float u = texcoord(i, Axis{s.W, s.powW}), v = texcoord(j, Axis{s.H, s.powH});
  const size_t o = (size_t)j * s.pitch + i, mo = (size_t)(j - m0) * s.pitch + i;  // (temp / color_out: from row m0)
  const float4 col = color_in[o];
  float4 src = col;  // Linux: raylib's default shader, texel * colDiffuse (1) * vertex colour (1) = the texel
  if (!linux_merge) {
    const float4 g = sample_bilinear_gi<GI>(gi, c.pitch, Axis{c.CW, c.powW}, Axis{c.CH, c.powH}, u, v);
    src = make_float4(fminf(col.x + g.x, 1.0f), fminf(col.y + g.y, 1.0f), fminf(col.z + g.z, 1.0f), col.w);
  }
  const float4 t = GI::RT::blend_black(src);  // tempRT as cleared by ClearAllRTs
  temp[mo] = t;
  color_out[mo] = GI::RT::blend(t, col);      // tempRT -> colorRT, default shader, blended
}

hipError_t launch_merge(const BlurArgs &a, ScreenDims s, CascadeDims c, hipStream_t st, bool linux_merge) {
  int row0 = a.row0, row1 = a.row1;
  clamp_rows(s.H, row0, row1);
  if (row0 >= row1) return hipSuccess;
  if (row0 < a.m0) return hipErrorInvalidValue;  // (temp / color_out start at row m0)
  with_gi(c, [&](auto gi) {
    using GI = decltype(gi);
    hipLaunchKernelGGL(k_merge<GI>, grid2d(s.W, row1 - row0), dim3(256), 0, st, a.color_in, tex<GI>(a.gi_in), a.temp,
                       a.color_out, s, c, row0, row1, (int)linux_merge, a.m0);
  });
  return hipGetLastError();
}

// A row-strip shard's fused kernels stage rows outside the ones it computed (whole tiles), so they do not report for
// it (flag nullptr): this scan of the level-0 rows [row0, row1) it did compute does -- every row the redo of its rows
// reads (plan_frame: level 0 holds the blur's rows +- ceil(radius) + 2).  gi_in as k_blur_rows takes it (g0, gn).
template <class GI>
__global__ __launch_bounds__(256) void k_blur_odd_rows(const typename GI::T *__restrict__ gi_in, CascadeDims c,
                                                       int row0, int row1, int g0, int gn,
                                                       unsigned *__restrict__ flag, unsigned epoch) {
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  const int j = row0 + blockIdx.y * 4 + (threadIdx.x >> 6);
  if (i >= c.CW || j >= row1) return;
  const int gy = min((j - g0) & (c.CH - 1), gn - 1);
  if (absmax4(GI::ld(&gi_in[(size_t)gy * c.pitch + i])) >= kOddBits) *flag = epoch;
}

hipError_t launch_blur_odd_rows(const BlurArgs &a, CascadeDims c, hipStream_t st) {
  if (c.gi_u8 || !(c.powW && c.powH) || !a.flag) return hipErrorInvalidValue;
  int row0 = a.row0, row1 = a.row1;
  clamp_rows(c.CH, row0, row1);
  if (row0 >= row1) return hipSuccess;
  const int g0 = a.gn <= 0 ? 0 : a.g0, gn = a.gn <= 0 ? c.CH : a.gn;
  with_gi<false>(c, [&](auto gi) {
    using GI = decltype(gi);
    hipLaunchKernelGGL(k_blur_odd_rows<GI>, grid2d(c.CW, row1 - row0), dim3(256), 0, st, tex<GI>(a.gi_in), c, row0,
                       row1, g0, gn, a.flag, a.epoch);
  });
  return hipGetLastError();
}

// The fused blur kernels' frame redone tap by tap, for a frame in which one of them staged such a value (*flag ==
// epoch; otherwise every workgroup returns at once).  Each texel evaluates k_blur, k_blur_copyback and (MERGE)
// k_merge as they are written -- the blur of every texel in its copy-back's LINEAR footprint, the copied-back GI of
// every texel in the merge's footprint -- from G_0 alone, so no pass waits for another.  Slow (nothing is shared
// between texels or footprints: 5 blur texels of 9 taps each, 21 with MERGE) and rare.  A workgroup strides over the
// rows (a small grid: the launch costs little when it is idle).  Rows [row0, row1) of a power-of-two cascade; a
// row-strip shard's layouts as k_blur_rows has them: gi_in holds rows [g0, g0 + gn) cyclically, temp / color_out
// hold rows from m0 on, and so do blur_out / gi_out when STRIP (then the rows are the shard's own).
template <bool MERGE, class GI>
__global__ __launch_bounds__(256) void k_blur_exact(const unsigned *__restrict__ flag, unsigned epoch,
                                                    const typename GI::T *__restrict__ gi_in,
                                                    float4 *__restrict__ blur_out, typename GI::T *__restrict__ gi_out,
                                                    CascadeDims c, float radius, const float4 *__restrict__ color_in,
                                                    float4 *__restrict__ temp, float4 *__restrict__ color_out,
                                                    ScreenDims s, int row0, int row1, int m0, int strip, int g0,
                                                    int gn) {
  if (*flag != epoch) return;
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  if (i >= c.CW) return;
  const Axis ax{c.CW, c.powW}, ay{c.CH, c.powH};
  const float tsx = 1.0f / (float)c.CW, tsy = 1.0f / (float)c.CH;
  auto g0_at = [&](int x, int y) {  // G_0's texel (x, y), 0 <= y < CH
    return &gi_in[(size_t)min((y - g0) & (c.CH - 1), gn - 1) * c.pitch + x];
  };
  auto blur_at = [&](int x, int y) {  // k_blur's texel (x, y)
    const float u = texcoord(x, ax), v = texcoord(y, ay);
    const float kx[9] = {-1.f, 1.f, -1.f, 1.f, 0.f, 0.f, -1.f, 1.f, 0.f};
    const float ky[9] = {-1.f, -1.f, 1.f, 1.f, -1.f, 1.f, 0.f, 0.f, 0.f};
    float4 res = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll 1
    for (int k = 0; k < 9; ++k) {
      float su = u, sv = v, w = 0.250f;
      if (k < 8) {
        su = u + (kx[k] * tsx) * radius;
        sv = v + (ky[k] * tsy) * radius;
        w = k < 4 ? 0.0625f : 0.125f;
      }
      int xa, xb, ya, yb;  // (sample_bilinear_gi on the rows as gi_in holds them)
      float wx, wy;
      wrap_linear(su, ax, xa, xb, wx);
      wrap_linear(sv, ay, ya, yb, wy);
      const float4 t = GI::bilerp(GI::ld_stage(g0_at(xa, ya)), GI::ld_stage(g0_at(xb, ya)),
                                  GI::ld_stage(g0_at(xa, yb)), GI::ld_stage(g0_at(xb, yb)), wx, wy);
      res.x = res.x + t.x * w;
      res.y = res.y + t.y * w;
      res.z = res.z + t.z * w;
      res.w = res.w + t.w * w;
    }
    return GI::RT::blend_black(res);
  };
  auto gi_at = [&](int x, int y) {  // k_blur_copyback's texel (x, y), as it reads back
    int xa, xb, ya, yb;
    float wx, wy;
    wrap_linear(texcoord(x, ax), ax, xa, xb, wx);
    wrap_linear(texcoord(y, ay), ay, ya, yb, wy);
    const float4 sm = GI::RT::bilerp(blur_at(xa, ya), blur_at(xb, ya), blur_at(xa, yb), blur_at(xb, yb), wx, wy);
    return GI::round(GI::blend(sm, GI::ld(g0_at(x, y))));
  };
  for (int j = row0 + blockIdx.y * 4 + (threadIdx.x >> 6); j < row1; j += 4 * (int)gridDim.y) {
    const size_t o = (size_t)(strip ? j - m0 : j) * c.pitch + i;
    blur_out[o] = blur_at(i, j);
    GI::st(&gi_out[o], gi_at(i, j));
    if constexpr (MERGE) {  // k_merge (cascade == screen)
      int xa, xb, ya, yb;
      float wx, wy;
      wrap_linear(texcoord(i, Axis{s.W, s.powW}), ax, xa, xb, wx);
      wrap_linear(texcoord(j, Axis{s.H, s.powH}), ay, ya, yb, wy);
      const float4 g = GI::bilerp(gi_at(xa, ya), gi_at(xb, ya), gi_at(xa, yb), gi_at(xb, yb), wx, wy);
      const size_t so = (size_t)j * s.pitch + i, mo = (size_t)(j - m0) * s.pitch + i;
      const float4 col = color_in[so];
      const float4 src = make_float4(fminf(col.x + g.x, 1.0f), fminf(col.y + g.y, 1.0f), fminf(col.z + g.z, 1.0f), col.w);
      const float4 t = GI::RT::blend_black(src);
      temp[mo] = t;
      color_out[mo] = GI::RT::blend(t, col);
    }
  }
}

hipError_t launch_blur_exact(const BlurArgs &a, ScreenDims s, CascadeDims c, hipStream_t st) {
  if (c.gi_u8 || !(c.powW && c.powH) || (a.merge && !(s.W == c.CW && s.H == c.CH))) return hipErrorInvalidValue;
  int row0 = a.row0, row1 = a.row1;
  clamp_rows(c.CH, row0, row1);
  if (row0 >= row1) return hipSuccess;
  // (the merge outputs, and blur_out / gi_out when a.strip, start at row m0 and end at m1)
  const int m1 = a.m1 < 0 ? s.H : a.m1;
  if ((a.merge || a.strip) && (row0 < a.m0 || row1 > m1)) return hipErrorInvalidValue;
  const int g0 = a.gn <= 0 ? 0 : a.g0, gn = a.gn <= 0 ? c.CH : a.gn;
  const dim3 grid(ceil_div(c.CW, 64), min(ceil_div(row1 - row0, 4), 32));  // (k_blur_exact strides over the rows)
  const unsigned *flag = a.flag;
  with_gi<false>(c, [&](auto gi) {
    using GI = decltype(gi);
#define RC2DGI_BLUR_EXACT(MV)                                                                                \
  hipLaunchKernelGGL((k_blur_exact<MV, GI>), grid, dim3(256), 0, st, flag, a.epoch, tex<GI>(a.gi_in), a.blur_out, \
                     tex<GI>(a.gi_out), c, a.radius, a.color_in, a.temp, a.color_out, s, row0, row1, a.m0,        \
                     (int)a.strip, g0, gn)
    if (a.merge) RC2DGI_BLUR_EXACT(true); else RC2DGI_BLUR_EXACT(false);
#undef RC2DGI_BLUR_EXACT
  });
  return hipGetLastError();
}

}  // namespace rc2dgi
