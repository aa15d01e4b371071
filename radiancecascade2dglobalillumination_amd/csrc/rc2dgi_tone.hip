// rc2dgi_tone.hip -- the display frame with an exposure and a tone curve per view (include/rc2dgi.h,
// rc2dgi_compose_tone / rc2dgi_compose_tone_device).
//
// k_present_tone is k_present (rc2dgi_present.hip) with one step changed: where a draw forms its 8-bit source from the
// sampled float4, the colour channels go through T(c * E) of the view -- E its exposure, one fp32 multiply, T either
// q8 or bin() over the 255 edges of the view's curve slot -- and alpha stays q8(a).  The lane-owns-four-pixels shape,
// the wave-uniform blit test and the per-pixel view walk are k_present's; rc2dgi_compose keeps k_present itself, which
// holds no tone code.
//
// The curves a call names are staged once a workgroup in LDS, 256 words each: the context's device tables already hold
// them as search trees (rc2dgi_tone.h), word 0 the +inf padding.  bin() is eight dependent LDS reads, k = 2k + (T[k] <=
// v), with no branch around a load: the view (so the curve) is uniform where it is chosen, the values differ per lane.
// Twelve such searches a lane in the blit (four pixels, three channels).
#include "rc2dgi_tone.h"

#include "rc2dgi_device.h"
#include "rc2dgi_present_dev.h"
#include "rc2dgi_texel.h"

namespace rc2dgi {

namespace {

// bin(v) over a staged curve; a NaN fails every comparison and ends at 0
__device__ __forceinline__ unsigned curve_bin(const float *T, float v) {
  unsigned k = 1;
#pragma unroll
  for (int s = 0; s < kCurveLevels; ++s) k = 2u * k + (T[k] <= v ? 1u : 0u);
  return k - (unsigned)kCurveWords;
}

// the 8-bit source of a draw: (T(r E), T(g E), T(b E), q8(a)); cv == 0: T = q8, else the staged curve of slot cv
// (cv is uniform where this is called)
__device__ __forceinline__ unsigned tone_pack(float4 t, float E, int cv, const float *lut) {
  const float r = t.x * E, g = t.y * E, b = t.z * E;
  if (cv == 0) return q8(r) | (q8(g) << 8) | (q8(b) << 16) | (q8(t.w) << 24);
  const float *T = lut + (cv - 1) * kCurveWords;
  return curve_bin(T, r) | (curve_bin(T, g) << 8) | (curve_bin(T, b) << 16) | (q8(t.w) << 24);
}

__global__ __launch_bounds__(256) void k_present_tone(const PresentArgs a, const ToneArgs tn,
                                                      unsigned char *__restrict__ dst, int pitch_bytes, int vec_ok) {
  __shared__ float lut[RC2DGI_MAX_CURVES][kCurveWords];
#pragma unroll
  for (int s = 0; s < RC2DGI_MAX_CURVES; ++s)
    if ((tn.used >> s) & 1u) lut[s][threadIdx.x] = tn.tables[s * kCurveWords + (int)threadIdx.x];
  __syncthreads();
  const int px0 = (int)(blockIdx.x * 256u + threadIdx.x) * 4, py = (int)blockIdx.y;
  const int wx0 = __builtin_amdgcn_readfirstlane(px0);  // the wave's pixels: [wx0, wx0 + 256) of row py
  if (wx0 >= a.out_w) return;
  const int wx1 = min(wx0 + 256, a.out_w);
  unsigned o[4];
  PresentBlit f;
  bool blit = (wx1 - wx0) % 4 == 0 && present_blit(a, wx0, wx1, py, f);
  if (px0 >= a.out_w) return;
  if (!blit) blit = px0 + 4 <= a.out_w && present_blit(a, px0, px0 + 4, py, f);
  if (blit) {
    // 0 <= i and i + 3 < w = nx, 0 <= j < h = ny: the four pixels lie inside the 1:1 view
    const int i = px0 - f.x, j = f.h - 1 - (py - f.y);
    const size_t at = (size_t)j * f.pitch + i;
    const float E = tn.exposure[f.k];
    const int cv = tn.curve[f.k];
    float4 t[4];
    if (f.u8) {
      const unsigned *p = static_cast<const unsigned *>(f.src) + at;
#pragma unroll
      for (int q = 0; q < 4; ++q) t[q] = GiU8::unpack(p[q]);
    } else {
      const float4 *p = static_cast<const float4 *>(f.src) + at;
#pragma unroll
      for (int q = 0; q < 4; ++q) t[q] = p[q];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = blend8(tone_pack(t[q], E, cv, &lut[0][0]), a.clear);
  } else {
    for (int q = 0; q < 4; ++q) {
      const int px = px0 + q;
      unsigned d = a.clear;
      if (px < a.out_w) {
        for (int k = 0; k < a.n; ++k) {
          const PresentView &v = a.v[k];
          const unsigned i = (unsigned)px - (unsigned)v.x, jj = (unsigned)py - (unsigned)v.y;
          if (i >= (unsigned)v.w || jj >= (unsigned)v.h) continue;
          const int j = v.h - 1 - (int)jj;
          const float tu = ((float)(int)i + 0.5f) / (float)v.w, tv = ((float)j + 0.5f) / (float)v.h;
          const int cv = tn.curve[k];
          d = blend8(tone_pack(present_sample(v, tu, tv), tn.exposure[k], cv, &lut[0][0]), d);
          if ((v.border >> 24) != 0u && (i == 0u || i == (unsigned)v.w - 1u || jj == 0u || jj == (unsigned)v.h - 1u))
            d = blend8(v.border, d);
        }
      }
      o[q] = d;
    }
  }
  unsigned char *row = dst + (size_t)py * (size_t)pitch_bytes + (size_t)px0 * 4;
  if (vec_ok && px0 + 4 <= a.out_w) {
    *reinterpret_cast<uint4 *>(row) = make_uint4(o[0], o[1], o[2], o[3]);
  } else {
    for (int q = 0; q < 4; ++q)
      if (px0 + q < a.out_w) reinterpret_cast<unsigned *>(row)[q] = o[q];
  }
}

// dst[i] = chunk.v[i], i < n; zero[i] = 0, i < nzero (grid-stride)
__global__ __launch_bounds__(256) void k_store_table(const TableChunk chunk, int n, float *__restrict__ dst,
                                                     unsigned *__restrict__ zero, size_t nzero) {
  const size_t i0 = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i0 < (size_t)n) dst[i0] = chunk.v[i0];
  for (size_t i = i0; i < nzero; i += (size_t)gridDim.x * 256u) zero[i] = 0u;
}

}  // namespace

hipError_t launch_store_table(const TableChunk &chunk, int n, float *dst, unsigned *zero, size_t nzero, hipStream_t st) {
  const size_t work = nzero > (size_t)n ? nzero : (size_t)n;
  const size_t blocks = (work + 255) / 256;
  const unsigned grid = (unsigned)(blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks));  // (at least n / 256 = 2 blocks)
  hipLaunchKernelGGL(k_store_table, dim3(grid), dim3(256), 0, st, chunk, n, dst, zero, nzero);
  return hipGetLastError();
}

hipError_t launch_present_tone(const PresentArgs &a, const ToneArgs &t, void *dst, int pitch_bytes, hipStream_t st) {
  const int groups = (a.out_w + 3) / 4;
  const dim3 grid((unsigned)((groups + 255) / 256), (unsigned)a.out_h);
  const int vec_ok = (reinterpret_cast<uintptr_t>(dst) % 16 == 0 && pitch_bytes % 16 == 0) ? 1 : 0;
  hipLaunchKernelGGL(k_present_tone, grid, dim3(256), 0, st, a, t, static_cast<unsigned char *>(dst), pitch_bytes,
                     vec_ok);
  return hipGetLastError();
}

}  // namespace rc2dgi
