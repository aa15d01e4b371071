// rc2dgi_present.hip -- the display frame composed on the device (include/rc2dgi.h, rc2dgi_compose).
//
// The reference ends its frame by drawing colorRT to the window and seven 100 x 100 debug thumbnails over it
// (RC2DGI.cs:135-165, DrawTexturePro with a negative source height, 435-448).  k_present restates those draws for
// a list of views: every window pixel starts as the clear colour and takes, view by view, the view's sampled texel
// and then its border colour, each blended in 8 bits as the RGBA8 passes blend (GiU8::blend, rc2dgi_device.h).
// A texel is decoded from the texture's stored format to the value rc2dgi_download returns for it.
//
// A lane owns four consecutive pixels of one row (one 16-byte store; a wave covers 256 pixels of a row, a workgroup
// 1024).  Where those four are covered by exactly one view and that view is a 1:1 POINT view of float4 or RGBA8
// texels -- the main blit -- the lane loads its four texels (64 contiguous bytes of a float4 texture) and blends
// them over the clear colour.  The test is made once for the wave's 256 pixels with scalar operands; only a wave
// that fails it (a thumbnail, a border or the window's edge crosses it) repeats it per lane, and the lanes that fail
// that too walk the view list per pixel.  The float4 loads are plain: the blit reads colorRT right after the
// merge wrote it, and non-temporal loads (ntload4) measured slower in an A/B of two builds, alternating runs
// (4096^2: 87 us against 58 us, 1200x900: 14 against 9.5; profiles/present/nt_ab.json).
#include "rc2dgi_present.h"
#include "rc2dgi_device.h"

namespace rc2dgi {

namespace {

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

// the value of texel (i, j), 0 <= i < nx, 0 <= j < ny, as rc2dgi_download returns it
__device__ __forceinline__ float4 present_texel(const PresentView &v, int i, int j) {
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

// texture(T, (u, v)) of a view: POINT, or LINEAR with the bilerp of the texture's storage
__device__ __forceinline__ float4 present_sample(const PresentView &v, float tu, float tv) {
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

// The plain-blit test for pixels [x0, x1) of row py: exactly one view's clipped rectangle meets them, and they lie
// inside that view's blit rectangle.  Returns the view's source in `f` (k is uniform, so the view fields are scalar
// loads; x0 / x1 may be per lane).
struct PresentBlit {
  const void *src;
  int pitch, u8, x, y, h;
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
  }
  return hits == 1 && inside;
}

__global__ __launch_bounds__(256) void k_present(const PresentArgs a, unsigned char *__restrict__ dst, int pitch_bytes,
                                                 int vec_ok) {
  const int px0 = (int)(blockIdx.x * 256u + threadIdx.x) * 4, py = (int)blockIdx.y;
  const int wx0 = __builtin_amdgcn_readfirstlane(px0);  // the wave's pixels: [wx0, wx0 + 256) of row py
  if (wx0 >= a.out_w) return;
  const int wx1 = min(wx0 + 256, a.out_w);
  unsigned o[4];
  PresentBlit f;
  // (a wave whose last group is cut by the window's edge decides per lane: x1 - x0 is a multiple of 4 below)
  bool blit = (wx1 - wx0) % 4 == 0 && present_blit(a, wx0, wx1, py, f);
  if (px0 >= a.out_w) return;
  if (!blit) blit = px0 + 4 <= a.out_w && present_blit(a, px0, px0 + 4, py, f);
  if (blit) {
    // 0 <= i and i + 3 < w = nx, 0 <= j < h = ny: the four pixels lie inside the 1:1 view
    const int i = px0 - f.x, j = f.h - 1 - (py - f.y);
    const size_t at = (size_t)j * f.pitch + i;
    if (f.u8) {
      const unsigned *p = static_cast<const unsigned *>(f.src) + at;
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = blend8(p[q], a.clear);  // (q8 of a texel k * (1/255) is k)
    } else {
      const float4 *p = static_cast<const float4 *>(f.src) + at;
      float4 t[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) t[q] = p[q];
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = blend8(GiU8::pack(t[q]), a.clear);
    }
  } else {
    for (int q = 0; q < 4; ++q) {
      const int px = px0 + q;
      unsigned d = a.clear;
      if (px < a.out_w) {
        for (int k = 0; k < a.n; ++k) {
          const PresentView &v = a.v[k];
          // (wrapping differences: 0 <= px - x < w exactly when the unsigned difference is below w)
          const unsigned i = (unsigned)px - (unsigned)v.x, jj = (unsigned)py - (unsigned)v.y;
          if (i >= (unsigned)v.w || jj >= (unsigned)v.h) continue;
          const int j = v.h - 1 - (int)jj;
          const float tu = ((float)(int)i + 0.5f) / (float)v.w, tv = ((float)j + 0.5f) / (float)v.h;
          d = blend8(GiU8::pack(present_sample(v, tu, tv)), d);
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

}  // namespace

hipError_t launch_present(const PresentArgs &a, void *dst, int pitch_bytes, hipStream_t st) {
  const int groups = (a.out_w + 3) / 4;
  const dim3 grid((unsigned)((groups + 255) / 256), (unsigned)a.out_h);
  const int vec_ok = (reinterpret_cast<uintptr_t>(dst) % 16 == 0 && pitch_bytes % 16 == 0) ? 1 : 0;
  hipLaunchKernelGGL(k_present, grid, dim3(256), 0, st, a, static_cast<unsigned char *>(dst), pitch_bytes, vec_ok);
  return hipGetLastError();
}

}  // namespace rc2dgi
