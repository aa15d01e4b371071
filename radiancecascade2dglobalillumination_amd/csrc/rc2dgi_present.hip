// rc2dgi_present.hip -- the display frame composed on the device (include/rc2dgi.h, rc2dgi_compose).
//
// The reference ends its frame by drawing colorRT to the window and seven 100 x 100 debug thumbnails over it
// (RC2DGI.cs:135-165, DrawTexturePro with a negative source height, 435-448).  k_present restates those draws for
// a list of views: every window pixel starts as the clear colour and takes, view by view, the view's sampled texel
// and then its border colour, each blended in 8 bits as the RGBA8 passes blend (GiU8::blend, rc2dgi_device.h).
// A texel is decoded from the texture's stored format to the value rc2dgi_download returns for it (present_texel /
// present_sample, rc2dgi_texel.h, shared with the point samples of rc2dgi_query.hip).
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
#include "rc2dgi_present_dev.h"
#include "rc2dgi_texel.h"

namespace rc2dgi {

namespace {

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
