// rc2dgi_write.hip -- an image into a rectangle of an input texture (include/rc2dgi.h, rc2dgi_write /
// rc2dgi_write_device): k_read the other way.
//
// k_write: a lane owns one pixel column of kWriteRows image rows.  Adjacent lanes take adjacent pixels, so a wave
// loads 64 consecutive pixels of a source row (1 KiB of RGBA32F, 512 bytes of RGBA16F, 256 of RGBA8: one dwordx4,
// dwordx2 or dword a lane, the source and its pitch being multiples of a pixel) and stores 64 consecutive texels, one
// aligned dwordx4 a lane: the texture is float4 in every storage mode and its pitch is in texels.  Rows of up to 256
// pixels are packed 256 / lr rows a pass (lr the power of two >= w), wider ones are walked by blockIdx.x, as k_read
// packs its segments.  All of a lane's loads -- the kWriteRows pixels and, with the blend, the kWriteRows texels
// under them -- are issued before the first conversion, unconditionally and at addresses clamped into the rectangle;
// a lane outside it drops what it loaded and stores nothing.  RC2DGI_WRITE_FLIP is the sign of the row step.  The
// kernel is specialised on the source format (a template argument) and on the storage kind and the blend flag (a
// uniform switch into templates), as k_read and k_hist are.  No LDS, no scratch.
//
// RGBA16F is the hardware's half -> float conversion (v_cvt_f32_f16), exact for every half, subnormals included: that
// needs the kernel's f16 denormal mode to keep them, hipcc's default (rc2dgi_read.hip relies on it for the other
// direction); tests/test_write_gpu.py widens every half.
#include "rc2dgi_write.h"

#include "rc2dgi_device.h"

namespace rc2dgi {

namespace {

// (WritePixel and write_value, the value a pixel becomes, are in rc2dgi_write.h: rc2dgi_sprites.hip shares them)

// the rows and pixels of one workgroup; a row gets 1 << lsh lanes (lsh at most 8)
template <bool U8, bool BLEND, int FMT>
__device__ __forceinline__ void write_block(const WriteArgs &a, int lsh) {
  typedef typename WritePixel<FMT>::T P;
  constexpr int PXB = read_pixel_bytes(FMT);
  const int tid = (int)threadIdx.x, lr = 1 << lsh, gr = 256 >> lsh;
  const int i = (int)blockIdx.x * lr + (tid & (lr - 1));
  const int row0 = (int)blockIdx.y * (gr * kWriteRows) + (tid >> lsh);
  const int ic = min(i, a.w - 1);

  P p[kWriteRows];
  float4 d[kWriteRows];
  float4 *out[kWriteRows];
#pragma unroll
  for (int k = 0; k < kWriteRows; ++k) {
    const int jr = min(row0 + k * gr, a.rows - 1);
    p[k] = *reinterpret_cast<const P *>(a.src + (size_t)jr * a.pitch + (size_t)ic * PXB);
    out[k] = a.dst + (size_t)(a.y0 + a.ystep * jr) * (size_t)a.dpitch + (size_t)(a.x + ic);
    if (BLEND) d[k] = *out[k];
  }
  // Every lane converts what it loaded (the conversions read no memory) and only the store is conditional.  hipcc
  // still moves the loads of row 0 under that row's condition, the one block no store precedes; they stay ahead of
  // the first s_waitcnt, so all of a lane's loads are in flight before the first conversion.
#pragma unroll
  for (int k = 0; k < kWriteRows; ++k) {
    float4 v = write_value<U8, FMT>(p[k]);
    if (BLEND) v = U8 ? GiU8::blend(v, d[k]) : blend(v, d[k]);
    if (i < a.w && row0 + k * gr < a.rows) *out[k] = v;
  }
}

template <int FMT>
__global__ __launch_bounds__(256) void k_write(const WriteArgs a, const int lsh, const int mode) {
  switch (mode) {  // (uniform) bit 0: RGBA8_COMPAT storage, bit 1: the blend
    case 0: write_block<false, false, FMT>(a, lsh); break;
    case 1: write_block<true, false, FMT>(a, lsh); break;
    case 2: write_block<false, true, FMT>(a, lsh); break;
    default: write_block<true, true, FMT>(a, lsh); break;
  }
}

}  // namespace

hipError_t launch_write(const WriteArgs &a, int format, bool u8, bool blend, hipStream_t st) {
  int lsh = 0;
  while (lsh < 8 && (1 << lsh) < a.w) ++lsh;
  const int rows_wg = (256 >> lsh) * kWriteRows;
  const dim3 grid((unsigned)((a.w + (1 << lsh) - 1) >> lsh), (unsigned)((a.rows + rows_wg - 1) / rows_wg));
  const int mode = (u8 ? 1 : 0) | (blend ? 2 : 0);
  switch (format) {
    case RC2DGI_FMT_RGBA32F: hipLaunchKernelGGL(k_write<RC2DGI_FMT_RGBA32F>, grid, dim3(256), 0, st, a, lsh, mode); break;
    case RC2DGI_FMT_RGBA16F: hipLaunchKernelGGL(k_write<RC2DGI_FMT_RGBA16F>, grid, dim3(256), 0, st, a, lsh, mode); break;
    case RC2DGI_FMT_RGBA8: hipLaunchKernelGGL(k_write<RC2DGI_FMT_RGBA8>, grid, dim3(256), 0, st, a, lsh, mode); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace rc2dgi
