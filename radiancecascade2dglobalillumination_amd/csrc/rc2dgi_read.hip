// rc2dgi_read.hip -- a rectangle of a render texture as an image (include/rc2dgi.h, rc2dgi_read / rc2dgi_read_device).
//
// k_read: a lane owns 16-byte SEGMENTS of output rows -- one RGBA32F pixel, two RGBA16F, four RGBA8 -- and stores a
// whole one as one dwordx4.  The segments of a row are cut at the 16-byte lines of memory, not at the row's first
// pixel: the ABI admits a destination aligned to a pixel only and any pitch that is a multiple of a pixel, so a row of
// RGBA8 may start at byte 4, 8 or 12 of a line and the next row somewhere else.  With `off` the pixels between the
// line's start and the row's, segment s holds pixels [s * G - off, (s + 1) * G - off) of the row, G pixels a segment;
// the first and the last one of a row may hold fewer than G pixels of it, and those store pixel by pixel (a dword or a
// dwordx2 each).  No store touches a byte outside the w pixels of a row.
//
// A lane converts four texels (kReadTexels): G of one row, in 4 / G rows.  All four loads are issued before the first
// conversion, unconditionally and at addresses clamped into the rectangle, as k_reduce_rows and k_hist load; a lane
// without a segment drops what it loaded.  Rows of up to 256 segments are packed 256 / lr rows a pass (lr the power of
// two >= the segments a row can have), wider ones are walked by blockIdx.x.  RC2DGI_READ_FLIP is the sign of the row
// step.  The kernel is specialised on the output format (a template argument) and on the storage kind (a uniform switch
// into a template, so that present_texel's switch folds), as k_hist is.
//
// RGBA16F is the hardware's float -> half conversion (v_cvt_f16_f32 or its packed form): round to nearest even,
// 65520 and up to infinity, results below 2^-14 as subnormals.  That last point needs the kernel's f16 denormal mode
// to keep them, which is hipcc's default for every kernel (.amdhsa_float_denorm_mode_16_64 3, and round mode 0, in
// this unit's assembly); tests/test_read_gpu.py converts every half, every midpoint and its two neighbours.  It is NOT
// GiF16::pack (rc2dgi_device.h), which rounds toward zero as the F16 storage does.
#include "rc2dgi_read.h"

#include "rc2dgi_device.h"
#include "rc2dgi_texel.h"

namespace rc2dgi {

namespace {

typedef _Float16 h2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned half2_rne(float a, float b) {
  const h2_t h = {(_Float16)a, (_Float16)b};
  return __builtin_bit_cast(unsigned, h);
}

// the pixel of a texel in the output format: PXB / 4 dwords from o[0] on
template <int FMT>
__device__ __forceinline__ void read_pack(float4 v, unsigned *o) {
  if (FMT == RC2DGI_FMT_RGBA32F) {
    o[0] = __float_as_uint(v.x);
    o[1] = __float_as_uint(v.y);
    o[2] = __float_as_uint(v.z);
    o[3] = __float_as_uint(v.w);
  } else if (FMT == RC2DGI_FMT_RGBA16F) {
    o[0] = half2_rne(v.x, v.y);
    o[1] = half2_rne(v.z, v.w);
  } else {
    o[0] = GiU8::pack(v);
  }
}

// the rows and segments of one workgroup, for a texture whose storage kind is the constant KIND; a row gets
// 1 << lsh lanes (lsh at most 8)
template <int KIND, int FMT>
__device__ __forceinline__ void read_block(TexSource t, const ReadArgs &a, int lsh) {
  t.kind = KIND;
  constexpr int PXB = read_pixel_bytes(FMT), G = 16 / PXB, NR = kReadTexels / G;
  const int tid = (int)threadIdx.x, lr = 1 << lsh, gr = 256 >> lsh;
  const int s = (int)blockIdx.x * lr + (tid & (lr - 1));
  const int row0 = (int)blockIdx.y * (gr * NR) + (tid >> lsh);

  float4 v[NR][G];
  int p0[NR];
  unsigned char *line[NR];  // the 16-byte line of the segment (before the row's first pixel where p0 < 0: not stored to)
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    const int jr = min(row0 + k * gr, a.rows - 1);
    unsigned char *row = a.dst + (size_t)jr * a.pitch;
    const int off = (int)(reinterpret_cast<uintptr_t>(row) & 15u) / PXB;  // (0 where a pixel is a line)
    p0[k] = s * G - off;
    line[k] = row - (size_t)off * PXB + (size_t)s * 16;
    const int ty = a.y0 + a.ystep * jr;
#pragma unroll
    for (int q = 0; q < G; ++q) v[k][q] = present_texel(t, a.x + min(max(p0[k] + q, 0), a.w - 1), ty);
  }
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    if (row0 + k * gr >= a.rows || p0[k] >= a.w) continue;  // (p0 + G > 0 always: off < G)
    unsigned o[4];
#pragma unroll
    for (int q = 0; q < G; ++q) read_pack<FMT>(v[k][q], o + q * (PXB / 4));
    if (G == 1 || (p0[k] >= 0 && p0[k] + G <= a.w)) {  // (a segment of one pixel is whole: 0 <= p0 < w here)
      *reinterpret_cast<uint4 *>(line[k]) = make_uint4(o[0], o[1], o[2], o[3]);
      continue;
    }
    // the head or the tail of a row: the pixels of the segment that are pixels of the row, one store each
#pragma unroll
    for (int q = 0; q < G; ++q) {
      if (p0[k] + q < 0 || p0[k] + q >= a.w) continue;
      if (PXB == 8) *reinterpret_cast<uint2 *>(line[k] + q * 8) = make_uint2(o[2 * q], o[2 * q + 1]);
      else *reinterpret_cast<unsigned *>(line[k] + q * 4) = o[q];
    }
  }
}

template <int FMT>
__global__ __launch_bounds__(256) void k_read(const TexSource t, const ReadArgs a, const int lsh) {
  switch (t.kind) {  // (uniform)
    case PK_F32: read_block<PK_F32, FMT>(t, a, lsh); break;
    case PK_F16: read_block<PK_F16, FMT>(t, a, lsh); break;
    case PK_U8: read_block<PK_U8, FMT>(t, a, lsh); break;
    case PK_JUMP: read_block<PK_JUMP, FMT>(t, a, lsh); break;
    case PK_JUMP8: read_block<PK_JUMP8, FMT>(t, a, lsh); break;
    case PK_DIST: read_block<PK_DIST, FMT>(t, a, lsh); break;
    case PK_DIST8: read_block<PK_DIST8, FMT>(t, a, lsh); break;
    default: read_block<PK_CONST, FMT>(t, a, lsh); break;
  }
}

}  // namespace

hipError_t launch_read(const TexSource &t, const ReadArgs &a, int format, hipStream_t st) {
  const int g = 16 / read_pixel_bytes(format), nr = kReadTexels / g;
  const int nseg = (a.w + 2 * (g - 1)) / g;  // segments of a row at most: its first pixel may be a line's last
  int lsh = 0;
  while (lsh < 8 && (1 << lsh) < nseg) ++lsh;
  const int rows_wg = (256 >> lsh) * nr;
  const dim3 grid((unsigned)((nseg + (1 << lsh) - 1) >> lsh), (unsigned)((a.rows + rows_wg - 1) / rows_wg));
  switch (format) {
    case RC2DGI_FMT_RGBA32F: hipLaunchKernelGGL(k_read<RC2DGI_FMT_RGBA32F>, grid, dim3(256), 0, st, t, a, lsh); break;
    case RC2DGI_FMT_RGBA16F: hipLaunchKernelGGL(k_read<RC2DGI_FMT_RGBA16F>, grid, dim3(256), 0, st, t, a, lsh); break;
    case RC2DGI_FMT_RGBA8: hipLaunchKernelGGL(k_read<RC2DGI_FMT_RGBA8>, grid, dim3(256), 0, st, t, a, lsh); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace rc2dgi
