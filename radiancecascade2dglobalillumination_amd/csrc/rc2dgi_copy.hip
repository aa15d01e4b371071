// rc2dgi_copy.hip -- what moves texels without being a pass of the chain: the upload format conversions and the
// batched device copies of the shard exchanges (gfx950).  A unit of its own: the buffers and group code call
// these, not the frame.
#include "rc2dgi_device.h"
#include "rc2dgi_kernels.h"
#include "rc2dgi_launch.h"

#include <algorithm>

namespace rc2dgi {

// ---------------------------------------------------------------- format conversion
__global__ __launch_bounds__(256) void k_unorm8_to_f32(const unsigned char *__restrict__ src, int src_pitch,
                                                       float4 *__restrict__ dst, int dst_pitch, int W, int H,
                                                       int u8) {
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (i >= W || j >= H) return;
  const uchar4 b = *reinterpret_cast<const uchar4 *>(src + (size_t)j * src_pitch + 4 * (size_t)i);
  dst[(size_t)j * dst_pitch + i] =
      u8 ? make_float4((float)b.x * kInv255, (float)b.y * kInv255, (float)b.z * kInv255, (float)b.w * kInv255)
         : make_float4((float)b.x / 255.0f, (float)b.y / 255.0f, (float)b.z / 255.0f, (float)b.w / 255.0f);
}

hipError_t launch_unorm8_to_f32(const unsigned char *src, int src_pitch_bytes, float4 *dst, int dst_pitch, int W,
                                int H, hipStream_t st, bool u8) {
  hipLaunchKernelGGL(k_unorm8_to_f32, grid2d(W, H), dim3(256), 0, st, src, src_pitch_bytes, dst, dst_pitch, W, H,
                     (int)u8);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_quantize_u8(float4 *__restrict__ buf, int pitch, int W, int H) {
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (i >= W || j >= H) return;
  float4 &v = buf[(size_t)j * pitch + i];
  v = GiU8::unpack(GiU8::pack(v));
}

hipError_t launch_quantize_u8(float4 *buf, int pitch, int W, int H, hipStream_t st) {
  hipLaunchKernelGGL(k_quantize_u8, grid2d(W, H), dim3(256), 0, st, buf, pitch, W, H);
  return hipGetLastError();
}

// ---------------------------------------------------------------- batched device copies
// piece blockIdx.y, 16-byte words strided over the x workgroups
__global__ __launch_bounds__(256) void k_copy_batch(CopyBatch b) {
  if ((int)blockIdx.y >= b.n) return;
  const CopyPiece d = b.p[blockIdx.y];
  const uint4 *__restrict__ src = static_cast<const uint4 *>(d.src);
  uint4 *__restrict__ dst = static_cast<uint4 *>(d.dst);
  const size_t n16 = d.bytes >> 4;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n16; e += (size_t)gridDim.x * 256) dst[e] = src[e];
}

hipError_t launch_copy_batch(const CopyBatch &b, hipStream_t st) {
  if (b.n <= 0) return hipSuccess;
  if (b.n > kCopyBatchMax) return hipErrorInvalidValue;
  size_t most = 0;
  for (int k = 0; k < b.n; ++k) {
    if (!copy_piece_ok(b.p[k].src, b.p[k].dst, b.p[k].bytes)) return hipErrorInvalidValue;
    most = std::max(most, b.p[k].bytes);
  }
  const size_t wg = std::min<size_t>(std::max<size_t>((most / 16 + 255) / 256, 1), 2048);
  hipLaunchKernelGGL(k_copy_batch, dim3((unsigned)wg, (unsigned)b.n), dim3(256), 0, st, b);
  return hipGetLastError();
}

}  // namespace rc2dgi
