// rc2dgi_shapes.hip -- rc2dgi_shapes_device: a device-resident list of rectangles, circles, triangles, thick lines and
// ellipses painted into an input texture.  rc2dgi_paint_device's sequence of kernels per batch on the
// same working memory, with a set-up and a binning pass of its own:
//   k_shapes_setup      one lane a shape (shapes_setup_record, rc2dgi_shapes_setup.h, the text rc2dgi_gradients.hip
//                       shares): the eight words, the refusal test of its kind (a refused shape gets no
//                       triangles and is counted), the kind's vertex list in the header's float operations, then
//                       paint_dev_window / paint_dev_emit (rc2dgi_paint_setup.h) into the PaintPrim / PaintTri records
//                       k_paint_dev_raster reads, 36 triangle slots a shape.  RECT and CIRCLE are k_paint_dev_setup's
//                       arithmetic term for term.
//   k_shapes_bin        one wave a shape, lanes over the tiles of its clipped box: bit k of a tile's mask is set only
//                       if some triangle of the shape is not "out" on the pixel centres of tile and box
//                       (paint_tri_out, rc2dgi_tile_test.h).  A rejected tile holds no centre the shape covers, so the
//                       raster's result cannot depend on the rejection; or-ing bits gives the same words in any order.
//                       The shape's triangles are staged in LDS (2304 bytes a wave); a box of more than 64 tiles is
//                       walked in blocks of 8 x 8 tiles, each tested as one rectangle first.
//   k_paint_dev_raster  unchanged (paint_dev_enqueue_raster).
//   k_paint_dev_finish  unchanged (paint_dev_enqueue_finish).
// What is read from the list becomes an index only after the refusal test and the clip of the pixel box to the target;
// the count is clamped by min(max(*count_dev, 0), n).  The unit is built with -ffp-contract=off.
#include "rc2dgi_shapes.h"

#include "rc2dgi_device.h"
#include "rc2dgi_paint_raster.h"
#include "rc2dgi_paint_setup.h"
#include "rc2dgi_shapes_setup.h"
#include "rc2dgi_tile_test.h"

#include <algorithm>

namespace rc2dgi {

namespace {

__global__ __launch_bounds__(256) void k_shapes_setup(const unsigned *__restrict__ list, int n,
                                                      const int *__restrict__ count_dev, int base, int batch,
                                                      PaintPrim *__restrict__ prims, PaintTri *__restrict__ tris,
                                                      unsigned *__restrict__ counters, PaintXform xf, PaintCircle tab) {
  shapes_setup_record<8, false>(list, n, count_dev, base, batch, prims, tris, counters, xf, tab);
}

__global__ __launch_bounds__(256) void k_shapes_bin(const PaintPrim *__restrict__ prims,
                                                    const PaintTri *__restrict__ tris, int n,
                                                    const int *__restrict__ count_dev, int base, int batch,
                                                    unsigned *__restrict__ masks, int tiles_x, int th_shift) {
  __shared__ PaintTri s_tri[4][kPaintDevTris];  // a wave's shape: its triangles, read at one address by every lane
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, k = blockIdx.x * 4 + wave;
  PaintPrim p{};
  if (k < paint_dev_batch(count_dev, n, base, batch)) p = prims[k];
  const int ntri = min(p.ntri, kPaintDevTris);  // (the set-up's count, at most 36; 0: nothing to bin)
  if (lane < ntri) s_tri[wave][lane] = tris[p.tri0 + lane];
  __syncthreads();  // (every wave of the workgroup arrives: none has left yet)
  if (ntri <= 0) return;
  // the box is clipped to the target: every tile index below names a tile of the target
  const int tx0 = p.x0 >> 6, tx1 = p.x1 >> 6, ty0 = p.y0 >> th_shift, ty1 = p.y1 >> th_shift;
  const int nx = tx1 - tx0 + 1, ny = ty1 - ty0 + 1;
  const int stride = batch >> 5;
  const unsigned bit = 1u << (k & 31);
  // no pixel centre of the tiles [txa, txb] x [tya, tyb] and the box can be covered: every triangle is out there
  auto out = [&](int txa, int txb, int tya, int tyb) {
    const long long X0 = 256LL * max(txa << 6, p.x0) + 128, X1 = 256LL * min((txb << 6) + 63, p.x1) + 128;
    const long long Y0 = 256LL * max(tya << th_shift, p.y0) + 128,
                    Y1 = 256LL * min(((tyb + 1) << th_shift) - 1, p.y1) + 128;
    bool keep = false;
    for (int q = 0; q < ntri && !keep; ++q) keep = !paint_tri_out(s_tri[wave][q], X0, Y0, X1, Y1);
    return !keep;
  };
  auto tile = [&](int tx, int ty) {
    if (!out(tx, tx, ty, ty)) atomicOr(&masks[((size_t)ty * tiles_x + tx) * stride + (k >> 5)], bit);
  };
  if (nx * ny <= 64) {  // a lane a tile
    if (lane < nx * ny) tile(tx0 + lane % nx, ty0 + lane / nx);
    return;
  }
  // a larger box: the same test on blocks of 8 x 8 tiles first, a lane a block; then, kept block by kept block, a lane
  // a tile.  A block that is out holds only tiles that are out, so the bits set are those of the tile-by-tile walk.
  const int bx = (nx + 7) >> 3, nblk = bx * ((ny + 7) >> 3);
  for (int b0 = 0; b0 < nblk; b0 += 64) {
    const int b = b0 + lane;
    bool kept = false;
    if (b < nblk) {
      const int cx = tx0 + (b % bx) * 8, cy = ty0 + (b / bx) * 8;
      kept = !out(cx, min(cx + 7, tx1), cy, min(cy + 7, ty1));
    }
    unsigned long long m = __ballot(kept);
    while (m) {  // (m is the same in every lane)
      const int bb = b0 + __ffsll(m) - 1;
      m &= m - 1;
      const int tx = tx0 + (bb % bx) * 8 + (lane & 7), ty = ty0 + (bb / bx) * 8 + (lane >> 3);
      if (tx <= tx1 && ty <= ty1) tile(tx, ty);
    }
  }
}

}  // namespace

void shapes_enqueue_bin(const void *prims, const void *tris, int n, const int *count_dev, int base, int nb,
                        const PaintDevPlan &plan, unsigned *masks, hipStream_t st) {
  int th_shift = 0;
  while ((1 << th_shift) < plan.tile_h) ++th_shift;
  hipLaunchKernelGGL(k_shapes_bin, dim3((nb + 3) / 4), dim3(256), 0, st, static_cast<const PaintPrim *>(prims),
                     static_cast<const PaintTri *>(tris), n, count_dev, base, plan.batch, masks, plan.tiles_x, th_shift);
}

hipError_t shapes_device(float4 *dst, int W, int H, int pitch, bool u8, const unsigned char *clear,
                         const void *shapes_dev, int n, const void *count_dev, void *status_dev, PaintDevBuffers &buf,
                         hipStream_t st) {
  const PaintDevPlan &plan = buf.plan;
  hipError_t e = hipSuccess;
  if (!buf.work) {  // the one place the call may wait: the first call's allocation (shared with the other lists)
    e = hipMalloc(reinterpret_cast<void **>(&buf.work), plan.bytes);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(buf.work, 0, plan.bytes, st);
    if (e != hipSuccess) return e;
  }
  unsigned *counters = reinterpret_cast<unsigned *>(buf.work);
  PaintPrim *prims = reinterpret_cast<PaintPrim *>(buf.work + plan.off_prims);
  PaintTri *tris = reinterpret_cast<PaintTri *>(buf.work + plan.off_tris);
  unsigned *masks = reinterpret_cast<unsigned *>(buf.work + plan.off_masks);
  const int *cnt = static_cast<const int *>(count_dev);
  PaintCircle tab;
  paint_circle_table(tab.c, tab.s);
  // to_window's constants (rc2dgi_paint.hip), evaluated here as it evaluates them
  const PaintXform xf{2.0f / (float)W, 2.0f / (float)(-H), (float)W * 0.5f, (float)H * 0.5f, W, H};
  const float4 cl = paint_dev_clear(clear, u8);
  // the batches follow each other on the stream: batch b + 1 blends over what batch b left, so the draw order holds
  const int batches = n == 0 ? (clear ? 1 : 0) : (n + plan.batch - 1) / plan.batch;
  for (int b = 0; b < batches; ++b) {
    const int base = b * plan.batch, nb = std::min(plan.batch, n - base);
    if (nb > 0) {
      hipLaunchKernelGGL(k_shapes_setup, dim3((nb + 255) / 256), dim3(256), 0, st,
                         static_cast<const unsigned *>(shapes_dev), n, cnt, base, plan.batch, prims, tris, counters, xf,
                         tab);
      shapes_enqueue_bin(prims, tris, n, cnt, base, nb, plan, masks, st);
    }
    paint_dev_enqueue_raster(dst, W, H, pitch, u8, clear && b == 0, cl, prims, tris, masks, n, cnt, base, plan, st);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (n > 0 || status_dev) {
    paint_dev_enqueue_finish(counters, cnt, n, static_cast<int *>(status_dev), st);
    e = hipGetLastError();
  }
  return e;
}

}  // namespace rc2dgi
