// rc2dgi_gradients.hip -- rc2dgi_gradients_device: a device-resident list of gradient shapes -- rectangles, circles,
// triangles, thick lines and ellipses with a colour a vertex and an HDR gain -- painted into an input texture
// (DESIGN.md §23).  rc2dgi_shapes_device's sequence of kernels per batch on the same working memory:
//   k_gradients_setup   shapes_setup_record<12, true> (rc2dgi_shapes_setup.h), the text of k_shapes_setup on the
//                       48-byte record: the same refusal test and vertex lists, the gain's test besides, and each
//                       triangle tagged with its vertices' colours BEFORE the counter-clockwise swap and the zero-area
//                       drop (PaintTri::pad, kGradSwapped); the gain's bits go to PaintPrim::pad0.  The raster reads
//                       nothing of the caller's list.
//   k_shapes_bin        unchanged (shapes_enqueue_bin): the tags sit in words it does not read.
//   k_gradients_raster  k_paint_dev_raster's shape -- one workgroup a 64 x tile_h tile, the tile's mask in registers,
//                       the readlane walk in draw order -- with grad_covers / grad_colour (rc2dgi_gradient_interp.h:
//                       the first covering triangle, its three edge values, the interpolation) where the flat raster
//                       has paint_covered and p.color.
//   k_paint_dev_finish  unchanged (paint_dev_enqueue_finish).
// What is read from the list becomes an index only after the refusal test and the clip of the pixel box to the target;
// colour bytes and the gain never become an address.  The unit is built with -ffp-contract=off.
#include "rc2dgi_gradients.h"

#include "rc2dgi_device.h"
#include "rc2dgi_gradient_interp.h"
#include "rc2dgi_paint_raster.h"
#include "rc2dgi_paint_setup.h"
#include "rc2dgi_shapes.h"
#include "rc2dgi_shapes_setup.h"

#include <algorithm>

namespace rc2dgi {

namespace {

__global__ __launch_bounds__(256) void k_gradients_setup(const unsigned *__restrict__ list, int n,
                                                         const int *__restrict__ count_dev, int base, int batch,
                                                         PaintPrim *__restrict__ prims, PaintTri *__restrict__ tris,
                                                         unsigned *__restrict__ counters, PaintXform xf,
                                                         PaintCircle tab) {
  shapes_setup_record<12, true>(list, n, count_dev, base, batch, prims, tris, counters, xf, tab);
}

__global__ __launch_bounds__(256) void k_gradients_raster(float4 *__restrict__ dst, int W, int H, int pitch,
                                                          int clear_on, float4 clear,
                                                          const PaintPrim *__restrict__ prims,
                                                          const PaintTri *__restrict__ tris, unsigned *__restrict__ masks,
                                                          int n, const int *__restrict__ count_dev, int base, int batch,
                                                          int tile_h, int u8) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int mb = paint_dev_batch(count_dev, n, base, batch);
  const int nwords = (mb + 31) >> 5, stride = batch >> 5;
  unsigned *mask = masks + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * stride;
  unsigned wd[4];
  bool any = false;
#pragma unroll
  for (int q = 0; q < 4; ++q) {  // word q * 64 + lane: below nwords <= stride, so inside the tile's mask
    const int wi = q * 64 + lane;
    wd[q] = wi < nwords ? mask[wi] : 0u;
    any = any || __ballot(wd[q] != 0u) != 0ull;
  }
  if (!any && !clear_on) return;  // (every wave loaded the same words: the whole workgroup leaves)
  if (any) {
    __syncthreads();  // every wave holds the mask: the words found set go back to zero for the next batch
    if (wave == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (wd[q] != 0u) mask[q * 64 + lane] = 0u;
    }
  }
  const int i = blockIdx.x * 64 + lane;
  const long long X = 256LL * i + 128;
  for (int r = 0; r < tile_h; r += 4) {
    const int j = blockIdx.y * tile_h + r + wave;
    if (blockIdx.y * tile_h + r >= H) break;
    const bool in = i < W && j < H;
    const long long Y = 256LL * j + 128;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    bool touched = clear_on != 0;
    if (in) v = clear_on ? clear : dst[(size_t)j * pitch + i];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      unsigned long long nz = __ballot(wd[q] != 0u);
      while (nz) {
        const int l = __ffsll((unsigned long long)nz) - 1;
        nz &= nz - 1;
        unsigned w = (unsigned)__builtin_amdgcn_readlane((int)wd[q], l);  // (l is the same in every lane)
        while (w) {
          const int k = ((q * 64 + l) << 5) + (__ffs(w) - 1);
          w &= w - 1;
          const PaintPrim &p = prims[k];
          if (!in || i < p.x0 || i > p.x1 || j < p.y0 || j > p.y1) continue;
          // grad_first_covering's walk, one grad_covers a step, in a loop the whole wave stays in until each of its
          // lanes has its triangle or the slots run out: u is uniform, so the records come through scalar loads
          long long E[3] = {0, 0, 0};
          unsigned c0 = 0u, c1 = 0u, c2 = 0u;
          const PaintTri *pt = tris + p.tri0;  // (tri0 = k * 36 and ntri <= 36, the set-up's: inside the batch's slots)
          bool found = false;
          for (int u = 0; u < p.ntri; ++u) {
            const PaintTri &tr = pt[u];
            if (!found && grad_covers(tr, X, Y, E)) {
              found = true;
              c0 = tr.pad[0];
              c1 = tr.pad[1];
              c2 = tr.pad[2];
            }
            if (__ballot(!found) == 0ull) break;
          }
          if (found) {  // SRC_ALPHA, ONE_MINUS_SRC_ALPHA, as k_paint blends
            float s[4];
            grad_colour(c0, c1, c2, E, __int_as_float(p.pad0), s);
            const float4 src = make_float4(s[0], s[1], s[2], s[3]);
            v = u8 ? GiU8::blend(src, v) : GiF32::blend(src, v);
            touched = true;
          }
        }
      }
    }
    if (in && touched) dst[(size_t)j * pitch + i] = v;
  }
}

}  // namespace

hipError_t gradients_device(float4 *dst, int W, int H, int pitch, bool u8, const unsigned char *clear,
                            const void *grads_dev, int n, const void *count_dev, void *status_dev,
                            PaintDevBuffers &buf, hipStream_t st) {
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
      hipLaunchKernelGGL(k_gradients_setup, dim3((nb + 255) / 256), dim3(256), 0, st,
                         static_cast<const unsigned *>(grads_dev), n, cnt, base, plan.batch, prims, tris, counters, xf,
                         tab);
      shapes_enqueue_bin(prims, tris, n, cnt, base, nb, plan, masks, st);
    }
    hipLaunchKernelGGL(k_gradients_raster, dim3(plan.tiles_x, plan.tiles_y), dim3(256), 0, st, dst, W, H, pitch,
                       clear && b == 0 ? 1 : 0, cl, static_cast<const PaintPrim *>(prims),
                       static_cast<const PaintTri *>(tris), masks, n, cnt, base, plan.batch, plan.tile_h, (int)u8);
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
