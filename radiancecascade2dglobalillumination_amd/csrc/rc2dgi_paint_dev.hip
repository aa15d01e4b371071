// rc2dgi_paint_dev.hip -- rc2dgi_paint_device: the painter of rc2dgi_paint.hip fed from device memory.
//
// The primitive list, and optionally its length, live in device memory; nothing of them is known on the host, so the
// call enqueues a fixed sequence of kernels per batch of the list and returns.  A batch is `batch` primitives
// (PaintDevPlan), a tile 64 x tile_h pixels:
//   k_paint_dev_setup   one lane a primitive: rc2dgi_paint's refusal test (a refused primitive gets no triangles and is
//                       counted), then paint_prims' vertex arithmetic, to_window's snap, the CCW swap, the integer edge
//                       equations and the clipped pixel box, into the PaintPrim / PaintTri records k_paint reads.
//                       Every float operation is one IEEE single operation (__fmul_rn / __fadd_rn: nothing contracts),
//                       the four viewport constants and the 37 cosf / sinf values are the host's, passed as arguments.
//   k_paint_dev_bin     one wave a primitive: bit k of the mask of every tile its box meets, by atomicOr.  Or-ing bits
//                       gives the same words in any order, so the masks do not depend on scheduling.
//   k_paint_dev_raster  one workgroup a tile: each wave loads the tile's mask (a lane holds up to 4 words), a tile with
//                       no bit set and no clear to apply exits before it reads a texel; otherwise the bits are walked in
//                       ascending order -- the draw order -- with k_paint's coverage test and blends.  The workgroup
//                       zeroes the words it found set, so the masks are clear again when the batch is done.
//   k_paint_dev_finish  {m, refused} to the caller's status words; the refusal counter back to zero.
// Everything read from the list is validated before it is used: the kind and the coordinates by the refusal test, the
// count by min(max(*count_dev, 0), n).  Indices derive from the clipped pixel box and from k < batch alone.
#include "rc2dgi_paint.h"
#include "rc2dgi_device.h"
#include "rc2dgi_paint_raster.h"
#include "rc2dgi_paint_setup.h"

#include <algorithm>
#include <climits>

namespace rc2dgi {

namespace {

__global__ __launch_bounds__(256) void k_paint_dev_setup(const unsigned *__restrict__ list, int n,
                                                         const int *__restrict__ count_dev, int base, int batch,
                                                         PaintPrim *__restrict__ prims, PaintTri *__restrict__ tris,
                                                         unsigned *__restrict__ counters, PaintXform xf, PaintCircle tab) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  const int mb = paint_dev_batch(count_dev, n, base, batch);
  bool refused = false;
  if (k < mb) {  // (base + k < m <= n: inside the list)
    const unsigned *q = list + (size_t)(base + k) * 6;
    const int kind = (int)q[0];
    const float x = __uint_as_float(q[1]), y = __uint_as_float(q[2]), w = __uint_as_float(q[3]),
                h = __uint_as_float(q[4]);
    const unsigned rgba = q[5];
    const float lim = 4194304.0f;  // 2^22 pixels: rc2dgi_paint's test, term for term
    const bool rect = kind == RC2DGI_PRIM_RECT, circle = kind == RC2DGI_PRIM_CIRCLE;
    bool ok = (rect || circle) && fabsf(x) < lim && fabsf(y) < lim && fabsf(w) < lim;
    if (rect) ok = ok && fabsf(h) < lim && fabsf(__fadd_rn(x, w)) < lim && fabsf(__fadd_rn(y, h)) < lim;
    if (circle) ok = ok && __fadd_rn(fabsf(x), fabsf(w)) < lim && __fadd_rn(fabsf(y), fabsf(w)) < lim;
    refused = !ok;
    PaintPrim pp{};
    pp.tri0 = k * kPaintDevTris;
    PaintAcc A{tris + (size_t)k * kPaintDevTris, 0, LLONG_MAX, LLONG_MAX, LLONG_MIN, LLONG_MIN};
    if (ok && rect) {  // DrawRectanglePro (rotation 0): TL, BL, BR, TR as (0, 1, 2), (0, 2, 3)
      const float xr = __fadd_rn(x, w), yb = __fadd_rn(y, h);
      const PaintSnap tl = paint_dev_window(x, y, xf), tr = paint_dev_window(xr, y, xf),
                      bl = paint_dev_window(x, yb, xf), br = paint_dev_window(xr, yb, xf);
      paint_dev_emit(A, tl, bl, br);
      paint_dev_emit(A, tl, br, tr);
    } else if (ok) {  // DrawCircleSector(c, r, 0, 360, 36) as 18 quads (c, P(a+20), P(a+10), P(a))
      const float r = w <= 0.0f ? 0.1f : w;
      const PaintSnap c = paint_dev_window(x, y, xf);
      PaintSnap p0 = paint_dev_window(__fadd_rn(x, __fmul_rn(tab.c[0], r)), __fadd_rn(y, __fmul_rn(tab.s[0], r)), xf);
#pragma unroll 1
      for (int s = 0; s < 18; ++s) {
        const int a = 2 * s;
        const PaintSnap p1 = paint_dev_window(__fadd_rn(x, __fmul_rn(tab.c[a + 1], r)),
                                              __fadd_rn(y, __fmul_rn(tab.s[a + 1], r)), xf);
        const PaintSnap p2 = paint_dev_window(__fadd_rn(x, __fmul_rn(tab.c[a + 2], r)),
                                              __fadd_rn(y, __fmul_rn(tab.s[a + 2], r)), xf);
        paint_dev_emit(A, c, p2, p1);
        paint_dev_emit(A, c, p1, p0);
        p0 = p2;
      }
    }
    pp.ntri = A.nt;
    if (pp.ntri > 0) {  // pixels whose centre 256 i + 128 lies in [min, max], clipped to the target
      pp.x0 = (int)max(0LL, -paint_dev_floor_div(-(A.mnx - 128), 256));
      pp.x1 = (int)min((long long)xf.W - 1, paint_dev_floor_div(A.mxx - 128, 256));
      pp.y0 = (int)max(0LL, -paint_dev_floor_div(-(A.mny - 128), 256));
      pp.y1 = (int)min((long long)xf.H - 1, paint_dev_floor_div(A.mxy - 128, 256));
      if (pp.x0 > pp.x1 || pp.y0 > pp.y1) pp.ntri = 0;
    }
    pp.color = make_float4(__fmul_rn((float)(rgba & 255u), kInv255), __fmul_rn((float)((rgba >> 8) & 255u), kInv255),
                           __fmul_rn((float)((rgba >> 16) & 255u), kInv255), __fmul_rn((float)(rgba >> 24), kInv255));
    prims[k] = pp;
  }
  const unsigned long long b = __ballot(refused);  // integer adds: the sum is the same in any order
  if (b != 0 && (threadIdx.x & 63) == 0) atomicAdd(&counters[0], (unsigned)__popcll(b));
}

__global__ __launch_bounds__(256) void k_paint_dev_bin(const PaintPrim *__restrict__ prims, int n,
                                                       const int *__restrict__ count_dev, int base, int batch,
                                                       unsigned *__restrict__ masks, int tiles_x, int th_shift) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= paint_dev_batch(count_dev, n, base, batch)) return;
  const PaintPrim &p = prims[k];
  if (p.ntri <= 0) return;
  // the box is clipped to the target: every tile index below names a tile of the target
  const int tx0 = p.x0 >> 6, tx1 = p.x1 >> 6, ty0 = p.y0 >> th_shift, ty1 = p.y1 >> th_shift;
  const int nx = tx1 - tx0 + 1, cnt = nx * (ty1 - ty0 + 1);
  const int stride = batch >> 5;
  const unsigned bit = 1u << (k & 31);
  for (int t = lane; t < cnt; t += 64) {
    const int ty = ty0 + t / nx, tx = tx0 + t % nx;
    atomicOr(&masks[((size_t)ty * tiles_x + tx) * stride + (k >> 5)], bit);
  }
}

__global__ __launch_bounds__(256) void k_paint_dev_raster(float4 *__restrict__ dst, int W, int H, int pitch,
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
          if (paint_covered(p, tris, X, Y)) {  // SRC_ALPHA, ONE_MINUS_SRC_ALPHA, as k_paint blends
            v = u8 ? GiU8::blend(p.color, v) : GiF32::blend(p.color, v);
            touched = true;
          }
        }
      }
    }
    if (in && touched) dst[(size_t)j * pitch + i] = v;
  }
}

__global__ void k_paint_dev_finish(unsigned *__restrict__ counters, const int *__restrict__ count_dev, int n,
                                   int *__restrict__ status) {
  if (status) {
    status[0] = paint_dev_total(count_dev, n);
    status[1] = (int)counters[0];
  }
  counters[0] = 0u;
}

}  // namespace

PaintDevPlan paint_dev_plan(int W, int H, int code) {
  PaintDevPlan p;
  p.tiles_x = (W + 63) / 64;
  auto mask_bytes = [&] { return (size_t)p.tiles_x * (size_t)((H + p.tile_h - 1) / p.tile_h) * (size_t)(p.batch / 8); };
  if (code != 0) {  // (a "paint_plan" code the knob table accepted)
    p.tile_h = 1 << (code & 255);
    p.batch = 2048 * (code >> 8);
  }
  while (code == 0 && mask_bytes() > kPaintDevMaskBytes) {  // taller tiles first, then shorter batches, then taller tiles
    if (p.tile_h < 16) p.tile_h *= 2;
    else if (p.batch > 2048) p.batch /= 2;
    else p.tile_h *= 2;
  }
  p.tiles_y = (H + p.tile_h - 1) / p.tile_h;
  p.off_prims = kPaintDevHead;
  p.off_tris = p.off_prims + (size_t)p.batch * sizeof(PaintPrim);
  p.off_masks = p.off_tris + (size_t)p.batch * kPaintDevTris * sizeof(PaintTri);
  p.bytes = p.off_masks + mask_bytes();
  return p;
}

float4 paint_dev_clear(const unsigned char *clear, bool u8) {
  if (clear && u8)  // ClearBackground into RGBA8: the texel is c itself, read as c * (1/255)
    return make_float4((float)clear[0] * kInv255, (float)clear[1] * kInv255, (float)clear[2] * kInv255,
                       (float)clear[3] * kInv255);
  if (clear)  // ClearBackground: rlClearColor(c / 255)
    return make_float4((float)clear[0] / 255.0f, (float)clear[1] / 255.0f, (float)clear[2] / 255.0f,
                       (float)clear[3] / 255.0f);
  return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

void paint_dev_enqueue_bin(const void *recs, int n, const int *count_dev, int base, int nb, const PaintDevPlan &plan,
                           unsigned *masks, hipStream_t st) {
  int th_shift = 0;
  while ((1 << th_shift) < plan.tile_h) ++th_shift;
  hipLaunchKernelGGL(k_paint_dev_bin, dim3((nb + 3) / 4), dim3(256), 0, st, static_cast<const PaintPrim *>(recs), n,
                     count_dev, base, plan.batch, masks, plan.tiles_x, th_shift);
}

void paint_dev_enqueue_raster(float4 *dst, int W, int H, int pitch, bool u8, bool clear_on, float4 clear,
                              const void *prims, const void *tris, unsigned *masks, int n, const int *count_dev,
                              int base, const PaintDevPlan &plan, hipStream_t st) {
  hipLaunchKernelGGL(k_paint_dev_raster, dim3(plan.tiles_x, plan.tiles_y), dim3(256), 0, st, dst, W, H, pitch,
                     clear_on ? 1 : 0, clear, static_cast<const PaintPrim *>(prims),
                     static_cast<const PaintTri *>(tris), masks, n, count_dev, base, plan.batch, plan.tile_h, (int)u8);
}

void paint_dev_enqueue_finish(unsigned *counters, const int *count_dev, int n, int *status, hipStream_t st) {
  hipLaunchKernelGGL(k_paint_dev_finish, dim3(1), dim3(1), 0, st, counters, count_dev, n, status);
}

void PaintDevBuffers::release() {
  if (work) (void)hipFree(work);
  work = nullptr;
}

hipError_t paint_prims_device(float4 *dst, int W, int H, int pitch, bool u8, const unsigned char *clear,
                              const void *prims_dev, int n, const void *count_dev, void *status_dev,
                              PaintDevBuffers &buf, hipStream_t st) {
  const PaintDevPlan &plan = buf.plan;
  hipError_t e = hipSuccess;
  if (!buf.work) {  // the one place the call may wait: the first call's allocation (and the first after a new plan)
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
      hipLaunchKernelGGL(k_paint_dev_setup, dim3((nb + 255) / 256), dim3(256), 0, st,
                         static_cast<const unsigned *>(prims_dev), n, cnt, base, plan.batch, prims, tris, counters, xf,
                         tab);
      paint_dev_enqueue_bin(prims, n, cnt, base, nb, plan, masks, st);
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
