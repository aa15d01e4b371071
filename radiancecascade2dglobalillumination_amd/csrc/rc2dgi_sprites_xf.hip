// rc2dgi_sprites_xf.hip -- rc2dgi_sprites_xf_device: a device-resident list of atlas sprites, each mapped onto a
// parallelogram of the screen, into an input texture.  rc2dgi_sprites_device's sequence of kernels per
// batch on the same working memory, with a set-up and a raster of its own:
//   k_sprites_xf_setup   one lane a sprite: the twelve words, the refusal test in the header's form (a refused sprite
//                        draws nothing and is counted), the inverse of (A, B) and the pixel box of the parallelogram's
//                        corners, clipped to the target and turned into GL rows.  The box and `on` go where
//                        k_paint_dev_bin reads them (SpriteXfBox over PaintPrim); the map, the source rectangle, the
//                        tint and the flags go into one 64-byte slot of the triangle region (SpriteXfMap), which the
//                        sprite calls leave unused and rc2dgi_paint_device rewrites before it reads.
//   k_paint_dev_bin      unchanged (paint_dev_enqueue_bin): bit k of the mask of every tile the box meets.
//   k_sprites_xf_raster  sprites_walk_tile (rc2dgi_sprites_tile.h) as k_sprites_raster runs it.  Per set bit the two
//                        records are read at addresses the whole wave shares; a lane inside the box maps its pixel
//                        centre back into the source rectangle with the header's float operations; a covered lane
//                        loads one atlas pixel (POINT) or four (RC2DGI_SPRITE_LINEAR) -- a dword, dwordx2 or dwordx4
//                        each by the format -- and applies write_value, the unfused lerps, the tint and the blend or
//                        the replacement.
//   k_paint_dev_finish   unchanged (paint_dev_enqueue_finish).
// What is read from the list becomes an index only after the refusal test: the texel indices derive from the box
// clipped to the target, the atlas indices from taps clamped to a source rectangle the test found inside the atlas.
// The unit is built with -ffp-contract=off: every a * b + c below is two roundings, as the header states them.
#include "rc2dgi_sprites_xf.h"

#include "rc2dgi_device.h"
#include "rc2dgi_paint_raster.h"
#include "rc2dgi_sprites_tile.h"
#include "rc2dgi_write.h"

#include <algorithm>

namespace rc2dgi {

namespace {

// What k_paint_dev_bin reads of a sprite set up: laid over PaintPrim.
struct SpriteXfBox {
  int x0, y0, x1, y1;  // texel box (inclusive, GL rows), clipped to the target
  int pad0;
  int on;              // 1: draws (PaintPrim::ntri)
  int pad[6];
};
static_assert(sizeof(SpriteXfBox) == sizeof(PaintPrim) && offsetof(SpriteXfBox, x0) == offsetof(PaintPrim, x0) &&
                  offsetof(SpriteXfBox, y1) == offsetof(PaintPrim, y1) &&
                  offsetof(SpriteXfBox, on) == offsetof(PaintPrim, ntri),
              "k_paint_dev_bin reads a sprite's box and its `on` word where PaintPrim keeps them");

// The rest of it, in slot k of the triangle region: with d = (X + 0.5 - px, Y + 0.5 - py) the pixel centre lies at
// (a, b) = (d.x * i00 + d.y * i01, d.x * i10 + d.y * i11) of the parallelogram, (0, 0) its corner P.
struct SpriteXfMap {
  float i00, i01, i10, i11;
  float px, py;
  int sx, sy, w, h;
  unsigned flags;
  unsigned pad;
  float4 tint;
};
static_assert(sizeof(SpriteXfMap) == sizeof(PaintTri), "a sprite's map takes one of the batch * 36 triangle slots");

constexpr float kXfLim = 0x1p20f, kXfDet = 0x1p-20f;

__global__ __launch_bounds__(256) void k_sprites_xf_setup(const unsigned *__restrict__ list, int n,
                                                          const int *__restrict__ count_dev, int base, int batch,
                                                          SpriteXfBox *__restrict__ recs,
                                                          SpriteXfMap *__restrict__ maps,
                                                          unsigned *__restrict__ counters, int W, int H, int AW, int AH,
                                                          int u8) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  const int mb = paint_dev_batch(count_dev, n, base, batch);
  bool refused = false;
  if (k < mb) {  // (base + k < m <= n: inside the list)
    const unsigned *q = list + (size_t)(base + k) * 12;
    const int sx = (int)q[0], sy = (int)q[1], w = (int)q[2], h = (int)q[3];
    const float px = __uint_as_float(q[4]), py = __uint_as_float(q[5]), ax = __uint_as_float(q[6]),
                ay = __uint_as_float(q[7]), bx = __uint_as_float(q[8]), by = __uint_as_float(q[9]);
    const unsigned rgba = q[10], flags = q[11];
    const float det = ax * by - ay * bx;
    // (each comparison is false for a NaN, so a NaN or an infinity anywhere refuses)
    const bool ok = (flags & ~(unsigned)(RC2DGI_SPRITE_REPLACE | RC2DGI_SPRITE_LINEAR)) == 0u && w >= 1 && h >= 1 &&
                    sx >= 0 && sy >= 0 && w <= AW - sx && h <= AH - sy && fabsf(px) <= kXfLim && fabsf(py) <= kXfLim &&
                    fabsf(ax) <= kXfLim && fabsf(ay) <= kXfLim && fabsf(bx) <= kXfLim && fabsf(by) <= kXfLim &&
                    fabsf(det) >= kXfDet;
    refused = !ok;
    SpriteXfBox r{};
    if (ok) {
      // the corners are finite and below 2^22 in magnitude: the conversions are safe
      const float cx1 = px + ax, cx2 = px + bx, cx3 = cx1 + bx, cy1 = py + ay, cy2 = py + by, cy3 = cy1 + by;
      const float lox = fminf(fminf(px, cx1), fminf(cx2, cx3)), hix = fmaxf(fmaxf(px, cx1), fmaxf(cx2, cx3));
      const float loy = fminf(fminf(py, cy1), fminf(cy2, cy3)), hiy = fmaxf(fmaxf(py, cy1), fmaxf(cy2, cy3));
      const int X0 = max((int)floorf(lox) - 1, 0), X1 = min((int)floorf(hix) + 1, W - 1);
      const int Y0 = max((int)floorf(loy) - 1, 0), Y1 = min((int)floorf(hiy) + 1, H - 1);
      r.x0 = X0;
      r.x1 = X1;
      r.y0 = H - 1 - Y1;  // screen row Y is texel row H - 1 - Y
      r.y1 = H - 1 - Y0;
      r.on = X0 <= X1 && Y0 <= Y1 ? 1 : 0;
      SpriteXfMap m;
      m.i00 = by / det;
      m.i01 = (-bx) / det;
      m.i10 = (-ay) / det;
      m.i11 = ax / det;
      m.px = px;
      m.py = py;
      m.sx = sx;
      m.sy = sy;
      m.w = w;
      m.h = h;
      m.flags = flags;
      m.pad = 0u;
      const float tr = (float)(rgba & 255u), tg = (float)((rgba >> 8) & 255u), tb = (float)((rgba >> 16) & 255u),
                  ta = (float)(rgba >> 24);
      m.tint = u8 ? make_float4(tr * kInv255, tg * kInv255, tb * kInv255, ta * kInv255)
                  : make_float4(tr / 255.0f, tg / 255.0f, tb / 255.0f, ta / 255.0f);
      maps[k] = m;  // (k < mb <= batch: inside the first `batch` of the region's batch * 36 slots)
    }
    recs[k] = r;
  }
  const unsigned long long b = __ballot(refused);  // integer adds: the sum is the same in any order
  if (b != 0 && (threadIdx.x & 63) == 0) atomicAdd(&counters[0], (unsigned)__popcll(b));
}

// lerp(p, q, f) = p + f * (q - p): a difference, a product and a sum (not the GI textures' fmaf lerp)
__device__ __forceinline__ float4 xf_lerp(float4 p, float4 q, float f) {
  return make_float4(p.x + f * (q.x - p.x), p.y + f * (q.y - p.y), p.z + f * (q.z - p.z), p.w + f * (q.w - p.w));
}

template <bool U8, int FMT>
__device__ __forceinline__ void sprites_xf_tile(float4 *__restrict__ dst, int W, int H, int pitch, int clear_on,
                                                float cr, float cg, float cb, float ca,
                                                const SpriteXfBox *__restrict__ recs,
                                                const SpriteXfMap *__restrict__ maps, unsigned *__restrict__ masks,
                                                int mb, int batch, int tile_h,
                                                const unsigned char *__restrict__ atlas, size_t apitch) {
  typedef typename WritePixel<FMT>::T P;
  constexpr int PXB = read_pixel_bytes(FMT);
  sprites_walk_tile(dst, W, H, pitch, clear_on, cr, cg, cb, ca, masks, mb, batch, tile_h,
                    [&](int k, bool in, int i, int j, float4 &v) {
    const SpriteXfBox &p = recs[k];  // (k is the same in every lane: one read a wave)
    if (!in || i < p.x0 || i > p.x1 || j < p.y0 || j > p.y1) return false;
    const SpriteXfMap &m = maps[k];
    const float dxp = ((float)i + 0.5f) - m.px, dyp = ((float)(H - 1 - j) + 0.5f) - m.py;
    const float a = dxp * m.i00 + dyp * m.i01, b = dxp * m.i10 + dyp * m.i11;
    if (!(a >= 0.0f && a < 1.0f && b >= 0.0f && b < 1.0f)) return false;  // (a NaN fails)
    // covered: 0 <= s <= w and 0 <= t <= h, and every tap below is clamped into the source rectangle, which the
    // refusal test found inside the atlas
    const float s = a * (float)m.w, t = b * (float)m.h;
    auto tap = [&](int c, int r) {
      return write_value<U8, FMT>(
          *reinterpret_cast<const P *>(atlas + (size_t)(m.sy + r) * apitch + (size_t)(m.sx + c) * PXB));
    };
    float4 val;
    if (m.flags & RC2DGI_SPRITE_LINEAR) {
      const float xs = s - 0.5f, ys = t - 0.5f;
      const int i0 = (int)floorf(xs), j0 = (int)floorf(ys);
      const float fx = xs - (float)i0, fy = ys - (float)j0;
      const int c0 = min(max(i0, 0), m.w - 1), c1 = min(max(i0 + 1, 0), m.w - 1);
      const int r0 = min(max(j0, 0), m.h - 1), r1 = min(max(j0 + 1, 0), m.h - 1);
      const float4 p00 = tap(c0, r0), p10 = tap(c1, r0), p01 = tap(c0, r1), p11 = tap(c1, r1);
      val = xf_lerp(xf_lerp(p00, p10, fx), xf_lerp(p01, p11, fx), fy);
    } else {
      val = tap(min((int)s, m.w - 1), min((int)t, m.h - 1));
    }
    const float4 src = make_float4(val.x * m.tint.x, val.y * m.tint.y, val.z * m.tint.z, val.w * m.tint.w);
    if (m.flags & RC2DGI_SPRITE_REPLACE) v = U8 ? GiU8::unpack(GiU8::pack(src)) : src;
    else v = U8 ? GiU8::blend(src, v) : blend(src, v);
    return true;
  });
}

// (the clear colour travels as four floats: a float4 argument is copied to the stack, a store nothing reads)
template <int FMT>
__global__ __launch_bounds__(256) void k_sprites_xf_raster(float4 *__restrict__ dst, int W, int H, int pitch,
                                                           int clear_on, float cr, float cg, float cb, float ca,
                                                           const SpriteXfBox *__restrict__ recs,
                                                           const SpriteXfMap *__restrict__ maps,
                                                           unsigned *__restrict__ masks, int n,
                                                           const int *__restrict__ count_dev, int base, int batch,
                                                           int tile_h, int u8, const unsigned char *__restrict__ atlas,
                                                           size_t apitch) {
  const int mb = paint_dev_batch(count_dev, n, base, batch);
  if (u8) sprites_xf_tile<true, FMT>(dst, W, H, pitch, clear_on, cr, cg, cb, ca, recs, maps, masks, mb, batch, tile_h,
                                      atlas, apitch);
  else sprites_xf_tile<false, FMT>(dst, W, H, pitch, clear_on, cr, cg, cb, ca, recs, maps, masks, mb, batch, tile_h,
                                      atlas, apitch);
}

template <int FMT>
void enqueue_raster(const dim3 &grid, hipStream_t st, float4 *dst, int W, int H, int pitch, int clear_on, float4 cl,
                    const SpriteXfBox *recs, const SpriteXfMap *maps, unsigned *masks, int n, const int *cnt, int base,
                    const PaintDevPlan &plan, bool u8, const SpriteAtlas &atlas) {
  hipLaunchKernelGGL(k_sprites_xf_raster<FMT>, grid, dim3(256), 0, st, dst, W, H, pitch, clear_on, cl.x, cl.y, cl.z,
                     cl.w, recs, maps, masks, n, cnt, base, plan.batch, plan.tile_h, (int)u8, atlas.dev, atlas.pitch);
}

}  // namespace

hipError_t sprites_xf_device(float4 *dst, int W, int H, int pitch, bool u8, const unsigned char *clear,
                             const SpriteAtlas &atlas, const void *sprites_dev, int n, const void *count_dev,
                             void *status_dev, PaintDevBuffers &buf, hipStream_t st) {
  const PaintDevPlan &plan = buf.plan;
  static_assert(sizeof(SpriteXfBox) == 48, "a batch of set-up records fills the PaintPrim region of the plan");
  hipError_t e = hipSuccess;
  if (!buf.work) {  // the one place the call may wait: the first call's allocation (shared with the other two lists)
    e = hipMalloc(reinterpret_cast<void **>(&buf.work), plan.bytes);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(buf.work, 0, plan.bytes, st);
    if (e != hipSuccess) return e;
  }
  unsigned *counters = reinterpret_cast<unsigned *>(buf.work);
  SpriteXfBox *recs = reinterpret_cast<SpriteXfBox *>(buf.work + plan.off_prims);
  SpriteXfMap *maps = reinterpret_cast<SpriteXfMap *>(buf.work + plan.off_tris);
  unsigned *masks = reinterpret_cast<unsigned *>(buf.work + plan.off_masks);
  const int *cnt = static_cast<const int *>(count_dev);
  const float4 cl = paint_dev_clear(clear, u8);
  // the batches follow each other on the stream: batch b + 1 blends over what batch b left, so the draw order holds
  const int batches = n == 0 ? (clear ? 1 : 0) : (n + plan.batch - 1) / plan.batch;
  for (int b = 0; b < batches; ++b) {
    const int base = b * plan.batch, nb = std::min(plan.batch, n - base);
    if (nb > 0) {
      hipLaunchKernelGGL(k_sprites_xf_setup, dim3((nb + 255) / 256), dim3(256), 0, st,
                         static_cast<const unsigned *>(sprites_dev), n, cnt, base, plan.batch, recs, maps, counters, W,
                         H, atlas.w, atlas.h, (int)u8);
      paint_dev_enqueue_bin(recs, n, cnt, base, nb, plan, masks, st);
    }
    const dim3 grid(plan.tiles_x, plan.tiles_y);
    const int clear_on = clear && b == 0 ? 1 : 0;
    switch (atlas.format) {
      case RC2DGI_FMT_RGBA32F:
        enqueue_raster<RC2DGI_FMT_RGBA32F>(grid, st, dst, W, H, pitch, clear_on, cl, recs, maps, masks, n, cnt, base,
                                           plan, u8, atlas);
        break;
      case RC2DGI_FMT_RGBA16F:
        enqueue_raster<RC2DGI_FMT_RGBA16F>(grid, st, dst, W, H, pitch, clear_on, cl, recs, maps, masks, n, cnt, base,
                                           plan, u8, atlas);
        break;
      case RC2DGI_FMT_RGBA8:
        enqueue_raster<RC2DGI_FMT_RGBA8>(grid, st, dst, W, H, pitch, clear_on, cl, recs, maps, masks, n, cnt, base,
                                         plan, u8, atlas);
        break;
      default: return hipErrorInvalidValue;
    }
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
