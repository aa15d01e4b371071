// rc2dgi_sprites.hip -- rc2dgi_sprites_device: a device-resident list of atlas sprites into an input texture
// (DESIGN.md §19).  rc2dgi_write's values (write_value, the two blends) under rc2dgi_paint_device's list (the working
// memory, the masks, the count and the status of rc2dgi_paint_dev.hip): the same fixed sequence of kernels per batch,
// so that nothing of the list is known on the host.
//   k_sprites_setup   one lane a sprite: the refusal test (a refused sprite draws nothing and is counted), the pixel
//                     box clipped to the target and turned into GL rows, and -- in the 48 bytes of a PaintPrim, whose
//                     box and `ntri` words k_paint_dev_bin reads -- the source origin, the tint and the flags.
//   k_paint_dev_bin   unchanged (paint_dev_enqueue_bin): bit k of the mask of every tile the box meets.
//   k_sprites_raster  one workgroup a 64 x tile_h tile, a wave a texel row, a lane a texel.  The mask is loaded as
//                     k_paint_dev_raster loads it; a tile with no bit set and no clear exits before it reads a texel;
//                     the words found set are zeroed.  The set bits are walked in ascending order, the draw order
//                     (sprites_walk_tile, rc2dgi_sprites_tile.h, shared with rc2dgi_sprites_xf.hip).  A
//                     sprite's record is at an address the whole wave shares (scalar loads); the lanes inside its box
//                     load one atlas pixel each -- a dword, dwordx2 or dwordx4 by the format, adjacent lanes adjacent
//                     pixels of one atlas row, RC2DGI_SPRITE_FLIP_X only reversing the segment -- and apply
//                     write_value, the tint and the blend or the replacement.  A texel is stored only if touched.
//   k_paint_dev_finish  unchanged (paint_dev_enqueue_finish).
// What is read from the list becomes an index only after the refusal test: the texel indices derive from the box
// clipped to the target, the atlas indices from that box and a source rectangle the test found inside the atlas.
#include "rc2dgi_sprites.h"

#include "rc2dgi_device.h"
#include "rc2dgi_paint_raster.h"
#include "rc2dgi_sprites_tile.h"
#include "rc2dgi_write.h"

#include <algorithm>

namespace rc2dgi {

namespace {

// A sprite set up: laid over PaintPrim so that k_paint_dev_bin bins it.  Texel (i, j) of the box shows atlas pixel
// (u0 + i or u0 - i, v0 - j or v0 + j): FLIP_X turns the first sign, FLIP_Y the second (the texture's rows run upwards).
struct SpriteRec {
  int x0, y0, x1, y1;  // texel box (inclusive, GL rows), clipped to the target
  int u0;
  int on;              // 1: draws (PaintPrim::ntri)
  int v0;
  unsigned flags;
  float4 tint;
};
static_assert(sizeof(SpriteRec) == sizeof(PaintPrim) && offsetof(SpriteRec, x0) == offsetof(PaintPrim, x0) &&
                  offsetof(SpriteRec, y1) == offsetof(PaintPrim, y1) && offsetof(SpriteRec, on) == offsetof(PaintPrim, ntri),
              "k_paint_dev_bin reads a sprite's box and its `on` word where PaintPrim keeps them");

constexpr int kSpriteLim = 1 << 22;  // |dx|, |dy| at most: rc2dgi_paint's 2^22 pixels

__global__ __launch_bounds__(256) void k_sprites_setup(const int *__restrict__ list, int n,
                                                       const int *__restrict__ count_dev, int base, int batch,
                                                       SpriteRec *__restrict__ recs, unsigned *__restrict__ counters,
                                                       int W, int H, int AW, int AH, int u8) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  const int mb = paint_dev_batch(count_dev, n, base, batch);
  bool refused = false;
  if (k < mb) {  // (base + k < m <= n: inside the list)
    const int *q = list + (size_t)(base + k) * 8;
    const int sx = q[0], sy = q[1], w = q[2], h = q[3], dx = q[4], dy = q[5];
    const unsigned rgba = (unsigned)q[6], flags = (unsigned)q[7];
    const bool ok = (flags & ~7u) == 0u && w >= 1 && h >= 1 && sx >= 0 && sy >= 0 && w <= AW - sx && h <= AH - sy &&
                    dx >= -kSpriteLim && dx <= kSpriteLim && dy >= -kSpriteLim && dy <= kSpriteLim;
    refused = !ok;
    SpriteRec r{};
    if (ok) {  // (w, h <= 32768 and |dx|, |dy| <= 2^22: the sums below stay far inside an int)
      const int X0 = max(dx, 0), X1 = min(dx + w - 1, W - 1);  // screen columns and rows (y down), clipped
      const int Y0 = max(dy, 0), Y1 = min(dy + h - 1, H - 1);
      r.x0 = X0;
      r.x1 = X1;
      r.y0 = H - 1 - Y1;  // screen row Y is texel row H - 1 - Y
      r.y1 = H - 1 - Y0;
      r.on = X0 <= X1 && Y0 <= Y1 ? 1 : 0;
      // column i is sprite column i - dx, texel row j is sprite row H - 1 - j - dy; a flip mirrors it in w - 1 or h - 1
      r.u0 = (flags & RC2DGI_SPRITE_FLIP_X) ? sx + w - 1 + dx : sx - dx;
      r.v0 = (flags & RC2DGI_SPRITE_FLIP_Y) ? sy + h - 1 - (H - 1 - dy) : sy + (H - 1 - dy);
      r.flags = flags;
      const float tr = (float)(rgba & 255u), tg = (float)((rgba >> 8) & 255u), tb = (float)((rgba >> 16) & 255u),
                  ta = (float)(rgba >> 24);
      r.tint = u8 ? make_float4(tr * kInv255, tg * kInv255, tb * kInv255, ta * kInv255)
                  : make_float4(tr / 255.0f, tg / 255.0f, tb / 255.0f, ta / 255.0f);
    }
    recs[k] = r;
  }
  const unsigned long long b = __ballot(refused);  // integer adds: the sum is the same in any order
  if (b != 0 && (threadIdx.x & 63) == 0) atomicAdd(&counters[0], (unsigned)__popcll(b));
}

template <bool U8, int FMT>
__device__ __forceinline__ void sprites_tile(float4 *__restrict__ dst, int W, int H, int pitch, int clear_on,
                                             float cr, float cg, float cb, float ca,
                                             const SpriteRec *__restrict__ recs,
                                             unsigned *__restrict__ masks, int mb, int batch, int tile_h,
                                             const unsigned char *__restrict__ atlas, size_t apitch) {
  typedef typename WritePixel<FMT>::T P;
  constexpr int PXB = read_pixel_bytes(FMT);
  sprites_walk_tile(dst, W, H, pitch, clear_on, cr, cg, cb, ca, masks, mb, batch, tile_h,
                    [&](int k, bool in, int i, int j, float4 &v) {
    const SpriteRec &p = recs[k];  // (k is the same in every lane: one read a wave)
    if (!in || i < p.x0 || i > p.x1 || j < p.y0 || j > p.y1) return false;
    // inside the clipped box: (u, v) lies in the source rectangle, which lies in the atlas
    const int pu = (p.flags & RC2DGI_SPRITE_FLIP_X) ? p.u0 - i : p.u0 + i;
    const int pv = (p.flags & RC2DGI_SPRITE_FLIP_Y) ? p.v0 + j : p.v0 - j;
    const P px = *reinterpret_cast<const P *>(atlas + (size_t)pv * apitch + (size_t)pu * PXB);
    const float4 val = write_value<U8, FMT>(px);
    const float4 src = make_float4(val.x * p.tint.x, val.y * p.tint.y, val.z * p.tint.z, val.w * p.tint.w);
    if (p.flags & RC2DGI_SPRITE_REPLACE) v = U8 ? GiU8::unpack(GiU8::pack(src)) : src;
    else v = U8 ? GiU8::blend(src, v) : blend(src, v);
    return true;
  });
}

// (the clear colour travels as four floats: a float4 argument is copied to the stack, a store nothing reads)
template <int FMT>
__global__ __launch_bounds__(256) void k_sprites_raster(float4 *__restrict__ dst, int W, int H, int pitch, int clear_on,
                                                        float cr, float cg, float cb, float ca,
                                                        const SpriteRec *__restrict__ recs,
                                                        unsigned *__restrict__ masks, int n,
                                                        const int *__restrict__ count_dev, int base, int batch,
                                                        int tile_h, int u8, const unsigned char *__restrict__ atlas,
                                                        size_t apitch) {
  const int mb = paint_dev_batch(count_dev, n, base, batch);
  if (u8) sprites_tile<true, FMT>(dst, W, H, pitch, clear_on, cr, cg, cb, ca, recs, masks, mb, batch, tile_h, atlas,
                                   apitch);
  else sprites_tile<false, FMT>(dst, W, H, pitch, clear_on, cr, cg, cb, ca, recs, masks, mb, batch, tile_h, atlas,
                                   apitch);
}

}  // namespace

hipError_t sprites_device(float4 *dst, int W, int H, int pitch, bool u8, const unsigned char *clear,
                          const SpriteAtlas &atlas, const void *sprites_dev, int n, const void *count_dev,
                          void *status_dev, PaintDevBuffers &buf, hipStream_t st) {
  const PaintDevPlan &plan = buf.plan;
  static_assert(sizeof(SpriteRec) == 48, "a batch of set-up records fills the PaintPrim region of the plan");
  hipError_t e = hipSuccess;
  if (!buf.work) {  // the one place the call may wait: the first call's allocation (rc2dgi_paint_device's, if it ran)
    e = hipMalloc(reinterpret_cast<void **>(&buf.work), plan.bytes);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(buf.work, 0, plan.bytes, st);
    if (e != hipSuccess) return e;
  }
  unsigned *counters = reinterpret_cast<unsigned *>(buf.work);
  SpriteRec *recs = reinterpret_cast<SpriteRec *>(buf.work + plan.off_prims);
  unsigned *masks = reinterpret_cast<unsigned *>(buf.work + plan.off_masks);
  const int *cnt = static_cast<const int *>(count_dev);
  const float4 cl = paint_dev_clear(clear, u8);
  // the batches follow each other on the stream: batch b + 1 blends over what batch b left, so the draw order holds
  const int batches = n == 0 ? (clear ? 1 : 0) : (n + plan.batch - 1) / plan.batch;
  for (int b = 0; b < batches; ++b) {
    const int base = b * plan.batch, nb = std::min(plan.batch, n - base);
    if (nb > 0) {
      hipLaunchKernelGGL(k_sprites_setup, dim3((nb + 255) / 256), dim3(256), 0, st,
                         static_cast<const int *>(sprites_dev), n, cnt, base, plan.batch, recs, counters, W, H, atlas.w,
                         atlas.h, (int)u8);
      paint_dev_enqueue_bin(recs, n, cnt, base, nb, plan, masks, st);
    }
    const dim3 grid(plan.tiles_x, plan.tiles_y);
    const int clear_on = clear && b == 0 ? 1 : 0;
    switch (atlas.format) {
      case RC2DGI_FMT_RGBA32F:
        hipLaunchKernelGGL(k_sprites_raster<RC2DGI_FMT_RGBA32F>, grid, dim3(256), 0, st, dst, W, H, pitch, clear_on, cl.x,
                           cl.y, cl.z, cl.w,
                           static_cast<const SpriteRec *>(recs), masks, n, cnt, base, plan.batch, plan.tile_h, (int)u8,
                           atlas.dev, atlas.pitch);
        break;
      case RC2DGI_FMT_RGBA16F:
        hipLaunchKernelGGL(k_sprites_raster<RC2DGI_FMT_RGBA16F>, grid, dim3(256), 0, st, dst, W, H, pitch, clear_on, cl.x,
                           cl.y, cl.z, cl.w,
                           static_cast<const SpriteRec *>(recs), masks, n, cnt, base, plan.batch, plan.tile_h, (int)u8,
                           atlas.dev, atlas.pitch);
        break;
      case RC2DGI_FMT_RGBA8:
        hipLaunchKernelGGL(k_sprites_raster<RC2DGI_FMT_RGBA8>, grid, dim3(256), 0, st, dst, W, H, pitch, clear_on, cl.x,
                           cl.y, cl.z, cl.w,
                           static_cast<const SpriteRec *>(recs), masks, n, cnt, base, plan.batch, plan.tile_h, (int)u8,
                           atlas.dev, atlas.pitch);
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
