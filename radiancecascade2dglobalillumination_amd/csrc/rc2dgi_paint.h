// rc2dgi_paint.h -- on-device scene producer: raylib 5.5 rectangles and circles
// rasterized into colorRT / emissiveRT the way RenderScene / RedrawSceneToRTs paint them
// (RC2DGI.cs:224-264, 528-545).  See rc2dgi_paint.hip.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/rc2dgi.h"
#include "rc2dgi_kernels.h"

namespace rc2dgi {

// device copies of the primitive setup, grown on demand (owned by the context)
struct PaintBuffers {
  void *prims = nullptr;  // PaintPrim[]
  void *edges = nullptr;  // PaintTri[]
  size_t prim_cap = 0, tri_cap = 0;
  void release();
  ~PaintBuffers() { release(); }
};

// BeginTextureMode(dst); [ClearBackground(clear)]; draw prims[0..n); EndTextureMode.
// dst: W x H float4 render texture (pitch in texels), GL row order; u8: an RGBA8 texture (values
// k * (1/255), 8-bit blends).  Synchronous w.r.t. the host arrays (they are copied before
// returning); the raster runs on `st`.
hipError_t paint_prims(float4 *dst, int W, int H, int pitch, bool u8, const unsigned char *clear,
                       const rc2dgi_prim *prims, int n, PaintBuffers &buf, hipStream_t st);

// raylib's host-side cosf / sinf of DEG2RAD * 10k, k = 0 .. 36 (glibc's, as paint_prims uses them)
void paint_circle_table(float cos37[37], float sin37[37]);

// ---- rc2dgi_paint_device (rc2dgi_paint_dev.hip): the same painting from a primitive list in device memory, set up,
// binned and rasterised on the device.
// The plan of a W x H target (host arithmetic only): a tile is 64 x tile_h pixels, a batch `batch` primitives, and the
// working memory holds, in this order, kPaintDevHead bytes of counters, `batch` set-up records, batch * 36 triangle
// records and one mask of `batch` bits a tile.
constexpr size_t kPaintDevMaskBytes = (size_t)40 << 20;  // the masks' share of the 64 MiB the interface promises
struct PaintDevPlan {
  int tile_h = 4;     // 4 .. 128, a power of two
  int batch = 8192;   // 2048, 4096 or 8192: 64 lanes x (batch / 2048) words x 32 bits
  int tiles_x = 0, tiles_y = 0;
  size_t off_prims = 0, off_tris = 0, off_masks = 0, bytes = 0;
  size_t mask_bytes() const { return bytes - off_masks; }
};
// code 0: the smallest tiles and the longest batch whose masks fit kPaintDevMaskBytes; otherwise the tile height and
// the batch of a "paint_plan" code (paint_plan_code_ok, rc2dgi_tuning.h), whatever their masks take: the caller compares
// mask_bytes() with kPaintDevMaskBytes.
PaintDevPlan paint_dev_plan(int W, int H, int code = 0);

struct PaintDevBuffers {
  PaintDevPlan plan;              // the plan in force (set with the context and by the "paint_plan" knob)
  unsigned char *work = nullptr;  // plan.bytes, allocated at the first call and laid out by `plan`; the masks and
                                  // counters are zero between calls (the kernels leave them so)
  void release();
  ~PaintDevBuffers() { release(); }
};

// enqueues the whole painting on `st` and returns (no wait but the first call's allocation).  prims_dev: n records of
// rc2dgi_prim; count_dev: null or one int32; status_dev: null or two int32 {m, refused}.
hipError_t paint_prims_device(float4 *dst, int W, int H, int pitch, bool u8, const unsigned char *clear,
                              const void *prims_dev, int n, const void *count_dev, void *status_dev,
                              PaintDevBuffers &buf, hipStream_t st);

// The steps rc2dgi_sprites_device (rc2dgi_sprites.hip) runs unchanged on the same working memory.
// ClearBackground(clear) as a texel (zero without a clear colour).
float4 paint_dev_clear(const unsigned char *clear, bool u8);
// k_paint_dev_bin over the nb records of the batch at `base`.  recs: `batch` records of 48 bytes that begin as
// PaintPrim does -- the clipped pixel box in words 0 .. 3, word 5 (ntri) positive when the record draws.
void paint_dev_enqueue_bin(const void *recs, int n, const int *count_dev, int base, int nb, const PaintDevPlan &plan,
                           unsigned *masks, hipStream_t st);
// k_paint_dev_raster over every tile of the plan, for the batch at `base`: prims / tris are the batch's PaintPrim and
// PaintTri records (rc2dgi_paint_raster.h), clear_on applies `clear` first (the first batch of a call with a clear).
// rc2dgi_shapes_device (rc2dgi_shapes.hip) runs it unchanged on records of its own set-up.
void paint_dev_enqueue_raster(float4 *dst, int W, int H, int pitch, bool u8, bool clear_on, float4 clear,
                              const void *prims, const void *tris, unsigned *masks, int n, const int *count_dev,
                              int base, const PaintDevPlan &plan, hipStream_t st);
// k_paint_dev_finish: {m, refused} to `status` (null: nothing) and the refusal counter, counters[0], back to zero.
void paint_dev_enqueue_finish(unsigned *counters, const int *count_dev, int n, int *status, hipStream_t st);

}  // namespace rc2dgi
