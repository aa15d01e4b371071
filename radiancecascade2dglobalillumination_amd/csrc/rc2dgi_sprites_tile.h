// rc2dgi_sprites_tile.h -- the tile walk the two sprite rasters share (rc2dgi_sprites.hip, rc2dgi_sprites_xf.hip): one
// workgroup a 64 x tile_h tile, a wave a texel row, a lane a texel.  The mask is loaded as k_paint_dev_raster loads it;
// a tile with no bit set and no clear exits before it reads a texel; the words found set are zeroed.  The set bits are
// walked in ascending order, the draw order, and `apply(k, in, i, j, v)` is called for each with k the same in every
// lane: it draws record k of the batch into the lane's texel value v and returns whether it touched it.  A texel is
// stored only if touched.  Device units only.
#pragma once

#include <hip/hip_runtime.h>

namespace rc2dgi {

template <class Apply>
__device__ __forceinline__ void sprites_walk_tile(float4 *__restrict__ dst, int W, int H, int pitch, int clear_on,
                                                  float cr, float cg, float cb, float ca,
                                                  unsigned *__restrict__ masks, int mb, int batch, int tile_h,
                                                  Apply apply) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
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
  for (int r = 0; r < tile_h; r += 4) {
    const int j = blockIdx.y * tile_h + r + wave;
    if (blockIdx.y * tile_h + r >= H) break;
    const bool in = i < W && j < H;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    bool touched = clear_on != 0;
    if (in) v = clear_on ? make_float4(cr, cg, cb, ca) : dst[(size_t)j * pitch + i];
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
          if (apply(k, in, i, j, v)) touched = true;
        }
      }
    }
    if (in && touched) dst[(size_t)j * pitch + i] = v;
  }
}

}  // namespace rc2dgi
