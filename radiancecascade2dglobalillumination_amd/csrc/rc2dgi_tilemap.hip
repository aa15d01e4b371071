// rc2dgi_tilemap.hip -- rc2dgi_tilemap_device: a grid of cell words drawn from a tile set.
//
// A grid is not a list: a texel's cell is a division of its own coordinates and cells never overlap, so there is no
// draw order, no binning, no set-up pass and no working memory.  The whole layer is one streaming kernel of the shape
// of k_write (rc2dgi_write.hip):
//   k_tilemap   a workgroup is 64 columns by 4 * kTileRows screen rows, a wave 64 adjacent columns of kTileRows
//               adjacent rows, a lane one column of them.  The column's cell and offset come from one division a lane
//               (tilemap_axis), the first row's from one division a wave, the rows after it from an increment.  All of
//               a lane's cell words and -- with the blend and no clear -- the texels under them are loaded first; then
//               the words are decoded and tested (tilemap_decode, rc2dgi_tilemap_cell.h) and the atlas pixels loaded,
//               a dword, dwordx2 or dwordx4 a lane by the format, adjacent lanes inside a cell adjacent pixels of one
//               atlas row (a flipped tile reverses the segment); then write_value, the tint and the blend or the
//               replacement, the definitions k_sprites_raster uses.  A texel is stored (one aligned dwordx4 a lane, a
//               wave's columns starting on a multiple of 64) only if a cell or the clear touched it.  The lane on a
//               cell's first visible pixel counts it: one atomicAdd a wave and counter, of the ballots' popcounts,
//               into one of kTileSlots counter pairs a cache line apart (the wave's number picks it): 16384 adds to
//               one address cost more than the whole raster, DESIGN.md §22.
//   k_tilemap_finish   one wave, a lane a slot: the sums {drawn, refused} to the caller's status words, the slots back
//               to zero.
// The kernel is specialised on the atlas format (a template argument) and on the storage kind and the replacement (a
// uniform switch into templates).  No LDS, no scratch.
// What is read from the grid becomes an index only after the refusal test: the cell index derives from the texel's own
// coordinates and lies inside the grid, the atlas index from a tile the test found inside the atlas.
#include "rc2dgi_tilemap.h"

#include "rc2dgi_device.h"
#include "rc2dgi_write.h"

#include <algorithm>

namespace rc2dgi {

namespace {

constexpr int kTileRows = 4;  // rows a lane draws a texel of, as kWriteRows
constexpr int kTileSlots = 64, kTileSlotWords = 32;  // counter pairs, and the words from one to the next (128 bytes)

struct TilemapArgs {
  float4 *dst;  // the input texture, GL row order: screen row Y is texel row H - 1 - Y
  int dpitch, H;
  int xa;                 // the launch's first column: a multiple of 64, at most x0
  int x0, x1, y0, y1;     // the screen box the launch draws (inclusive), inside the target
  const unsigned *cells;
  TilemapGeom g;
  const unsigned char *atlas;
  size_t apitch;
  float tr, tg, tb, ta;   // the tint
  float cr, cg, cb, ca;   // the clear's value (clear_on)
  int clear_on;
  unsigned *counters;     // kTileSlots pairs {drawn, refused}; null: nothing is counted
};

template <bool U8, bool REPLACE, int FMT>
__device__ __forceinline__ void tilemap_block(const TilemapArgs &a) {
  typedef typename WritePixel<FMT>::T P;
  constexpr int PXB = read_pixel_bytes(FMT);
  const TilemapGeom &m = a.g;
  const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int X = a.xa + (int)blockIdx.x * 64 + lane;
  const int Y0 = a.y0 + ((int)blockIdx.y * 4 + wave) * kTileRows;  // (the same in every lane of the wave)
  int c, offx, r, offy;
  const bool inx = tilemap_axis(X, m.ox, m.tile_w, m.cols, c, offx) && X >= a.x0 && X <= a.x1;
  bool iny = tilemap_axis(Y0, m.oy, m.tile_h, m.rows, r, offy);
  const int Xc = min(max(X, a.x0), a.x1);
  const float4 clear = make_float4(a.cr, a.cg, a.cb, a.ca);

  unsigned g[kTileRows];
  int oy[kTileRows];
  float4 d[kTileRows];
  float4 *out[kTileRows];
#pragma unroll
  for (int k = 0; k < kTileRows; ++k) {
    const int Y = Y0 + k;
    if (k > 0) iny = tilemap_axis_next(Y, m.oy, m.tile_h, m.rows, r, offy);
    // (c < cols, r < rows and the launch box lies in the target: inside the grid)
    g[k] = inx && iny && Y <= a.y1 ? a.cells[(size_t)r * (size_t)m.pitch + (size_t)c] : 0u;
    oy[k] = offy;
    out[k] = a.dst + (size_t)(a.H - 1 - min(Y, a.y1)) * (size_t)a.dpitch + (size_t)Xc;  // clamped into the box
    d[k] = clear;
    if (!REPLACE && !a.clear_on) d[k] = *out[k];
  }
  P p[kTileRows];
  int st[kTileRows];
#pragma unroll
  for (int k = 0; k < kTileRows; ++k) {
    int tx, ty, u, v;
    st[k] = tilemap_decode(g[k], m, tx, ty);  // (a word that was not loaded is 0: TILE_EMPTY)
    p[k] = P{};
    if (st[k] == TILE_DRAWN) {  // (u, v) lies in the tile's rectangle, which lies in the atlas
      tilemap_source(g[k], m, tx, ty, offx, oy[k], u, v);
      p[k] = *reinterpret_cast<const P *>(a.atlas + (size_t)v * a.apitch + (size_t)u * PXB);
    }
  }
  unsigned nd = 0u, nr = 0u;
#pragma unroll
  for (int k = 0; k < kTileRows; ++k) {
    const int Y = Y0 + k;
    const float4 val = write_value<U8, FMT>(p[k]);
    const float4 src = make_float4(val.x * a.tr, val.y * a.tg, val.z * a.tb, val.w * a.ta);
    float4 v;
    if (REPLACE) v = U8 ? GiU8::unpack(GiU8::pack(src)) : src;
    else v = U8 ? GiU8::blend(src, d[k]) : blend(src, d[k]);
    const bool drawn = st[k] == TILE_DRAWN;
    if (drawn) *out[k] = v;
    else if (a.clear_on && X >= a.x0 && X <= a.x1 && Y <= a.y1) *out[k] = clear;
    if (a.counters) {  // integer adds: the sums are the same in any order
      const bool first = tilemap_first_pixel(X, Y, offx, oy[k]);
      nd += (unsigned)__popcll(__ballot(first && drawn));
      nr += (unsigned)__popcll(__ballot(first && st[k] == TILE_REFUSED));
    }
  }
  if (a.counters && lane == 0) {
    const unsigned w = ((unsigned)blockIdx.y * gridDim.x + (unsigned)blockIdx.x) * 4u + (unsigned)wave;
    unsigned *slot = a.counters + (size_t)(w % kTileSlots) * kTileSlotWords;
    if (nd) atomicAdd(&slot[0], nd);
    if (nr) atomicAdd(&slot[1], nr);
  }
}

template <int FMT>
__global__ __launch_bounds__(256) void k_tilemap(const TilemapArgs a, const int mode) {
  switch (mode) {  // (uniform) bit 0: RGBA8_COMPAT storage, bit 1: RC2DGI_SPRITE_REPLACE
    case 0: tilemap_block<false, false, FMT>(a); break;
    case 1: tilemap_block<true, false, FMT>(a); break;
    case 2: tilemap_block<false, true, FMT>(a); break;
    default: tilemap_block<true, true, FMT>(a); break;
  }
}

__global__ __launch_bounds__(64) void k_tilemap_finish(unsigned *__restrict__ counters, int *__restrict__ status) {
  static_assert(kTileSlots == 64, "a lane a slot");
  unsigned *slot = counters + (size_t)threadIdx.x * kTileSlotWords;
  unsigned nd = slot[0], nr = slot[1];
  slot[0] = 0u;
  slot[1] = 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {  // integer adds: the sums are the same in any order
    nd += __shfl_down(nd, o);
    nr += __shfl_down(nr, o);
  }
  if (threadIdx.x == 0) {
    status[0] = (int)nd;
    status[1] = (int)nr;
  }
}

}  // namespace

hipError_t tilemap_device(float4 *dst, int W, int H, int pitch, bool u8, const unsigned char *clear,
                          const SpriteAtlas &atlas, const TilemapLayer &map, void *status_dev, unsigned **counters,
                          hipStream_t st) {
  const TilemapGeom &g = map.g;
  hipError_t e = hipSuccess;
  if (status_dev && !*counters) {  // the one place the call may wait: the first counted call's allocation
    e = hipMalloc(reinterpret_cast<void **>(counters), kTilemapCounterBytes);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(*counters, 0, kTilemapCounterBytes, st);
    if (e != hipSuccess) return e;
  }
  // the map's pixel box (cols * tile_w <= 2^30, |ox| <= 2^22), clipped to the target; the whole target with a clear
  const long long mx1 = (long long)g.ox + (long long)g.cols * g.tile_w - 1,
                  my1 = (long long)g.oy + (long long)g.rows * g.tile_h - 1;
  int x0 = std::max(g.ox, 0), y0 = std::max(g.oy, 0);
  int x1 = (int)std::min<long long>(mx1, W - 1), y1 = (int)std::min<long long>(my1, H - 1);
  if (clear) {
    x0 = y0 = 0;
    x1 = W - 1;
    y1 = H - 1;
  }
  if (x0 <= x1 && y0 <= y1) {
    const float4 cl = paint_dev_clear(clear, u8);
    const float tr = (float)map.tint[0], tg = (float)map.tint[1], tb = (float)map.tint[2], ta = (float)map.tint[3];
    TilemapArgs a{};
    a.dst = dst;
    a.dpitch = pitch;
    a.H = H;
    a.xa = x0 & ~63;
    a.x0 = x0;
    a.x1 = x1;
    a.y0 = y0;
    a.y1 = y1;
    a.cells = map.cells;
    a.g = g;
    a.atlas = atlas.dev;
    a.apitch = atlas.pitch;
    if (u8) {  // the tint of rc2dgi_sprites_device, per storage
      a.tr = tr * kInv255, a.tg = tg * kInv255, a.tb = tb * kInv255, a.ta = ta * kInv255;
    } else {
      a.tr = tr / 255.0f, a.tg = tg / 255.0f, a.tb = tb / 255.0f, a.ta = ta / 255.0f;
    }
    a.cr = cl.x, a.cg = cl.y, a.cb = cl.z, a.ca = cl.w;
    a.clear_on = clear ? 1 : 0;
    a.counters = status_dev ? *counters : nullptr;
    const int rows_wg = 4 * kTileRows;
    const dim3 grid((unsigned)((x1 - a.xa) / 64 + 1), (unsigned)((y1 - y0) / rows_wg + 1));
    const int mode = (u8 ? 1 : 0) | (map.replace ? 2 : 0);
    switch (atlas.format) {
      case RC2DGI_FMT_RGBA32F: hipLaunchKernelGGL(k_tilemap<RC2DGI_FMT_RGBA32F>, grid, dim3(256), 0, st, a, mode); break;
      case RC2DGI_FMT_RGBA16F: hipLaunchKernelGGL(k_tilemap<RC2DGI_FMT_RGBA16F>, grid, dim3(256), 0, st, a, mode); break;
      case RC2DGI_FMT_RGBA8: hipLaunchKernelGGL(k_tilemap<RC2DGI_FMT_RGBA8>, grid, dim3(256), 0, st, a, mode); break;
      default: return hipErrorInvalidValue;
    }
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (status_dev) {
    hipLaunchKernelGGL(k_tilemap_finish, dim3(1), dim3(64), 0, st, *counters, static_cast<int *>(status_dev));
    e = hipGetLastError();
  }
  return e;
}

}  // namespace rc2dgi
