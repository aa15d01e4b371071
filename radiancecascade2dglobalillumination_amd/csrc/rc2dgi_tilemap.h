// rc2dgi_tilemap.h -- rc2dgi_tilemap_device (include/rc2dgi.h): a regular grid of cell words on the device, each an
// index into a tile set (an atlas image), drawn as one layer into colorRT / emissiveRT with rc2dgi_sprites_device's
// values.  No list, no binning, no working memory: one streaming kernel.  See rc2dgi_tilemap.hip.
#pragma once

#include <hip/hip_runtime.h>

#include "rc2dgi_sprites.h"
#include "rc2dgi_tilemap_cell.h"

namespace rc2dgi {

struct TilemapLayer {  // rc2dgi_tilemap, validated
  const unsigned *cells;
  TilemapGeom g;
  unsigned char tint[4];
  bool replace;
};

// enqueues the whole drawing on `st` and returns (no wait but the first counted call's allocation of *counters).
// status_dev: null or two int32 {drawn, refused}.  *counters: the context's counters, kTilemapCounterBytes of device
// memory that are zero between calls (64 pairs a cache line apart, summed by the finishing wave); null until the first
// call with a status allocates them (the context frees them).
constexpr size_t kTilemapCounterBytes = 64 * 128;
hipError_t tilemap_device(float4 *dst, int W, int H, int pitch, bool u8, const unsigned char *clear,
                          const SpriteAtlas &atlas, const TilemapLayer &map, void *status_dev, unsigned **counters,
                          hipStream_t st);

}  // namespace rc2dgi
