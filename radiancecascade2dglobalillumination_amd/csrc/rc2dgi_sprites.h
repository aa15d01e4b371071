// rc2dgi_sprites.h -- rc2dgi_sprites_device (include/rc2dgi.h): a device-resident list of sprites, each a rectangle of
// one atlas image drawn 1:1 at an integer position with a tint, into colorRT / emissiveRT with rc2dgi_write's values
// and rc2dgi_paint_device's ordered, binned, count-on-the-device list.  See rc2dgi_sprites.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "rc2dgi_paint.h"

namespace rc2dgi {

struct SpriteAtlas {  // rc2dgi_atlas, validated: the pitch resolved, in bytes and a multiple of a pixel
  const unsigned char *dev;
  int w, h;
  size_t pitch;
  int format;
};

// enqueues the whole drawing on `st` and returns (no wait but the first call's allocation of buf, which the call
// shares with paint_prims_device).  sprites_dev: n records of rc2dgi_sprite; count_dev: null or one int32; status_dev:
// null or two int32 {m, refused}.
hipError_t sprites_device(float4 *dst, int W, int H, int pitch, bool u8, const unsigned char *clear,
                          const SpriteAtlas &atlas, const void *sprites_dev, int n, const void *count_dev,
                          void *status_dev, PaintDevBuffers &buf, hipStream_t st);

}  // namespace rc2dgi
