// rc2dgi_sprites_xf.h -- rc2dgi_sprites_xf_device (include/rc2dgi.h): a device-resident list of sprites, each a
// rectangle of one atlas image mapped onto a parallelogram of the screen (scaled, rotated, sheared or mirrored; POINT or
// LINEAR), into colorRT / emissiveRT with rc2dgi_write's values and rc2dgi_paint_device's ordered, binned,
// count-on-the-device list.  See rc2dgi_sprites_xf.hip.
#pragma once

#include "rc2dgi_sprites.h"

namespace rc2dgi {

// enqueues the whole drawing on `st` and returns (no wait but the first call's allocation of buf, which the call
// shares with paint_prims_device and sprites_device).  sprites_dev: n records of rc2dgi_sprite_xf; count_dev: null or
// one int32; status_dev: null or two int32 {m, refused}.
hipError_t sprites_xf_device(float4 *dst, int W, int H, int pitch, bool u8, const unsigned char *clear,
                             const SpriteAtlas &atlas, const void *sprites_dev, int n, const void *count_dev,
                             void *status_dev, PaintDevBuffers &buf, hipStream_t st);

}  // namespace rc2dgi
