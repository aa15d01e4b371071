// rc2dgi_shapes.h -- rc2dgi_shapes_device (include/rc2dgi.h): a device-resident list of 32-byte shape records --
// rectangles, circles, triangles, thick lines and ellipses, mixed and in list order -- painted into colorRT /
// emissiveRT as rc2dgi_paint_device paints its primitives.  See rc2dgi_shapes.hip.
#pragma once

#include "rc2dgi_paint.h"

namespace rc2dgi {

// enqueues the whole painting on `st` and returns (no wait but the first call's allocation of buf, which the call
// shares with paint_prims_device and the sprite lists).  shapes_dev: n records of rc2dgi_shape; count_dev: null or one
// int32; status_dev: null or two int32 {m, refused}.
hipError_t shapes_device(float4 *dst, int W, int H, int pitch, bool u8, const unsigned char *clear,
                         const void *shapes_dev, int n, const void *count_dev, void *status_dev, PaintDevBuffers &buf,
                         hipStream_t st);

// k_shapes_bin over the nb records of the batch at `base`, as shapes_device launches it: prims / tris are the batch's
// PaintPrim and PaintTri records.  rc2dgi_gradients_device (rc2dgi_gradients.hip) runs it unchanged on records of its
// own set-up.
void shapes_enqueue_bin(const void *prims, const void *tris, int n, const int *count_dev, int base, int nb,
                        const PaintDevPlan &plan, unsigned *masks, hipStream_t st);

}  // namespace rc2dgi
