// rc2dgi_gradients.h -- rc2dgi_gradients_device (include/rc2dgi.h): a device-resident list of 48-byte gradient records
// -- rc2dgi_shapes_device's five kinds with a colour a vertex and an HDR gain -- painted into colorRT / emissiveRT.
// See rc2dgi_gradients.hip.
#pragma once

#include "rc2dgi_paint.h"

namespace rc2dgi {

// enqueues the whole painting on `st` and returns (no wait but the first call's allocation of buf, which the call
// shares with the other list painters; it owns no memory of its own).  grads_dev: n records of rc2dgi_gradient, read
// by the set-up alone; count_dev: null or one int32; status_dev: null or two int32 {m, refused}.
hipError_t gradients_device(float4 *dst, int W, int H, int pitch, bool u8, const unsigned char *clear,
                            const void *grads_dev, int n, const void *count_dev, void *status_dev,
                            PaintDevBuffers &buf, hipStream_t st);

}  // namespace rc2dgi
