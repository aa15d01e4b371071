// rc2dgi_present.h -- the display frame composed on the device (rc2dgi_compose / rc2dgi_compose_device,
// include/rc2dgi.h): the reference's final blit and debug thumbnails (RC2DGI.cs:135-165, 435-448) as one kernel
// over the render textures in their stored formats.  See rc2dgi_present.hip.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/rc2dgi.h"

namespace rc2dgi {

// how a render texture is stored (what a texel fetch decodes)
enum PresentKind {
  PK_F32 = 0,    // float4
  PK_F16 = 1,    // RGBA16F (giRT1 / giRT2 of RC2DGI_STORAGE_F16)
  PK_U8 = 2,     // RGBA8 bytes (giRT1 / giRT2 / cascadeBlurRT of RC2DGI_STORAGE_RGBA8_COMPAT)
  PK_JUMP = 3,   // packed seed sj << 16 | si, 0x80008000 = none -> (u, v, 0, 1) / (0, 0, 0, 1)
  PK_JUMP8 = 4,  // unorm8 seed uv kv << 16 | ku -> (ku, kv, 0, 255) * (1/255)
  PK_DIST = 5,   // 16-bit q -> (hi / 255, lo / 255, 0, 1)
  PK_DIST8 = 6,  // the same as RGBA8 texels: (hi, lo, 0, 255) * (1/255)
  PK_CONST = 7   // (0, 0, 0, 1): giRT2 with one cascade (ClearAllRTs content)
};

// a render texture resolved on the host (resolve_texture, rc2dgi_accessory.h): the source in its stored format, as
// rc2dgi_download reads it.  What k_present fetches for a view and k_sample (rc2dgi_query.hip) for a point; the
// decoder of both is rc2dgi_texel.h.
struct TexSource {
  const void *src;
  int pitch;           // texels a row
  int nx, powx;        // texture width, and whether it is a power of two (GL wrap arithmetic differs)
  int ny, powy;
  int kind;            // PresentKind
  int linear;          // LINEAR filter (else POINT)
};

// one view, resolved on the host: its texture and the rectangles the kernel tests
struct PresentView : TexSource {
  int x, y, w, h;      // the view's rectangle as given (may hang over the window)
  unsigned border;     // r | g << 8 | b << 16 | a << 24; a == 0: none
  int cx0, cx1, cy0, cy1;  // the rectangle clipped to the window, [c*0, c*1)
  int fx0, fx1, fy0, fy1;  // where a pixel is the plain blit of one texel: the clipped rectangle without the border
                           // of a 1:1 POINT view of float4 / RGBA8 texels, else empty
};

struct PresentArgs {
  PresentView v[RC2DGI_MAX_VIEWS];
  int n;
  unsigned clear;  // r | g << 8 | b << 16 | a << 24
  int out_w, out_h;
};

// One launch on `st`: the out_w x out_h window into dst (row 0 = top, pitch_bytes a row, a multiple of 4 as dst is).
hipError_t launch_present(const PresentArgs &a, void *dst, int pitch_bytes, hipStream_t st);

}  // namespace rc2dgi
