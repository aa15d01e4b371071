// rc2dgi_accessory.h -- what the host units of the accessory calls share: rc2dgi_display.cpp (the display frame and
// its tone curves), rc2dgi_regions.cpp (rectangles: reduce, histogram, read) and rc2dgi_points.cpp (points: sample,
// raycast).  A render texture id resolved as rc2dgi_download reads it, the refusal of a row-strip shard, and the
// frame of a host variant: synchronise, report a chain timeout, grow a buffer, enqueue, copy back, synchronise.
#pragma once

#include "rc2dgi_ctx.h"

namespace rc2dgi {

inline bool linear_rt(int which) {  // the textures the reference filters LINEAR (RC2DGI.cs:89-98)
  return which == RC2DGI_RT_GI1 || which == RC2DGI_RT_GI2 || which == RC2DGI_RT_BLUR || which == RC2DGI_RT_FINAL_GI;
}

// A render texture id and a filter resolved to source pointer, pitch, axes, storage kind and filter, as
// rc2dgi_download reads that texture: what a compose view draws, a point sample fetches and a rectangle call reads.
// `tag` heads the message.
inline int resolve_texture(rc2dgi_ctx *c, int which, int filter, const std::string &tag, TexSource &v) {
  if (which < RC2DGI_RT_COLOR || which > RC2DGI_RT_FINAL_GI) return fail(c, RC2DGI_E_ARG, tag + "bad render texture id");
  if (filter != RC2DGI_FILTER_RT && filter != RC2DGI_FILTER_POINT && filter != RC2DGI_FILTER_LINEAR)
    return fail(c, RC2DGI_E_ARG, tag + "bad filter");
  if (filter == RC2DGI_FILTER_LINEAR && !linear_rt(which))
    return fail(c, RC2DGI_E_UNSUPPORTED, tag + "LINEAR is for GI1 / GI2 / BLUR / FINAL_GI");
  v.linear = filter == RC2DGI_FILTER_LINEAR || (filter == RC2DGI_FILTER_RT && linear_rt(which));
  if (which == RC2DGI_RT_FINAL_GI) which = (c->N % 2 == 0) ? RC2DGI_RT_GI2 : RC2DGI_RT_GI1;
  const bool scr = !linear_rt(which);
  v.nx = scr ? c->W : c->CW;
  v.ny = scr ? c->H : c->CH;
  v.powx = is_pow2(v.nx);
  v.powy = is_pow2(v.ny);
  v.pitch = scr ? c->sd.pitch : c->cd.pitch;
  const bool u8 = rgba8(c);
  const int gi_kind = u8 ? PK_U8 : (c->storage == RC2DGI_STORAGE_F16 ? PK_F16 : PK_F32);
  switch (which) {
    case RC2DGI_RT_COLOR: v.src = c->frame_done ? c->color_out : c->color_in; v.kind = PK_F32; break;
    case RC2DGI_RT_EMISSIVE: v.src = c->emissive; v.kind = PK_F32; break;
    case RC2DGI_RT_TEMP: v.src = c->temp; v.kind = PK_F32; break;
    case RC2DGI_RT_JUMP1: v.src = c->jump1; v.kind = u8 ? PK_JUMP8 : PK_JUMP; break;
    case RC2DGI_RT_JUMP2: v.src = c->jump2; v.kind = u8 ? PK_JUMP8 : PK_JUMP; break;
    case RC2DGI_RT_DIST: v.src = c->dist; v.kind = u8 ? PK_DIST8 : PK_DIST; break;
    case RC2DGI_RT_GI1: v.src = c->gi1; v.kind = gi_kind; break;
    case RC2DGI_RT_GI2: v.src = c->gi2; v.kind = c->N == 1 ? PK_CONST : gi_kind; break;  // never drawn with one cascade
    default: v.src = c->blur; v.kind = u8 ? PK_U8 : PK_F32; break;  // RC2DGI_RT_BLUR
  }
  return RC2DGI_OK;
}

inline bool aligned_to(const void *p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// A row-strip shard's textures hold windows and bands, so every accessory call refuses one.  `verb`: "query",
// "reduce on", "compose on", "histogram on", "read on".
inline int refuse_shard(rc2dgi_ctx *c, const char *verb) {
  if (c->world <= 1) return RC2DGI_OK;
  return fail(c, RC2DGI_E_UNSUPPORTED,
              std::string("a row-strip shard's textures hold windows and bands: ") + verb + " an unsharded context");
}

// grow one of the context's on-demand buffers (the stream is idle: nothing uses the old one)
inline int grow_buffer(rc2dgi_ctx *c, unsigned char *&buf, size_t &cap, size_t need) {
  if (need <= cap) return RC2DGI_OK;
  if (buf) HIPCHK(c, hipFree(buf));
  buf = nullptr;
  cap = 0;
  HIPCHK(c, alloc(&buf, need));
  cap = need;
  return RC2DGI_OK;
}

// how every host variant begins: the stream is idle afterwards, and a chain timeout of the last frame is reported
inline int host_begin(rc2dgi_ctx *c) {
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return check_chain(c);
}

// A host variant whole: host_begin, the context's query buffers grown to in_bytes (0: the call uploads nothing) and
// out_bytes, `in` uploaded, enqueue(device in, device out) on the context stream, `out` copied back, synchronised.
template <class Enqueue>
int host_call(rc2dgi_ctx *c, const void *in, size_t in_bytes, void *out, size_t out_bytes, Enqueue enqueue) {
  if (int rc = host_begin(c)) return rc;
  if (in_bytes)
    if (int rc = grow_buffer(c, c->query_in, c->query_in_cap, in_bytes)) return rc;
  if (int rc = grow_buffer(c, c->query_out, c->query_out_cap, out_bytes)) return rc;
  if (in_bytes) HIPCHK(c, hipMemcpyAsync(c->query_in, in, in_bytes, hipMemcpyHostToDevice, c->stream));
  if (int rc = enqueue(c->query_in, c->query_out)) return rc;
  HIPCHK(c, hipMemcpyAsync(out, c->query_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return RC2DGI_OK;
}

}  // namespace rc2dgi
