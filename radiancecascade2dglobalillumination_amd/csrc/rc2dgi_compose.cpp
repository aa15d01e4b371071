// rc2dgi_compose.cpp -- the display frame of the C ABI (include/rc2dgi.h): the reference's display layout
// (RC2DGI.cs:139-163), and the views resolved to their stored textures for k_present (rc2dgi_present.hip).  The
// queries too (rc2dgi_sample / rc2dgi_raycast, rc2dgi_query.hip): a point sample resolves its texture as a view does,
// and so do the region statistics (rc2dgi_reduce, rc2dgi_reduce.hip), whose rectangles are planned here.  Last the
// edge tables: the tone curves of the views (rc2dgi_set_curve / rc2dgi_compose_tone, rc2dgi_tone.hip) and the
// histograms of rectangles (rc2dgi_histogram, rc2dgi_hist.hip), planned as the reductions are -- and a rectangle read as
// an image (rc2dgi_read, rc2dgi_read.hip), staged through a bounded buffer for the host.
#include "rc2dgi_ctx.h"

#include <cstddef>

namespace {

constexpr int kMaxOut = 32768;

bool linear_rt(int which) {  // the textures the reference filters LINEAR (RC2DGI.cs:89-98)
  return which == RC2DGI_RT_GI1 || which == RC2DGI_RT_GI2 || which == RC2DGI_RT_BLUR || which == RC2DGI_RT_FINAL_GI;
}

unsigned pack_rgba(const unsigned char *p) {
  return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
}

int clampi(long long v, int lo, int hi) { return (int)std::min<long long>(std::max<long long>(v, lo), hi); }

// A render texture id and a filter resolved to source pointer, pitch, axes, storage kind and filter, as
// rc2dgi_download reads that texture: what a compose view draws and a point sample fetches.  `tag` heads the message.
int resolve_texture(rc2dgi_ctx *c, int which, int filter, const std::string &tag, TexSource &v) {
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

// the checks the four query calls share; n == 0 is left to the caller (a successful no-op)
int query_args(rc2dgi_ctx *c, const void *in, int n, const void *out) {
  if (!c) return RC2DGI_E_ARG;
  RC2DGI_USABLE(c);
  if (n < 0 || n > kQueryMax) return fail(c, RC2DGI_E_ARG, "n is 0 .. 1 << 24");
  if (n > 0 && (!in || !out)) return fail(c, RC2DGI_E_ARG, "null argument");
  if (c->world > 1)
    return fail(c, RC2DGI_E_UNSUPPORTED, "a row-strip shard's textures hold windows and bands: query an unsharded context");
  return RC2DGI_OK;
}

int ray_scene(rc2dgi_ctx *c, RayScene &s) {
  if (!c->have_frame) return fail(c, RC2DGI_E_STATE, "a ray cast marches the last frame's distRT: run a frame first");
  const float mx = (float)std::max(c->W, c->H);
  s = RayScene{c->dist, c->color_in, c->emissive, c->sd.pitch, c->W, is_pow2(c->W) ? 1 : 0, c->H, is_pow2(c->H) ? 1 : 0,
               (float)c->W / mx, (float)c->H / mx, c->reflectivity};
  return RC2DGI_OK;
}

// grow one of the context's query buffers (the stream is idle: nothing uses the old one)
int query_buffer(rc2dgi_ctx *c, unsigned char *&buf, size_t &cap, size_t need) {
  if (need <= cap) return RC2DGI_OK;
  if (buf) HIPCHK(c, hipFree(buf));
  buf = nullptr;
  cap = 0;
  HIPCHK(c, alloc(&buf, need));
  cap = need;
  return RC2DGI_OK;
}

// The host variants: synchronise, report a chain timeout, upload `in`, run `launch` over the context's buffers, copy
// `out` back.
template <class Launch>
int query_host(rc2dgi_ctx *c, const void *in, size_t in_bytes, void *out, size_t out_bytes, Launch launch) {
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (int rc = check_chain(c)) return rc;
  if (int rc = query_buffer(c, c->query_in, c->query_in_cap, in_bytes)) return rc;
  if (int rc = query_buffer(c, c->query_out, c->query_out_cap, out_bytes)) return rc;
  HIPCHK(c, hipMemcpyAsync(c->query_in, in, in_bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, launch(c->query_in, c->query_out));
  HIPCHK(c, hipMemcpyAsync(out, c->query_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return RC2DGI_OK;
}

bool aligned_to(const void *p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

static_assert(sizeof(rc2dgi_ray) == 24 && sizeof(rc2dgi_rayhit) == 44, "the query records are 24 and 44 bytes");

// ---- region statistics (rc2dgi_reduce.hip): the host validates the rectangles and cuts them into work items

static_assert(sizeof(rc2dgi_rect) == 16 && sizeof(rc2dgi_stats) == 88 && offsetof(rc2dgi_stats, sum) == 56,
              "the region records are 16 and 88 bytes");

// the device side of one batch: [items, then joins | band partials], a fixed size whatever the call
constexpr size_t kReducePlanBytes = (size_t)kReduceBatch * (sizeof(ReduceItem) + sizeof(ReduceJoin));
constexpr size_t reduce_bytes = kReducePlanBytes + (size_t)kReduceBatch * sizeof(ReducePartial);

struct ReduceBatch {
  std::vector<ReduceItem> items;
  std::vector<ReduceJoin> joins;
  std::vector<unsigned char> blob;  // the two as uploaded
  int parts = 0;
};

bool rect_valid(const rc2dgi_rect &r, int tw, int th) {  // (in this form nothing overflows)
  return r.w >= 1 && r.h >= 1 && r.x >= 0 && r.y >= 0 && r.w <= tw - r.x && r.h <= th - r.y;
}

// Rows of a band of a w x h rectangle, a power of two: a wave gets about 4096 texels (whole passes of 64 / lanes-a-row
// rows when the rows are narrow, k_reduce_rows; at most 1024 rows), and a rectangle at most kReduceMaxBands bands
// (only a rectangle of more than 2^22 rows gets taller bands for that).
int reduce_band_rows(int w, int h) {
  long long rw = 1;
  if (w <= kReduceChunk) {
    int lr = 1;
    while (lr * kReduceLeaves < w) lr <<= 1;
    rw = 64 / lr;
    while (rw * w < 4096 && rw < 1024) rw <<= 1;
  } else {
    while (rw * 2 * w <= 4096) rw <<= 1;
  }
  while ((h + rw - 1) / rw > kReduceMaxBands) rw <<= 1;
  return (int)std::min<long long>(rw, 1 << 30);
}

// one batch: upload its plan in one copy (stream-ordered, after the kernels that read the previous one), two launches
int reduce_flush(rc2dgi_ctx *c, const TexSource &t, ReduceBatch &b, void *stats_dev) {
  if (b.items.empty()) return RC2DGI_OK;
  const int ni = (int)b.items.size(), nj = (int)b.joins.size();
  // the joins ride behind the items in the host vector and on the device
  static_assert(alignof(ReduceJoin) == 4 && alignof(ReduceItem) == 4, "a join may follow any number of items");
  const size_t ibytes = (size_t)ni * sizeof(ReduceItem), jbytes = (size_t)nj * sizeof(ReduceJoin);
  std::vector<unsigned char> &blob = b.blob;
  blob.resize(ibytes + jbytes);
  std::memcpy(blob.data(), b.items.data(), ibytes);
  if (nj) std::memcpy(blob.data() + ibytes, b.joins.data(), jbytes);
  ReduceItem *items = reinterpret_cast<ReduceItem *>(c->reduce_buf);
  ReduceJoin *joins = reinterpret_cast<ReduceJoin *>(c->reduce_buf + ibytes);
  ReducePartial *parts = reinterpret_cast<ReducePartial *>(c->reduce_buf + kReducePlanBytes);
  const ReduceInline none{};
  HIPCHK(c, hipMemcpyAsync(c->reduce_buf, blob.data(), blob.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, launch_reduce_rows(t, none, items, ni, parts, stats_dev, c->stream));
  if (nj) HIPCHK(c, launch_reduce_bands(none, joins, nj, parts, stats_dev, c->stream));
  return RC2DGI_OK;
}

// n >= 1 rectangles of t into the device records stats_dev, enqueued on the context stream.  The scratch is one
// batch's, however long the list and however tall a rectangle: a full batch is launched and the next one planned.
int reduce_enqueue(rc2dgi_ctx *c, const TexSource &t, const rc2dgi_rect *rects, int n, void *stats_dev) {
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->reduce_buf) HIPCHK(c, alloc(&c->reduce_buf, reduce_bytes));
  ReducePartial *parts = reinterpret_cast<ReducePartial *>(c->reduce_buf + kReducePlanBytes);
  if (n <= kReduceInline) {  // the plan fits the kernels' arguments: no upload
    ReduceInline inl{};
    inl.n = n;
    int items = 0, nparts = 0;
    for (int k = 0; k < n; ++k) {
      const rc2dgi_rect &r = rects[k];
      ReduceDesc &d = inl.d[k];
      d = ReduceDesc{0, 0, 0, 0, 1, items, nparts, k};
      int nb = 1;
      if (rect_valid(r, t.nx, t.ny)) {
        const int rw = reduce_band_rows(r.w, r.h);
        nb = (int)(((long long)r.h + rw - 1) / rw);
        d = ReduceDesc{r.x, r.y, r.w, r.h, rw, items, nparts, k};
      }
      items += nb;
      if (nb > 1) nparts += nb;
    }
    HIPCHK(c, launch_reduce_rows(t, inl, nullptr, items, parts, stats_dev, c->stream));
    if (nparts) HIPCHK(c, launch_reduce_bands(inl, nullptr, n, parts, stats_dev, c->stream));
    return RC2DGI_OK;
  }
  // One batch of host vectors, planned again after each flush: the copy of a flush has consumed them when it returns
  // (pageable memory, as paint_prims relies on for its vectors), so host memory is one batch's too.
  ReduceBatch b;
  for (int k = 0; k < n; ++k) {
    const rc2dgi_rect &r = rects[k];
    const bool ok = rect_valid(r, t.nx, t.ny);
    const int rw = ok ? reduce_band_rows(r.w, r.h) : 1;
    const int nb = ok ? (int)(((long long)r.h + rw - 1) / rw) : 1;
    if (b.items.size() + (size_t)nb > (size_t)kReduceBatch) {
      if (int rc = reduce_flush(c, t, b, stats_dev)) return rc;
      b.items.clear();
      b.joins.clear();
      b.parts = 0;
    }
    if (!ok) {
      b.items.push_back(ReduceItem{0, 0, 0, 0, 0, (unsigned)k | kReduceFinal});
    } else if (nb == 1) {
      b.items.push_back(ReduceItem{r.x, r.y, r.w, 0, r.h, (unsigned)k | kReduceFinal});
    } else {
      b.joins.push_back(ReduceJoin{b.parts, nb, k, r.w * r.h});
      for (int i = 0; i < nb; ++i)
        b.items.push_back(ReduceItem{r.x, r.y, r.w, i * rw, (int)std::min<long long>((long long)(i + 1) * rw, r.h),
                                     (unsigned)b.parts++});
    }
  }
  return reduce_flush(c, t, b, stats_dev);
}

// the checks the two calls share; n == 0 is left to the caller (a successful no-op)
int reduce_args(rc2dgi_ctx *c, int which, const rc2dgi_rect *rects, int n, const void *stats, TexSource &t) {
  if (!c) return RC2DGI_E_ARG;
  RC2DGI_USABLE(c);
  if (n < 0 || n > kReduceMax) return fail(c, RC2DGI_E_ARG, "reduce: n is 0 .. 1 << 20");
  if (n > 0 && (!rects || !stats)) return fail(c, RC2DGI_E_ARG, "reduce: null argument");
  if (int rc = resolve_texture(c, which, RC2DGI_FILTER_POINT, "reduce: ", t)) return rc;
  if (c->world > 1)
    return fail(c, RC2DGI_E_UNSUPPORTED, "a row-strip shard's textures hold windows and bands: reduce on an unsharded context");
  return RC2DGI_OK;
}

// Validate the call and resolve every view to source pointer, pitch, axes, storage kind and filter, as
// rc2dgi_download reads that texture.  Views that miss the window are dropped.
// With `tones` (n records, or null) the tone of every kept view goes to `tn`, and *toned tells whether any differs from
// {1.0f, 0}: where none does the call is rc2dgi_compose's own kernel.
int resolve_views(rc2dgi_ctx *c, const rc2dgi_view *views, int n, int out_w, int out_h, const unsigned char *clear,
                  const void *dst, int *pitch_bytes, PresentArgs &a, const rc2dgi_tone *tones = nullptr,
                  ToneArgs *tn = nullptr, bool *toned = nullptr) {
  if (!c || !views || !dst) return fail(c, RC2DGI_E_ARG, "null argument");
  RC2DGI_USABLE(c);
  if (c->world > 1)
    return fail(c, RC2DGI_E_UNSUPPORTED, "a row-strip shard's textures hold windows and bands: compose on an unsharded context");
  if (n < 1 || n > RC2DGI_MAX_VIEWS) return fail(c, RC2DGI_E_ARG, "1 .. RC2DGI_MAX_VIEWS views");
  if (out_w < 1 || out_h < 1 || out_w > kMaxOut || out_h > kMaxOut)
    return fail(c, RC2DGI_E_ARG, "the window is 1 .. 32768 pixels on each side");
  if (*pitch_bytes == 0) *pitch_bytes = out_w * 4;
  if (*pitch_bytes < out_w * 4) return fail(c, RC2DGI_E_ARG, "pitch smaller than a row");
  if (*pitch_bytes % 4 != 0) return fail(c, RC2DGI_E_ARG, "the pitch is a multiple of 4 bytes");
  static const unsigned char black[4] = {0, 0, 0, 255};
  a.n = 0;
  a.clear = pack_rgba(clear ? clear : black);
  a.out_w = out_w;
  a.out_h = out_h;
  for (int k = 0; k < n; ++k) {
    const rc2dgi_view &q = views[k];
    const std::string tag = "view " + std::to_string(k) + ": ";
    if (q.which < RC2DGI_RT_COLOR || q.which > RC2DGI_RT_FINAL_GI) return fail(c, RC2DGI_E_ARG, tag + "bad render texture id");
    if (q.w < 1 || q.h < 1) return fail(c, RC2DGI_E_ARG, tag + "w and h are at least 1");
    PresentView v{};
    if (int rc = resolve_texture(c, q.which, q.filter, tag, v)) return rc;
    const rc2dgi_tone tone = tones ? tones[k] : rc2dgi_tone{1.0f, 0};
    if (!(tone.exposure >= 0.0f) || std::isinf(tone.exposure))
      return fail(c, RC2DGI_E_ARG, tag + "the exposure is finite and not negative");
    if (tone.curve < 0 || tone.curve > RC2DGI_MAX_CURVES)
      return fail(c, RC2DGI_E_ARG, tag + "the curve is 0 .. RC2DGI_MAX_CURVES");
    if (tone.curve > 0 && c->curve_host[tone.curve - 1].empty())
      return fail(c, RC2DGI_E_STATE, tag + "its curve slot is not set (rc2dgi_set_curve)");
    v.x = q.x;
    v.y = q.y;
    v.w = q.w;
    v.h = q.h;
    v.border = q.a ? pack_rgba(&q.r) : 0u;
    const long long x1 = (long long)q.x + q.w, y1 = (long long)q.y + q.h;
    v.cx0 = clampi(q.x, 0, out_w);
    v.cx1 = clampi(x1, 0, out_w);
    v.cy0 = clampi(q.y, 0, out_h);
    v.cy1 = clampi(y1, 0, out_h);
    if (v.cx0 >= v.cx1 || v.cy0 >= v.cy1) continue;  // wholly outside the window
    const bool blit = !v.linear && q.w == v.nx && q.h == v.ny && (v.kind == PK_F32 || v.kind == PK_U8);
    const int b = q.a ? 1 : 0;
    if (blit) {
      v.fx0 = clampi((long long)q.x + b, 0, out_w);
      v.fx1 = clampi(x1 - b, 0, out_w);
      v.fy0 = clampi((long long)q.y + b, 0, out_h);
      v.fy1 = clampi(y1 - b, 0, out_h);
    }
    if (tn) {
      tn->exposure[a.n] = tone.exposure;
      tn->curve[a.n] = tone.curve;
      if (tone.curve > 0) tn->used |= 1u << (tone.curve - 1);
      if (tone.exposure != 1.0f || tone.curve != 0) *toned = true;
    }
    a.v[a.n++] = v;
  }
  return RC2DGI_OK;
}

// ---- edge tables

int check_edges(const float *e, int m) {
  if (!e || m < 1) return RC2DGI_E_ARG;
  for (int i = 0; i < m; ++i)
    if (std::isnan(e[i]) || (i + 1 < m && e[i] > e[i + 1])) return RC2DGI_E_ARG;
  return RC2DGI_OK;
}

// q8 as rc2dgi_device.h states it (the host's rintf rounds to nearest even, as v_rndne does)
unsigned q8_host(float x) { return (unsigned)std::rint(std::fmin(std::fmax(x, 0.0f), 1.0f) * 255.0f); }

float bits_float(uint32_t b) {
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}

// the two kernels of a display frame: k_present where no view is toned
int launch_frame(rc2dgi_ctx *c, const PresentArgs &a, ToneArgs &tn, bool toned, void *dst, int pitch_bytes) {
  if (!toned) {
    HIPCHK(c, launch_present(a, dst, pitch_bytes, c->stream));
    return RC2DGI_OK;
  }
  tn.tables = c->curves_dev;  // (a named slot is set, so the tables exist)
  HIPCHK(c, launch_present_tone(a, tn, dst, pitch_bytes, c->stream));
  return RC2DGI_OK;
}

int compose_device(rc2dgi_ctx *c, const rc2dgi_view *views, const rc2dgi_tone *tones, int n, int out_w, int out_h,
                   const unsigned char *clear_rgba, void *dev, int pitch_bytes) {
  PresentArgs a;
  ToneArgs tn{};
  bool toned = false;
  if (int rc = resolve_views(c, views, n, out_w, out_h, clear_rgba, dev, &pitch_bytes, a, tones, &tn, &toned)) return rc;
  if (reinterpret_cast<uintptr_t>(dev) % 4 != 0) return fail(c, RC2DGI_E_ARG, "the destination is aligned to 4 bytes");
  HIPCHK(c, hipSetDevice(c->device));
  return launch_frame(c, a, tn, toned, dev, pitch_bytes);
}

int compose_host(rc2dgi_ctx *c, const rc2dgi_view *views, const rc2dgi_tone *tones, int n, int out_w, int out_h,
                 const unsigned char *clear_rgba, void *host, int pitch_bytes) {
  PresentArgs a;
  ToneArgs tn{};
  bool toned = false;
  if (int rc = resolve_views(c, views, n, out_w, out_h, clear_rgba, host, &pitch_bytes, a, tones, &tn, &toned)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (int rc = check_chain(c)) return rc;
  const size_t dpitch = (size_t)round_up(out_w, 4) * 4, need = dpitch * (size_t)out_h;  // 16-byte rows: vector stores
  if (need > c->present_cap) {  // (the stream is idle: nothing reads the old image)
    if (c->present_buf) HIPCHK(c, hipFree(c->present_buf));
    c->present_buf = nullptr;
    c->present_cap = 0;
    HIPCHK(c, alloc(&c->present_buf, need));
    c->present_cap = need;
  }
  if (int rc = launch_frame(c, a, tn, toned, c->present_buf, (int)dpitch)) return rc;
  HIPCHK(c, hipMemcpy2DAsync(host, (size_t)pitch_bytes, c->present_buf, dpitch, (size_t)out_w * 4, (size_t)out_h,
                             hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return RC2DGI_OK;
}

// ---- histograms (rc2dgi_hist.hip): the host validates the rectangles and cuts them into row blocks

// the device side: the tree of the edges, then one batch of work items -- a fixed size whatever the call
constexpr size_t kHistTreeBytes = (size_t)kHistTreeWords * sizeof(float);
constexpr size_t hist_bytes = kHistTreeBytes + (size_t)kHistBatch * sizeof(HistItem);

// Rows of a block of a w x h rectangle: a 1024th of the rectangle, but between kHistMinItemTexels and kHistItemTexels
// texels (a texture of any size then spreads over the device, and a large one does not flush a record's counters more
// often than it must), in whole passes of the workgroup (256 / lanes-a-row rows when the rows are narrow, k_hist), at
// most kHistMaxBlocks blocks a rectangle.  Any cut gives the same counts.
int hist_block_rows(int w, int h) {
  long long gr = 1;
  if (w <= 1024) {
    int lr = 1;
    while (lr * 4 < w) lr <<= 1;
    gr = 256 / lr;
  }
  const long long target =
      std::min<long long>(std::max<long long>((long long)w * h / 1024, kHistMinItemTexels), kHistItemTexels);
  long long rows = (target + w - 1) / w;
  rows = (rows + gr - 1) / gr * gr;
  while ((h + rows - 1) / rows > kHistMaxBlocks) rows <<= 1;
  return (int)std::min<long long>(rows, 1 << 30);
}

// n >= 1 rectangles of t into the device records counts_dev, enqueued on the context stream: the launches that store
// the tree (the first one clears the records too), then one launch an inline plan or a batch.
int hist_enqueue(rc2dgi_ctx *c, const TexSource &t, int channel, const rc2dgi_rect *rects, int n, const float *edges,
                 int m, void *counts_dev) {
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->hist_buf) HIPCHK(c, alloc(&c->hist_buf, hist_bytes));
  float *tree_dev = reinterpret_cast<float *>(c->hist_buf);
  HistItem *items_dev = reinterpret_cast<HistItem *>(c->hist_buf + kHistTreeBytes);
  const int levels = tree_levels(m), words = 1 << levels;
  float tree[kHistTreeWords];
  tree_layout(edges, m, levels, std::numeric_limits<float>::quiet_NaN(), tree);
  for (int w0 = 0; w0 < words; w0 += kTableChunk) {
    TableChunk ch;
    const int nw = std::min(kTableChunk, words - w0);
    std::memcpy(ch.v, tree + w0, (size_t)nw * sizeof(float));
    HIPCHK(c, launch_store_table(ch, nw, tree_dev + w0, w0 == 0 ? static_cast<unsigned *>(counts_dev) : nullptr,
                                 w0 == 0 ? (size_t)n * (size_t)(m + 4) : 0, c->stream));
  }
  const HistTable tab{tree_dev, levels, m, channel};
  if (n <= kHistInline) {  // the plan fits the kernel's arguments: no upload
    HistInline inl{};
    inl.n = n;
    int items = 0;
    for (int k = 0; k < n; ++k) {
      const rc2dgi_rect &r = rects[k];
      int nb = 1;
      inl.d[k] = HistDesc{0, 0, 0, 0, 1, items, k, 0};
      if (rect_valid(r, t.nx, t.ny)) {
        const int rows = hist_block_rows(r.w, r.h);
        nb = (int)(((long long)r.h + rows - 1) / rows);
        inl.d[k] = HistDesc{r.x, r.y, r.w, r.h, rows, items, k, 0};
      }
      items += nb;
    }
    HIPCHK(c, launch_hist(t, inl, nullptr, items, tab, counts_dev, c->stream));
    return RC2DGI_OK;
  }
  // One batch of host items at a time, as reduce_enqueue: the copy of a flush has consumed the vector when it returns.
  const HistInline none{};
  std::vector<HistItem> b;
  auto flush = [&]() -> int {
    if (b.empty()) return RC2DGI_OK;
    HIPCHK(c, hipMemcpyAsync(items_dev, b.data(), b.size() * sizeof(HistItem), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_hist(t, none, items_dev, (int)b.size(), tab, counts_dev, c->stream));
    b.clear();
    return RC2DGI_OK;
  };
  for (int k = 0; k < n; ++k) {
    const rc2dgi_rect &r = rects[k];
    if (!rect_valid(r, t.nx, t.ny)) {
      if (b.size() + 1 > (size_t)kHistBatch)
        if (int rc = flush()) return rc;
      b.push_back(HistItem{0, 0, 0, 0, 0, 0, (unsigned)k | kHistSingle | kHistFirst});
      continue;
    }
    const int rows = hist_block_rows(r.w, r.h);
    const int nb = (int)(((long long)r.h + rows - 1) / rows);
    for (int i = 0; i < nb; ++i) {  // (the blocks of a rectangle may fall into different batches: they only add)
      if (b.size() + 1 > (size_t)kHistBatch)
        if (int rc = flush()) return rc;
      b.push_back(HistItem{r.x, r.y, r.w, i * rows, (int)std::min<long long>((long long)(i + 1) * rows, r.h), r.w * r.h,
                           (unsigned)k | (nb == 1 ? kHistSingle : 0u) | (i == 0 ? kHistFirst : 0u)});
    }
  }
  return flush();
}

// the checks the two calls share; n == 0 is left to the caller (a successful no-op)
int hist_args(rc2dgi_ctx *c, int which, int channel, const rc2dgi_rect *rects, int n, const float *edges, int m,
              const void *counts, TexSource &t) {
  if (!c) return RC2DGI_E_ARG;
  RC2DGI_USABLE(c);
  if (n < 0 || n > kHistMax) return fail(c, RC2DGI_E_ARG, "histogram: n is 0 .. 1 << 20");
  if (m < 1 || m > RC2DGI_HIST_MAX_EDGES) return fail(c, RC2DGI_E_ARG, "histogram: m is 1 .. RC2DGI_HIST_MAX_EDGES");
  if ((long long)n * (m + 4) > kHistMaxWords) return fail(c, RC2DGI_E_ARG, "histogram: n * (m + 4) is at most 1 << 26");
  if (check_edges(edges, m) != RC2DGI_OK)
    return fail(c, RC2DGI_E_ARG, "histogram: the edges are m ascending floats, none a NaN (rc2dgi_check_edges)");
  if (channel < RC2DGI_CH_R || channel > RC2DGI_CH_LUMA) return fail(c, RC2DGI_E_ARG, "histogram: bad channel");
  if (n > 0 && (!rects || !counts)) return fail(c, RC2DGI_E_ARG, "histogram: null argument");
  if (int rc = resolve_texture(c, which, RC2DGI_FILTER_POINT, "histogram: ", t)) return rc;
  if (c->world > 1)
    return fail(c, RC2DGI_E_UNSUPPORTED,
                "a row-strip shard's textures hold windows and bands: histogram on an unsharded context");
  return RC2DGI_OK;
}

// ---- a rectangle as an image (rc2dgi_read.hip)

// The checks the two calls share, in the header's order; r becomes the rectangle (the whole texture for null) and
// *pitch_bytes the tight row where it is 0.  A device destination and its pitch are multiples of a pixel; a host
// destination may be anything.
int read_args(rc2dgi_ctx *c, int which, const rc2dgi_rect *rect, int format, int flags, const void *dst,
              int *pitch_bytes, bool device, TexSource &t, rc2dgi_rect &r) {
  if (!c) return RC2DGI_E_ARG;
  RC2DGI_USABLE(c);
  if (!dst) return fail(c, RC2DGI_E_ARG, "read: null argument");
  if (int rc = resolve_texture(c, which, RC2DGI_FILTER_POINT, "read: ", t)) return rc;
  if (format != RC2DGI_FMT_RGBA8 && format != RC2DGI_FMT_RGBA32F && format != RC2DGI_FMT_RGBA16F)
    return fail(c, RC2DGI_E_ARG, "read: bad format");
  if (flags & ~RC2DGI_READ_FLIP) return fail(c, RC2DGI_E_ARG, "read: the only flag is RC2DGI_READ_FLIP");
  r = rect ? *rect : rc2dgi_rect{0, 0, t.nx, t.ny};
  if (!rect_valid(r, t.nx, t.ny))
    return fail(c, RC2DGI_E_ARG, "read: the rectangle does not lie inside the texture (no wrap, no clipping)");
  const int pxb = read_pixel_bytes(format), row = r.w * pxb;  // (w <= 32768)
  if (*pitch_bytes == 0) *pitch_bytes = row;
  if (*pitch_bytes < row) return fail(c, RC2DGI_E_ARG, "read: pitch smaller than a row");
  if (device && (!aligned_to(dst, (uintptr_t)pxb) || *pitch_bytes % pxb != 0))
    return fail(c, RC2DGI_E_ARG, "read: the destination and the pitch are multiples of a pixel (16 / 8 / 4 bytes)");
  if (c->world > 1)
    return fail(c, RC2DGI_E_UNSUPPORTED, "a row-strip shard's textures hold windows and bands: read on an unsharded context");
  return RC2DGI_OK;
}

// image rows [j0, j0 + rows) of rectangle r into dst (the first of them at dst), enqueued on the context stream
int read_enqueue(rc2dgi_ctx *c, const TexSource &t, const rc2dgi_rect &r, int format, int flags, int j0, int rows,
                 void *dst, size_t pitch) {
  const bool flip = (flags & RC2DGI_READ_FLIP) != 0;
  const ReadArgs a{r.x, r.w, flip ? r.y + r.h - 1 - j0 : r.y + j0, flip ? -1 : 1, rows,
                   static_cast<unsigned char *>(dst), pitch};
  HIPCHK(c, launch_read(t, a, format, c->stream));
  return RC2DGI_OK;
}

}  // namespace

extern "C" {

int rc2dgi_display_layout(const rc2dgi_config *cfg, rc2dgi_view *views, int max_views) {
  if (!cfg || max_views < 0 || (max_views > 0 && !views)) return RC2DGI_E_ARG;
  const int W = cfg->screen_width, H = cfg->screen_height;
  // DrawTexturePro(colorRT.Texture, ..) over the window, then DrawDebugRT per thumbnail (RC2DGI.cs:139-163, 435-448)
  static const int thumbs[7] = {RC2DGI_RT_COLOR, RC2DGI_RT_EMISSIVE, RC2DGI_RT_JUMP2, RC2DGI_RT_DIST,
                                RC2DGI_RT_GI1,   RC2DGI_RT_GI2,      RC2DGI_RT_TEMP};
  for (int k = 0; k < 8 && k < max_views; ++k) {
    rc2dgi_view v{};
    if (k == 0) {
      v = rc2dgi_view{RC2DGI_RT_COLOR, 0, 0, W, H, RC2DGI_FILTER_RT, 0, 0, 0, 0};
    } else {
      const int t = k - 1;
      v = rc2dgi_view{thumbs[t], W - 110, 10 * (t + 1) + 100 * t, 100, 100, RC2DGI_FILTER_RT, 230, 41, 55, 255};
    }
    views[k] = v;
  }
  return 8;
}

int rc2dgi_compose_device(rc2dgi_ctx *c, const rc2dgi_view *views, int n, int out_w, int out_h,
                          const unsigned char *clear_rgba, void *dev, int pitch_bytes) {
  return compose_device(c, views, nullptr, n, out_w, out_h, clear_rgba, dev, pitch_bytes);
}

int rc2dgi_compose(rc2dgi_ctx *c, const rc2dgi_view *views, int n, int out_w, int out_h, const unsigned char *clear_rgba,
                   void *host, int pitch_bytes) {
  return compose_host(c, views, nullptr, n, out_w, out_h, clear_rgba, host, pitch_bytes);
}

// ---- edge tables, toned views (rc2dgi_tone.hip)
int rc2dgi_check_edges(const float *edges, int m) { return check_edges(edges, m); }

int rc2dgi_curve_q8(float *edges255) {
  if (!edges255) return RC2DGI_E_ARG;
  for (unsigned k = 1; k <= 255u; ++k) {
    // the smallest bit pattern in [0, bits(1.0f)] whose float has q8 >= k: q8 is monotone there, q8(1.0f) = 255
    uint32_t lo = 0u, hi = 0x3F800000u;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (q8_host(bits_float(mid)) >= k) hi = mid;
      else lo = mid + 1;
    }
    edges255[k - 1] = bits_float(lo);
  }
  return RC2DGI_OK;
}

int rc2dgi_set_curve(rc2dgi_ctx *c, int slot, const float *edges255) {
  if (!c) return RC2DGI_E_ARG;
  RC2DGI_USABLE(c);
  if (slot < 1 || slot > RC2DGI_MAX_CURVES) return fail(c, RC2DGI_E_ARG, "set_curve: the slot is 1 .. RC2DGI_MAX_CURVES");
  if (!edges255) {
    c->curve_host[slot - 1].clear();  // (the device table stays: a compose enqueued earlier still reads it)
    return RC2DGI_OK;
  }
  if (check_edges(edges255, RC2DGI_CURVE_EDGES) != RC2DGI_OK)
    return fail(c, RC2DGI_E_ARG, "set_curve: 255 ascending edges, none a NaN (rc2dgi_check_edges)");
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->curves_dev) HIPCHK(c, alloc(&c->curves_dev, (size_t)RC2DGI_MAX_CURVES * kCurveWords * sizeof(float)));
  std::vector<float> copy(edges255, edges255 + RC2DGI_CURVE_EDGES);
  TableChunk ch;
  tree_layout(copy.data(), RC2DGI_CURVE_EDGES, kCurveLevels, std::numeric_limits<float>::infinity(), ch.v);
  HIPCHK(c, launch_store_table(ch, kCurveWords, c->curves_dev + (size_t)(slot - 1) * kCurveWords, nullptr, 0, c->stream));
  c->curve_host[slot - 1].swap(copy);
  return RC2DGI_OK;
}

int rc2dgi_compose_tone_device(rc2dgi_ctx *c, const rc2dgi_view *views, const rc2dgi_tone *tones, int n, int out_w,
                               int out_h, const unsigned char *clear_rgba, void *dev, int pitch_bytes) {
  return compose_device(c, views, tones, n, out_w, out_h, clear_rgba, dev, pitch_bytes);
}

int rc2dgi_compose_tone(rc2dgi_ctx *c, const rc2dgi_view *views, const rc2dgi_tone *tones, int n, int out_w, int out_h,
                        const unsigned char *clear_rgba, void *host, int pitch_bytes) {
  return compose_host(c, views, tones, n, out_w, out_h, clear_rgba, host, pitch_bytes);
}

// ---- histograms (rc2dgi_hist.hip)
int rc2dgi_histogram_device(rc2dgi_ctx *c, int which, int channel, const rc2dgi_rect *rects, int n, const float *edges,
                            int m, void *counts_dev) {
  TexSource t{};
  if (int rc = hist_args(c, which, channel, rects, n, edges, m, counts_dev, t)) return rc;
  if (n == 0) return RC2DGI_OK;
  if (!aligned_to(counts_dev, 4)) return fail(c, RC2DGI_E_ARG, "histogram: the records are aligned to 4 bytes");
  return hist_enqueue(c, t, channel, rects, n, edges, m, counts_dev);
}

int rc2dgi_histogram(rc2dgi_ctx *c, int which, int channel, const rc2dgi_rect *rects, int n, const float *edges, int m,
                     unsigned *counts) {
  TexSource t{};
  if (int rc = hist_args(c, which, channel, rects, n, edges, m, counts, t)) return rc;
  if (n == 0) return RC2DGI_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (int rc = check_chain(c)) return rc;
  const size_t bytes = (size_t)n * (size_t)(m + 4) * sizeof(unsigned);
  if (int rc = query_buffer(c, c->query_out, c->query_out_cap, bytes)) return rc;
  if (int rc = hist_enqueue(c, t, channel, rects, n, edges, m, c->query_out)) return rc;
  HIPCHK(c, hipMemcpyAsync(counts, c->query_out, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return RC2DGI_OK;
}

// ---- a rectangle as an image (rc2dgi_read.hip)
int rc2dgi_read_device(rc2dgi_ctx *c, int which, const rc2dgi_rect *rect, int format, int flags, void *dev,
                       int pitch_bytes) {
  TexSource t{};
  rc2dgi_rect r{};
  if (int rc = read_args(c, which, rect, format, flags, dev, &pitch_bytes, true, t, r)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return read_enqueue(c, t, r, format, flags, 0, r.h, dev, (size_t)pitch_bytes);
}

int rc2dgi_read(rc2dgi_ctx *c, int which, const rc2dgi_rect *rect, int format, int flags, void *host, int pitch_bytes) {
  TexSource t{};
  rc2dgi_rect r{};
  if (int rc = read_args(c, which, rect, format, flags, host, &pitch_bytes, false, t, r)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (int rc = check_chain(c)) return rc;
  // Staged rows are whole 16-byte lines (every segment a dwordx4), and a block is as many of them as the buffer holds.
  // The blocks follow each other on the stream: a block's kernel runs when the copy of the one before has read the buffer.
  const size_t row = (size_t)r.w * read_pixel_bytes(format), spitch = (row + 15) / 16 * 16;
  static_assert(kReadChunkBytes >= (size_t)32768 * 16, "a row of the widest texture fits the buffer: a block is >= 1 row");
  const int block = (int)std::min<size_t>(kReadChunkBytes / spitch, (size_t)r.h);
  if (!c->read_buf) HIPCHK(c, alloc(&c->read_buf, kReadChunkBytes));
  for (int j0 = 0; j0 < r.h; j0 += block) {
    const int rows = std::min(block, r.h - j0);
    if (int rc = read_enqueue(c, t, r, format, flags, j0, rows, c->read_buf, spitch)) return rc;
    HIPCHK(c, hipMemcpy2DAsync(static_cast<unsigned char *>(host) + (size_t)j0 * (size_t)pitch_bytes, (size_t)pitch_bytes,
                               c->read_buf, spitch, row, (size_t)rows, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return RC2DGI_OK;
}

// ---- queries (rc2dgi_query.hip)
int rc2dgi_sample_device(rc2dgi_ctx *c, int which, int filter, const void *uv_dev, int n, void *rgba_dev) {
  if (int rc = query_args(c, uv_dev, n, rgba_dev)) return rc;
  TexSource t{};
  if (int rc = resolve_texture(c, which, filter, "sample: ", t)) return rc;
  if (n == 0) return RC2DGI_OK;
  if (!aligned_to(uv_dev, 8) || !aligned_to(rgba_dev, 16))
    return fail(c, RC2DGI_E_ARG, "the points are aligned to 8 bytes and the results to 16");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, launch_sample(t, uv_dev, n, rgba_dev, c->stream));
  return RC2DGI_OK;
}

int rc2dgi_sample(rc2dgi_ctx *c, int which, int filter, const float *uv, int n, float *rgba) {
  if (int rc = query_args(c, uv, n, rgba)) return rc;
  TexSource t{};
  if (int rc = resolve_texture(c, which, filter, "sample: ", t)) return rc;
  if (n == 0) return RC2DGI_OK;
  return query_host(c, uv, (size_t)n * 8, rgba, (size_t)n * 16,
                    [&](void *in, void *out) { return launch_sample(t, in, n, out, c->stream); });
}

int rc2dgi_raycast_device(rc2dgi_ctx *c, const void *rays_dev, int n, void *hits_dev) {
  if (int rc = query_args(c, rays_dev, n, hits_dev)) return rc;
  RayScene s{};
  if (int rc = ray_scene(c, s)) return rc;
  if (n == 0) return RC2DGI_OK;
  if (!aligned_to(rays_dev, 4) || !aligned_to(hits_dev, 4))
    return fail(c, RC2DGI_E_ARG, "the rays and the hit records are aligned to 4 bytes");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, launch_raycast(s, rays_dev, n, hits_dev, c->stream));
  return RC2DGI_OK;
}

int rc2dgi_raycast(rc2dgi_ctx *c, const rc2dgi_ray *rays, int n, rc2dgi_rayhit *hits) {
  if (int rc = query_args(c, rays, n, hits)) return rc;
  RayScene s{};
  if (int rc = ray_scene(c, s)) return rc;
  if (n == 0) return RC2DGI_OK;
  return query_host(c, rays, (size_t)n * sizeof(rc2dgi_ray), hits, (size_t)n * sizeof(rc2dgi_rayhit),
                    [&](void *in, void *out) { return launch_raycast(s, in, n, out, c->stream); });
}

// ---- region statistics (rc2dgi_reduce.hip)
int rc2dgi_reduce_device(rc2dgi_ctx *c, int which, const rc2dgi_rect *rects, int n, void *stats_dev) {
  TexSource t{};
  if (int rc = reduce_args(c, which, rects, n, stats_dev, t)) return rc;
  if (n == 0) return RC2DGI_OK;
  if (!aligned_to(stats_dev, 8)) return fail(c, RC2DGI_E_ARG, "reduce: the records are aligned to 8 bytes");
  return reduce_enqueue(c, t, rects, n, stats_dev);
}

int rc2dgi_reduce(rc2dgi_ctx *c, int which, const rc2dgi_rect *rects, int n, rc2dgi_stats *stats) {
  TexSource t{};
  if (int rc = reduce_args(c, which, rects, n, stats, t)) return rc;
  if (n == 0) return RC2DGI_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (int rc = check_chain(c)) return rc;
  const size_t bytes = (size_t)n * sizeof(rc2dgi_stats);
  if (int rc = query_buffer(c, c->query_out, c->query_out_cap, bytes)) return rc;
  if (int rc = reduce_enqueue(c, t, rects, n, c->query_out)) return rc;
  HIPCHK(c, hipMemcpyAsync(stats, c->query_out, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return RC2DGI_OK;
}

}  // extern "C"
