// rc2dgi_regions.cpp -- the rectangle calls of the C ABI (include/rc2dgi.h): the region statistics (rc2dgi_reduce,
// rc2dgi_reduce.hip), the histograms (rc2dgi_histogram, rc2dgi_hist.hip) and a rectangle read as an image
// (rc2dgi_read, rc2dgi_read.hip) and an image written into a rectangle of an input (rc2dgi_write, rc2dgi_write.hip),
// each with its _device variant.  The rectangles are validated and cut into work by rc2dgi_rectplan.cpp; here are the
// argument checks, the uploads and the launches.
#include "rc2dgi_accessory.h"
#include "rc2dgi_rectplan.h"
#include "rc2dgi_write.h"

#include <cstddef>

namespace {

static_assert(sizeof(rc2dgi_rect) == 16 && sizeof(rc2dgi_stats) == 88 && offsetof(rc2dgi_stats, sum) == 56,
              "the region records are 16 and 88 bytes");

// ---- region statistics

// the device side of one batch: [items, then joins | band partials], a fixed size whatever the call
constexpr size_t kReducePlanBytes = (size_t)kReduceBatch * (sizeof(ReduceItem) + sizeof(ReduceJoin));
constexpr size_t reduce_bytes = kReducePlanBytes + (size_t)kReduceBatch * sizeof(ReducePartial);

// n >= 1 rectangles of t into the device records stats_dev, enqueued on the context stream: two launches an inline
// plan or a batch.  A batch's plan goes up in one copy (stream-ordered, after the kernels that read the previous
// one), the joins behind the items on the host (appended to the items' vector) as on the device; the copy has
// consumed the host memory when it returns (pageable memory, as paint_prims relies on for its vectors), so the
// scratch is one batch's on both sides, however long the list.
int reduce_enqueue(rc2dgi_ctx *c, const TexSource &t, const rc2dgi_rect *rects, int n, void *stats_dev) {
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->reduce_buf) HIPCHK(c, alloc(&c->reduce_buf, reduce_bytes));
  ReducePartial *parts = reinterpret_cast<ReducePartial *>(c->reduce_buf + kReducePlanBytes);
  if (n <= kRectInline) {  // the plan fits the kernels' arguments: no upload
    int items, nparts;
    const RectInline inl = rect_inline_plan(rects, n, t.nx, t.ny, false, &items, &nparts);
    HIPCHK(c, launch_reduce_rows(t, inl, nullptr, items, parts, stats_dev, c->stream));
    if (nparts) HIPCHK(c, launch_reduce_bands(inl, nullptr, n, parts, stats_dev, c->stream));
    return RC2DGI_OK;
  }
  static_assert(alignof(ReduceJoin) == 4 && alignof(ReduceItem) == 4, "a join may follow any number of items");
  const RectInline none{};
  return rect_batches(rects, n, t.nx, t.ny, false, [&](RectBatch &b) -> int {
    const int ni = (int)b.items.size(), nj = (int)b.joins.size();
    const size_t ibytes = (size_t)ni * sizeof(ReduceItem), jbytes = (size_t)nj * sizeof(ReduceJoin);
    b.items.resize((ibytes + jbytes + sizeof(ReduceItem) - 1) / sizeof(ReduceItem));
    if (nj) std::memcpy(b.items.data() + ni, b.joins.data(), jbytes);
    const ReduceItem *items = reinterpret_cast<ReduceItem *>(c->reduce_buf);
    const ReduceJoin *joins = reinterpret_cast<ReduceJoin *>(c->reduce_buf + ibytes);
    HIPCHK(c, hipMemcpyAsync(c->reduce_buf, b.items.data(), ibytes + jbytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_reduce_rows(t, none, items, ni, parts, stats_dev, c->stream));
    if (nj) HIPCHK(c, launch_reduce_bands(none, joins, nj, parts, stats_dev, c->stream));
    return RC2DGI_OK;
  });
}

// the checks the two calls share; n == 0 is left to the caller (a successful no-op)
int reduce_args(rc2dgi_ctx *c, int which, const rc2dgi_rect *rects, int n, const void *stats, TexSource &t) {
  if (!c) return RC2DGI_E_ARG;
  RC2DGI_USABLE(c);
  if (n < 0 || n > kReduceMax) return fail(c, RC2DGI_E_ARG, "reduce: n is 0 .. 1 << 20");
  if (n > 0 && (!rects || !stats)) return fail(c, RC2DGI_E_ARG, "reduce: null argument");
  if (int rc = resolve_texture(c, which, RC2DGI_FILTER_POINT, "reduce: ", t)) return rc;
  return refuse_shard(c, "reduce on");
}

// ---- histograms

// the device side: the tree of the edges, then one batch of work items -- a fixed size whatever the call
constexpr size_t kHistTreeBytes = (size_t)kHistTreeWords * sizeof(float);
constexpr size_t hist_bytes = kHistTreeBytes + (size_t)kHistBatch * sizeof(HistItem);

// n >= 1 rectangles of t into the device records counts_dev, enqueued on the context stream: the launches that store
// the tree (the first one clears the records too), then one launch an inline plan or a batch (uploaded as the
// reduction's is).
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
  if (n <= kRectInline) {  // the plan fits the kernel's arguments: no upload
    int items, nparts;
    const RectInline inl = rect_inline_plan(rects, n, t.nx, t.ny, true, &items, &nparts);
    HIPCHK(c, launch_hist(t, inl, nullptr, items, tab, counts_dev, c->stream));
    return RC2DGI_OK;
  }
  const RectInline none{};
  return rect_batches(rects, n, t.nx, t.ny, true, [&](RectBatch &b) -> int {
    HIPCHK(c, hipMemcpyAsync(items_dev, b.blocks.data(), b.blocks.size() * sizeof(HistItem), hipMemcpyHostToDevice,
                             c->stream));
    HIPCHK(c, launch_hist(t, none, items_dev, (int)b.blocks.size(), tab, counts_dev, c->stream));
    return RC2DGI_OK;
  });
}

// the checks the two calls share; n == 0 is left to the caller (a successful no-op)
int hist_args(rc2dgi_ctx *c, int which, int channel, const rc2dgi_rect *rects, int n, const float *edges, int m,
              const void *counts, TexSource &t) {
  if (!c) return RC2DGI_E_ARG;
  RC2DGI_USABLE(c);
  if (n < 0 || n > kHistMax) return fail(c, RC2DGI_E_ARG, "histogram: n is 0 .. 1 << 20");
  if (m < 1 || m > RC2DGI_HIST_MAX_EDGES) return fail(c, RC2DGI_E_ARG, "histogram: m is 1 .. RC2DGI_HIST_MAX_EDGES");
  if ((long long)n * (m + 4) > kHistMaxWords) return fail(c, RC2DGI_E_ARG, "histogram: n * (m + 4) is at most 1 << 26");
  if (rc2dgi_check_edges(edges, m) != RC2DGI_OK)
    return fail(c, RC2DGI_E_ARG, "histogram: the edges are m ascending floats, none a NaN (rc2dgi_check_edges)");
  if (channel < RC2DGI_CH_R || channel > RC2DGI_CH_LUMA) return fail(c, RC2DGI_E_ARG, "histogram: bad channel");
  if (n > 0 && (!rects || !counts)) return fail(c, RC2DGI_E_ARG, "histogram: null argument");
  if (int rc = resolve_texture(c, which, RC2DGI_FILTER_POINT, "histogram: ", t)) return rc;
  return refuse_shard(c, "histogram on");
}

// ---- a rectangle as an image

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
  return refuse_shard(c, "read on");
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

// ---- an image into a rectangle of an input

// The checks the two calls share, in the header's order; r becomes the rectangle (the whole texture for null) and
// *pitch_bytes the tight row where it is 0.  A device source and its pitch are multiples of a pixel; a host source may
// be anything.  A row-strip shard is accepted as rc2dgi_upload accepts one: the inputs are whole on every rank.
int write_args(rc2dgi_ctx *c, int which, const rc2dgi_rect *rect, int format, int flags, const void *src,
               int *pitch_bytes, bool device, rc2dgi_rect &r) {
  if (!c) return RC2DGI_E_ARG;
  RC2DGI_USABLE(c);
  if (!src) return fail(c, RC2DGI_E_ARG, "write: null argument");
  if (which != RC2DGI_RT_COLOR && which != RC2DGI_RT_EMISSIVE)
    return fail(c, RC2DGI_E_ARG, "write: only COLOR and EMISSIVE are inputs");
  if (format != RC2DGI_FMT_RGBA8 && format != RC2DGI_FMT_RGBA32F && format != RC2DGI_FMT_RGBA16F)
    return fail(c, RC2DGI_E_ARG, "write: bad format");
  if (flags & ~(RC2DGI_WRITE_FLIP | RC2DGI_WRITE_BLEND))
    return fail(c, RC2DGI_E_ARG, "write: the flags are RC2DGI_WRITE_FLIP and RC2DGI_WRITE_BLEND");
  r = rect ? *rect : rc2dgi_rect{0, 0, c->W, c->H};
  if (!rect_valid(r, c->W, c->H))
    return fail(c, RC2DGI_E_ARG, "write: the rectangle does not lie inside the texture (no wrap, no clipping)");
  const int pxb = read_pixel_bytes(format), row = r.w * pxb;  // (w <= 32768)
  if (*pitch_bytes == 0) *pitch_bytes = row;
  if (*pitch_bytes < row) return fail(c, RC2DGI_E_ARG, "write: pitch smaller than a row");
  if (device && (!aligned_to(src, (uintptr_t)pxb) || *pitch_bytes % pxb != 0))
    return fail(c, RC2DGI_E_ARG, "write: the source and the pitch are multiples of a pixel (16 / 8 / 4 bytes)");
  return RC2DGI_OK;
}

// image rows [j0, j0 + rows) of rectangle r from src (the first of them at src), enqueued on the context stream
int write_enqueue(rc2dgi_ctx *c, int which, const rc2dgi_rect &r, int format, int flags, int j0, int rows,
                  const void *src, size_t pitch) {
  const bool flip = (flags & RC2DGI_WRITE_FLIP) != 0;
  const WriteArgs a{which == RC2DGI_RT_COLOR ? c->color_in : c->emissive, c->sd.pitch, r.x, r.w,
                    flip ? r.y + r.h - 1 - j0 : r.y + j0, flip ? -1 : 1, rows,
                    static_cast<const unsigned char *>(src), pitch};
  HIPCHK(c, launch_write(a, format, rgba8(c), (flags & RC2DGI_WRITE_BLEND) != 0, c->stream));
  return RC2DGI_OK;
}

}  // namespace

extern "C" {

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
  return host_call(c, nullptr, 0, stats, (size_t)n * sizeof(rc2dgi_stats),
                   [&](void *, void *out) { return reduce_enqueue(c, t, rects, n, out); });
}

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
  return host_call(c, nullptr, 0, counts, (size_t)n * (size_t)(m + 4) * sizeof(unsigned),
                   [&](void *, void *out) { return hist_enqueue(c, t, channel, rects, n, edges, m, out); });
}

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
  if (int rc = host_begin(c)) return rc;
  // The blocks follow each other on the stream: a block's kernel runs when the copy of the one before has read the
  // buffer, a fixed one of kReadChunkBytes.
  const size_t row = (size_t)r.w * read_pixel_bytes(format), spitch = read_staged_pitch(row);
  const int block = read_block_rows(row, r.h);
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

int rc2dgi_write_device(rc2dgi_ctx *c, int which, const rc2dgi_rect *rect, int format, int flags, const void *dev,
                        int pitch_bytes) {
  rc2dgi_rect r{};
  if (int rc = write_args(c, which, rect, format, flags, dev, &pitch_bytes, true, r)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = write_enqueue(c, which, r, format, flags, 0, r.h, dev, (size_t)pitch_bytes)) return rc;
  if (which == RC2DGI_RT_COLOR) c->frame_done = false;
  return RC2DGI_OK;
}

int rc2dgi_write(rc2dgi_ctx *c, int which, const rc2dgi_rect *rect, int format, int flags, const void *host,
                 int pitch_bytes) {
  rc2dgi_rect r{};
  if (int rc = write_args(c, which, rect, format, flags, host, &pitch_bytes, false, r)) return rc;
  if (int rc = host_begin(c)) return rc;
  // rc2dgi_read's staging the other way: a block's rows go up in the image's own format, padded to whole 16-byte
  // lines, and its kernel follows on the stream; the copy of the next block waits for that kernel.  The copy has
  // consumed the (pageable) host rows when it returns.
  const size_t row = (size_t)r.w * read_pixel_bytes(format), spitch = read_staged_pitch(row);
  const int block = read_block_rows(row, r.h);
  if (!c->read_buf) HIPCHK(c, alloc(&c->read_buf, kReadChunkBytes));
  for (int j0 = 0; j0 < r.h; j0 += block) {
    const int rows = std::min(block, r.h - j0);
    HIPCHK(c, hipMemcpy2DAsync(c->read_buf, spitch, static_cast<const unsigned char *>(host) + (size_t)j0 * (size_t)pitch_bytes,
                               (size_t)pitch_bytes, row, (size_t)rows, hipMemcpyHostToDevice, c->stream));
    if (int rc = write_enqueue(c, which, r, format, flags, j0, rows, c->read_buf, spitch)) return rc;
    if (which == RC2DGI_RT_COLOR) c->frame_done = false;  // (a later block may fail: the texture has changed)
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return RC2DGI_OK;
}

}  // extern "C"
