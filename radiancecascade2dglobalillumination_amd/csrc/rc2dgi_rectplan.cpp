// rc2dgi_rectplan.cpp -- the host's planning of the rectangle calls and of a view's geometry (rc2dgi_rectplan.h).
// Pure arithmetic: no HIP runtime call.
#include "rc2dgi_rectplan.h"

#include <algorithm>

namespace rc2dgi {

bool rect_valid(const rc2dgi_rect &r, int tw, int th) {
  return r.w >= 1 && r.h >= 1 && r.x >= 0 && r.y >= 0 && r.w <= tw - r.x && r.h <= th - r.y;
}

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

int rect_desc(const rc2dgi_rect &r, int tw, int th, bool hist, int item0, int part0, int out, RectDesc &d) {
  if (!rect_valid(r, tw, th)) {
    d = RectDesc{0, 0, 0, 0, 1, item0, part0, out};
    return 1;
  }
  const int rows = hist ? hist_block_rows(r.w, r.h) : reduce_band_rows(r.w, r.h);
  d = RectDesc{r.x, r.y, r.w, r.h, rows, item0, part0, out};
  return (int)(((long long)r.h + rows - 1) / rows);
}

RectInline rect_inline_plan(const rc2dgi_rect *rects, int n, int tw, int th, bool hist, int *items, int *parts) {
  RectInline inl{};
  inl.n = n;
  *items = *parts = 0;
  for (int k = 0; k < n; ++k) {
    const int nb = rect_desc(rects[k], tw, th, hist, *items, *parts, k, inl.d[k]);
    *items += nb;
    if (!hist && nb > 1) *parts += nb;
  }
  return inl;
}

int rect_batches(const rc2dgi_rect *rects, int n, int tw, int th, bool hist,
                 const std::function<int(RectBatch &)> &flush) {
  RectBatch b;
  // (every rectangle is an item at least: the lists do not grow by doubling through a long call of sprites)
  if (hist) b.blocks.reserve(std::min<size_t>((size_t)n, (size_t)kHistBatch));
  else b.items.reserve(std::min<size_t>((size_t)n, (size_t)kReduceBatch));
  auto flush_if_over = [&](size_t have, size_t more, size_t cap) -> int {
    if (have + more <= cap) return 0;
    const int rc = flush(b);
    b.items.clear();
    b.joins.clear();
    b.blocks.clear();
    b.parts = 0;
    return rc;
  };
  for (int k = 0; k < n; ++k) {
    RectDesc d;
    const int nb = rect_desc(rects[k], tw, th, hist, 0, 0, k, d);
    if (hist) {
      for (int i = 0; i < nb; ++i) {
        if (int rc = flush_if_over(b.blocks.size(), 1, (size_t)kHistBatch)) return rc;
        b.blocks.push_back(hist_item_of(d, i));
      }
      continue;
    }
    if (int rc = flush_if_over(b.items.size(), (size_t)nb, (size_t)kReduceBatch)) return rc;
    d.part0 = b.parts;
    if (nb > 1) {
      b.joins.push_back(reduce_join_of(d));
      b.parts += nb;
    }
    for (int i = 0; i < nb; ++i) b.items.push_back(reduce_item_of(d, i));
  }
  return b.empty() ? 0 : flush(b);
}

static_assert(kReadChunkBytes >= (size_t)32768 * 16, "a row of the widest texture fits the buffer: a block is >= 1 row");

int read_block_rows(size_t row_bytes, int h) {
  return (int)std::min<size_t>(kReadChunkBytes / read_staged_pitch(row_bytes), (size_t)h);
}

static int clampi(long long v, int lo, int hi) { return (int)std::min<long long>(std::max<long long>(v, lo), hi); }

bool clip_view(int x, int y, int w, int h, int out_w, int out_h, int border, bool blit, ViewClip &v) {
  const long long x1 = (long long)x + w, y1 = (long long)y + h;
  v = ViewClip{clampi(x, 0, out_w), clampi(x1, 0, out_w), clampi(y, 0, out_h), clampi(y1, 0, out_h), 0, 0, 0, 0};
  if (v.cx0 >= v.cx1 || v.cy0 >= v.cy1) return false;
  if (blit) {
    v.fx0 = clampi((long long)x + border, 0, out_w);
    v.fx1 = clampi(x1 - border, 0, out_w);
    v.fy0 = clampi((long long)y + border, 0, out_h);
    v.fy1 = clampi(y1 - border, 0, out_h);
  }
  return true;
}

}  // namespace rc2dgi
