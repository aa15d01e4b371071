// rc2dgi_rectplan.h -- the host's planning of the rectangle calls (rc2dgi_reduce, rc2dgi_histogram, rc2dgi_read) and
// the geometry of a view of the display frame: arithmetic only, no HIP runtime call, so that its invariants are
// swept on any machine (tests/sanitize/rects_check.cpp).  The callers (rc2dgi_regions.cpp, rc2dgi_display.cpp) keep
// the uploads and launches.
#pragma once

#include <cstddef>
#include <functional>
#include <vector>

#include "rc2dgi_hist.h"
#include "rc2dgi_read.h"
#include "rc2dgi_reduce.h"

namespace rc2dgi {

// the rectangle lies inside a tw x th texture and holds a texel (in this form nothing overflows)
bool rect_valid(const rc2dgi_rect &r, int tw, int th);

// Rows of a band of a w x h rectangle, a power of two: a wave gets about 4096 texels (whole passes of 64 / lanes-a-row
// rows when the rows are narrow, k_reduce_rows; at most 1024 rows), and a rectangle at most kReduceMaxBands bands
// (only a rectangle of more than 2^22 rows gets taller bands for that).
int reduce_band_rows(int w, int h);

// Rows of a block of a w x h rectangle: a 1024th of the rectangle, but between kHistMinItemTexels and kHistItemTexels
// texels (a texture of any size then spreads over the device, and a large one does not flush a record's counters more
// often than it must), in whole passes of the workgroup (256 / lanes-a-row rows when the rows are narrow, k_hist), at
// most kHistMaxBlocks blocks a rectangle.  Any cut gives the same counts.
int hist_block_rows(int w, int h);

// The cut of r, a rectangle of a tw x th texture, into bands (or with `hist` blocks) for record `out`, its items
// numbered from item0 and its partials from part0: the descriptor, and the count of its items.  An invalid rectangle
// is the w == 0 descriptor of one item.
int rect_desc(const rc2dgi_rect &r, int tw, int th, bool hist, int item0, int part0, int out, RectDesc &d);

// The plan of n <= kRectInline rectangles as the kernels' arguments.  *items: work items of the first launch;
// *parts: band partials, 0 where the reduction needs no second launch (the histogram has none).
RectInline rect_inline_plan(const rc2dgi_rect *rects, int n, int tw, int th, bool hist, int *items, int *parts);

// One batch of an uploaded plan: the reduction's bands and joins, or the histogram's blocks.
struct RectBatch {
  std::vector<ReduceItem> items;
  std::vector<ReduceJoin> joins;
  std::vector<HistItem> blocks;
  int parts = 0;  // band partials of the batch
  bool empty() const { return items.empty() && blocks.empty(); }
};
// Walks n rectangles and hands `flush` every batch of at most kReduceBatch / kHistBatch items, the last one short;
// a status other than 0 from it ends the walk and is returned (the batch is its to scribble on).  The reduction keeps
// a rectangle's bands in one batch and numbers partials (and so the joins' first partial) from 0 in each; the
// histogram's blocks only add, so they may fall into different batches.  One batch is held at a time, however long
// the list.
int rect_batches(const rc2dgi_rect *rects, int n, int tw, int th, bool hist,
                 const std::function<int(RectBatch &)> &flush);

// rc2dgi_read's host path stages rows of whole 16-byte lines (every segment a dwordx4) ...
inline size_t read_staged_pitch(size_t row_bytes) { return (row_bytes + 15) / 16 * 16; }
// ... in blocks of as many rows as kReadChunkBytes hold, of the h there are: at least one
int read_block_rows(size_t row_bytes, int h);

// A view's rectangle (x, y, w, h as given: it may hang over the out_w x out_h window) clipped to the window,
// [c*0, c*1), and with `blit` the clipped rectangle without a border of `border` (0 or 1) pixels, [f*0, f*1): where a
// pixel is the plain blit of one texel.  False: the view lies wholly outside the window.
struct ViewClip {
  int cx0, cx1, cy0, cy1;
  int fx0, fx1, fy0, fy1;  // empty (all 0) without `blit`
};
bool clip_view(int x, int y, int w, int h, int out_w, int out_h, int border, bool blit, ViewClip &v);

}  // namespace rc2dgi
