// rc2dgi_rects.h -- how a rectangle of a render texture is cut into work, stated once for the host and the device:
// the region statistics cut it into bands of rows, a wave each (rc2dgi_reduce.hip), the histograms into blocks of
// rows, a workgroup each (rc2dgi_hist.hip).  A rectangle's cut is its descriptor; the work item of band or block b and
// the join of the bands are functions of the descriptor.  A call of a few rectangles carries the descriptors in the
// kernels' arguments and the device derives its items; a longer call has the host evaluate the same functions into
// the lists it uploads (rc2dgi_rectplan.cpp).
#pragma once

#include <hip/hip_runtime.h>

namespace rc2dgi {

constexpr unsigned kReduceFinal = 0x80000000u;  // ReduceItem::out: the band is the rectangle, write its record
constexpr unsigned kHistSingle = 0x80000000u;   // HistItem::out: the block is the rectangle, its counts are stored
constexpr unsigned kHistFirst = 0x40000000u;    // HistItem::out: the rectangle's first block writes `texels`

// One wave's work: rows [r0, r1) of the rectangle at (x, y), w texels wide; r0 is a multiple of the rectangle's band
// height, a power of two (and of 64 / lanes-a-row when w <= kReduceChunk).  out: the band partial it writes, or with
// kReduceFinal the record.  w == 0: an invalid rectangle, record `out` becomes status -1 and zeros.
struct ReduceItem {
  int x, y, w, r0, r1;
  unsigned out;
};
// a rectangle of more than one band: partials [first, first + nb) in band order -> record `out`
struct ReduceJoin {
  int first, nb, out, texels;
};
// One workgroup's work: rows [r0, r1) of the rectangle at (x, y), w texels wide, into record `out & 0xFFFFF..`.
// w == 0: an invalid rectangle, the record's status becomes RC2DGI_STATS_INVALID (its other words are zero already).
struct HistItem {
  int x, y, w, r0, r1;
  int texels;      // w * h of the whole rectangle
  unsigned out;    // record index | kHistSingle | kHistFirst
};

static_assert(sizeof(ReduceItem) == 24 && sizeof(ReduceJoin) == 16, "plan records");
static_assert(sizeof(HistItem) == 28, "plan record");

// The cut of one rectangle: its items are [item0, item0 + ceil(h / rows)), band or block b of it rows
// [b * rows, min((b + 1) * rows, h)) -- and, of the reduction, partial part0 + b.  One band or block is the rectangle.
struct RectDesc {
  int x, y, w, h;   // w == 0: invalid
  int rows;         // rows a band or block (rc2dgi_rectplan.h: reduce_band_rows, hist_block_rows)
  int item0;
  int part0;        // (the histogram has no partials)
  int out;          // the record
};
// A call of up to kRectInline rectangles carries its plan in the kernels' arguments: nothing is uploaded.
constexpr int kRectInline = 4;
struct RectInline {
  int n;            // 0: the plan is the uploaded lists
  int pad;
  RectDesc d[kRectInline];
};

// the descriptor of the rectangle item k belongs to (static indices: the argument block stays in scalar registers)
__host__ __device__ __forceinline__ RectDesc inline_desc(const RectInline &inl, int k) {
  RectDesc d = inl.d[0];
#pragma unroll
  for (int r = 1; r < kRectInline; ++r)
    if (r < inl.n && k >= inl.d[r].item0) d = inl.d[r];
  return d;
}

// band b of the reduction of d
__host__ __device__ __forceinline__ ReduceItem reduce_item_of(const RectDesc &d, int b) {
  if (d.w == 0) return ReduceItem{0, 0, 0, 0, 0, (unsigned)d.out | kReduceFinal};
  const int r0 = b * d.rows;
  const int r1 = d.h - r0 < d.rows ? d.h : r0 + d.rows;
  return ReduceItem{d.x, d.y, d.w, r0, r1, d.rows >= d.h ? (unsigned)d.out | kReduceFinal : (unsigned)(d.part0 + b)};
}

// the join of the bands of d, a valid rectangle of more than one band (rows is a power of two)
__host__ __device__ __forceinline__ ReduceJoin reduce_join_of(const RectDesc &d) {
  return ReduceJoin{d.part0, (int)(((long long)d.h + d.rows - 1) >> __builtin_ctz((unsigned)d.rows)), d.out, d.w * d.h};
}

// block b of the histogram of d
__host__ __device__ __forceinline__ HistItem hist_item_of(const RectDesc &d, int b) {
  if (d.w == 0) return HistItem{0, 0, 0, 0, 0, 0, (unsigned)d.out | kHistSingle | kHistFirst};
  const int r0 = b * d.rows;
  const int r1 = d.h - r0 < d.rows ? d.h : r0 + d.rows;
  return HistItem{d.x, d.y, d.w, r0, r1, d.w * d.h,
                  (unsigned)d.out | (d.rows >= d.h ? kHistSingle : 0u) | (b == 0 ? kHistFirst : 0u)};
}

}  // namespace rc2dgi
