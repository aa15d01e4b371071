// rc2dgi_reduce.h -- rectangles of a render texture measured on the device (rc2dgi_reduce / rc2dgi_reduce_device,
// include/rc2dgi.h): per channel the count of non-finite values, the smallest and largest finite value and the
// float64 sum in the header's fixed order.  See rc2dgi_reduce.hip.
#pragma once

#include <hip/hip_runtime.h>

#include "rc2dgi_present.h"

namespace rc2dgi {

constexpr int kReduceMax = 1 << 20;        // rectangles a call
constexpr int kReduceLeaves = 4;           // consecutive leaves of a row a lane holds
constexpr int kReduceChunk = 64 * kReduceLeaves;  // leaves of a row a wave takes at once
constexpr int kReduceBatch = 1 << 16;      // work items (and band partials) of one pair of launches
constexpr int kReduceMaxBands = 4096;      // bands a rectangle is cut into, at most
constexpr unsigned kReduceFinal = 0x80000000u;  // ReduceItem::out: the band is the rectangle, write its record

// One wave's work: rows [r0, r1) of the rectangle at (x, y), w texels wide; r0 is a multiple of the rectangle's band
// height, a power of two (and of 64 / lanes-a-row when w <= kReduceChunk).  out: the band partial it writes, or with
// kReduceFinal the record.  w == 0: an invalid rectangle, record `out` becomes status -1 and zeros.
struct ReduceItem {
  int x, y, w, r0, r1;
  unsigned out;
};
// what a band leaves for the second launch
struct ReducePartial {
  double sum[4];
  float mn[4], mx[4];
  int nonfinite[4];
};
// a rectangle of more than one band: partials [first, first + nb) in band order -> record `out`
struct ReduceJoin {
  int first, nb, out, texels;
};

// A call of a few rectangles carries its plan in the kernels' arguments instead (no upload): rectangle r's items are
// [item0, item0 + ceil(h / rw)), band b of it rows [b * rw, (b + 1) * rw) and partial part0 + b.
constexpr int kReduceInline = 4;
struct ReduceDesc {
  int x, y, w, h;   // w == 0: invalid
  int rw;           // rows a band
  int item0, part0, out;
};
struct ReduceInline {
  int n;            // 0: the plan is the uploaded lists
  int pad;
  ReduceDesc d[kReduceInline];
};

static_assert(sizeof(ReduceItem) == 24 && sizeof(ReducePartial) == 80 && sizeof(ReduceJoin) == 16, "plan records");

// One launch on `st`, one wave per item (n >= 1): items (unused with an inline plan), partials and stats are device
// memory, stats the caller's rc2dgi_stats array (8-byte aligned).
hipError_t launch_reduce_rows(const TexSource &t, const ReduceInline &inl, const ReduceItem *items, int n,
                              ReducePartial *partials, void *stats, hipStream_t st);
// One launch on `st`, one wave per join (n >= 1), after launch_reduce_rows on the same stream.
// (with an inline plan: n = inl.n, a wave per rectangle, those of one band idle)
hipError_t launch_reduce_bands(const ReduceInline &inl, const ReduceJoin *joins, int n, const ReducePartial *partials,
                               void *stats, hipStream_t st);

}  // namespace rc2dgi
