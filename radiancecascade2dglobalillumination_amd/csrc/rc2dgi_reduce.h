// rc2dgi_reduce.h -- rectangles of a render texture measured on the device (rc2dgi_reduce / rc2dgi_reduce_device,
// include/rc2dgi.h): per channel the count of non-finite values, the smallest and largest finite value and the
// float64 sum in the header's fixed order.  See rc2dgi_reduce.hip.
#pragma once

#include <hip/hip_runtime.h>

#include "rc2dgi_present.h"
#include "rc2dgi_rects.h"

namespace rc2dgi {

constexpr int kReduceMax = 1 << 20;        // rectangles a call
constexpr int kReduceLeaves = 4;           // consecutive leaves of a row a lane holds
constexpr int kReduceChunk = 64 * kReduceLeaves;  // leaves of a row a wave takes at once
constexpr int kReduceBatch = 1 << 16;      // work items (and band partials) of one pair of launches
constexpr int kReduceMaxBands = 4096;      // bands a rectangle is cut into, at most

// what a band leaves for the second launch
struct ReducePartial {
  double sum[4];
  float mn[4], mx[4];
  int nonfinite[4];
};

static_assert(sizeof(ReducePartial) == 80, "plan record");

// One launch on `st`, one wave per item (n >= 1): items (unused with an inline plan), partials and stats are device
// memory, stats the caller's rc2dgi_stats array (8-byte aligned).
hipError_t launch_reduce_rows(const TexSource &t, const RectInline &inl, const ReduceItem *items, int n,
                              ReducePartial *partials, void *stats, hipStream_t st);
// One launch on `st`, one wave per join (n >= 1), after launch_reduce_rows on the same stream.
// (with an inline plan: n = inl.n, a wave per rectangle, those of one band idle)
hipError_t launch_reduce_bands(const RectInline &inl, const ReduceJoin *joins, int n, const ReducePartial *partials,
                               void *stats, hipStream_t st);

}  // namespace rc2dgi
