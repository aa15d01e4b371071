// rc2dgi_hist.h -- histograms of rectangles of a render texture (rc2dgi_histogram / rc2dgi_histogram_device,
// include/rc2dgi.h): per rectangle the count of texels whose scalar (a channel, or the luma) falls into each bin of
// an edge table.  See rc2dgi_hist.hip; the search tree of the edges is rc2dgi_tone.h's.
#pragma once

#include <hip/hip_runtime.h>

#include "rc2dgi_present.h"
#include "rc2dgi_rects.h"

namespace rc2dgi {

constexpr int kHistMax = 1 << 20;            // rectangles a call
constexpr long long kHistMaxWords = 1ll << 26;  // words of all the records of a call
constexpr int kHistTreeWords = 1024;         // the tree over RC2DGI_HIST_MAX_EDGES = 1023 edges, word 0 unused
constexpr int kHistItemTexels = 1 << 14;     // texels a workgroup takes, about: at most (a 4096^2 texture: 1024 blocks)
constexpr int kHistMinItemTexels = 1 << 11;  // and at least, where the rectangle is that large (hist_block_rows)
constexpr int kHistMaxBlocks = 4096;         // row blocks a rectangle is cut into, at most
constexpr int kHistBatch = 1 << 16;          // work items of one launch of an uploaded plan

static_assert(RC2DGI_HIST_MAX_EDGES == kHistTreeWords - 1, "the largest table is a full tree of ten levels");

struct HistTable {
  const float *tree;  // device: 2^levels words (rc2dgi_tone.h, tree_layout)
  int levels, m;
  int channel;        // RC2DGI_CH_*
};

// One launch on `st`, one workgroup per item (n >= 1).  counts: the caller's records of m + 4 words, every word zero
// (launch_store_table clears them in the launch that stores the tree).
hipError_t launch_hist(const TexSource &t, const RectInline &inl, const HistItem *items, int n, const HistTable &tab,
                       void *counts, hipStream_t st);

}  // namespace rc2dgi
