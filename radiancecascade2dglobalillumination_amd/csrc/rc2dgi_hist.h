// rc2dgi_hist.h -- histograms of rectangles of a render texture (rc2dgi_histogram / rc2dgi_histogram_device,
// include/rc2dgi.h): per rectangle the count of texels whose scalar (a channel, or the luma) falls into each bin of
// an edge table.  See rc2dgi_hist.hip; the search tree of the edges is rc2dgi_tone.h's.
#pragma once

#include <hip/hip_runtime.h>

#include "rc2dgi_present.h"

namespace rc2dgi {

constexpr int kHistMax = 1 << 20;            // rectangles a call
constexpr long long kHistMaxWords = 1ll << 26;  // words of all the records of a call
constexpr int kHistTreeWords = 1024;         // the tree over RC2DGI_HIST_MAX_EDGES = 1023 edges, word 0 unused
constexpr int kHistItemTexels = 1 << 14;     // texels a workgroup takes, about: at most (a 4096^2 texture: 1024 blocks)
constexpr int kHistMinItemTexels = 1 << 11;  // and at least, where the rectangle is that large (hist_block_rows)
constexpr int kHistMaxBlocks = 4096;         // row blocks a rectangle is cut into, at most
constexpr int kHistBatch = 1 << 16;          // work items of one launch of an uploaded plan
constexpr unsigned kHistSingle = 0x80000000u;  // HistItem::out: the block is the rectangle, its counts are stored
constexpr unsigned kHistFirst = 0x40000000u;   // HistItem::out: the rectangle's first block writes `texels`

static_assert(RC2DGI_HIST_MAX_EDGES == kHistTreeWords - 1, "the largest table is a full tree of ten levels");

// One workgroup's work: rows [r0, r1) of the rectangle at (x, y), w texels wide, into record `out & 0xFFFFF..`.
// w == 0: an invalid rectangle, the record's status becomes RC2DGI_STATS_INVALID (its other words are zero already).
struct HistItem {
  int x, y, w, r0, r1;
  int texels;      // w * h of the whole rectangle
  unsigned out;    // record index | kHistSingle | kHistFirst
};

// A call of a few rectangles carries its plan in the kernel's arguments (no upload): rectangle r's items are
// [item0, item0 + ceil(h / rows)), block b of it rows [b * rows, (b + 1) * rows).
constexpr int kHistInline = 4;
struct HistDesc {
  int x, y, w, h;   // w == 0: invalid
  int rows;         // rows a block
  int item0, out, pad;
};
struct HistInline {
  int n;            // 0: the plan is the uploaded list
  int pad;
  HistDesc d[kHistInline];
};

struct HistTable {
  const float *tree;  // device: 2^levels words (rc2dgi_tone.h, tree_layout)
  int levels, m;
  int channel;        // RC2DGI_CH_*
};

static_assert(sizeof(HistItem) == 28, "plan record");

// One launch on `st`, one workgroup per item (n >= 1).  counts: the caller's records of m + 4 words, every word zero
// (launch_store_table clears them in the launch that stores the tree).
hipError_t launch_hist(const TexSource &t, const HistInline &inl, const HistItem *items, int n, const HistTable &tab,
                       void *counts, hipStream_t st);

}  // namespace rc2dgi
