// rc2dgi_tone.h -- edge tables on the device (include/rc2dgi.h, "edge tables"): the toned display frame
// (rc2dgi_compose_tone, rc2dgi_tone.hip) and the histograms of rectangles (rc2dgi_histogram, rc2dgi_hist.hip).
//
// bin(v) = the number of edges e[i] <= v is evaluated as a branch-free descent of the implicit search tree over the
// sorted edges, stored level by level ("Eytzinger" order): node 1 is the root, node k has the children 2k and 2k + 1,
// and k = 2k + (T[k] <= v), `levels` times from k = 1, ends at k = 2^levels + bin(v).  The tree has 2^levels - 1
// nodes; the nodes past the m real edges hold a quiet NaN, which no value is >= to.  e[i] <= v is monotone along the
// sorted edges (repeats, -0.0 against +0.0 and +-inf included), so the descent counts exactly what the linear scan
// counts; a NaN v fails every comparison and ends at bin 0.  The nodes of a level are consecutive words: lanes that
// look for unrelated values read distinct banks down to the level of 32 nodes and broadcast where they agree,
// where a descent of the sorted array would put every probe of a step on one bank (indices k * 2s + s - 1).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>

#include "rc2dgi_present.h"

namespace rc2dgi {

constexpr int kCurveLevels = 8;                  // RC2DGI_CURVE_EDGES = 2^8 - 1: a full tree
constexpr int kCurveWords = 1 << kCurveLevels;   // word 0 is unused padding (+inf), nodes 1 .. 255
constexpr int kTableChunk = 512;                 // floats of a table one k_store_table launch carries in its arguments

static_assert(RC2DGI_CURVE_EDGES == kCurveWords - 1, "a curve is a full tree of eight levels");

// levels of the tree over m >= 1 edges: the smallest L with 2^L - 1 >= m
inline int tree_levels(int m) {
  int L = 1;
  while ((1 << L) - 1 < m) ++L;
  return L;
}

// The tree of m sorted edges as 2^levels words: T[0] = pad0, T[k] for node k, NaN past the real edges.  Node
// k = 2^d + j of depth d is the in-order element (2j + 1) * 2^(levels - 1 - d) - 1.
inline void tree_layout(const float *edges, int m, int levels, float pad0, float *T) {
  T[0] = pad0;
  for (int d = 0; d < levels; ++d)
    for (int j = 0; j < (1 << d); ++j) {
      const int i = (2 * j + 1) * (1 << (levels - 1 - d)) - 1;
      T[(1 << d) + j] = i < m ? edges[i] : std::numeric_limits<float>::quiet_NaN();
    }
}

// what the toned kernel adds to PresentArgs: per view (after the views outside the window are dropped) its exposure
// and curve slot (0: q8), the slots the call uses and the context's device tables (slot s at tables + (s - 1) * 256)
struct ToneArgs {
  float exposure[RC2DGI_MAX_VIEWS];
  int curve[RC2DGI_MAX_VIEWS];
  unsigned used;        // bit s - 1: slot s is named by a view
  const float *tables;
};

struct TableChunk {
  float v[kTableChunk];
};

// dst[0 .. n) = chunk.v[0 .. n) (n <= kTableChunk) and zero[0 .. nzero) = 0, one launch on `st`.  The table travels
// in the launch's arguments: nothing of the caller's memory is read after the call returns, and the store is ordered
// on the stream like any kernel.
hipError_t launch_store_table(const TableChunk &chunk, int n, float *dst, unsigned *zero, size_t nzero, hipStream_t st);

// k_present with the toned source bytes (rc2dgi_tone.hip); arguments as launch_present
hipError_t launch_present_tone(const PresentArgs &a, const ToneArgs &t, void *dst, int pitch_bytes, hipStream_t st);

}  // namespace rc2dgi
