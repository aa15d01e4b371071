// rc2dgi_hist.hip -- histograms of rectangles of a render texture (include/rc2dgi.h, rc2dgi_histogram /
// rc2dgi_histogram_device): per rectangle the record {status, texels, nan, bin[0] .. bin[m]} of 32-bit counts.
//
// Counts are integers: whatever order the additions happen in, the words are the same.  That is the whole determinism
// argument, and why this kernel may use atomics where rc2dgi_reduce.hip fixes a tree: integer atomics only, in LDS and
// in global memory, and no float is accumulated anywhere.
//
// k_hist: one WORKGROUP per work item (a rectangle and a block of its rows, 2048 to 16384 texels: hist_block_rows,
// rc2dgi_rectplan.cpp; the item is rc2dgi_rects.h's, derived here from an inline descriptor or on the host).  It
// stages the search tree of the edges in LDS (rc2dgi_tone.h: level order, so that the lanes' unrelated probes
// of a level fall on distinct banks) and keeps the record's m + 2 counters there: word 0 is `nan`, word 1 + b is bin b, the order of the record from its third word on.  A lane takes four consecutive texels of
// a row, as k_reduce_rows does: rows of more than 1024 texels are walked in chunks, narrow ones are packed 256 / lr
// rows a pass (lr the power of two >= w / 4 lanes).  The loads are unconditional, at addresses clamped into the block,
// and the next step's texels are loaded before the current ones are searched.  A texel's scalar is its channel or the
// luma; its counter is found by `levels` dependent LDS reads, k = 2k + (T[k] <= s), with no branch around a load.
//
// The hard case is a texture whose texels nearly all fall into one bin (a dark room): 64 lanes would add to one LDS
// word, one after another.  So before the atomic a wave aggregates, twice: the lanes that share the first pending
// lane's counter are counted by a ballot and that lane adds the population; what is still pending after two rounds
// (on a spread texture most lanes, on distinct words) adds for itself.  Looping until nothing is pending would cost a
// spread texture some 60 rounds a step; two rounds catch the dominant bin unless both leaders fall outside it.
//
// At the end the workgroup adds its non-zero counters to the record with global integer atomics -- or stores them
// when the block is the whole rectangle: the record's words are zero before the launch (launch_store_table).
#include "rc2dgi_hist.h"

#include "rc2dgi_device.h"
#include "rc2dgi_texel.h"

namespace rc2dgi {

namespace {

constexpr int kLeaves = 4;                 // consecutive texels of a row a lane holds
constexpr int kChunk = 256 * kLeaves;      // texels of a row a workgroup takes at once

struct Leaves {
  float4 p[kLeaves];
};

// the scalar of a texel (channel is uniform); the luma is five single operations (the unit is built -ffp-contract=off)
__device__ __forceinline__ float texel_scalar(float4 p, int channel) {
  switch (channel) {
    case RC2DGI_CH_R: return p.x;
    case RC2DGI_CH_G: return p.y;
    case RC2DGI_CH_B: return p.z;
    case RC2DGI_CH_A: return p.w;
    default: return ((0.2126f * p.x) + (0.7152f * p.y)) + (0.0722f * p.z);
  }
}

// the counter of a scalar: 0 for a NaN, else 1 + bin(s)
__device__ __forceinline__ unsigned counter_of(const float *tree, int levels, float s) {
  unsigned k = 1;
  for (int l = 0; l < levels; ++l) k = 2u * k + (tree[k] <= s ? 1u : 0u);
  return s != s ? 0u : 1u + k - (1u << levels);
}

// every lane with `in` adds one to bins[key]: two aggregation rounds, then one atomic a pending lane
__device__ __forceinline__ void wave_count(unsigned *bins, unsigned key, bool in, int lane) {
  unsigned long long rem = __builtin_amdgcn_ballot_w64(in);
#pragma unroll
  for (int round = 0; round < 2; ++round) {
    if (rem == 0) break;  // (uniform)
    const int leader = (int)__builtin_ctzll(rem);
    const unsigned lk = (unsigned)__builtin_amdgcn_readlane((int)key, leader);
    const unsigned long long same = __builtin_amdgcn_ballot_w64(in && key == lk) & rem;
    if (lane == leader) atomicAdd(&bins[lk], (unsigned)__builtin_popcountll(same));
    rem &= ~same;
  }
  if ((rem >> lane) & 1ull) atomicAdd(&bins[key], 1u);
}

// One item of a texture whose storage kind is the constant KIND (present_texel's switch folds to one case).
template <int KIND>
__device__ __forceinline__ void hist_item(TexSource t, const HistItem &it, int channel, int levels, const float *tree,
                                          unsigned *bins) {
  t.kind = KIND;
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int x = it.x, y = it.y, w = it.w, r0 = it.r0, r1 = it.r1;
  const bool wide = w > kChunk;
  int lr = 256, lsh = 8;  // lanes a row, and its log2
  if (!wide) {
    lr = 1;
    lsh = 0;
    while (lr * kLeaves < w) {
      lr <<= 1;
      ++lsh;
    }
  }
  const int gr = 256 >> lsh;  // rows a pass
  const int nch = wide ? (w + kChunk - 1) / kChunk : 1;
  const int sub = tid >> lsh, c0 = (tid & (lr - 1)) * kLeaves;

  // rows [row0, row0 + gr), chunk c: this lane's texels (a lane without one re-reads the block's last and drops it)
  auto fetch = [&](int row0, int c, Leaves &L) {
    const int row = row0 + sub, col = c * kChunk + c0;
#pragma unroll
    for (int q = 0; q < kLeaves; ++q) L.p[q] = present_texel(t, x + min(col + q, w - 1), y + min(row, r1 - 1));
  };

  int row0 = r0, c = 0;
  Leaves cur, nxt;
  fetch(row0, c, nxt);
  while (row0 < r1) {
    cur = nxt;
    int nrow0 = row0, nc = c + 1;
    if (nc == nch) {
      nc = 0;
      nrow0 += gr;
    }
    if (nrow0 < r1) fetch(nrow0, nc, nxt);
    const int row = row0 + sub, col = c * kChunk + c0;
#pragma unroll
    for (int q = 0; q < kLeaves; ++q) {
      const bool in = row < r1 && col + q < w;
      wave_count(bins, counter_of(tree, levels, texel_scalar(cur.p[q], channel)), in, lane);
    }
    row0 = nrow0;
    c = nc;
  }
}

__global__ __launch_bounds__(256) void k_hist(const TexSource t, const RectInline inl,
                                              const HistItem *__restrict__ items, const HistTable tab,
                                              unsigned *__restrict__ counts) {
  __shared__ float tree[kHistTreeWords];
  __shared__ unsigned bins[kHistTreeWords + 1];  // m + 2 <= 1025 counters
  const int k = (int)blockIdx.x, tid = (int)threadIdx.x;
  HistItem it;  // (k is uniform: scalar loads)
  if (inl.n > 0) {
    const RectDesc d = inline_desc(inl, k);
    it = hist_item_of(d, k - d.item0);
  } else {
    it = items[k];
  }
  unsigned *rec = counts + (size_t)(it.out & 0xFFFFFu) * (size_t)(tab.m + 4);
  if (it.w == 0) {  // an invalid rectangle: no texture memory is read, the other words are zero
    if (tid == 0) rec[0] = (unsigned)RC2DGI_STATS_INVALID;
    return;
  }
  const int words = 1 << tab.levels, nbins = tab.m + 2;
  for (int i = tid; i < words; i += 256) tree[i] = tab.tree[i];
  for (int i = tid; i < nbins; i += 256) bins[i] = 0u;
  __syncthreads();
  switch (t.kind) {  // (uniform)
    case PK_F32: hist_item<PK_F32>(t, it, tab.channel, tab.levels, tree, bins); break;
    case PK_F16: hist_item<PK_F16>(t, it, tab.channel, tab.levels, tree, bins); break;
    case PK_U8: hist_item<PK_U8>(t, it, tab.channel, tab.levels, tree, bins); break;
    case PK_JUMP: hist_item<PK_JUMP>(t, it, tab.channel, tab.levels, tree, bins); break;
    case PK_JUMP8: hist_item<PK_JUMP8>(t, it, tab.channel, tab.levels, tree, bins); break;
    case PK_DIST: hist_item<PK_DIST>(t, it, tab.channel, tab.levels, tree, bins); break;
    case PK_DIST8: hist_item<PK_DIST8>(t, it, tab.channel, tab.levels, tree, bins); break;
    default: hist_item<PK_CONST>(t, it, tab.channel, tab.levels, tree, bins); break;
  }
  __syncthreads();
  // record words: status (0, as cleared), texels, then the counters in the order they were kept
  if (tid == 0 && (it.out & kHistFirst)) rec[1] = (unsigned)it.texels;
  const bool single = (it.out & kHistSingle) != 0u;
  for (int i = tid; i < nbins; i += 256) {
    const unsigned n = bins[i];
    if (n == 0u) continue;
    if (single) rec[2 + i] = n;
    else atomicAdd(&rec[2 + i], n);
  }
}

}  // namespace

hipError_t launch_hist(const TexSource &t, const RectInline &inl, const HistItem *items, int n, const HistTable &tab,
                       void *counts, hipStream_t st) {
  hipLaunchKernelGGL(k_hist, dim3((unsigned)n), dim3(256), 0, st, t, inl, items, tab, static_cast<unsigned *>(counts));
  return hipGetLastError();
}

}  // namespace rc2dgi
