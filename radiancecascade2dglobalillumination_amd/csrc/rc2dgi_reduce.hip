// rc2dgi_reduce.hip -- rectangles of a render texture measured on the device (include/rc2dgi.h, rc2dgi_reduce /
// rc2dgi_reduce_device): per channel the non-finite count, min and max of the finite values and their float64 sum.
//
// The sum's order is fixed by the header: a row is the adjacent-pair tree over its leaves padded with +0.0 to a power
// of two, the row sums go through the same tree.  No leaf is -0.0 (a value enters as x + 0.0f), so x + 0.0 == x and
// a + b == b + a hold for every partial: padding can be skipped and operands swapped.  Two kernels, no atomics, no
// wait between workgroups.
//
// k_reduce_rows: one WAVE per work item (a rectangle and a band of its rows, rc2dgi_rects.h; the four waves of a
// workgroup are independent, no LDS).  A lane holds kReduceLeaves = 4 consecutive leaves of a row and adds them as
// (l0 + l1) + (l2 + l3), the tree's two lowest levels.  The next six are the DPP wave reduction (row_shr 1, 2, 4, 8,
// row_bcast15, row_bcast31): lane i with i % 2^k == 2^k - 1 takes s[i - 2^(k-1)] + s[i], the adjacent-pair tree
// mirrored towards lane 63; the four channels go through a level together, so that their moves and adds overlap.
//   wide rows (w > 256)  the wave walks a row in chunks of 256 leaves, lane l on leaves 256 c + 4 l .. + 3.  Chunk sums
//                        combine by a binary-carry stack (push, merge equal sizes as a counter carries; at the end
//                        fold from the smallest partial up): the padded tree with O(log) state.  The stack lives in
//                        ONE register pair a channel, level k in lane k, read with v_readlane.
//   narrow rows          lr = the power of two >= w / 4 lanes hold a row and the wave takes 64 / lr rows at once: the
//                        low DPP levels reduce rows, the high ones pair rows (r0 + r1) + (r2 + r3) .., which is the
//                        row tree since a band starts at a multiple of 64 / lr.  A sprite costs one wave a few passes.
// Row (or row-group) sums combine by a second such stack.  The next step's texels are loaded before the current ones are
// reduced.  min / max stay lane-local to the end of the item, counts are the population of the compare mask (their
// order is free).  A step whose values are all finite and present, the common one, takes a form without selects.
// The plan is the host's list of items, or for a call of up to kRectInline rectangles (the whole texture, one
// sprite) a few descriptors in the kernel's arguments, from which a wave derives its item by the functions the host
// fills its list with (rc2dgi_rects.h): nothing is uploaded then.
//
// k_reduce_bands: one wave per rectangle of more than one band, lane l on band partials 512 c + 8 l .. + 7 (loaded
// together, added by the pair tree), then the same wave tree and stack.
#include "rc2dgi_reduce.h"

#include "rc2dgi_device.h"
#include "rc2dgi_texel.h"

namespace rc2dgi {

namespace {

static_assert(kReduceLeaves == 4, "a lane adds two pairs of leaves");
static_assert(sizeof(rc2dgi_stats) == 88 && sizeof(rc2dgi_rect) == 16, "the records are 88 and 16 bytes");

// a lane's value from the lane the DPP control names; a lane without a source keeps its own
template <int CTRL, int ROWS>
__device__ __forceinline__ int dpp(int v) {
  return __builtin_amdgcn_update_dpp(v, v, CTRL, ROWS, 0xF, false);
}
template <int CTRL, int ROWS>
__device__ __forceinline__ float dpp(float v) {
  return __int_as_float(dpp<CTRL, ROWS>(__float_as_int(v)));
}
template <int CTRL, int ROWS>
__device__ __forceinline__ double dpp(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = dpp<CTRL, ROWS>((int)b), hi = dpp<CTRL, ROWS>((int)(b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}

// The adjacent-pair tree over the 64 lanes, mirrored: the result is in lane 63 (other lanes hold partial or
// meaningless combinations, all of finite values).  Every lane is active here.
template <class T, class Op>
__device__ __forceinline__ T wave_tree(T v, Op op) {
  v = op(dpp<0x111, 0xF>(v), v);  // row_shr:1
  v = op(dpp<0x112, 0xF>(v), v);  // row_shr:2
  v = op(dpp<0x114, 0xF>(v), v);  // row_shr:4
  v = op(dpp<0x118, 0xF>(v), v);  // row_shr:8
  v = op(dpp<0x142, 0xA>(v), v);  // row_bcast15 into rows 1, 3
  v = op(dpp<0x143, 0xC>(v), v);  // row_bcast31 into rows 2, 3
  return v;
}

// The same for the four channels' sums, level by level.  Here a lane without a source takes +0.0 and every row is
// written (row_bcast too: the rows it need not reach hold nothing the tree still reads), so that a move needs no
// previous value and is one instruction; x + 0.0 == x.
template <int CTRL>
__device__ __forceinline__ double dpp_or_zero(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xF, 0xF, true);
  return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
template <int CTRL>
__device__ __forceinline__ void tree_level4(double s[4]) {
  double t[4];
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) t[ch] = dpp_or_zero<CTRL>(s[ch]);
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) s[ch] = t[ch] + s[ch];
}
__device__ __forceinline__ void wave_tree4(double s[4]) {
  tree_level4<0x111>(s);  // row_shr:1, 2, 4, 8
  tree_level4<0x112>(s);
  tree_level4<0x114>(s);
  tree_level4<0x118>(s);
  tree_level4<0x142>(s);  // row_bcast15
  tree_level4<0x143>(s);  // row_bcast31
}

struct OpAdd {
  __device__ __forceinline__ double operator()(double a, double b) const { return a + b; }
  __device__ __forceinline__ int operator()(int a, int b) const { return a + b; }
};
struct OpMin {
  __device__ __forceinline__ float operator()(float a, float b) const { return a < b ? a : b; }
};
struct OpMax {
  __device__ __forceinline__ float operator()(float a, float b) const { return a > b ? a : b; }
};

// lane k's double, k wave-uniform
__device__ __forceinline__ double lane_f64(double v, int k) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)b, k), hi = __builtin_amdgcn_readlane((int)(b >> 32), k);
  return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}

// The binary-carry stack of one tree level's partial sums: level k (a sum of 2^k pushes) in lane k of st.
// push: s is the `count`-th push (from 0); it merges with the partials of count's trailing one bits, bigger + s.
__device__ __forceinline__ void stack_push(double st[4], double s[4], int count, int lane) {
  int k = 0;
  while (count & 1) {
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) s[ch] = lane_f64(st[ch], k) + s[ch];
    count >>= 1;
    ++k;
  }
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) st[ch] = lane == k ? s[ch] : st[ch];
}
// fold: the sum of n >= 1 pushes, from the smallest partial up
__device__ __forceinline__ void stack_fold(const double st[4], int n, double s[4]) {
  bool have = false;
  for (int k = 0; (n >> k) != 0; ++k) {
    if (!((n >> k) & 1)) continue;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      const double v = lane_f64(st[ch], k);
      s[ch] = have ? v + s[ch] : v;
    }
    have = true;
  }
}

// min / max / counts of the wave (free order), then lane 63 writes the band partial or the rectangle's record
struct LaneStats {
  float mn[4], mx[4];
  int nf[4];
};

__device__ __forceinline__ void lane_stats_init(LaneStats &a) {
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) {
    a.mn[ch] = __int_as_float(0x7F800000);
    a.mx[ch] = __int_as_float((int)0xFF800000u);
    a.nf[ch] = 0;
  }
}

// (counts: the lanes hold their own counts, to be added; else every lane holds the wave's count already)
__device__ __forceinline__ void lane_stats_join(LaneStats &a, bool counts) {
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) {
    a.mn[ch] = wave_tree(a.mn[ch], OpMin());
    a.mx[ch] = wave_tree(a.mx[ch], OpMax());
    if (counts) a.nf[ch] = wave_tree(a.nf[ch], OpAdd());
  }
}

__device__ __forceinline__ void write_stats(rc2dgi_stats *o, int texels, const LaneStats &a, const double s[4]) {
  o->status = RC2DGI_STATS_OK;
  o->texels = texels;
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) {
    o->nonfinite[ch] = a.nf[ch];
    o->min[ch] = a.mn[ch];
    o->max[ch] = a.mx[ch];
    o->sum[ch] = s[ch];
  }
}

// One value of a channel: its leaf, the lane's min / max and the WAVE's count (every lane is active).  `in`: the leaf
// exists (else padding, +0.0).  An excluded value goes to min / max as a quiet NaN, which v_min / v_max pass over.
__device__ __forceinline__ double leaf(float x, bool in, float &mn, float &mx, int &nf) {
  const float v = x + 0.0f;  // -0.0 -> +0.0, nothing else changes
  const bool fin = (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u;
  const bool use = in && fin;
  const float vs = use ? v : __uint_as_float(0x7FC00000u);
  mn = __builtin_fminf(mn, vs);
  mx = __builtin_fmaxf(mx, vs);
  nf += (int)__builtin_popcountll(__builtin_amdgcn_ballot_w64(in && !fin));
  return (double)(use ? v : 0.0f);
}

__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

// the same for a finite value of a leaf that exists
__device__ __forceinline__ double leaf_plain(float x, float &mn, float &mx) {
  const float v = x + 0.0f;
  mn = __builtin_fminf(mn, v);
  mx = __builtin_fmaxf(mx, v);
  return (double)v;
}

struct Leaves {
  float4 p[kReduceLeaves];
};

// One item of a texture whose storage kind is the constant KIND: present_texel's switch folds to one case, the loop
// carries no branch on it.
template <int KIND>
__device__ __forceinline__ void reduce_item(TexSource t, const ReduceItem &it, int lane,
                                            ReducePartial *__restrict__ partials, rc2dgi_stats *__restrict__ stats) {
  t.kind = KIND;
  const int x = it.x, y = it.y, w = it.w, r0 = it.r0, r1 = it.r1;
  const bool wide = w > kReduceChunk;
  int lr = 64, lsh = 6;  // lanes a row, and its log2
  if (!wide) {
    lr = 1;
    lsh = 0;
    while (lr * kReduceLeaves < w) {
      lr <<= 1;
      ++lsh;
    }
  }
  const int gr = 64 >> lsh;  // rows a pass
  const int nch = wide ? (w + kReduceChunk - 1) / kReduceChunk : 1;
  const int sub = lane >> lsh, c0 = (lane & (lr - 1)) * kReduceLeaves;

  // rows [row0, row0 + gr), chunk c: this lane's leaves.  The loads are unconditional, at addresses clamped into the
  // band, so that they sit in no divergent branch and are waited for only where the next step uses them.
  auto fetch = [&](int row0, int c, Leaves &L) {
    const int row = row0 + sub, col = c * kReduceChunk + c0;
#pragma unroll
    for (int q = 0; q < kReduceLeaves; ++q)  // (a lane without that leaf re-reads the band's last one and drops it)
      L.p[q] = present_texel(t, x + min(col + q, w - 1), y + min(row, r1 - 1));
  };

  LaneStats a;
  lane_stats_init(a);
  double cst[4] = {0.0, 0.0, 0.0, 0.0}, rst[4] = {0.0, 0.0, 0.0, 0.0};  // the chunk stack of a row, the row stack
  double s[4];
  int row0 = r0, c = 0, groups = 0;
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
    const int row = row0 + sub, col = c * kReduceChunk + c0;
    bool in[kReduceLeaves];
#pragma unroll
    for (int q = 0; q < kReduceLeaves; ++q) in[q] = row < r1 && col + q < w;
    // The common step: every lane holds four leaves and the wave's 1024 values are finite.  Then nothing is excluded
    // and the selects fall away; the values and their order are those of the general form below.
    bool plain = in[kReduceLeaves - 1];
#pragma unroll
    for (int q = 0; q < kReduceLeaves; ++q)
      plain = plain && finite_f(cur.p[q].x) && finite_f(cur.p[q].y) && finite_f(cur.p[q].z) && finite_f(cur.p[q].w);
    if (__builtin_amdgcn_ballot_w64(!plain) == 0) {
#define RC2DGI_LEAF(ch, f, q) leaf_plain(cur.p[q].f, a.mn[ch], a.mx[ch])
#define RC2DGI_LEAVES(ch, f) s[ch] = (RC2DGI_LEAF(ch, f, 0) + RC2DGI_LEAF(ch, f, 1)) + (RC2DGI_LEAF(ch, f, 2) + RC2DGI_LEAF(ch, f, 3))
      RC2DGI_LEAVES(0, x);
      RC2DGI_LEAVES(1, y);
      RC2DGI_LEAVES(2, z);
      RC2DGI_LEAVES(3, w);
#undef RC2DGI_LEAF
    } else {
#define RC2DGI_LEAF(ch, f, q) leaf(cur.p[q].f, in[q], a.mn[ch], a.mx[ch], a.nf[ch])
      RC2DGI_LEAVES(0, x);
      RC2DGI_LEAVES(1, y);
      RC2DGI_LEAVES(2, z);
      RC2DGI_LEAVES(3, w);
#undef RC2DGI_LEAVES
#undef RC2DGI_LEAF
    }
    wave_tree4(s);
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) s[ch] = lane_f64(s[ch], 63);
    if (wide) stack_push(cst, s, c, lane);
    if (nc == 0) {  // the row (or the pass's rows) is complete
      if (wide) stack_fold(cst, nch, s);
      stack_push(rst, s, groups, lane);
      ++groups;
    }
    row0 = nrow0;
    c = nc;
  }
  stack_fold(rst, groups, s);
  lane_stats_join(a, false);
  if (lane == 63) {
    if (it.out & kReduceFinal) {
      write_stats(stats + (it.out & ~kReduceFinal), w * (r1 - r0), a, s);
    } else {
      ReducePartial *o = partials + it.out;
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) {
        o->sum[ch] = s[ch];
        o->mn[ch] = a.mn[ch];
        o->mx[ch] = a.mx[ch];
        o->nonfinite[ch] = a.nf[ch];
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_reduce_rows(const TexSource t, const RectInline inl,
                                                     const ReduceItem *__restrict__ items, int n,
                                                     ReducePartial *__restrict__ partials,
                                                     rc2dgi_stats *__restrict__ stats) {
  const int lane = (int)(threadIdx.x & 63u);
  const int k = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (k >= n) return;
  ReduceItem it;  // (k is wave-uniform: scalar loads)
  if (inl.n > 0) {
    const RectDesc d = inline_desc(inl, k);
    it = reduce_item_of(d, k - d.item0);
  } else {
    it = items[k];
  }
  if (it.w == 0) {  // an invalid rectangle: no texture memory is read
    if (lane == 63) {
      rc2dgi_stats *o = stats + (it.out & ~kReduceFinal);
      o->status = RC2DGI_STATS_INVALID;
      o->texels = 0;
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) {
        o->nonfinite[ch] = 0;
        o->min[ch] = 0.0f;
        o->max[ch] = 0.0f;
        o->sum[ch] = 0.0;
      }
    }
    return;
  }
  switch (t.kind) {  // (wave-uniform)
    case PK_F32: reduce_item<PK_F32>(t, it, lane, partials, stats); break;
    case PK_F16: reduce_item<PK_F16>(t, it, lane, partials, stats); break;
    case PK_U8: reduce_item<PK_U8>(t, it, lane, partials, stats); break;
    case PK_JUMP: reduce_item<PK_JUMP>(t, it, lane, partials, stats); break;
    case PK_JUMP8: reduce_item<PK_JUMP8>(t, it, lane, partials, stats); break;
    case PK_DIST: reduce_item<PK_DIST>(t, it, lane, partials, stats); break;
    case PK_DIST8: reduce_item<PK_DIST8>(t, it, lane, partials, stats); break;
    default: reduce_item<PK_CONST>(t, it, lane, partials, stats); break;
  }
}

__global__ __launch_bounds__(256) void k_reduce_bands(const RectInline inl, const ReduceJoin *__restrict__ joins, int n,
                                                      const ReducePartial *__restrict__ partials,
                                                      rc2dgi_stats *__restrict__ stats) {
  const int lane = (int)(threadIdx.x & 63u);
  const int k = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (k >= n) return;
  ReduceJoin j;
  if (inl.n > 0) {  // rectangle k of the inline plan, if it has more than one band
    RectDesc d = inl.d[0];
#pragma unroll
    for (int r = 1; r < kRectInline; ++r)
      if (r == k) d = inl.d[r];
    if (d.w == 0 || d.rows >= d.h) return;
    j = reduce_join_of(d);
  } else {
    j = joins[k];
  }
  LaneStats a;
  lane_stats_init(a);
  double cst[4] = {0.0, 0.0, 0.0, 0.0};
  double s[4];
  // A lane holds kBandLeaves consecutive partials and adds them by the pair tree; all its loads are issued together
  // (unconditional, the index clamped into the rectangle's partials), so a step costs one memory latency.
  constexpr int kBandLeaves = 8, kBandChunk = 64 * kBandLeaves;
  const int nch = (j.nb + kBandChunk - 1) / kBandChunk;
  for (int c = 0; c < nch; ++c) {
    const int b0 = c * kBandChunk + lane * kBandLeaves;
    ReducePartial p[kBandLeaves];
#pragma unroll
    for (int q = 0; q < kBandLeaves; ++q) p[q] = partials[j.first + min(b0 + q, j.nb - 1)];
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      double v[kBandLeaves];
#pragma unroll
      for (int q = 0; q < kBandLeaves; ++q) {
        const bool in = b0 + q < j.nb;
        v[q] = in ? p[q].sum[ch] : 0.0;
        a.mn[ch] = in ? OpMin()(p[q].mn[ch], a.mn[ch]) : a.mn[ch];
        a.mx[ch] = in ? OpMax()(p[q].mx[ch], a.mx[ch]) : a.mx[ch];
        a.nf[ch] += in ? p[q].nonfinite[ch] : 0;
      }
      s[ch] = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
    wave_tree4(s);
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) s[ch] = lane_f64(s[ch], 63);
    stack_push(cst, s, c, lane);
  }
  stack_fold(cst, nch, s);
  lane_stats_join(a, true);
  if (lane == 63) write_stats(stats + j.out, j.texels, a, s);
}

}  // namespace

hipError_t launch_reduce_rows(const TexSource &t, const RectInline &inl, const ReduceItem *items, int n,
                              ReducePartial *partials, void *stats, hipStream_t st) {
  hipLaunchKernelGGL(k_reduce_rows, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, t, inl, items, n, partials,
                     static_cast<rc2dgi_stats *>(stats));
  return hipGetLastError();
}

hipError_t launch_reduce_bands(const RectInline &inl, const ReduceJoin *joins, int n, const ReducePartial *partials,
                               void *stats, hipStream_t st) {
  hipLaunchKernelGGL(k_reduce_bands, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, inl, joins, n, partials,
                     static_cast<rc2dgi_stats *>(stats));
  return hipGetLastError();
}

}  // namespace rc2dgi
