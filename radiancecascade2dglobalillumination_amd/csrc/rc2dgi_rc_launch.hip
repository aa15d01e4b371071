// rc2dgi_rc_launch.hip -- host glue of the cascade levels (k_rc_level, shaders/RadianceCascades.fs:30-161,
// RC2DGI.cs:342-362, 408-433): the levels no ray samples, the exactness proof of the level's divisions, the
// workgroup-order maps, the variant table, the level's parameters and launch_rc_level, which picks the unit
// (rc2dgi_rc_*.hip) that holds the variant; the buffer and exports of the diagnostic builds.
#include "rc2dgi_rc.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace rc2dgi {

// ---------------------------------------------------------------- cascade levels no ray samples
// A ray whose first position is off screen takes no sample and returns (0,0,0,1) (RadianceCascades.fs:65-69).  When
// that holds for every ray of a level, each texel is the merge of four such rays with the sky terms (top level) or
// with the upper level at the texel's sample positions; and when the upper level is such a level too, its texture is
// constant over each direction block, so the bilinear sample is that constant (the taps are block-local; a weight-0
// tap across a block edge leaves it so) and this level is constant per block as well.  The upper block of
// angleIndex ai is block ai of level L + 1.  k_rc_block_const evaluates k_rc_level's own merge expressions (f32
// cascades) once per block; k_rc_fill writes the texture: a store-bound pass in place of the level's launch.
template <bool TOP>
__global__ __launch_bounds__(256) void k_rc_block_const(const float4 *__restrict__ src, float4 *__restrict__ dst,
                                                        int nblk) {
  const int bi = (int)(blockIdx.x * 256 + threadIdx.x);
  if (bi >= nblk) return;
  float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
  for (int r4 = 0; r4 < 4; ++r4) {
    const int ai = bi * 4 + r4;
    float4 rad = make_float4(0.0f, 0.0f, 0.0f, 1.0f);  // the ray that takes no sample
    if constexpr (TOP) {
      const float4 sk = src[ai];
      rad.x = rad.x + sk.x;
      rad.y = rad.y + sk.y;
      rad.z = rad.z + sk.z;
    } else {
      const float4 cu = src[ai];
      const float4 up = GiF32::bilerp(cu, cu, cu, cu, 0.5f, 0.5f);  // (as k_rc_level filters its staged taps)
      const f2v_t rxy = f2v_t{rad.x, rad.y} + f2v_t{up.x, up.y} * f2v_t{rad.w, rad.w};
      rad.x = rxy.x;
      rad.y = rxy.y;
      rad.z = rad.z + up.z * rad.w;
      rad.w = rad.w * up.w;
    }
    const f2v_t q = {0.25f, 0.25f};
    const f2v_t axy = f2v_t{acc.x, acc.y} + f2v_t{rad.x, rad.y} * q;
    const f2v_t azw = f2v_t{acc.z, acc.w} + f2v_t{rad.z, rad.w} * q;
    acc = make_float4(axy.x, axy.y, azw.x, azw.y);
  }
  dst[bi] = GiF32::blend_black(acc);
}

// the level's texels from their direction block's value (4 rows per thread): probe rows [p0, p1) of every block (a
// row-strip shard's plan; else all), into a banded texture when bn > 0 (the block's band of bn rows from b0, as the
// RD marches store)
__global__ __launch_bounds__(256) void k_rc_fill(float4 *__restrict__ out, const float4 *__restrict__ cst,
                                                 CascadeDims c, int level, int p0, int p1, int b0, int bn) {
  const int bdx = c.CW >> level, bdy = c.CH >> level, np = p1 - p0;
  const int i = (int)(blockIdx.x * 64 + (threadIdx.x & 63));
  const int q0 = (int)(blockIdx.y * 16 + (threadIdx.x >> 6) * 4);
  if (i >= c.CW) return;
  const int bx = i / bdx;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int q = q0 + t;  // (block row, probe row) pairs, block rows outer
    if (q >= (np << level)) break;
    const int br = q / np, y = p0 + (q - br * np);
    const int j = bn > 0 ? br * bn + ((y - b0) & (bdy - 1)) : br * bdy + y;
    out[(size_t)j * c.pitch + i] = cst[(br << level) + bx];
  }
}

bool rc_level_all_off(ScreenDims s, CascadeDims c, int N, int level, float ray_range, const float2 *dirs, int div_x,
                      int div_y) {
  RcLevelArgs a{};
  a.level = level;
  a.N = N;
  a.ray_range = ray_range;
  a.div_x = div_x;
  a.div_y = div_y;
  const RcParams P = rc_level_params(a, s, c);
  if (!(P.t0 <= P.t1)) return false;
  // k_rc_level's whole-workgroup far-interval test (wg_off) with the block's extreme probes: the first positions
  // are monotone in the probe index, so these bound every probe's (the same float operations, on the host)
  auto dv = [](float x, float n, float inv, int mode) {
    if (mode == 1) return x * inv;
    if (mode == 2) {
      const float t = x * inv;
      return std::fma(std::fma(-t, n, x), inv, t);
    }
    return x / n;
  };
  const int dmx = c.powW ? 1 : (div_x ? 2 : 0), dmy = c.powH ? 1 : (div_y ? 2 : 0);
  const float oxl = dv(0.5f * (float)P.bsc, P.CRx, P.invCRx, dmx);
  const float oxh = dv(((float)(P.bdx - 1) + 0.5f) * (float)P.bsc, P.CRx, P.invCRx, dmx);
  const float oyl = dv(0.5f * (float)P.bsc, P.CRy, P.invCRy, dmy);
  const float oyh = dv(((float)(P.bdy - 1) + 0.5f) * (float)P.bsc, P.CRy, P.invCRy, dmy);
  const int nd = 4 << (2 * level);
  for (int k = 0; k < nd; ++k) {
    const float sx = (P.t0 * dirs[k].x) * P.aspy, sy = (P.t0 * dirs[k].y) * P.aspx;
    if (!((oxh + sx) < 0.0f || (oxl + sx) > 1.0f || (oyh + sy) < 0.0f || (oyl + sy) > 1.0f)) return false;
  }
  return true;
}

hipError_t launch_rc_block_const(bool top, const float4 *src, float4 *dst, int level, hipStream_t st) {
  const int nblk = 1 << (2 * level);
  const dim3 grid((unsigned)ceil_div(nblk, 256));
  if (top)
    hipLaunchKernelGGL(k_rc_block_const<true>, grid, dim3(256), 0, st, src, dst, nblk);
  else
    hipLaunchKernelGGL(k_rc_block_const<false>, grid, dim3(256), 0, st, src, dst, nblk);
  return hipGetLastError();
}

hipError_t launch_rc_fill(float4 *out, const float4 *cst, CascadeDims c, int level, hipStream_t st, int p0, int p1,
                          int b0, int bn) {
  if (c.gi_f16 || c.gi_u8) return hipErrorInvalidValue;  // (f32 cascades: the values are stored as computed)
  const int bdy = c.CH >> level;
  clamp_rows(bdy, p0, p1);
  if (p0 >= p1) return hipSuccess;
  const long rows = (long)(p1 - p0) << level;
  hipLaunchKernelGGL(k_rc_fill, dim3((unsigned)ceil_div(c.CW, 64), (unsigned)ceil_div((int)rows, 16)), dim3(256), 0, st,
                     out, cst, c, level, p0, p1, b0, bn);
  return hipGetLastError();
}

bool rc_div_exact(int n, int level, bool top) {
  const float fn = (float)n, inv = 1.0f / fn;
  const int bsc = 1 << level, bd = n >> level;
  const float bdf = fn / (float)bsc;  // (RcParams bdxf / bdyf)
  auto ok = [&](float a) {
    const float t = a * inv;
    return std::fma(std::fma(-t, fn, a), inv, t) == a / fn;
  };
  for (int c = 0; c < bd; ++c) {
    if (!ok(((float)c + 0.5f) * (float)bsc)) return false;
    if (top) continue;
    float pc = (float)c * 0.5f + 0.25f;
    pc = std::fmin(std::fmax(pc, 0.5f), bdf * 0.5f - 0.5f);
    for (int k = 0; k < 2 * bsc; ++k)
      if (!ok(pc + (float)k * (bdf * 0.5f))) return false;
  }
  return true;
}

RcMapCache::~RcMapCache() { clear(); }

void RcMapCache::retain(const std::vector<int> &codes) {
  std::vector<Entry> kept;
  for (auto &e : entries) {
    if (std::find(codes.begin(), codes.end(), e.code) != codes.end() || e.code == 0)
      kept.push_back(e);
    else if (e.dev)
      (void)hipFree(e.dev);
  }
  entries.swap(kept);
}

void RcMapCache::clear() {
  for (auto &e : entries)
    if (e.dev) (void)hipFree(e.dev);
  entries.clear();
}

// Logical workgroup order of one launch geometry: (tile, direction group) per logical id.
// code = px | py << 8 | dg << 16 | oriented << 24 | banded << 25 (an invalid patch or group size
// falls back to tile-major).  Banded orders (bit 25): for chunk of dg direction groups: tiles
// sorted by (band across the chunk's mean ray direction, position along it), bands py tile
// widths wide -- the rays of consecutive workgroups sweep one band along their own direction,
// at any angle.  tile_w x tile_h: a tile's size in probes (the bands are isotropic in probes).
static std::vector<uint2> rc_logical_order(int code, int tiles_x, int tiles_y, int ngrp, int tile_w, int tile_h) {
  int opx = code & 0xFF, opy = (code >> 8) & 0xFF, odg = (code >> 16) & 0xFF;
  const bool oriented = (code >> 24) & 1, banded = (code >> 25) & 1;
  if (odg <= 0 || opx <= 0 || opy <= 0 || ngrp % odg) opx = opy = odg = 0;
  const int ntiles = tiles_x * tiles_y, n = ntiles * ngrp;
  std::vector<uint2> out(n);
  if (odg > 0 && banded) {
    const double band = (double)opy * std::sqrt((double)tile_w * (double)tile_h);
    std::vector<std::pair<std::pair<long long, double>, int>> key(ntiles);
    int q = 0;
    for (int ch = 0; ch < ngrp / odg; ++ch) {
      const double th = 6.283185307179586 * ((double)ch * odg + 0.5 * odg) / (double)ngrp;
      const double c = std::cos(th), sn = std::sin(th);
      for (int t = 0; t < ntiles; ++t) {
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        const double x = (tx + 0.5) * tile_w, y = (ty + 0.5) * tile_h;
        const double u = x * c + y * sn, v = -x * sn + y * c;
        key[t] = {{(long long)std::floor(v / band), u}, t};
      }
      std::sort(key.begin(), key.end());
      for (int t = 0; t < ntiles; ++t)
        for (int gi = 0; gi < odg; ++gi) out[q++] = make_uint2((unsigned)key[t].second, (unsigned)(ch * odg + gi));
    }
    return out;
  }
  for (int l = 0; l < n; ++l) {
    int tile, dgi;
    rc_order_map(l, tiles_x, tiles_y, ngrp, opx, opy, odg, tile, dgi, oriented && odg > 0);
    out[l] = make_uint2((unsigned)tile, (unsigned)dgi);
  }
  return out;
}

// XCD interleave of the logical order (order code bits 26-30 = lc > 0): chunks of 2^lc consecutive logical
// workgroups are dealt round-robin to the 8 XCDs, so every XCD works over the whole frame instead of one
// eighth of it (xcd_logical_id: a contiguous eighth each -- the occluders, hence the march, are not spread
// evenly over those eighths); a chunk keeps its locality in one L2.  Whole rounds of 8 chunks only; the
// remainder keeps the contiguous split.  A bijection for any n.
// lc = 16 + t (t = 0..7): the Latin-square schedule instead.  The logical order is cut into 8 regions of S = 8 << t
// sub-chunks each; XCD x's j-th sub-chunk (j = 0 .. S-1, in its dispatch order) is sub-chunk j of region (x + j) mod 8.
// At any moment the 8 XCDs work in 8 different regions (disjoint working sets, each in its own L2: what the
// contiguous split had), and every XCD visits every region S / 8 times (the balance the round-robin deal had).
static int xcd_chunk_logical(int p, int n, int lc) {
  if (lc == 0) return xcd_logical_id(p, n);
  if (lc >= 16) {
    const long long S = 8ll << (lc - 16), unit = 8 * S;  // sub-chunks of all regions
    const long long nf = (long long)n / unit * unit;    // whole sub-chunks only; the remainder stays contiguous
    if (p < nf) {
      const long long c = nf / unit, rs = nf / 8;  // sub-chunk and region sizes
      const long long x = p & 7, i = p >> 3, j = i / c, r = i - j * c;
      return (int)(((x + j) & 7) * rs + j * c + r);
    }
    return (int)(nf + xcd_logical_id((int)(p - nf), (int)(n - nf)));
  }
  const long long C = 1ll << lc, round = 8 * C;
  const int full = (int)((long long)n / round * round);
  if (p < full) {
    const int x = p & 7, s = p >> 3;
    return (int)(((long long)(s >> lc)) * round + (long long)x * C + (s & (C - 1)));
  }
  return full + xcd_logical_id(p - full, n - full);
}

// the host-built workgroup map for one launch geometry (built once, then reused): physical
// workgroup -> XCD chunk of the logical order (xcd_logical_id) -> (tile x | y << 16, group)
const uint2 *rc_wg_map(RcMapCache *cache, int nwg, int tiles_x, int tiles_y, int ngrp, int code, int tile_w,
                              int tile_h) {
  if (!cache) return nullptr;
  {  // an order code that does not tile this geometry runs tile-major: share the code-0 map
    const int opx = code & 0xFF, opy = (code >> 8) & 0xFF, odg = (code >> 16) & 0xFF;
    if (odg <= 0 || opx <= 0 || opy <= 0 || ngrp % odg) code &= 31 << 26;  // (keeps the XCD interleave)
  }
  for (auto &e : cache->entries)
    if (e.nwg == nwg && e.tiles_x == tiles_x && e.tiles_y == tiles_y && e.ngrp == ngrp && e.code == code &&
        e.tile_w == tile_w && e.tile_h == tile_h)
      return e.dev;
  const std::vector<uint2> lo = rc_logical_order(code, tiles_x, tiles_y, ngrp, tile_w, tile_h);
  if ((int)lo.size() != nwg) return nullptr;
  std::vector<uint2> m(nwg);
  const int lc = (code >> 26) & 31;  // XCD interleave (order code bits 26-30, xcd_chunk_logical)
  for (int p = 0; p < nwg; ++p) {
    const uint2 v = lo[xcd_chunk_logical(p, nwg, lc)];
    const int ty = (int)v.x / tiles_x, tx = (int)v.x - ty * tiles_x;
    m[p] = make_uint2((unsigned)tx | ((unsigned)ty << 16), v.y);
  }
  RcMapCache::Entry e{nwg, tiles_x, tiles_y, ngrp, code, tile_w, tile_h, nullptr};
  if (hipMalloc(reinterpret_cast<void **>(&e.dev), (size_t)nwg * sizeof(uint2)) != hipSuccess) return nullptr;
  if (hipMemcpy(e.dev, m.data(), (size_t)nwg * sizeof(uint2), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(e.dev);
    return nullptr;
  }
  cache->entries.push_back(e);
  return e.dev;
}

int rc_wg_map_plan(int code, int tiles_x, int tiles_y, int tile_w, int tile_h, int ngrp, int *tiles, int *groups,
                   int n) {
  const std::vector<uint2> lo = rc_logical_order(code, tiles_x, tiles_y, ngrp, tile_w, tile_h);
  const int nwg = (int)lo.size(), lc = (code >> 26) & 31;
  for (int p = 0; p < n && p < nwg; ++p) {
    const uint2 v = lo[xcd_chunk_logical(p, nwg, lc)];
    tiles[p] = (int)v.x;
    groups[p] = (int)v.y;
  }
  return 0;
}

int rc_order_plan(int code, int tiles_x, int tiles_y, int tile_w, int tile_h, int ngrp, int *tiles, int *groups,
                  int n) {
  const std::vector<uint2> lo = rc_logical_order(code, tiles_x, tiles_y, ngrp, tile_w, tile_h);
  for (int q = 0; q < n && q < (int)lo.size(); ++q) {
    tiles[q] = (int)lo[q].x;
    groups[q] = (int)lo[q].y;
  }
  return 0;
}

// RC tile variants (tuning knob "rc_variant"): TXxTYxPY probes per workgroup, "dD" = D direction
// blocks per workgroup (needs 4^level >= D; falls back to d1 below that)
// ("u": march loop fully unrolled, "t": 8x8-tiled distance field, "p": packed 14-texel distance field,
// "n": nibble-predicted 26-texel distance field)
static const char *kRcVariantNames[] = {"16x16x1", "16x8x2",   "16x16x2",  "32x8x1",   "64x4x1",
                                        "8x8x1",   "32x8x2",   "16x16x1d2", "16x16x1d4", "16x8x1d2",
                                        "32x8x1d2", "16x8x1d4", "8x8x1d4", "16x16x1u", "16x16x1ut", "16x16x1t",
                                        "16x16x1up", "16x16x1un", "16x16x1p", "16x16x1n",
                                        "32x16x1", "16x32x1", "32x32x1", "32x16x1u", "32x32x1u", "16x16x1top"};
int rc_variant_count() { return (int)(sizeof(kRcVariantNames) / sizeof(kRcVariantNames[0])); }
bool rc_variant_tiled(int v) { return v == 14 || v == 15; }
bool rc_variant_packed(int v) { return v == 16 || v == 18; }
bool rc_variant_nib(int v) { return v == 17 || v == 19; }
bool rc_variant_one_probe(int v) { return v == 0 || (v >= 3 && v <= 5) || (v >= 13 && v < rc_variant_count()); }
const char *rc_variant_name(int v) { return (v >= 0 && v < rc_variant_count()) ? kRcVariantNames[v] : "?"; }

#if defined(RC2DGI_DIAG_STATS) || defined(RC2DGI_DIAG_TIMING)
// the diagnostic counters (one device buffer per process, zeroed when made): [16 levels][16], then (timing
// builds) kDiagSlots copies of it that rc2dgi_diag_stats sums
#ifdef RC2DGI_DIAG_TIMING
constexpr size_t kDiagWords = kDiagRecBase + ((size_t)8 << 17) * 2;
#else
constexpr size_t kDiagWords = 256;
#endif
unsigned long long *diag_stats_buffer() {
  static unsigned long long *d = nullptr;
  if (!d && hipMalloc(&d, kDiagWords * sizeof(unsigned long long)) == hipSuccess)
    (void)hipMemset(d, 0, kDiagWords * sizeof(unsigned long long));
  return d;
}
#endif

// the level's parameters that do not depend on the tile shape (rc_tile_params adds those)
RcParams rc_level_params(const RcLevelArgs &a, ScreenDims s, CascadeDims c) {
  RcParams P;
  std::memset(&P, 0, sizeof(P));  // (padding too: the chain compares whole argument blocks, rc2dgi_rc_chain.hip)
#if defined(RC2DGI_DIAG_STATS) || defined(RC2DGI_DIAG_TIMING)
  P.stats = diag_stats_buffer();
#endif
  P.s = s;
  P.c = c;
  P.level = a.level;
  P.bsc = 1 << a.level;
  P.bdx = c.CW >> a.level;
  P.bdy = c.CH >> a.level;
  P.p0 = a.p0 < 0 ? 0 : a.p0;
  P.p1 = (a.p1 < 0 || a.p1 > P.bdy) ? P.bdy : a.p1;
  P.CRx = (float)c.CW;
  P.CRy = (float)c.CH;
  P.invCRx = 1.0f / P.CRx;  // exact divisions when CW / CH are powers of two; else only the approximate WG-proof box
  P.invCRy = 1.0f / P.CRy;
  P.bdxf = P.CRx / (float)P.bsc;  // blockDim = _CascadeResolution / float(blockSqrtCount)
  P.bdyf = P.CRy / (float)P.bsc;
  P.bs2 = (float)(P.bsc * 2);
  rc_aspect(s.W, s.H, P.aspx, P.aspy);  // RC2DGI.cs:273
  // CalculateRayRange (RadianceCascades.fs:38-46)
  const int maxValue = (1 << (a.N * 2)) - 1;
  const int start = (1 << (a.level * 2)) - 1;
  const int end = (1 << (a.level * 2 + 2)) - 1;
  P.t0 = ((float)start / (float)maxValue) * a.ray_range;
  P.t1 = ((float)end / (float)maxValue) * a.ray_range;
  P.reflectivity = a.reflectivity;
  P.rdx = a.div_x;
  P.rdy = a.div_y;
  P.ob0 = a.out_b0;
  P.obn = a.out_bn;
  P.ub0 = a.up_b0;
  P.ubn = a.up_bn;
  return P;
}

hipError_t launch_rc_level(const RcLevelArgs &a, ScreenDims s, CascadeDims c, hipStream_t st) {
  const RcParams P = rc_level_params(a, s, c);
  // banded cascade textures: the derived-record marches only (launch_rc_tiles, P.rcol), never the top-level variant
  if ((a.out_bn > 0 || a.up_bn > 0) && (!a.rec_color || a.variant == 25 || c.gi_u8 || c.gi_f16))
    return hipErrorInvalidValue;
  hipError_t e;
  if (a.variant == 25)
    e = launch_rc_top(a, P, st);  // the barrier-free top level (any storage; elsewhere variant 13)
  else if (c.gi_u8)
    e = launch_rc_u8(a, P, st);  // RGBA8 cascades: the 16x16x1 family and 16x8x2, 32x8x1, 32x8x2
  else if (c.gi_f16)
    e = launch_rc_f16(a, P, st);  // RGBA16F cascades: the 16x16x1 family and 16x8x2, 32x8x1, 32x8x2
  else if (a.variant >= 20 && a.variant < rc_variant_count())
    e = launch_rc_f32_wide(a, P, st);
  else if (a.variant >= 13 && a.variant < rc_variant_count())
    e = launch_rc_f32_unrolled(a, P, st);
  else
    e = launch_rc_f32_rolled(a, P, st);
  if (e != hipSuccess) return e;
  return hipGetLastError();
}

}  // namespace rc2dgi

#if defined(RC2DGI_DIAG_STATS) || defined(RC2DGI_DIAG_TIMING)
#ifdef RC2DGI_DIAG_TIMING
extern "C" int rc2dgi_diag_raw(unsigned long long *out, long long n) {  // the per-workgroup records (timing builds)
  hipDeviceSynchronize();
  unsigned long long *d = rc2dgi::diag_stats_buffer();
  if (!d) return -3;
  const size_t m = std::min((size_t)n, rc2dgi::kDiagWords - rc2dgi::kDiagRecBase);
  return hipMemcpy(out, d + rc2dgi::kDiagRecBase, m * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -3;
}
#endif
extern "C" int rc2dgi_diag_stats(unsigned long long *out, int reset) {  // out: [16][16]
  hipDeviceSynchronize();
  unsigned long long *d = rc2dgi::diag_stats_buffer();
  if (!d) return -3;
  std::vector<unsigned long long> h(rc2dgi::kDiagWords);
  if (hipMemcpy(h.data(), d, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return -3;
  for (int i = 0; i < 256; ++i) {
    unsigned long long s = h[i];
#ifdef RC2DGI_DIAG_TIMING
    const size_t end = rc2dgi::kDiagRecBase;  // (the per-workgroup records follow the table copies)
#else
    const size_t end = h.size();
#endif
    for (size_t c = 256 + i; c < end; c += 256) s += h[c];
    out[i] = s;
  }
  if (reset && hipMemset(d, 0, h.size() * sizeof(unsigned long long)) != hipSuccess) return -3;
  return 0;
}
#endif
