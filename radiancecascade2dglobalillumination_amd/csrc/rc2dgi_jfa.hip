// rc2dgi_jfa.hip -- ScreenUV and JumpFlood (+ DistanceField): each kernel with its launcher (gfx950).
//   k_occupancy     shaders/ScreenUV.fs:10-28          (RC2DGI.cs:278-285), as a 1-bit mask
//   k_jfa_step      shaders/JumpFlood.fs:11-38         (RC2DGI.cs:296-326)
//                   + shaders/DistanceField.fs:12-34 fused into the last step (RC2DGI.cs:328-340)
//   jumpRT1/2: uint32 packed seed texel (sj<<16 | si); RGBA8 mode: the unorm8 seed uv (kv<<16 | ku)
//   distRT:    uint16 q = packUNorm16(d)
// (the whole chain's pass table and storage notes: rc2dgi_kernels.h)
#include "rc2dgi_device.h"
#include "rc2dgi_kernels.h"
#include "rc2dgi_launch.h"
#include "rc2dgi_shard.h"

namespace rc2dgi {

// ---------------------------------------------------------------- ScreenUV
// jumpRT texels hold a packed seed: (sj << 16) | si for the seed texel (si, sj), whose value in the
// reference is its fragTexCoord ((si+0.5)/W, (sj+0.5)/H); kNoSeed is the reference's (0,0).
constexpr unsigned kNoSeed = 0x80008000u;  // si = sj = 32768: never a texel (W, H <= 32768)

__device__ __forceinline__ unsigned pack_seed(int si, int sj) { return ((unsigned)sj << 16) | (unsigned)si; }

// RGBA8 jumpRT (ScreenDims::u8): a texel holds the unorm8 seed uv, packed kv << 16 | ku; it reads
// back as (ku, kv) * (1/255).  ScreenUV.fs stores the seed texel's fragTexCoord, quantized; the
// JumpFlood.fs test `peek.x != 0 && peek.y != 0` then rejects every ku == 0 or kv == 0 (no seed = 0).
__device__ __forceinline__ unsigned pack_seed_u8(int si, int sj, Axis ax, Axis ay) {
  return (q8(texcoord(sj, ay)) << 16) | q8(texcoord(si, ax));
}
__device__ __forceinline__ bool seed_u8_ok(unsigned sd) { return (sd & 0xFFFFu) != 0u && (sd >> 16) != 0u; }

// ScreenUV.fs:19 `any(greaterThan(color.rgb, 0))` as a 1-bit occupancy mask (one 64-texel ballot
// per wave; mask row pitch s.mpitch words).  The seed texture J0 itself is never observable when
// the JFA runs >= 2 steps (step 1 overwrites jumpRT1), so step 0 reads the mask instead.
constexpr int kOccRows = 16;  // rows per wave in k_occupancy (4 rows apart), all loads issued together
__global__ __launch_bounds__(256) void k_occupancy(const float4 *__restrict__ color, unsigned *__restrict__ mask,
                                                   ScreenDims s, int mpitch, int row0, int row1) {
  // kOccRows rows per wave, one 64-texel ballot per row; non-temporal loads (colorRT is read
  // again only by the merge, after the cascades have cycled the caches)
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  const int j0 = row0 + blockIdx.y * (4 * kOccRows) + (threadIdx.x >> 6);
  v4f_t c[kOccRows];
#pragma unroll
  for (int t = 0; t < kOccRows; ++t) {
    const int j = j0 + 4 * t;
    c[t] = __builtin_nontemporal_load(
        reinterpret_cast<const v4f_t *>(color + (size_t)min(j, row1 - 1) * s.pitch + min(i, s.W - 1)));
  }
#pragma unroll
  for (int t = 0; t < kOccRows; ++t) {
    const int j = j0 + 4 * t;
    const bool occ = i < s.W && j < row1 && (c[t].x > 0.0f || c[t].y > 0.0f || c[t].z > 0.0f);
    const unsigned long long b = __ballot(occ);
    if ((threadIdx.x & 63) == 0 && j < row1) {
      unsigned *row = mask + (size_t)j * mpitch + (blockIdx.x * 2);
      row[0] = (unsigned)b;
      row[1] = (unsigned)(b >> 32);
    }
  }
}

hipError_t launch_occupancy(const float4 *color, unsigned *mask, int mpitch, ScreenDims s, hipStream_t st, int row0,
                            int row1) {
  clamp_rows(s.H, row0, row1);
  if (row0 >= row1) return hipSuccess;
  hipLaunchKernelGGL(k_occupancy, dim3(ceil_div(s.W, 64), ceil_div(row1 - row0, 4 * kOccRows)), dim3(256), 0, st,
                     color, mask, s, mpitch, row0, row1);
  return hipGetLastError();
}

// J0 materialised from the mask (only needed when the JFA has a single step)
__global__ __launch_bounds__(256) void k_seeds_from_mask(const unsigned *__restrict__ mask, int mpitch,
                                                         unsigned *__restrict__ seeds, ScreenDims s) {
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (i >= s.W || j >= s.H) return;
  const bool occ = (mask[(size_t)j * mpitch + (i >> 5)] >> (i & 31)) & 1u;
  if (s.u8)
    seeds[(size_t)j * s.pitch + i] = occ ? pack_seed_u8(i, j, Axis{s.W, s.powW}, Axis{s.H, s.powH}) : 0u;
  else
    seeds[(size_t)j * s.pitch + i] = occ ? pack_seed(i, j) : kNoSeed;
}

hipError_t launch_seeds_from_mask(const unsigned *mask, int mpitch, unsigned *seeds, ScreenDims s, hipStream_t st) {
  hipLaunchKernelGGL(k_seeds_from_mask, grid2d(s.W, s.H), dim3(256), 0, st, mask, mpitch, seeds, s);
  return hipGetLastError();
}

// ---------------------------------------------------------------- JumpFlood (+ DistanceField)
struct JfaOffsets {
  float ox[3], oy[3];
  float rw, rh;  // 1 / W, 1 / H correctly rounded (TAB 2: tc_rcp)
};

// (i + 0.5) / n without a division: x * (1/n) and one fused correction, the IEEE quotient for every i < n when
// tc_rcp_exact(n) (checked on the host per context; the float-path step then uses it, TAB 2)
__host__ __device__ __forceinline__ float tc_rcp(int i, float n, float rn) {
  const float x = (float)i + 0.5f;
  const float t = x * rn;
  return fmaf(fmaf(-t, n, x), rn, t);
}

bool tc_rcp_exact(int n) {
  const float fn = (float)n, rn = 1.0f / fn;
  for (int i = 0; i < n; ++i)
    if (tc_rcp(i, fn, rn) != ((float)i + 0.5f) / fn) return false;
  return true;
}

void tc_table(int W, int H, float *out) {
  for (int i = 0; i < W; ++i) out[i] = ((float)i + 0.5f) / (float)W;  // (IEEE division: texcoord's, bit for bit)
  for (int j = 0; j < H; ++j) out[W + j] = ((float)j + 0.5f) / (float)H;
}

// One JumpFlood.fs step.  FIRST: taps read the occupancy mask (the ScreenUV seeds); otherwise the
// packed seeds of the previous step.  dist != nullptr fuses DistanceField.fs.  U8: RGBA8 jumpRT
// (quantized seed uv, pack_seed_u8).
// A 256-thread workgroup covers 64 x (4*JT) texels; each lane owns JT texels 4 rows apart and issues all 9*JT tap loads before the first compare (latency-bound gathers).
#ifndef RC2DGI_JFA_JT
#define RC2DGI_JFA_JT 4
#endif
constexpr int JT = RC2DGI_JFA_JT;

// RT: rows per lane (JT on large screens; 1 on small ones, where 4 rows per lane left about one wave per SIMD:
// 1200 x 900 = 1083 workgroups, each step a few exposed round trips)
// TAB 1 (non-power-of-two screens with W + H <= kTcTabMax): every fragTexCoord the step needs -- the texel's, each
// tap seed's -- read from a table of the W column and H row texcoords ((i + 0.5) / n, the same correctly rounded
// division, made once per context: tc_table) staged in LDS, instead of two IEEE divisions per tap.  TAB 2: computed
// by tc_rcp (three operations), where the host proved it equal to the division for every index (tc_rcp_exact).
constexpr int kTcTabMax = 8192;
template <bool FIRST, bool U8, int RT = JT, int TAB = 0>
__global__ __launch_bounds__(256) void k_jfa_step(const unsigned *__restrict__ src, int src_pitch,
                                                  unsigned *__restrict__ dst, unsigned short *__restrict__ dist,
                                                  ScreenDims s, JfaOffsets o, int row0, int row1, JfaSrc win,
                                                  int dst_row0, const float *__restrict__ tc) {
  extern __shared__ float s_tc[];  // (TAB 1: W column texcoords, then H row texcoords)
  if constexpr (TAB == 1) {
    for (int k = (int)threadIdx.x; k < s.W + s.H; k += 256) s_tc[k] = tc[k];
    __syncthreads();
  }
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  const int j0 = row0 + blockIdx.y * (4 * RT) + (threadIdx.x >> 6);
  if (i >= s.W) return;
  const Axis ax{s.W, s.powW}, ay{s.H, s.powH};
  const float fw = (float)s.W, fh = (float)s.H;
  auto tcx = [&](int q) { return TAB == 1 ? s_tc[q] : (TAB == 2 ? tc_rcp(q, fw, o.rw) : texcoord(q, ax)); };
  auto tcy = [&](int q) { return TAB == 1 ? s_tc[s.W + q] : (TAB == 2 ? tc_rcp(q, fh, o.rh) : texcoord(q, ay)); };
  const float u = tcx(i);
  int ti[3];
#pragma unroll
  for (int x = 0; x < 3; ++x) ti[x] = wrap_nearest(u + o.ox[x], ax);
  unsigned seed[RT][9];
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int j = min(j0 + 4 * t, row1 - 1);  // clamped rows are computed but not stored
    const float v = tcy(j);
#pragma unroll
    for (int y = 0; y < 3; ++y) {
      const int tj = wrap_nearest(v + o.oy[y], ay);
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        if (FIRST) {
          const bool occ = (src[(size_t)tj * src_pitch + (ti[x] >> 5)] >> (ti[x] & 31)) & 1u;
          if constexpr (U8)
            seed[t][y * 3 + x] = occ ? pack_seed_u8(ti[x], tj, ax, ay) : 0u;
          else
            seed[t][y * 3 + x] = occ ? pack_seed(ti[x], tj) : kNoSeed;
        } else if (win.on) {  // row-strip shard: the tap's rows sit in a local window (JfaSrc)
          int lr = tj - win.row0[y];
          lr += lr < 0 ? s.H : 0;
          seed[t][y * 3 + x] = win.base[y][(size_t)lr * src_pitch + ti[x]];
        } else {
          seed[t][y * 3 + x] = src[(size_t)tj * src_pitch + ti[x]];
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int j = j0 + 4 * t;
    if (j >= row1) break;
    const float v = tcy(j);
    float minDist = 1.0f, bx = 0.0f, by = 0.0f;
    unsigned best = U8 ? 0u : kNoSeed;
#pragma unroll
    for (int k = 0; k < 9; ++k) {  // y outer, x inner: the first of equal distances wins
      const unsigned sd = seed[t][k];
      if (U8 ? seed_u8_ok(sd) : sd != kNoSeed) {  // peek.x != 0 && peek.y != 0 (f32: a seed's uv is never 0)
        const float px = U8 ? (float)(sd & 0xFFFFu) * kInv255 : tcx((int)(sd & 0xFFFFu));
        const float py = U8 ? (float)(sd >> 16) * kInv255 : tcy((int)(sd >> 16));
        const float dx = px - u, dy = py - v;
        const float d = dx * dx + dy * dy;
        if (d < minDist) {
          minDist = d;
          bx = px;
          by = py;
          best = sd;
        }
      }
    }
    dst[(size_t)(j - dst_row0) * s.pitch + i] = best;
    if (dist) {
      // DistanceField.fs: distance(fragTexCoord, seed) -> packUNorm16: store the 16-bit q
      // (RadianceCascades.fs unpackUNorm16 recovers exactly q / 65535)
      const float dx = u - bx, dy = v - by;
      const float d = sqrtf(dx * dx + dy * dy);
      const float cl = fminf(fmaxf(d, 0.0f), 1.0f);
      dist[(size_t)j * s.pitch + i] = (unsigned short)(unsigned)(cl * 65535.0f + 0.5f);
    }
  }
}

// JumpFlood.fs's scan of a texel's 9 taps ("d < minDist" from minDist = 1, y outer, x inner: the first
// of equal distances wins) as a min over per-tap keys and a select from the last tap to the first (no
// compare-and-swap chain, whose VCC hand-offs serialise).  The keys are the shader's squared distance
// scaled by the power of two mx^2 (mx = max(W, H); o.scx = mx / W, o.scy = mx / H): every fragTexCoord
// difference is (si - i) / W exactly, and a power-of-two scale commutes with each rounding, so the keys
// order as the shader's.  Non-negative finite floats order as their bit patterns.
//   IKEY (W == H <= 4096): (si - i)^2 and (sj - j)^2 are integers below 2^24, exact in fp32, so the
//     rounded float sum is the integer sum converted with round-to-nearest-even: one packed 16-bit
//     subtract and one clamped 16-bit dot product per tap, compared as integers.
//   otherwise: the packed 16-bit difference converted (exact: |si - i| < 2^15; the no-seed value
//     0x8000 wraps to the same magnitude), scaled, squared and added in fp32 as the shader rounds.
//   hybrid (KM 2; W == H, 4096 < W <= 16384): the integer keys first.  When their minimum m is below 2^24, every
//     tap that can win has an integer key below 2^24 -- exact in fp32, so its float key equals it -- and every
//     other tap's float key is >= 2^24 (rounding never leaves the binade), so the integer argmin (first of
//     equal) is the shader's; m < 2^24 <= dinit is a seed.  Otherwise (the nearest candidate 4096 texels or
//     more away) the lane takes the float keys.
// A key >= dinit = mx^2 loses to the initial minDist (kNoSeed's is >= 2^28 >= dinit).  *key: the
// winner's key as a float; sqrt(*key) / mx is its distance (DistanceField.fs) to the bit, the same
// power-of-two argument.  KM: 0 float keys, 1 integer keys (IKEY), 2 hybrid.
template <int KM>
__device__ __forceinline__ unsigned jfa_best9(const unsigned sd[9], unsigned here, const JfaTaps &o, float *key) {
  typedef short v2s __attribute__((ext_vector_type(2)));
  if constexpr (KM == 2) {
    unsigned kb[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const v2s d = __builtin_bit_cast(v2s, sd[k]) - __builtin_bit_cast(v2s, here);
      kb[k] = (unsigned)__builtin_amdgcn_sdot2(d, d, 0, true);
    }
    const unsigned m =
        min(min(min(kb[0], kb[1]), min(kb[2], kb[3])), min(min(kb[4], kb[5]), min(min(kb[6], kb[7]), kb[8])));
    if (m < (1u << 24)) {
      unsigned best = sd[8];
#pragma unroll
      for (int k = 7; k >= 0; --k) best = kb[k] == m ? sd[k] : best;
      *key = (float)m;
      return best;
    }
    return jfa_best9<0>(sd, here, o, key);
  }
  constexpr bool IKEY = KM == 1;
  unsigned kb[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const v2s d = __builtin_bit_cast(v2s, sd[k]) - __builtin_bit_cast(v2s, here);
    if constexpr (IKEY) {
      kb[k] = (unsigned)__builtin_amdgcn_sdot2(d, d, 0, true);  // clamped: >= 0
    } else {
      const float fx = (float)d.x * o.scx, fy = (float)d.y * o.scy;
      kb[k] = __float_as_uint(fx * fx + fy * fy);
    }
  }
  const unsigned m = min(min(min(kb[0], kb[1]), min(kb[2], kb[3])), min(min(kb[4], kb[5]), min(min(kb[6], kb[7]), kb[8])));
  unsigned best = sd[8];
#pragma unroll
  for (int k = 7; k >= 0; --k) best = kb[k] == m ? sd[k] : best;
  *key = IKEY ? (float)m : __uint_as_float(m);
  return m >= (IKEY ? (unsigned)o.dinit : __float_as_uint(o.dinit)) ? kNoSeed : best;
}

// DistanceField.fs (distance(fragTexCoord, seed) -> packUNorm16) of texel (i, j) from its JumpFlood
// result: sqrt(key) / mx when a seed was found (jfa_best9), else the distance to uv (0, 0).
__device__ __forceinline__ unsigned short jfa_dist_q(unsigned best, float key, int i, int j, ScreenDims s, const JfaTaps &o) {
  float d;
  if (best != kNoSeed) {
    d = sqrtf(key) * o.inv_mx;
  } else {
    const Axis ax{s.W, 1}, ay{s.H, 1};
    const float dx = texcoord(i, ax), dy = texcoord(j, ay);
    d = sqrtf(dx * dx + dy * dy);
  }
  const float cl = fminf(fmaxf(d, 0.0f), 1.0f);
  return (unsigned short)(unsigned)(cl * 65535.0f + 0.5f);
}

// JumpFlood.fs step for power-of-two W and H.  There every fragTexCoord + offset is exact, so a
// tap's NEAREST texel is (i + dx, j + dy) & (size - 1) with integer dx, dy fixed per step (host:
// floor(0.5 + offset * size)); tap rows are wave-uniform (scalar row addresses).  Keys and the
// distance: jfa_best9 / jfa_dist_q.
// U8: RGBA8 jumpRT (quantized seed uv, pack_seed_u8): the same integer taps, the float distance of
// k_jfa_step's U8 path (the seed's uv is k * (1/255), not its texel centre).
// LDS: a short step (offset s <= 8 texels on both axes): the workgroup stages its 64 x 16 tile and
// an s-texel ring of the previous step in LDS (each texel loaded once, rows wrapped), then reads the
// 9 taps of every texel from LDS (tuning "jfa_lds"; same seeds, same bits).
constexpr int kJfaLdsMax = 8;
template <bool FIRST, int IKEY, bool U8 = false, bool LDS = false>  // (IKEY: the key mode of jfa_best9)
__global__ __launch_bounds__(256) void k_jfa_p2(const unsigned *__restrict__ src, int src_pitch,
                                                unsigned *__restrict__ dst, unsigned short *__restrict__ dist,
                                                ScreenDims s, JfaTaps o, int row0, int row1, int lattice,
                                                JfaSrc win, int dst_row0) {
  int bx = blockIdx.x, by = blockIdx.y;
  if (lattice) {
    // Lattice order for the long steps: the tiles (bx + a * ptx, by + b * pty) tap one another
    // (offsets are whole multiples of the 64 x 16 tile), so walk one such lattice after the
    // other, each XCD a contiguous run (xcd_logical_id): a tile's 9 taps are then read from that
    // XCD's L2 by the 9 workgroups that need them.  Powers of two throughout (host-checked).
    const int gx = gridDim.x, gy = gridDim.y;
    const int l = xcd_logical_id(by * gx + bx, gx * gy);
    const int sx = __builtin_ctz((unsigned)max(1, o.dx[2] >> 6)), sy = __builtin_ctz((unsigned)max(1, o.dy[2] / (4 * JT)));
    const int lxs = __builtin_ctz((unsigned)gx) - sx, lys = __builtin_ctz((unsigned)gy) - sy;  // log2 lattice extent
    const int ph = l >> (lxs + lys), k = l & ((1 << (lxs + lys)) - 1);
    bx = (ph & ((1 << sx) - 1)) + ((k & ((1 << lxs) - 1)) << sx);
    by = (ph >> sx) + ((k >> lxs) << sy);
  }
  const int i = bx * 64 + (threadIdx.x & 63);
  const int j0 = row0 + by * (4 * JT) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (i >= s.W) return;
  unsigned ti[3];  // unsigned: scalar row base + 32-bit lane offset addressing
#pragma unroll
  for (int x = 0; x < 3; ++x) ti[x] = (unsigned)(i + o.dx[x]) & (unsigned)(s.W - 1);
  unsigned seed[JT][9];
  unsigned qx[3];  // U8 first step: the quantized u of each tap column (pack_seed_u8's low half)
#pragma unroll
  for (int x = 0; x < 3; ++x) qx[x] = (FIRST && U8) ? pack_seed_u8((int)ti[x], 0, Axis{s.W, 1}, Axis{s.H, 1}) & 0xFFFFu : 0u;
  if constexpr (LDS && !FIRST) {
    constexpr int TWM = 64 + 2 * kJfaLdsMax, THM = 4 * JT + 2 * kJfaLdsMax;
    __shared__ unsigned tile[THM * TWM];
    const int sh = o.dy[2], TW = 64 + 2 * sh, TH = 4 * JT + 2 * sh;  // host: dx[2] == dy[2] = sh <= 8
    const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    const int jb = row0 + by * (4 * JT) - sh, ib = bx * 64 - sh;
    // wave w stages rows w, w + 4, ...; a lane two columns; every load issued before the first store
    constexpr int RPW = THM / 4;
    unsigned va[RPW], vb[RPW];
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
      const int r = min(wv + 4 * q, TH - 1);
      const unsigned *row = src + (size_t)((unsigned)(jb + r) & (unsigned)(s.H - 1)) * src_pitch;
      va[q] = row[(unsigned)(ib + lane) & (unsigned)(s.W - 1)];
      vb[q] = row[(unsigned)(ib + 64 + min(lane, TW - 65)) & (unsigned)(s.W - 1)];
    }
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
      const int r = wv + 4 * q;
      if (r < TH) {
        tile[r * TWM + lane] = va[q];
        if (lane < TW - 64) tile[r * TWM + 64 + lane] = vb[q];
      }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < JT; ++t) {
      const int rl = wv + 4 * t + sh;  // the texel's tile row (clamped rows are computed, not stored)
#pragma unroll
      for (int y = 0; y < 3; ++y)
#pragma unroll
        for (int x = 0; x < 3; ++x) seed[t][y * 3 + x] = tile[(rl + o.dy[y]) * TWM + lane + sh + o.dx[x]];
    }
  } else {
#pragma unroll
  for (int t = 0; t < JT; ++t) {
    const int j = min(j0 + 4 * t, row1 - 1);  // clamped rows are computed but not stored
#pragma unroll
    for (int y = 0; y < 3; ++y) {
      const unsigned tj = (unsigned)(j + o.dy[y]) & (unsigned)(s.H - 1);
      // row-strip shard (not the first step): the tap's rows sit in a local window (JfaSrc)
      const unsigned *row = (!FIRST && win.on)
                                ? win.base[y] + (size_t)((tj - (unsigned)win.row0[y]) & (unsigned)(s.H - 1)) * src_pitch
                                : src + (size_t)tj * src_pitch;
      const unsigned qy = (FIRST && U8) ? pack_seed_u8(0, (int)tj, Axis{s.W, 1}, Axis{s.H, 1}) & 0xFFFF0000u : 0u;
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        if (FIRST) {
          const bool occ = (row[ti[x] >> 5] >> (ti[x] & 31)) & 1u;
          if constexpr (U8)
            seed[t][y * 3 + x] = occ ? (qy | qx[x]) : 0u;  // = pack_seed_u8(ti[x], tj)
          else
            seed[t][y * 3 + x] = occ ? ((tj << 16) | ti[x]) : kNoSeed;
        } else {
          seed[t][y * 3 + x] = *reinterpret_cast<const unsigned *>(reinterpret_cast<const char *>(row) + (ti[x] << 2));
        }
      }
    }
  }
  }
#pragma unroll
  for (int t = 0; t < JT; ++t) {
    const int j = j0 + 4 * t;
    if (j >= row1) break;
    if constexpr (U8) {  // JumpFlood.fs on RGBA8 seeds, as k_jfa_step<., true>
      const Axis ax{s.W, 1}, ay{s.H, 1};
      const float u = texcoord(i, ax), v = texcoord(j, ay);
      // The sequential "d < minDist" update (minDist = 1) keeps the first valid tap holding the
      // minimum, if below 1.  Distances are non-negative finite floats, ordered as their bit
      // patterns: a min3 tree over the 9 keys (an invalid tap keys 1.0), then a select from the
      // last tap to the first; the winner's uv is recomputed from its seed (same bits).
      unsigned kb[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const unsigned sd = seed[t][k];
        const float px = (float)(sd & 0xFFFFu) * kInv255, py = (float)(sd >> 16) * kInv255;
        const float dx = px - u, dy = py - v;
        kb[k] = seed_u8_ok(sd) ? __float_as_uint(dx * dx + dy * dy) : 0x3f800000u;
      }
      const unsigned m = min(min(min(kb[0], kb[1]), min(kb[2], kb[3])),
                             min(min(kb[4], kb[5]), min(min(kb[6], kb[7]), kb[8])));
      unsigned best = seed[t][8];
#pragma unroll
      for (int k = 7; k >= 0; --k) best = kb[k] == m ? seed[t][k] : best;
      if (m >= 0x3f800000u) best = 0u;
      dst[(size_t)(j - dst_row0) * s.pitch + i] = best;
      if (dist) {
        const float bx = best ? (float)(best & 0xFFFFu) * kInv255 : 0.0f;
        const float by = best ? (float)(best >> 16) * kInv255 : 0.0f;
        const float dx = u - bx, dy = v - by;
        const float d = sqrtf(dx * dx + dy * dy);
        const float cl = fminf(fmaxf(d, 0.0f), 1.0f);
        dist[(size_t)j * s.pitch + i] = (unsigned short)(unsigned)(cl * 65535.0f + 0.5f);
      }
      continue;
    }
    float key;
    const unsigned best = jfa_best9<IKEY>(seed[t], pack_seed(i, j), o, &key);
    dst[(size_t)(j - dst_row0) * s.pitch + i] = best;
    if (dist) dist[(size_t)j * s.pitch + i] = jfa_dist_q(best, key, i, j, s, o);  // DistanceField.fs
  }
}

// JumpFlood.fs step with a short isotropic offset S (1, 2 or 4 texels on both axes) on a power-of-two screen: a
// lane owns JR consecutive rows of one column instead of JT rows 4 apart, so the 3 x JR tap rows of its texels are
// the JR + 2 S rows j0 - S .. j0 + JR - 1 + S, each loaded once (3 (JR + 2 S) loads for JR texels: S = 1 at JR = 8
// issues 30 tap loads where k_jfa_p2 issues 72).  Same taps, scan order, keys and selection (jfa_best9) as
// k_jfa_p2, so the same seeds and distances.  Tuning "jfa_rows" (0: off).
template <int S, int JR, int IKEY>
__global__ __launch_bounds__(256) void k_jfa_rows(const unsigned *__restrict__ src, int src_pitch,
                                                  unsigned *__restrict__ dst, unsigned short *__restrict__ dist,
                                                  ScreenDims s, JfaTaps o, int row0, int row1) {
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  const int j0 = row0 + (int)blockIdx.y * (4 * JR) + JR * __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  if (i >= s.W) return;
  unsigned ti[3];  // byte offsets of the tap columns (scalar row base + 32-bit lane offset addressing)
#pragma unroll
  for (int x = 0; x < 3; ++x) ti[x] = ((unsigned)(i + (x - 1) * S) & (unsigned)(s.W - 1)) << 2;
  constexpr int NR = JR + 2 * S;
  unsigned v[NR][3];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const char *row = reinterpret_cast<const char *>(src + (size_t)((unsigned)(j0 - S + r) & (unsigned)(s.H - 1)) * src_pitch);
#pragma unroll
    for (int x = 0; x < 3; ++x) v[r][x] = *reinterpret_cast<const unsigned *>(row + ti[x]);
  }
#pragma unroll
  for (int t = 0; t < JR; ++t) {
    const int j = j0 + t;
    if (j >= row1) break;
    unsigned sd[9];  // y outer (rows j - S, j, j + S), x inner: JumpFlood.fs's scan order
#pragma unroll
    for (int y = 0; y < 3; ++y)
#pragma unroll
      for (int x = 0; x < 3; ++x) sd[y * 3 + x] = v[t + y * S][x];
    float key;
    const unsigned best = jfa_best9<IKEY>(sd, pack_seed(i, j), o, &key);
    dst[(size_t)j * s.pitch + i] = best;
    if (dist) dist[(size_t)j * s.pitch + i] = jfa_dist_q(best, key, i, j, s, o);  // DistanceField.fs
  }
}

hipError_t launch_jfa_step(const JfaStepArgs &a, ScreenDims s, hipStream_t st) {
  JfaSrc win{};
  if (a.window && !a.first) win = *a.window;
  int row0 = a.row0, row1 = a.row1;
  clamp_rows(s.H, row0, row1);
  if (row0 >= row1) return hipSuccess;
  JfaOffsets o;
  for (int k = 0; k < 3; ++k) {
    o.ox[k] = a.off_x[k];
    o.oy[k] = a.off_y[k];
  }
  o.rw = 1.0f / (float)s.W;
  o.rh = 1.0f / (float)s.H;
  const dim3 grid(ceil_div(s.W, 64), ceil_div(row1 - row0, 4 * JT));
  // float-path steps on small screens: one row per lane (k_jfa_step RT)
  const bool small = (size_t)s.W * (size_t)(row1 - row0) <= ((size_t)1 << 21) && a.small_rt != JT;
  const bool rt2 = a.small_rt == 2;  // two rows per lane (8-row workgroups)
  const dim3 grid1(ceil_div(s.W, 64), ceil_div(row1 - row0, rt2 ? 8 : 4));
  JfaTaps tp;
  const bool p2 = jfa_p2_taps(s, a.off_x, a.off_y, &tp);
  // lattice order (k_jfa_p2) for whole-frame launches whose steps span several tiles (not the
  // first step: its taps read the 2 MB occupancy mask, which every L2 holds anyway)
  const bool full = !a.first && !win.on && row0 == 0 && row1 == s.H && s.W >= 64 && s.H >= 4 * JT && s.H % (4 * JT) == 0;
  const int lattice = p2 && full && (tp.dx[2] >= 128 || tp.dy[2] >= 64) && tp.dx[2] >= 0 && tp.dy[2] >= 0 &&
                      (tp.dx[2] & (tp.dx[2] - 1)) == 0 && (tp.dy[2] & (tp.dy[2] - 1)) == 0 &&
                      tp.dx[2] <= s.W && tp.dy[2] <= s.H;
  // every kernel of the family takes these first
#define RC2DGI_JFA_IO a.src, a.src_pitch, a.dst, a.dist, s
  // short isotropic steps: consecutive rows per lane, each tap row loaded once (k_jfa_rows)
  const int sh = tp.dy[2];
  if (p2 && !s.u8 && !a.first && !win.on && a.dst_row0 == 0 && (a.jrows == 4 || a.jrows == 8) && s.W % 64 == 0 &&
      tp.dx[0] == -sh && tp.dx[1] == 0 && tp.dx[2] == sh && tp.dy[0] == -sh && tp.dy[1] == 0 && (sh == 1 || sh == 2 || sh == 4)) {
    const bool ikey = s.W == s.H && s.W <= 4096;
    const dim3 gr(s.W / 64, ceil_div(row1 - row0, 4 * a.jrows));
#define RC2DGI_JR(SV, JV)                                                                                  \
  do {                                                                                                     \
    if (ikey)                                                                                              \
      hipLaunchKernelGGL((k_jfa_rows<SV, JV, true>), gr, dim3(256), 0, st, RC2DGI_JFA_IO, tp, row0, row1);  \
    else                                                                                                   \
      hipLaunchKernelGGL((k_jfa_rows<SV, JV, false>), gr, dim3(256), 0, st, RC2DGI_JFA_IO, tp, row0, row1); \
  } while (0)
    if (a.jrows == 8) {
      if (sh == 1) RC2DGI_JR(1, 8); else if (sh == 2) RC2DGI_JR(2, 8); else RC2DGI_JR(4, 8);
    } else {
      if (sh == 1) RC2DGI_JR(1, 4); else if (sh == 2) RC2DGI_JR(2, 4); else RC2DGI_JR(4, 4);
    }
#undef RC2DGI_JR
    return hipGetLastError();
  }
  // k_jfa_p2<F, K, U, L>: lattice order LAT
#define RC2DGI_JFA(F, K, U, L, LAT)                                                                       \
  hipLaunchKernelGGL((k_jfa_p2<F, K, U, L>), grid, dim3(256), 0, st, RC2DGI_JFA_IO, tp, row0, row1, LAT, win, \
                     a.dst_row0)
  // k_jfa_step<FV, UV, RV, TV> on grid G with LDS bytes of dynamic LDS and the texcoord table TC
#define RC2DGI_JFA_S(G, FV, UV, RV, TV, LDS, TC)                                                            \
  hipLaunchKernelGGL((k_jfa_step<FV, UV, RV, TV>), G, dim3(256), LDS, st, RC2DGI_JFA_IO, o, row0, row1, win, \
                     a.dst_row0, TC)
  if (s.u8 && p2) {  // RGBA8 jumpRT on a power-of-two screen: integer taps, quantized-uv distance
    if (a.first) RC2DGI_JFA(true, false, true, false, lattice); else RC2DGI_JFA(false, false, true, false, lattice);
  } else if (s.u8) {  // RGBA8 jumpRT: quantized seed uv, the float path
#define RC2DGI_JFA_U8(G, RV)                                \
  do {                                                      \
    if (a.first)                                            \
      RC2DGI_JFA_S(G, true, true, RV, 0, 0, nullptr);       \
    else                                                    \
      RC2DGI_JFA_S(G, false, true, RV, 0, 0, nullptr);      \
  } while (0)
    if (small && rt2) RC2DGI_JFA_U8(grid1, 2); else if (small) RC2DGI_JFA_U8(grid1, 1); else RC2DGI_JFA_U8(grid, JT);
#undef RC2DGI_JFA_U8
  } else if (p2 && a.lds && !a.first && !win.on && tp.dx[2] == tp.dy[2] && tp.dy[2] >= 1 && tp.dy[2] <= kJfaLdsMax &&
             (row1 - row0) % (4 * JT) == 0 && s.W % 64 == 0) {
    const bool ikey = s.W == s.H && s.W <= 4096;
    if (ikey) RC2DGI_JFA(false, true, false, true, 0); else RC2DGI_JFA(false, false, false, true, 0);
  } else if (p2) {
    // key mode (jfa_best9): integer keys on square screens up to 4096, hybrid up to 16384, else float
    const int km = s.W == s.H ? (s.W <= 4096 ? 1 : (s.W <= 16384 ? 2 : 0)) : 0;
#define RC2DGI_JFA_K(F, K) RC2DGI_JFA(F, K, false, false, lattice)
    if (a.first) {
      if (km == 1) RC2DGI_JFA_K(true, 1); else if (km == 2) RC2DGI_JFA_K(true, 2); else RC2DGI_JFA_K(true, 0);
    } else {
      if (km == 1) RC2DGI_JFA_K(false, 1); else if (km == 2) RC2DGI_JFA_K(false, 2); else RC2DGI_JFA_K(false, 0);
    }
#undef RC2DGI_JFA_K
  } else {
    // the float path: texcoords by tc_rcp where the host proved it exact (tmode 2), from the context's table
    // (tmode 1), else divided (k_jfa_step TAB)
    const int tm = a.tmode == 2 ? 2 : ((a.tmode == 1 && a.tc && s.W + s.H <= kTcTabMax) ? 1 : 0);
    const size_t tab_bytes = tm == 1 ? (size_t)(s.W + s.H) * sizeof(float) : 0;
#define RC2DGI_JFA_F(G, FV, RV)                                               \
  do {                                                                        \
    if (tm == 1)                                                              \
      RC2DGI_JFA_S(G, FV, false, RV, 1, tab_bytes, a.tc);                     \
    else if (tm == 2)                                                         \
      RC2DGI_JFA_S(G, FV, false, RV, 2, 0, nullptr);                          \
    else                                                                      \
      RC2DGI_JFA_S(G, FV, false, RV, 0, 0, nullptr);                          \
  } while (0)
    if (small && rt2) {
      if (a.first) RC2DGI_JFA_F(grid1, true, 2); else RC2DGI_JFA_F(grid1, false, 2);
    } else if (small) {
      if (a.first) RC2DGI_JFA_F(grid1, true, 1); else RC2DGI_JFA_F(grid1, false, 1);
    } else {
      if (a.first) RC2DGI_JFA_F(grid, true, JT); else RC2DGI_JFA_F(grid, false, JT);
    }
#undef RC2DGI_JFA_F
  }
#undef RC2DGI_JFA_S
#undef RC2DGI_JFA
#undef RC2DGI_JFA_IO
  return hipGetLastError();
}

// ---------------------------------------------------------------- JumpFlood: the long steps in one kernel
// The long steps (JumpFlood.fs, RC2DGI.cs:296-326).  On a square power-of-two screen step t taps at
// +-s_t = W / 2^(t+1) texels on both axes, so the texels (x0 + a g, y0 + b g) of one residue
// (x0, y0) modulo g = W / 16 tap only one another in the steps with s_t >= g (t = 0..3): a 16 x 16
// torus whose steps tap +-8, 4, 2, 1 lattice points.  A workgroup holds 32 adjacent residues (one
// 128-byte segment at each of the 256 lattice points, 32 KB of LDS), seeds them from the ScreenUV
// mask (step 0's input), runs the four steps in LDS and writes J_3 -- each texel read and written
// once, no intermediate image in HBM.  A thread owns texel u of segment a at every lattice row b, so
// every tap row is a compile-time LDS offset.  Same taps, order and keys as k_jfa_p2.
// Lattice side LAT = 16: steps 0-3, a workgroup of 32 residues (one 128-byte segment per lattice point, 32 KB of
// LDS, 512 threads).  LAT = 32 (round 5): steps 0-4 on a 32 x 32 torus (g = W / 32) whose steps tap +-16 ... 1
// lattice points, 16 residues per workgroup (64-byte segments, 64 KB of LDS, 1024 threads of 16 rows) -- one
// more step in LDS instead of a pass over HBM.
template <int LAT>
struct CosetGeo {
  static constexpr int SEG = LAT == 16 ? 32 : 16;    // residues (adjacent texels) per workgroup
  static constexpr int PLANE = SEG * LAT;             // texels per lattice row of the workgroup
  static constexpr int NTHR = LAT == 16 ? 512 : 1024;  // LAT 32: two threads per (segment, texel), 16 rows each
  static constexpr int RT = LAT * PLANE / NTHR;        // lattice rows per thread (16)
  static constexpr int STEPS = LAT == 16 ? 4 : 5;
};
// threads: one per (segment a, texel u) and all (LAT 16) or half (LAT 32) of the lattice rows (the float keys
// spill a few row coordinates at 128 VGPRs; splitting the rows over two threads to avoid it measured slower at
// 8192^2: 0.72 vs 0.58 ms)
template <int IKEY, int LAT>
__global__ __launch_bounds__(CosetGeo<LAT>::NTHR) __attribute__((amdgpu_waves_per_eu(4))) void k_jfa_coset(
    const unsigned *__restrict__ mask, int mpitch, unsigned *__restrict__ dst, ScreenDims s, JfaTaps o) {
  using G = CosetGeo<LAT>;
  constexpr int RT = G::RT, SEG = G::SEG, PLANE = G::PLANE;
  __shared__ unsigned img[LAT * PLANE];
  const int g = s.W / LAT;  // lattice spacing (host: W == H, g a multiple of SEG)
  const int nx = g / SEG;
  const int x0 = (blockIdx.x % nx) * SEG, y0 = blockIdx.x / nx;
  const int tid = (int)threadIdx.x, col0 = tid & (PLANE - 1), u = tid & (SEG - 1), a = col0 / SEG;
  const int b0 = __builtin_amdgcn_readfirstlane((tid / PLANE) * RT);  // the thread's first lattice row (per wave)
  const int x = x0 + a * g + u;
  unsigned m[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) m[r] = mask[(size_t)(y0 + (b0 + r) * g) * mpitch + (x >> 5)];
  unsigned v[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) {  // ScreenUV seeds (k_jfa_p2<FIRST>)
    const unsigned y = (unsigned)(y0 + (b0 + r) * g);
    v[r] = ((m[r] >> (x & 31)) & 1u) ? ((y << 16) | (unsigned)x) : kNoSeed;
    img[(b0 + r) * PLANE + col0] = v[r];
  }
#pragma unroll
  for (int st = 0; st < G::STEPS; ++st) {
    const int k = (LAT / 2) >> st;  // tap offset in lattice points
    __syncthreads();
    int col[3];
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) col[dx] = (((a + (dx - 1) * k) & (LAT - 1)) * SEG) + u;
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      unsigned sd[9];
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) sd[dy * 3 + dx] = img[((b0 + r + (dy - 1) * k) & (LAT - 1)) * PLANE + col[dx]];
      float key;
      v[r] = jfa_best9<IKEY>(sd, ((unsigned)(y0 + (b0 + r) * g) << 16) | (unsigned)x, o, &key);
    }
    if (st < G::STEPS - 1) {
      __syncthreads();
#pragma unroll
      for (int r = 0; r < RT; ++r) img[(b0 + r) * PLANE + col0] = v[r];
    }
  }
#pragma unroll
  for (int r = 0; r < RT; ++r) dst[(size_t)(y0 + (b0 + r) * g) * s.pitch + x] = v[r];
}

// the taps of a one-texel step: the fused kernels take their key scale, dinit and 1 / max(W, H) from them (the same
// for every step)
static bool jfa_unit_taps(ScreenDims s, JfaTaps *tp) {
  const float ox[3] = {-1.0f / (float)s.W, 0.0f / (float)s.W, 1.0f / (float)s.W};
  const float oy[3] = {-1.0f / (float)s.H, 0.0f / (float)s.H, 1.0f / (float)s.H};
  return jfa_p2_taps(s, ox, oy, tp);
}

int jfa_coset_steps(ScreenDims s, int S, int lat) {
  // steps 0 .. log2(lat) - 1 tap +-W/2 ... W/lat on a square power-of-two screen whose lattice spacing W / lat
  // holds whole segments; the steps must not be the last two (J_{S-2}, J_{S-1} are visible) nor overlap the
  // fused short steps
  const int nst = lat == 32 ? 5 : 4, seg = lat == 32 ? CosetGeo<32>::SEG : CosetGeo<16>::SEG;
  if (!(s.powW && s.powH) || s.u8 || s.W != s.H || s.W < lat * seg || s.W > 16384 || S < nst + 5) return 0;
  for (int t = 0; t < nst; ++t) {
    float ox[3], oy[3];
    jfa_offsets(s.W, s.H, t, ox, oy);
    JfaTaps tp;
    if (!jfa_p2_taps(s, ox, oy, &tp)) return 0;
    const int o = s.W >> (t + 1);
    if (tp.dx[0] != -o || tp.dx[2] != o || tp.dy[0] != -o || tp.dy[2] != o) return 0;
  }
  return nst;
}

hipError_t launch_jfa_coset(const unsigned *mask, int mpitch, unsigned *dst, ScreenDims s, hipStream_t st, int lat) {
  JfaTaps tp;
  if (!jfa_unit_taps(s, &tp)) return hipErrorInvalidValue;
  // key mode: integer up to 4096 (lattice 32 runs there only), hybrid above (jfa_coset_steps: square, <= 16384)
#define RC2DGI_COSET(L, K)                                                                                        \
  do {                                                                                                            \
    const int g = s.W / L;                                                                                        \
    const dim3 grid((g / CosetGeo<L>::SEG) * g);                                                                  \
    hipLaunchKernelGGL((k_jfa_coset<K, L>), grid, dim3(CosetGeo<L>::NTHR), 0, st, mask, mpitch, dst, s, tp);       \
  } while (0)
  if (lat == 32) {
    if (s.W > 4096) return hipErrorInvalidValue;
    RC2DGI_COSET(32, 1);
  } else if (s.W <= 4096) {
    RC2DGI_COSET(16, 1);
  } else {
    RC2DGI_COSET(16, 2);
  }
#undef RC2DGI_COSET
  return hipGetLastError();
}

// ---------------------------------------------------------------- JumpFlood: the last steps in one kernel
// One step of k_jfa_tail: offset D texels, from `in` (the tile grown by 2D - 1 texels, the ring the later steps
// still need plus this step's reach) to `out` (grown by D - 1).  Texel (lx, ly) of `out` is screen texel
// (x0 - (D - 1) + lx, y0 - (D - 1) + ly) wrapped (REPEAT); its taps sit at in columns lx, lx + D, lx + 2D.
template <int D, int T, int NTHR, int KM>
__device__ __forceinline__ void jfa_tail_step(const unsigned *in, unsigned *out, int x0, int y0, unsigned mw,
                                              unsigned mh, const JfaTaps &o) {
  constexpr int RO = D - 1, WI = T + 2 * (2 * D - 1), WO = T + 2 * RO, NO = WO * WO;
  constexpr int NIT = (NO + NTHR - 1) / NTHR, NP = 2;  // texels per thread, taken NP at a time (their LDS reads overlap)
#pragma unroll
  for (int it = 0; it < NIT; it += NP) {
    unsigned sd[NP][9], here[NP];
    int kk[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      kk[p] = (int)threadIdx.x + (it + p) * NTHR;
      const int k = min(kk[p], NO - 1);  // (past the end: a valid texel, not stored)
      const int ly = k / WO, lx = k - ly * WO;
#pragma unroll
      for (int y = 0; y < 3; ++y)
#pragma unroll
        for (int x = 0; x < 3; ++x) sd[p][y * 3 + x] = in[(ly + y * D) * WI + lx + x * D];
      here[p] = pack_seed((int)((unsigned)(x0 - RO + lx) & mw), (int)((unsigned)(y0 - RO + ly) & mh));
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      float key;
      const unsigned b = jfa_best9<KM>(sd[p], here[p], o, &key);
      if (it + p < NIT && kk[p] < NO) out[kk[p]] = b;
    }
  }
}

// The last NT JumpFlood steps (offsets 2^(NT-1) .. 2, 1 texels) of a square power-of-two screen up to 16384 (integer
// keys up to 4096, hybrid above) in one kernel.  A workgroup loads a T x T tile of J_{S-NT-1} grown by the 2^NT - 1 texels the steps reach
// (rows and columns wrap) into LDS once, runs the steps there -- the step of offset d on the tile grown by d - 1,
// the ring the later steps still read -- and writes its tile of J_{S-1} with the DistanceField, and of J_{S-2} (the
// centre tap of the last step): the two JumpFlood textures a frame leaves visible.  Same taps, keys and selection
// (jfa_best9) as k_jfa_p2: the same seeds and distances.  Per texel one 4-byte read (plus the ring, mostly from L2)
// and 10 bytes written, where NT separate steps read and write 4 bytes each per step; the grown tiles cost
// 1.19 x the texel-steps at NT = 4, T = 64.  XCD-contiguous tile order (neighbours share their rings in one L2).
template <int NT, int T, int NTHR, int KM>  // (KM: the key mode of jfa_best9, integer or hybrid)
__global__ __launch_bounds__(NTHR) void k_jfa_tail(const unsigned *__restrict__ src, unsigned *__restrict__ dst,
                                                   unsigned *__restrict__ dst_prev, unsigned short *__restrict__ dist,
                                                   ScreenDims s, JfaTaps o) {
  static_assert(NT >= 2 && NT <= 4, "two to four fused steps");
  constexpr int W0 = T + 2 * ((1 << NT) - 1), W1 = T + 2 * ((1 << (NT - 1)) - 1);
  __shared__ unsigned bufA[W0 * W0];
  __shared__ unsigned bufB[W1 * W1];
  const int gx = (int)gridDim.x, n = gx * (int)gridDim.y;
  const int l = xcd_logical_id((int)(blockIdx.y * gridDim.x + blockIdx.x), n);
  const int x0 = (l % gx) * T, y0 = (l / gx) * T;
  const unsigned mw = (unsigned)s.W - 1u, mh = (unsigned)s.H - 1u;
  constexpr int R0 = (1 << NT) - 1, N0 = W0 * W0, NL = (N0 + NTHR - 1) / NTHR;
  {  // every load issued before the first LDS store
    unsigned v[NL];
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      const int k = min((int)threadIdx.x + q * NTHR, N0 - 1);
      const int ly = k / W0, lx = k - ly * W0;
      v[q] = src[((unsigned)(y0 - R0 + ly) & mh) * (unsigned)s.pitch + ((unsigned)(x0 - R0 + lx) & mw)];
    }
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      const int k = (int)threadIdx.x + q * NTHR;
      if (k < N0) bufA[k] = v[q];
    }
  }
  __syncthreads();
  if constexpr (NT == 4) {
    jfa_tail_step<8, T, NTHR, KM>(bufA, bufB, x0, y0, mw, mh, o);
    __syncthreads();
    jfa_tail_step<4, T, NTHR, KM>(bufB, bufA, x0, y0, mw, mh, o);
    __syncthreads();
    jfa_tail_step<2, T, NTHR, KM>(bufA, bufB, x0, y0, mw, mh, o);
  } else if constexpr (NT == 3) {
    jfa_tail_step<4, T, NTHR, KM>(bufA, bufB, x0, y0, mw, mh, o);
    __syncthreads();
    jfa_tail_step<2, T, NTHR, KM>(bufB, bufA, x0, y0, mw, mh, o);
  } else {
    jfa_tail_step<2, T, NTHR, KM>(bufA, bufB, x0, y0, mw, mh, o);
  }
  __syncthreads();
  const unsigned *in = NT == 3 ? bufA : bufB;  // J_{S-2} on the tile grown by 1
  constexpr int WI = T + 2, NIT = T * T / NTHR;
  static_assert(T * T % (2 * NTHR) == 0, "whole pairs of texels per thread");
#pragma unroll
  for (int it = 0; it < NIT; it += 2) {
    unsigned sd[2][9];
    int i[2], j[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int k = (int)threadIdx.x + (it + p) * NTHR, ly = k / T, lx = k - ly * T;
#pragma unroll
      for (int y = 0; y < 3; ++y)
#pragma unroll
        for (int x = 0; x < 3; ++x) sd[p][y * 3 + x] = in[(ly + y) * WI + lx + x];
      i[p] = x0 + lx;
      j[p] = y0 + ly;
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      float key;
      const unsigned best = jfa_best9<KM>(sd[p], pack_seed(i[p], j[p]), o, &key);
      const unsigned g = (unsigned)j[p] * (unsigned)s.pitch + (unsigned)i[p];
      dst[g] = best;
      dst_prev[g] = sd[p][4];
      dist[g] = jfa_dist_q(best, key, i[p], j[p], s, o);  // DistanceField.fs
    }
  }
}

constexpr int kJfaTailT = 64, kJfaTailThreads = 512;

bool jfa_tail_ok(ScreenDims s, int S, int nt) {
  if (nt < 2 || nt > 4 || s.u8 || !(s.powW && s.powH) || s.W != s.H || s.W > 16384 || s.W < kJfaTailT ||
      s.W % kJfaTailT != 0 || S < nt + 1)
    return false;
  for (int t = S - nt; t < S; ++t) {  // offsets 2^(nt-1) .. 1 texels, both axes, in the shader's tap order
    float ox[3], oy[3];
    jfa_offsets(s.W, s.H, t, ox, oy);
    JfaTaps tp;
    if (!jfa_p2_taps(s, ox, oy, &tp)) return false;
    const int d = 1 << (S - 1 - t);
    if (tp.dx[0] != -d || tp.dx[1] != 0 || tp.dx[2] != d || tp.dy[0] != -d || tp.dy[1] != 0 || tp.dy[2] != d) return false;
  }
  return true;
}

hipError_t launch_jfa_tail(const unsigned *src, unsigned *dst, unsigned *dst_prev, unsigned short *dist, ScreenDims s,
                           int S, int nt, hipStream_t st) {
  if (!jfa_tail_ok(s, S, nt) || !src || !dst || !dst_prev || !dist || src == dst || src == dst_prev)
    return hipErrorInvalidValue;
  JfaTaps tp;
  if (!jfa_unit_taps(s, &tp)) return hipErrorInvalidValue;
  const dim3 grid(s.W / kJfaTailT, s.H / kJfaTailT);
  constexpr int T = kJfaTailT, NTHR = kJfaTailThreads;
#define RC2DGI_TAIL(K)                                                                                           \
  do {                                                                                                           \
    if (nt == 4)                                                                                                 \
      hipLaunchKernelGGL((k_jfa_tail<4, T, NTHR, K>), grid, dim3(NTHR), 0, st, src, dst, dst_prev, dist, s, tp);  \
    else if (nt == 3)                                                                                            \
      hipLaunchKernelGGL((k_jfa_tail<3, T, NTHR, K>), grid, dim3(NTHR), 0, st, src, dst, dst_prev, dist, s, tp);  \
    else                                                                                                         \
      hipLaunchKernelGGL((k_jfa_tail<2, T, NTHR, K>), grid, dim3(NTHR), 0, st, src, dst, dst_prev, dist, s, tp);  \
  } while (0)
  if (s.W <= 4096) RC2DGI_TAIL(1); else RC2DGI_TAIL(2);  // integer keys, hybrid above 4096 (jfa_best9)
#undef RC2DGI_TAIL
  return hipGetLastError();
}

}  // namespace rc2dgi
