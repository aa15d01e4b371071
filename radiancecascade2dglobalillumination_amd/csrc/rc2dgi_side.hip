// rc2dgi_side.hip -- the side pass between the DistanceField and the cascades: what the RC march reads besides
// distRT, each kernel with its launcher (gfx950).  No reference shader: the surface records restate the hit branch
// of RadianceCascades.fs:79-86, the tables bound distRT from below, the re-layouts hold the same q.
//   surface records (k_shade), bound table (k_dist_cmin), both with palettes and the march field (k_shade_cmin,
//   k_shade_scan + k_shade_cells), directional clear distances (k_dir_clear), distRT tiled / packed / nibble-packed
// Includes rc2dgi_rc.h for decode_dist (the march's own hit test) and the packet formats k_rc_level reads.
#include "rc2dgi_device.h"
#include "rc2dgi_kernels.h"
#include "rc2dgi_rc.h"

#include <cmath>

namespace rc2dgi {

// ---------------------------------------------------------------- surface records
// The hit branch of SampleRadianceSDF (RadianceCascades.fs:79-86) resolved once per frame: for
// every texel a ray can stop on (decode_dist(q) < 0.001, the march's own test) the record is
// (emission, 1) when length(emission) > 0, else (albedo, _Reflectivity).  The march then needs
// one load per hit instead of an emissive load plus, for albedo hits, a second dependent one.
// Texels no ray can stop on are not written (and never read).  A wave covers 256 texels of a row
// in four 64-texel passes (every load and store instruction of the wave is one contiguous run);
// the emission and the albedo of every hittable texel are loaded together (one round trip after
// the field, not a second, dependent one for the albedo hits).
__global__ __launch_bounds__(256) void k_shade(const unsigned short *__restrict__ dist, const float4 *__restrict__ color,
                                               const float4 *__restrict__ emis, float4 *__restrict__ shade,
                                               ScreenDims s, float reflectivity) {
  const int lane = threadIdx.x & 63;
  const int i0 = blockIdx.x * 256 + lane;
  const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (j >= s.H) return;
  const size_t row = (size_t)j * s.pitch;
  unsigned q[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) q[t] = i0 + 64 * t < s.W ? dist[row + i0 + 64 * t] : 0xFFFFu;
  bool h[4];
  float4 e[4], c[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    h[t] = decode_dist(q[t]) < 0.001f;  // q = 0xFFFF (beyond the row) decodes to 1
    e[t] = c[t] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (h[t]) {
      e[t] = emis[row + i0 + 64 * t];
      c[t] = color[row + i0 + 64 * t];
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (h[t]) {
      float4 r = make_float4(e[t].x, e[t].y, e[t].z, 1.0f);
      if (!(sqrtf(e[t].x * e[t].x + e[t].y * e[t].y + e[t].z * e[t].z) > 0.0f))
        r = make_float4(c[t].x, c[t].y, c[t].z, reflectivity);
      shade[row + i0 + 64 * t] = r;
    }
  }
}

hipError_t launch_shade(const ShadeCminArgs &a, ScreenDims s, hipStream_t st) {
  hipLaunchKernelGGL(k_shade, dim3(ceil_div(s.W, 256), ceil_div(s.H, 4)), dim3(256), 0, st, a.dist, a.color, a.emis,
                     a.shade, s, a.reflectivity);
  return hipGetLastError();
}

// ---------------------------------------------------------------- coarse lower bound of the field
// One workgroup per cell of 2^csh x 2^csh texels (a kCminDim x kCminDim grid covers the screen): the cell's
// smallest distance decode_dist(min q), or 0 when some texel of the cell passes the march's hit
// test.  decode_dist is monotone, so the value bounds every texel of the cell from below: a ray
// whose sample lies in the cell advances by at least that much and does not stop there
// (k_rc_level's exit proof, kCminDim).
__global__ __launch_bounds__(256) void k_dist_cmin(const unsigned short *__restrict__ dist, int pitch,
                                                   CminT *__restrict__ cmin, int W, int H, int csh,
                                                   unsigned char *__restrict__ hitc) {
  const int x0 = (int)blockIdx.x << csh, y0 = (int)blockIdx.y << csh;
  unsigned m = 0xFFFFu;
  const bool in = x0 < W && y0 < H;
  if (in) {
    const int x1 = min(W, x0 + (1 << csh)), y1 = min(H, y0 + (1 << csh));
    if (csh >= 3 && x1 - x0 == (1 << csh) && y1 - y0 == (1 << csh)) {
      // whole cell: 16-byte loads of 8 texels (rows of 64-texel pitch keep them aligned), shifts
      // instead of the general path's integer division, several loads in flight
      const int sh = csh - 3, tot = 1 << (2 * csh - 3);
#pragma unroll 4
      for (int e = (int)threadIdx.x; e < tot; e += 256) {
        const uint4 v = *reinterpret_cast<const uint4 *>(dist + (size_t)(y0 + (e >> sh)) * pitch + x0 +
                                                          ((e & ((1 << sh) - 1)) << 3));
        const unsigned a = min(min(v.x & 0xFFFFu, v.x >> 16), min(v.y & 0xFFFFu, v.y >> 16));
        const unsigned b = min(min(v.z & 0xFFFFu, v.z >> 16), min(v.w & 0xFFFFu, v.w >> 16));
        m = min(m, min(a, b));
      }
    } else {
      const int n4 = (x1 - x0 + 3) >> 2;  // 4-texel groups per row of the cell
      const int tot = n4 * (y1 - y0);
      for (int e = (int)threadIdx.x; e < tot; e += 256) {
        const int r = e / n4;
        const int xx = x0 + 4 * (e - r * n4);
        const unsigned short *p = dist + (size_t)(y0 + r) * pitch + xx;
        if (csh >= 2 && xx + 3 < x1) {  // 8-byte aligned: x0 is a multiple of 4, rows of 64-texel pitch
          const uint2 v = *reinterpret_cast<const uint2 *>(p);
          m = min(m, min(min(v.x & 0xFFFFu, v.x >> 16), min(v.y & 0xFFFFu, v.y >> 16)));
        } else {
          for (int t = 0; t < 4; ++t)
            if (xx + t < x1) m = min(m, (unsigned)p[t]);
        }
      }
    }
  }
  if (in) {
    // REPEAT wrap: a march sample at u = 1 reads column 0 of its row, at v = 1 row 0 of its column, at
    // (1, 1) texel (0, 0) -- those texels belong to the bound of the last cell column / row too
    const int x1 = min(W, x0 + (1 << csh)), y1 = min(H, y0 + (1 << csh));
    if (x1 == W)
      for (int e = (int)threadIdx.x; e < y1 - y0; e += 256) m = min(m, (unsigned)dist[(size_t)(y0 + e) * pitch]);
    if (y1 == H)
      for (int e = (int)threadIdx.x; e < x1 - x0; e += 256) m = min(m, (unsigned)dist[x0 + e]);
    if (x1 == W && y1 == H && threadIdx.x == 0) m = min(m, (unsigned)dist[0]);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = min(m, (unsigned)__shfl_xor((int)m, o, 64));
  __shared__ unsigned s_m[4];
  if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = min(min(s_m[0], s_m[1]), min(s_m[2], s_m[3]));
    const float d = decode_dist(m);
    if (hitc) hitc[blockIdx.y * kCminDim + blockIdx.x] = (in && d < 0.001f) ? 1 : 0;
    // floor(d * scale) / scale <= d (power-of-two scaling and floor are exact); 0 where a texel hits
    cmin[blockIdx.y * kCminDim + blockIdx.x] = (in && d >= 0.001f) ? (CminT)fminf(floorf(d * kCminScale), 255.0f) : (CminT)0;
  }
}

int dist_cmin_shift(int W, int H) {
  int s = 0;
  while (((W - 1) >> s) >= kCminDim || ((H - 1) >> s) >= kCminDim) ++s;
  return s;
}

hipError_t launch_dist_cmin(const ShadeCminArgs &a, ScreenDims s, hipStream_t st) {
  hipLaunchKernelGGL(k_dist_cmin, dim3(kCminDim, kCminDim), dim3(256), 0, st, a.dist, s.pitch, a.cmin, s.W, s.H,
                     dist_cmin_shift(s.W, s.H), a.hitc);
  return hipGetLastError();
}

// k_shade and k_dist_cmin in one pass over distRT, for square power-of-two screens with cells of >= 64
// texels (W = H = kCminDim << csh, csh >= 6: 4096^2 and up).  One workgroup of NTH lanes per cell; wave w
// takes rows w, w + NW, ... of it (NW = NTH / 64 waves), a lane one column of each 64-column run, 64 / NW rows
// at a time (each load instruction one contiguous run: 128 B of distance, 1 KB of emission or albedo).  Same records, same bound table and
// flags as the two kernels (the cell minimum includes the REPEAT-wrap texels of the last row / column).
// PAL: also the cell's surface palette and the march field (see kCellPal): the distinct records of the
// cell's hittable texels in cpal[cell * kCellPalStride + i] (deduplicated in LDS; two waves inserting one record
// at once may both add it -- a wasted entry, never a wrong one), and mf = distRT with every hittable texel's
// q replaced by its palette entry i (kCellPal: no entry left, the march reads its record from shade).
// (one cell (bx, by); TAB: also its bound-table entry and hit flag)
template <bool PAL, int NTH, bool TAB>
__device__ __forceinline__ void shade_cell(const unsigned short *__restrict__ dist, const float4 *__restrict__ color,
                                           const float4 *__restrict__ emis, float4 *__restrict__ shade, ScreenDims s,
                                           float reflectivity, int csh, CminT *__restrict__ cmin,
                                           unsigned char *__restrict__ hitc, unsigned short *__restrict__ mf,
                                           float4 *__restrict__ cpal, const int bx, const int by) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int cw = 1 << csh;
  const int x0 = bx << csh, y0 = by << csh;
  __shared__ float4 s_pal[PAL ? kCellPal : 1];
  __shared__ unsigned s_rdy[PAL ? kCellPal : 1];  // entry i holds its record (set after the record is written)
  __shared__ unsigned s_npal;
  if (PAL) {
    if (threadIdx.x == 0) s_npal = 0u;
    if (threadIdx.x < kCellPal) s_rdy[threadIdx.x] = 0u;
    __syncthreads();
  }
  float4 *const gpal = PAL ? cpal + (size_t)(by * kCminDim + bx) * kCellPalStride : nullptr;
  unsigned m = 0xFFFFu;
  constexpr int NW = NTH / 64, RPW = 64 / NW;  // waves; a wave's rows of a 64-row block (NW apart)
  constexpr int GR = RPW < 8 ? RPW : 8;         // rows per record group (8; 4 with 1024 lanes)
  constexpr unsigned GM = (1u << GR) - 1u;
  const size_t rstep = (size_t)NW * s.pitch;
  for (int c = lane; c < cw; c += 64) {
    for (int rb = 0; rb < cw; rb += 64) {
      // the wave's 16 rows of this 64-row block: every distance load in flight at once, then the records
      // of the hittable texels 8 rows at a time (two round trips, not one per 4 rows)
      const size_t base = (size_t)(y0 + rb + w) * s.pitch + x0 + c;
      unsigned q[RPW];
#pragma unroll
      for (int t = 0; t < RPW; ++t) q[t] = dist[base + t * rstep];
      unsigned hm = 0;
#pragma unroll
      for (int t = 0; t < RPW; ++t) {
        m = min(m, q[t]);
        hm |= decode_dist(q[t]) < 0.001f ? 1u << t : 0u;
      }
#pragma unroll
      for (int h = 0; h < RPW / GR; ++h) {
        // (with palettes the skip is wave-uniform: the palette code below needs every lane of the wave)
        if (PAL ? __ballot((hm >> (GR * h) & GM) != 0u) == 0ull : !(hm >> (GR * h) & GM)) {
          if (PAL) {
#pragma unroll
            for (int k = 0; k < GR; ++k) mf[base + (GR * h + k) * rstep] = (unsigned short)q[GR * h + k];
          }
          continue;
        }
        float4 e[GR], cl[GR];
#pragma unroll
        for (int k = 0; k < GR; ++k) {
          e[k] = cl[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
          if (hm >> (GR * h + k) & 1u) {
            e[k] = emis[base + (GR * h + k) * rstep];
            cl[k] = color[base + (GR * h + k) * rstep];
          }
        }
        float4 rec[GR];
#pragma unroll
        for (int k = 0; k < GR; ++k) {
          const bool hit = hm >> (GR * h + k) & 1u;
          rec[k] = make_float4(e[k].x, e[k].y, e[k].z, 1.0f);
          if (!(sqrtf(e[k].x * e[k].x + e[k].y * e[k].y + e[k].z * e[k].z) > 0.0f))
            rec[k] = make_float4(cl[k].x, cl[k].y, cl[k].z, reflectivity);
          if (hit && shade) shade[base + (GR * h + k) * rstep] = rec[k];  // (no record texture: strip tables)
        }
        if (PAL) {
          // the wave's distinct records of these 8 rows, one at a time (usually one or two: a surface's texels
          // share it): the first remaining (row, lane)'s record, every (row, lane) holding the same bits, the
          // entry found or added by lane 0 of the wave -- one round per distinct record, not per row
          unsigned idx[GR];
          unsigned long long rem[GR];
#pragma unroll
          for (int k = 0; k < GR; ++k) {
            idx[k] = kCellPal;
            rem[k] = __ballot(hm >> (GR * h + k) & 1u);
          }
          for (;;) {
            int kk = -1;
#pragma unroll
            for (int k = GR - 1; k >= 0; --k) kk = rem[k] ? k : kk;  // (wave-uniform)
            if (kk < 0) break;
            unsigned long long rk = rem[0];
            float4 rv = rec[0];
#pragma unroll
            for (int k = 1; k < GR; ++k)
              if (kk == k) {
                rk = rem[k];
                rv = rec[k];
              }
            const int ld = __ffsll((long long)rk) - 1;
            const float rx = __shfl(rv.x, ld, 64), ry = __shfl(rv.y, ld, 64), rz = __shfl(rv.z, ld, 64),
                        rw = __shfl(rv.w, ld, 64);
            const auto same = [&](float4 v) {
              return __float_as_uint(v.x) == __float_as_uint(rx) && __float_as_uint(v.y) == __float_as_uint(ry) &&
                     __float_as_uint(v.z) == __float_as_uint(rz) && __float_as_uint(v.w) == __float_as_uint(rw);
            };
            unsigned long long mine[GR];
#pragma unroll
            for (int k = 0; k < GR; ++k) mine[k] = __ballot((hm >> (GR * h + k) & 1u) && same(rec[k])) & rem[k];
            // the lanes below the palette's fill compare one entry each; lane 0 adds the record if none holds it
            const unsigned n = min(__builtin_amdgcn_readfirstlane(*(volatile unsigned *)&s_npal), (unsigned)kCellPal);
            // (an entry counted but not yet written is skipped: at worst the record is added twice)
            bool hold = false;
            if ((unsigned)lane < n) {
              const bool rdy = *(volatile unsigned *)&s_rdy[lane] != 0u;
              __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
              const volatile float *pe = reinterpret_cast<const volatile float *>(&s_pal[lane]);
              hold = rdy && same(make_float4(pe[0], pe[1], pe[2], pe[3]));
            }
            const unsigned long long found = __ballot(hold);
            unsigned e_idx;
            if (found) {
              e_idx = (unsigned)(__ffsll((long long)found) - 1);
            } else {
              unsigned slot = 0;
              if (lane == 0) {
                slot = atomicAdd(&s_npal, 1u);
                if (slot < (unsigned)kCellPal) {
                  s_pal[slot] = make_float4(rx, ry, rz, rw);
                  gpal[slot] = make_float4(rx, ry, rz, rw);
                  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
                  *(volatile unsigned *)&s_rdy[slot] = 1u;
                }
              }
              e_idx = min((unsigned)__builtin_amdgcn_readfirstlane((int)slot), (unsigned)kCellPal);
            }
#pragma unroll
            for (int k = 0; k < GR; ++k) {
              if ((mine[k] >> lane) & 1ull) idx[k] = e_idx;
              rem[k] &= ~mine[k];
            }
          }
#pragma unroll
          for (int k = 0; k < GR; ++k)
            mf[base + (GR * h + k) * rstep] = (unsigned short)((hm >> (GR * h + k) & 1u) ? idx[k] : q[GR * h + k]);
        }
      }
    }
  }
  if constexpr (TAB) {
    // REPEAT wrap (k_dist_cmin): samples at u = 1 / v = 1 read column 0 / row 0
    if (x0 + cw == s.W)
      for (int e = (int)threadIdx.x; e < cw; e += NTH) m = min(m, (unsigned)dist[(size_t)(y0 + e) * s.pitch]);
    if (y0 + cw == s.H)
      for (int e = (int)threadIdx.x; e < cw; e += NTH) m = min(m, (unsigned)dist[x0 + e]);
    if (x0 + cw == s.W && y0 + cw == s.H && threadIdx.x == 0) m = min(m, (unsigned)dist[0]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = min(m, (unsigned)__shfl_xor((int)m, o, 64));
    __shared__ unsigned s_m[NW];
    if (lane == 0) s_m[w] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int i = 1; i < NW; ++i) m = min(m, s_m[i]);
      const float d = decode_dist(m);
      if (hitc) hitc[by * kCminDim + bx] = d < 0.001f ? 1 : 0;
      cmin[by * kCminDim + bx] = d >= 0.001f ? (CminT)fminf(floorf(d * kCminScale), 255.0f) : (CminT)0;
    }
  } else {
    (void)m;
    __syncthreads();  // (the next cell of this workgroup reuses the palette's LDS)
  }
}

// (cell rows from cr0: a row-strip shard's own cells, strip tables)
template <bool PAL, int NTH = 256>
__global__ __launch_bounds__(NTH) void k_shade_cmin(const unsigned short *__restrict__ dist,
                                                    const float4 *__restrict__ color, const float4 *__restrict__ emis,
                                                    float4 *__restrict__ shade, ScreenDims s, float reflectivity,
                                                    int csh, CminT *__restrict__ cmin, unsigned char *__restrict__ hitc,
                                                    unsigned short *__restrict__ mf, float4 *__restrict__ cpal, int cr0) {
  shade_cell<PAL, NTH, true>(dist, color, emis, shade, s, reflectivity, csh, cmin, hitc, mf, cpal, (int)blockIdx.x,
                             (int)blockIdx.y + cr0);
}

// The same pass split in two (tuning shade_split; round 5).  Most cells hold no hittable texel (demo frame:
// 262 of 4096), yet every cell ran in the 114-VGPR kernel above (2 workgroups per CU, 8 rounds).
// k_shade_scan: one light workgroup per cell -- 16-byte distance loads, the bound table and hit flag, the march
// field copied where the cell holds no hit, and the cells that do appended to `list` (count in list[p], cells
// from list[2]; p = the frame's parity).  k_shade_cells: the records, palette and march field of the listed cells,
// shade_cell's code; it clears the other parity's count for the next frame.  Same outputs bit for bit.
template <int NR>  // runs per lane: 2 (64-texel cells)
__global__ __launch_bounds__(256) void k_shade_scan(const unsigned short *__restrict__ dist, ScreenDims s, int csh,
                                                    CminT *__restrict__ cmin, unsigned char *__restrict__ hitc,
                                                    unsigned short *__restrict__ mf, unsigned *__restrict__ list,
                                                    int p, int cr0) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int cw = 1 << csh, sh = csh - 3;  // 2^sh runs of 8 texels per cell row
  const int cby = (int)blockIdx.y + cr0;  // (cell rows from cr0: a row-strip shard's own cells, strip tables)
  const int x0 = (int)blockIdx.x << csh, y0 = cby << csh;
  constexpr int nr = NR;
  uint4 v[NR];
  size_t base[NR];
  unsigned m = 0xFFFFu;
  bool hit = false;
#pragma unroll
  for (int g = 0; g < NR; ++g) {
    {
      const int e = g * 256 + (int)threadIdx.x;
      base[g] = (size_t)(y0 + (e >> sh)) * s.pitch + x0 + ((e & ((1 << sh) - 1)) << 3);
      v[g] = *reinterpret_cast<const uint4 *>(dist + base[g]);
    }
  }
#pragma unroll
  for (int g = 0; g < NR; ++g) {
    {
      const unsigned wd[4] = {v[g].x, v[g].y, v[g].z, v[g].w};
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const unsigned q = (wd[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
        m = min(m, q);
        hit |= decode_dist(q) < 0.001f;
      }
    }
  }
  const bool cell_hit = __syncthreads_or(hit);
  if (!cell_hit) {
#pragma unroll
    for (int g = 0; g < NR; ++g) *reinterpret_cast<uint4 *>(mf + base[g]) = v[g];
  } else if (threadIdx.x == 0) {
    list[2 + atomicAdd(&list[p], 1u)] = cby * kCminDim + blockIdx.x;
  }
  // REPEAT wrap (k_dist_cmin): samples at u = 1 / v = 1 read column 0 / row 0
  if (x0 + cw == s.W)
    for (int e = (int)threadIdx.x; e < cw; e += 256) m = min(m, (unsigned)dist[(size_t)(y0 + e) * s.pitch]);
  if (y0 + cw == s.H)
    for (int e = (int)threadIdx.x; e < cw; e += 256) m = min(m, (unsigned)dist[x0 + e]);
  if (x0 + cw == s.W && y0 + cw == s.H && threadIdx.x == 0) m = min(m, (unsigned)dist[0]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = min(m, (unsigned)__shfl_xor((int)m, o, 64));
  __shared__ unsigned s_m[4];
  if (lane == 0) s_m[w] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = min(min(s_m[0], s_m[1]), min(s_m[2], s_m[3]));
    const float d = decode_dist(m);
    if (hitc) hitc[cby * kCminDim + blockIdx.x] = d < 0.001f ? 1 : 0;
    cmin[cby * kCminDim + blockIdx.x] = d >= 0.001f ? (CminT)fminf(floorf(d * kCminScale), 255.0f) : (CminT)0;
  }
}

#ifndef RC2DGI_SHADE_CELLS_NTH
#define RC2DGI_SHADE_CELLS_NTH 512  // (A/B builds: 1024 lanes, record groups of 4 rows)
#endif
constexpr int kShadeCellsWG = 512;
// k_dir_clear's LDS (dir_clear_block below)
struct DirClearLds {
  unsigned short part[kCminDim * 4];  // 16-cell pieces of the rows
  unsigned long long rows[kCminDim];
  int4 box[kCminDim];                 // per step: cell offsets x0, x1, y0, y1 relative to the start cell
};
__device__ __forceinline__ void dir_clear_block(const unsigned char *__restrict__, const int4 *__restrict__,
                                                unsigned char *__restrict__, int, int, DirClearLds &);
// DC (side_overlap 2): k_dir_clear's workgroups appended to the grid, two per workgroup (lanes 0-255 / 256-511),
// beside the hit cells on the CUs they leave idle -- no second stream, no events
template <bool DC>
__global__ __launch_bounds__(RC2DGI_SHADE_CELLS_NTH) void k_shade_cells(const unsigned short *__restrict__ dist,
                                                     const float4 *__restrict__ color, const float4 *__restrict__ emis,
                                                     float4 *__restrict__ shade, ScreenDims s, float reflectivity,
                                                     int csh, unsigned short *__restrict__ mf, float4 *__restrict__ cpal,
                                                     unsigned *__restrict__ list, int p, const unsigned char *__restrict__ hitc,
                                                     const int4 *__restrict__ boxes, unsigned char *__restrict__ dclr) {
  if constexpr (DC) {
    static_assert(RC2DGI_SHADE_CELLS_NTH == 512, "two k_dir_clear workgroups per workgroup");
    // (after the records' workgroups: with them first, L5 + side kernels took 2.5 us more, ab/ab_dclr_merged.txt)
    if (blockIdx.x >= (unsigned)kShadeCellsWG) {
      extern __shared__ __attribute__((aligned(16))) unsigned char dc_lds[];  // (DirClearLds holds int4 / u64)
      DirClearLds *const L = reinterpret_cast<DirClearLds *>(dc_lds);
      const int h = (int)threadIdx.x >> 8;
      dir_clear_block(hitc, boxes, dclr, 2 * ((int)blockIdx.x - kShadeCellsWG) + h, (int)threadIdx.x & 255, L[h]);
      return;
    }
  }
  const unsigned n = *(volatile unsigned *)&list[p];
  if (blockIdx.x == 0 && threadIdx.x == 0) list[p ^ 1] = 0u;  // (the next frame's count)
  for (unsigned i = blockIdx.x; i < n; i += kShadeCellsWG) {
    const unsigned cell = list[2 + i];
    shade_cell<true, RC2DGI_SHADE_CELLS_NTH, false>(dist, color, emis, shade, s, reflectivity, csh, nullptr, nullptr, mf, cpal,
                                 (int)(cell % kCminDim), (int)(cell / kCminDim));
  }
}

// ---------------------------------------------------------------- directional clear distances (march proofs)
// dclr[j][c] = s: from any point of cell c (kCminDim x kCminDim cells of 2^csh texels, k_dist_cmin's grid) and
// for every direction of angular bin j (angles [2 pi j / kDirBins, 2 pi (j + 1) / kDirBins)), the ray stays
// clear of the cells holding a texel that passes the hit test (hitc, REPEAT wrap included) for s cells of
// distance (s * 2^csh texels); 255: the whole grid.  Step s covers radii [s C, (s + 1) C) texels: the points
// u + d r (u in the cell, d in the bin, r in the step) lie in the box of the four chord corners grown by
// the sagitta r (1 - cos(dtheta / 2)) and one texel (the fp32 rounding of positions and directions), and
// the step's cells are the cells that box touches.  Cells off the grid are off screen: never sampled.
// A wave per (bin, row of cells), one lane per step: the step's row OR and box, then per cell of the row one
// ballot of the steps that meet a hit cell: kDirBins x 16 workgroups of 4 rows; the flag grid as one 64-bit
// word per row in LDS.
// Transpose of the wave's 64 x 64 bit matrix (row = lane, column = bit): returns to lane c the bits
// [r] = bit c of lane r's x.  Round k swaps the off-diagonal j x j blocks (j = 32 ... 1) with lane ^ j.
__device__ __forceinline__ unsigned long long bit_transpose64(unsigned long long x, int lane) {
  constexpr unsigned long long kLow[6] = {0x00000000FFFFFFFFull, 0x0000FFFF0000FFFFull, 0x00FF00FF00FF00FFull,
                                          0x0F0F0F0F0F0F0F0Full, 0x3333333333333333ull, 0x5555555555555555ull};
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const int j = 32 >> r;
    const unsigned long long mlo = kLow[r];
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)x, j, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(x >> 32), j, 64);
    const unsigned long long p = (unsigned long long)hi << 32 | lo;
    x = (lane & j) ? (x & ~mlo) | ((p & ~mlo) >> j) : (x & mlo) | ((p & mlo) << j);
  }
  return x;
}

// One workgroup's work (bin vb / 16, rows 4 (vb % 16) .. + 3) by 256 threads t; the LDS arrays passed in (the
// merged launch below runs two per 512-lane workgroup, barriers shared)
__device__ __forceinline__ void dir_clear_block(const unsigned char *__restrict__ hitc, const int4 *__restrict__ boxes,
                                                unsigned char *__restrict__ dclr, int vb, int t, DirClearLds &L) {
  constexpr int D = kCminDim, NS = kCminDim;
  static_assert(D == 64, "one 64-bit word per row, a wave per row");
  unsigned short *const part = L.part;
  unsigned long long *const rows = L.rows;
  int4 *const box = L.box;
  const int j = vb >> 4, c = (vb & 15) * 256 + t;
  {  // thread t packs cells 16 t .. 16 t + 15 (row t / 4, piece t % 4)
    const uint4 v = reinterpret_cast<const uint4 *>(hitc)[t];
    unsigned m = 0;
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 16; ++q) m |= ((w[q >> 2] >> (8 * (q & 3))) & 0xFFu) ? 1u << q : 0u;
    part[t] = (unsigned short)m;
  }
  if (t < NS) box[t] = boxes[j * NS + t];  // host-built (dir_clear_boxes)
  __syncthreads();
  if (t < D)
    rows[t] = (unsigned long long)part[4 * t] | (unsigned long long)part[4 * t + 1] << 16 |
              (unsigned long long)part[4 * t + 2] << 32 | (unsigned long long)part[4 * t + 3] << 48;
  __syncthreads();
  const int cy = __builtin_amdgcn_readfirstlane(c / D);
  const int lane = t & 63;
  // lane s holds step s of this wave's row: the OR of the grid rows its box covers (the rows do not
  // depend on the cell's column) and the box's column offsets
  const int4 bl = box[lane];
  const int ly0 = max(0, cy + bl.z), ly1 = min(D - 1, cy + bl.w);
  unsigned long long orow = 0;
  for (int y = ly0; y <= ly1; ++y) orow |= rows[y];
  // the boxes move outwards along the bin's directions: from the first step whose rows lie off the grid on,
  // nothing is reached
  const unsigned long long voff = __ballot(ly0 > ly1);
  const int nsteps = voff ? (int)__builtin_ctzll(voff) : NS;
  // Lane s, for every cell cx of the row at once (bit cx): hm -- the box [cx + bl.x, cx + bl.y] meets a hit
  // column of orow (orow dilated by the box's column offsets), om -- the box lies wholly off the grid
  // sideways.  Then per cell (wave-uniform loop), every step at once: the first step whose box meets a hit
  // cell, unless the box has left the grid sideways (so have the later steps) or vertically first.
  unsigned long long hm = 0, om = 0;
  for (int d = bl.x; d <= bl.y; ++d)
    hm |= d >= 0 ? (d < 64 ? orow >> d : 0ull) : (d > -64 ? orow << -d : 0ull);
  // off: cx + bl.y < 0 or cx + bl.x > 63
  const int lo = -bl.y, hi = D - 1 - bl.x;  // on-grid cells: lo <= cx <= hi
  if (lo > D - 1 || hi < 0 || lo > hi) {
    om = ~0ull;
  } else {
    const int a = max(0, lo), b = min(D - 1, hi);
    const unsigned long long on = (b - a == 63 ? ~0ull : ((1ull << (b - a + 1)) - 1ull)) << a;
    om = ~on;
  }
  hm &= ~om;
  // lane cx: the steps (bits) whose box meets a hit cell / lies off the grid for cell cx -- the 64 x 64 bit
  // matrices transposed in six shuffle rounds (round 5; was one pair of ballots per cell, 64 rounds)
  const unsigned long long hb = bit_transpose64(hm, lane), ob = bit_transpose64(om, lane);
  const int first_hit = hb ? (int)__builtin_ctzll(hb) : NS;
  const int first_off = min(nsteps, ob ? (int)__builtin_ctzll(ob) : NS);
  const int clear = first_hit < first_off ? first_hit : 255;
  dclr[(size_t)j * D * D + c] = (unsigned char)clear;
}

__global__ __launch_bounds__(256) void k_dir_clear(const unsigned char *__restrict__ hitc,
                                                   const int4 *__restrict__ boxes,
                                                   unsigned char *__restrict__ dclr) {
  __shared__ DirClearLds L;
  dir_clear_block(hitc, boxes, dclr, (int)blockIdx.x, (int)threadIdx.x, L);
}

void dir_clear_boxes(int csh, int4 *boxes) {
  const double C = (double)(1 << csh), PI2 = 6.283185307179586;
  for (int j = 0; j < kDirBins; ++j) {
    const double ta = PI2 * j / kDirBins, tb = PI2 * (j + 1) / kDirBins;
    const double sag = 1.0 - std::cos(0.5 * (tb - ta));
    const double ds[2][2] = {{std::cos(ta), std::sin(ta)}, {std::cos(tb), std::sin(tb)}};
    for (int s = 0; s < kCminDim; ++s) {
      const double r0 = s * C, r1 = (s + 1) * C;
      double lox = 1e30, hix = -1e30, loy = 1e30, hiy = -1e30;
      for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) {
          const double r = b ? r1 : r0;
          lox = std::fmin(lox, ds[a][0] * r);
          hix = std::fmax(hix, ds[a][0] * r);
          loy = std::fmin(loy, ds[a][1] * r);
          hiy = std::fmax(hiy, ds[a][1] * r);
        }
      const double m = r1 * sag + 1.0;
      boxes[j * kCminDim + s] = make_int4((int)std::floor((lox - m) / C), (int)std::floor((hix + m + C - 1e-6) / C),
                                          (int)std::floor((loy - m) / C), (int)std::floor((hiy + m + C - 1e-6) / C));
    }
  }
}

hipError_t launch_dir_clear(const unsigned char *hitc, const int4 *boxes, unsigned char *dclr, hipStream_t st) {
  hipLaunchKernelGGL(k_dir_clear, dim3(kDirBins * 16), dim3(256), 0, st, hitc, boxes, dclr);
  return hipGetLastError();
}

// the split pass: 64-texel cells (4096^2; at 8192^2 the scan would hold 8 runs per lane, 130 VGPRs)
bool shade_split_ok(int W, int H) { return dist_cmin_shift(W, H) == 6; }

bool shade_cmin_fused_ok(int W, int H, int pitch) {
  const int csh = dist_cmin_shift(W, H);
  return csh >= 6 && W == H && W == (kCminDim << csh) && pitch % 64 == 0;
}

// (after k_dir_clear: the split pass launches it too)
hipError_t launch_shade_cmin(const ShadeCminArgs &a, ScreenDims s, hipStream_t st) {
  if (!shade_cmin_fused_ok(s.W, s.H, s.pitch)) return hipErrorInvalidValue;
  if (a.cr0 < 0 || a.ncr < 1 || a.cr0 + a.ncr > kCminDim) return hipErrorInvalidValue;
  if ((a.cr0 != 0 || a.ncr != kCminDim || !a.shade) && !(a.mf && a.cpal)) return hipErrorInvalidValue;  // (partial: palettes)
  const int csh = dist_cmin_shift(s.W, s.H);
  if (a.mf && a.cpal && a.list) {
    // every argument check before the first launch: an error leaves nothing enqueued
    if (!shade_split_ok(s.W, s.H)) return hipErrorInvalidValue;
    if (a.dclr && (!a.hitc || !a.boxes)) return hipErrorInvalidValue;
    const int p = a.parity & 1;
    hipLaunchKernelGGL(k_shade_scan<2>, dim3(kCminDim, a.ncr), dim3(256), 0, st, a.dist, s, csh, a.cmin, a.hitc, a.mf,
                       a.list, p, a.cr0);
    if (a.after_scan) {  // (the bound table and hit flags are final here)
      const hipError_t e = hipEventRecord(a.after_scan, st);
      if (e != hipSuccess) return e;
    }
    constexpr bool kMerge = RC2DGI_SHADE_CELLS_NTH == 512;  // (two k_dir_clear workgroups per workgroup)
    if constexpr (kMerge) {
      if (a.dclr) {
        hipLaunchKernelGGL(k_shade_cells<kMerge>, dim3(kShadeCellsWG + kDirBins * 16 / 2), dim3(RC2DGI_SHADE_CELLS_NTH),
                           2 * sizeof(DirClearLds), st, a.dist, a.color, a.emis, a.shade, s, a.reflectivity, csh, a.mf,
                           a.cpal, a.list, p, a.hitc, a.boxes, a.dclr);
        return hipGetLastError();
      }
    }
    hipLaunchKernelGGL(k_shade_cells<false>, dim3(kShadeCellsWG), dim3(RC2DGI_SHADE_CELLS_NTH), 0, st, a.dist, a.color,
                       a.emis, a.shade, s, a.reflectivity, csh, a.mf, a.cpal, a.list, p, nullptr, nullptr, nullptr);
    if (a.dclr) hipLaunchKernelGGL(k_dir_clear, dim3(kDirBins * 16), dim3(256), 0, st, a.hitc, a.boxes, a.dclr);
    return hipGetLastError();
  }
  if (a.mf && a.cpal)
    hipLaunchKernelGGL((k_shade_cmin<true, 512>), dim3(kCminDim, a.ncr), dim3(512), 0, st, a.dist, a.color, a.emis,
                       a.shade, s, a.reflectivity, csh, a.cmin, a.hitc, a.mf, a.cpal, a.cr0);
  else
    hipLaunchKernelGGL(k_shade_cmin<false>, dim3(kCminDim, kCminDim), dim3(256), 0, st, a.dist, a.color, a.emis,
                       a.shade, s, a.reflectivity, csh, a.cmin, a.hitc, a.mf, a.cpal, 0);
  return hipGetLastError();
}

// ---------------------------------------------------------------- tiled distance field
// dist (pitch-linear) -> 8x8 tiles of 64 texels (one 128-byte line), tiles row-major, tpr tiles per
// row; a thread moves one 16-byte row segment (8 texels) of one tile
__global__ __launch_bounds__(256) void k_dist_tile(const unsigned short *__restrict__ dist, int pitch,
                                                   unsigned short *__restrict__ tiled, int tpr, int W, int H) {
  const int seg = blockIdx.x * 64 + (threadIdx.x & 63);  // 8-texel segment = tile column
  const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (seg >= tpr || j >= H) return;
  const uint4 v = *reinterpret_cast<const uint4 *>(dist + (size_t)j * pitch + seg * 8);
  *reinterpret_cast<uint4 *>(tiled + (((size_t)(j >> 3) * tpr + seg) << 6) + ((j & 7) << 3)) = v;
  (void)W;
}

hipError_t launch_dist_tile(const unsigned short *dist, int pitch, unsigned short *tiled, int W, int H,
                            hipStream_t st) {
  const int tpr = (W + 7) / 8;
  hipLaunchKernelGGL(k_dist_tile, dim3(ceil_div(tpr, 64), ceil_div(H, 4)), dim3(256), 0, st, dist, pitch, tiled, tpr,
                     W, H);
  return hipGetLastError();
}

// dist (pitch-linear) -> packed 14-texel packets (kPackTexels); one thread per packet, rows of ppr
// packets.  Texel t of packet k is column 14k + t; columns past W repeat the packet's minimum.
__global__ __launch_bounds__(256) void k_dist_pack(const unsigned short *__restrict__ dist, int pitch,
                                                   uint4 *__restrict__ packed, int ppr, int W, int H) {
  const int k = blockIdx.x * 256 + (int)threadIdx.x, j = blockIdx.y;
  if (k >= ppr || j >= H) return;
  const int x0 = k * kPackTexels;
  // 14 texels = 7 aligned dwords (the row starts 128-byte aligned, a packet at 28k bytes)
  const unsigned *src = reinterpret_cast<const unsigned *>(dist + (size_t)j * pitch + x0);
  unsigned q[kPackTexels];
#pragma unroll
  for (int w = 0; w < kPackTexels / 2; ++w) {
    const unsigned v = x0 + 2 * w < W ? src[w] : 0xFFFFFFFFu;
    q[2 * w] = v & 0xFFFFu;
    q[2 * w + 1] = v >> 16;
  }
  unsigned lo = q[0];
#pragma unroll
  for (int t = 1; t < kPackTexels; ++t)
    if (x0 + t < W) lo = min(lo, q[t]);
  unsigned b[16];
  b[0] = lo & 0xFFu;
  b[1] = lo >> 8;
#pragma unroll
  for (int t = 0; t < kPackTexels; ++t) b[2 + t] = x0 + t < W ? min(q[t] - lo, 255u) : 0u;
  uint4 o;
  o.x = b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24;
  o.y = b[4] | b[5] << 8 | b[6] << 16 | b[7] << 24;
  o.z = b[8] | b[9] << 8 | b[10] << 16 | b[11] << 24;
  o.w = b[12] | b[13] << 8 | b[14] << 16 | b[15] << 24;
  packed[(size_t)j * ppr + k] = o;
}

size_t dist_packed_bytes(int W, int H) { return (size_t)pack_per_row(W) * H * sizeof(uint4); }

hipError_t launch_dist_pack(const unsigned short *dist, int pitch, uint4 *packed, int W, int H, hipStream_t st) {
  const int ppr = pack_per_row(W);
  hipLaunchKernelGGL(k_dist_pack, dim3(ceil_div(ppr, 256), H), dim3(256), 0, st, dist, pitch, packed, ppr, W, H);
  return hipGetLastError();
}

// dist (pitch-linear) -> nibble-predicted packets (kNibTexels, packet_q<3>): one thread per packet.
// The slope is the best (fewest escapes) of five around the packet's end-to-end slope; the base
// centres the residuals of that slope, clamped to 16 bits.  Texels past the row's end are escapes.
__global__ __launch_bounds__(256) void k_dist_nib(const unsigned short *__restrict__ dist, int pitch,
                                                  uint4 *__restrict__ packed, int ppr, int W, int H) {
  const int k = blockIdx.x * 256 + (int)threadIdx.x, j = blockIdx.y;
  if (k >= ppr || j >= H) return;
  const int x0 = k * kNibTexels;
  const int cnt = min(kNibTexels, W - x0);
  // 26 texels = 13 dwords, 4-byte aligned (a packet starts at byte 52 k of a 128-byte aligned row)
  const unsigned *src = reinterpret_cast<const unsigned *>(dist + (size_t)j * pitch + x0);
  int q[kNibTexels];
#pragma unroll
  for (int w = 0; w < kNibTexels / 2; ++w) {
    const unsigned v = x0 + 2 * w < W ? src[w] : 0u;
    q[2 * w] = (int)(v & 0xFFFFu);
    q[2 * w + 1] = (int)(v >> 16);
  }
  const int qa = q[0], qb = q[cnt - 1 < 0 ? 0 : cnt - 1];
  const int s0 = cnt > 1 ? (int)floorf((float)(qb - qa) / (float)(cnt - 1) + 0.5f) : 0;
  int best_s = 0, best_base = 0, best_esc = kNibTexels + 1;
  for (int ds = -2; ds <= 2; ++ds) {
    const int sl = min(127, max(-128, s0 + ds));
    int lo = 1 << 30, hi = -(1 << 30);
#pragma unroll
    for (int t = 0; t < kNibTexels; ++t)
      if (t < cnt) {
        const int r = q[t] - sl * t;
        lo = min(lo, r);
        hi = max(hi, r);
      }
    const int base = min(65535, max(0, (lo + hi) >> 1));
    int esc = 0;
#pragma unroll
    for (int t = 0; t < kNibTexels; ++t) {
      const int r = q[t] - sl * t - base;
      esc += (t < cnt && (r < -7 || r > 7)) ? 1 : 0;
    }
    if (esc < best_esc) {
      best_esc = esc;
      best_s = sl;
      best_base = base;
    }
  }
  unsigned w[4] = {(unsigned)best_base | ((unsigned)(best_s & 0xFF) << 16), 0u, 0u, 0u};
#pragma unroll
  for (int t = 0; t < kNibTexels; ++t) {
    const int r = q[t] - best_s * t - best_base;
    const unsigned n = (t < cnt && r >= -7 && r <= 7) ? (unsigned)(r + 7) : 15u;
    const int b = 24 + 4 * t;
    w[b >> 5] |= n << (b & 31);
  }
  packed[(size_t)j * ppr + k] = make_uint4(w[0], w[1], w[2], w[3]);
}

size_t dist_nib_bytes(int W, int H) { return (size_t)nib_per_row(W) * H * sizeof(uint4); }

hipError_t launch_dist_nib(const unsigned short *dist, int pitch, uint4 *packed, int W, int H, hipStream_t st) {
  const int ppr = nib_per_row(W);
  hipLaunchKernelGGL(k_dist_nib, dim3(ceil_div(ppr, 256), H), dim3(256), 0, st, dist, pitch, packed, ppr, W, H);
  return hipGetLastError();
}

}  // namespace rc2dgi
