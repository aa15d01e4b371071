// rc2dgi_buffers.cpp -- what a context holds: derived sizes, the render textures and side tables (allocation,
// reallocation for shards and knobs), the transcendental tables and texture readback.  Mirrors RC2DGI.cs:57-109.
#include "rc2dgi_ctx.h"

namespace rc2dgi {

constexpr float kTau = 6.28318530718f;  // RadianceCascades.fs:27

// RC2DGI.cs:70-77 and :289-292 (double arithmetic as in C#)
void derive_sizes(int W, int H, int N, float rs, int &CW, int &CH, int &S) {
  const double powVal = std::pow(2.0, N);
  CW = (int)std::ceil((double)((float)W * rs) / powVal) * (int)powVal;
  CH = (int)std::ceil((double)((float)H * rs) / powVal) * (int)powVal;
  const int mx = W > H ? W : H;
  S = (int)std::ceil(std::log((double)mx) / std::log(2.0));
  if (S < 1) S = 1;
}

// Flags of the timing events (per pass, per cascade level).  They only timestamp the stream, so they skip
// the system-scope fence (L2 writeback / invalidate) a default event performs: with it every event left
// the next kernel a colder cache (RC pass 1.473 -> 1.461 ms, profiles/r03/ab/events.txt).  Every event
// still leaves a ~5 us idle gap before the next kernel (rocprofv3 trace), hence timing mode 2 (passes
// only, rc2dgi_set_timing).  RC2DGI_TIMING_EVENT_FLAGS (an int) overrides the flags for experiments.
unsigned timing_event_flags() {
  static const unsigned f = [] {
    const char *v = getenv("RC2DGI_TIMING_EVENT_FLAGS");
    return v ? (unsigned)strtoul(v, nullptr, 0) : (unsigned)hipEventDisableSystemFence;
  }();
  return f;
}


size_t dir_table_len(int N) {  // sum over levels of 4^(L+1)
  size_t n = 0;
  for (int L = 0; L < N; ++L) n += (size_t)4 << (2 * L);
  return n;
}
size_t dir_table_offset(int L) {
  size_t n = 0;
  for (int q = 0; q < L; ++q) n += (size_t)4 << (2 * q);
  return n;
}

void free_level_bufs(rc2dgi_ctx *c) {
  for (float4 *p : c->level_bufs)
    if (p) (void)hipFree(p);
  c->level_bufs.clear();
}

void free_chain(rc2dgi_ctx *c) {
  for (float4 *p : c->chain_bufs)
    if (p) (void)hipFree(p);
  c->chain_bufs.clear();
  rc_chain_destroy(c->chain);
  c->chain = nullptr;
}

// the cascade chain runs this frame: asked for, f32 cascades, one process (whole levels), >= 3 levels
bool chain_active(const rc2dgi_ctx *c) {
  return c->rc_chain && c->storage == RC2DGI_STORAGE_F32 && c->world == 1 && c->N >= 3 && rc_chain_ok(c->N);
}

// A chained frame whose workgroup stopped waiting for its upper tiles merged texels that were not written: no
// silent wrong frame.  The kernel sets a host-mapped word; the next rc2dgi_sync / rc2dgi_download /
// rc2dgi_download_level / rc2dgi_compose / rc2dgi_reduce / rc2dgi_compose_tone / rc2dgi_histogram / rc2dgi_read / rc2dgi_do /
// rc2dgi_do_phase returns RC2DGI_E_DEVICE and the context
// falls back to one launch per level from then on.
int check_chain(rc2dgi_ctx *c) {
  if (!c->chain || !rc_chain_take_error(c->chain)) return RC2DGI_OK;
  c->rc_chain = 0;
  return fail(c, RC2DGI_E_DEVICE,
              "cascade chain: a workgroup stopped waiting for its upper tiles, so a frame's cascades are wrong "
              "(rc_chain_timeouts counts them); the chain is off for this context from now on");
}

void free_buffers(rc2dgi_ctx *c) {
  free_level_bufs(c);
  free_chain(c);
  c->rc_maps.clear();
  c->paint_buf.release();
  c->paint_dev.release();
  if (c->tilemap_cnt) (void)hipFree(c->tilemap_cnt);
  c->tilemap_cnt = nullptr;
  if (c->present_buf) (void)hipFree(c->present_buf);
  c->present_buf = nullptr;
  c->present_cap = 0;
  if (c->query_in) (void)hipFree(c->query_in);
  if (c->query_out) (void)hipFree(c->query_out);
  c->query_in = c->query_out = nullptr;
  c->query_in_cap = c->query_out_cap = 0;
  if (c->reduce_buf) (void)hipFree(c->reduce_buf);
  c->reduce_buf = nullptr;
  if (c->hist_buf) (void)hipFree(c->hist_buf);
  c->hist_buf = nullptr;
  if (c->read_buf) (void)hipFree(c->read_buf);
  c->read_buf = nullptr;
  void *bufs[] = {c->color_in, c->emissive, c->temp, c->color_out, c->jump1, c->jump2, c->dist, c->occ,
                  c->gi1,      c->gi2,      c->blur, c->dirs,      c->sky, c->gi_spare, c->dist_t, c->dist_p, c->dist_n, c->shade,
                  c->cmin,     c->dexit, c->hitc, c->dclr, c->dboxes, c->mfield, c->cell_pal, c->shade_list, c->jtail,
                  c->tc, c->bconst, c->odd_flag};
  for (void *p : bufs)
    if (p) (void)hipFree(p);
  for (unsigned *&b : c->jblk) {
    if (b) (void)hipFree(b);
    b = nullptr;
  }
  c->color_in = c->emissive = c->temp = c->color_out = nullptr;
  c->jump1 = c->jump2 = nullptr;
  c->occ = nullptr;
  c->dist = c->dist_t = nullptr;
  c->dist_p = nullptr;
  c->dist_n = nullptr;
  c->shade = nullptr;
  c->cmin = nullptr;
  c->hitc = c->dclr = nullptr;
  c->mfield = nullptr;
  c->cell_pal = nullptr;
  c->shade_list = nullptr;
  c->jtail = nullptr;
  c->tc = nullptr;
  c->bconst = nullptr;
  c->odd_flag = nullptr;
  c->built_hitc = c->built_cmin = c->built_dclr = c->built_pal = false;
  c->dboxes = nullptr;
  c->gi1 = c->gi2 = c->blur = c->gi_spare = nullptr;
  c->dirs = nullptr;
  c->dexit = nullptr;
  c->sky = nullptr;
}

// jumpRT1 / jumpRT2 for the sharding: full-size textures, or (world > 1, >= 2 JFA steps) the
// strip windows of the JumpFlood exchange (rows [y0 - m, y1 + m) of the strip) and its two
// block buffers (plan_jfa_exchange)
int jfa_buffers(rc2dgi_ctx *c) {
  const bool strip = c->world > 1 && c->S >= 2;
  for (unsigned **b : {&c->jump1, &c->jump2, &c->jblk[0], &c->jblk[1]}) {
    if (*b) (void)hipFree(*b);
    *b = nullptr;
  }
  c->strip = strip;
  const size_t sp = (size_t)c->sd.pitch;
  if (!strip) {
    c->jwin_rows = (size_t)c->H;
    HIPCHK(c, alloc(&c->jump1, sp * c->H * sizeof(unsigned)));
    HIPCHK(c, alloc(&c->jump2, sp * c->H * sizeof(unsigned)));
    return RC2DGI_OK;
  }
  c->jx = plan_jfa_exchange(c->W, c->H, c->S, c->world);
  c->jwin_rows = (size_t)c->jx.hmax + 2 * (size_t)c->jx.m;
  HIPCHK(c, alloc(&c->jump1, sp * c->jwin_rows * sizeof(unsigned)));
  HIPCHK(c, alloc(&c->jump2, sp * c->jwin_rows * sizeof(unsigned)));
  bool blocks = false;
  for (size_t t = 1; t < c->jx.steps.size(); ++t) blocks |= !c->jx.steps[t].halo;
  if (blocks) {
    const size_t br = (size_t)c->jx.hmax + 2 * (size_t)c->jx.mg_max;
    HIPCHK(c, alloc(&c->jblk[0], sp * br * sizeof(unsigned)));
    HIPCHK(c, alloc(&c->jblk[1], sp * br * sizeof(unsigned)));
  }
  return RC2DGI_OK;
}

// the last jfa_tail JumpFlood steps run as one kernel (k_jfa_tail): whole-frame contexts on the screens it takes
bool jfa_tail_apply(const rc2dgi_ctx *c) {
  return c->jfa_tail > 0 && !c->strip && c->world == 1 && jfa_tail_ok(c->sd, c->S, c->jfa_tail);
}

// exit proofs on for this frame: auto (1) turns them on for large screens only -- at 1200x900 the bound table's
// staging and barrier cost more than the skipped samples save (RC 0.338 vs 0.376 ms, measured)
bool proofs_on(const rc2dgi_ctx *c) { return c->rc_skip > 1 || (c->rc_skip == 1 && std::max(c->W, c->H) >= 2048); }

// Strip tables (row-strip shards): the side pass of a shard covers only the bound-table cells
// of its own rows -- their records' palettes, bound table and hit flags, and its rows of the march field -- and the
// shards exchange those rows (the march field in place of distRT: same 2 bytes a texel; 64 B of bound table, 64 B of
// hit flags and 16 KB of palettes a cell row).  Every level then marches on the march field and takes a hit's record
// from its cell's palette, or (palette full) derives it from colorRT / emissiveRT, which every shard holds whole:
// no record texture.  Applies where the side pass is the fused palette pass (square power-of-two screens >= 4096),
// every strip boundary falls on a cell row, and every level marches on the plain field.
bool strip_tables_apply(const rc2dgi_ctx *c) {
  if (c->world < 2 || !c->strip_tables || !c->rc_pal || !c->shade_fused || !proofs_on(c)) return false;
  if (c->storage != RC2DGI_STORAGE_F32) return false;  // (the derived-record marches are built for f32 cascades)
  if (!shade_cmin_fused_ok(c->W, c->H, c->sd.pitch) || (size_t)c->sd.pitch * c->H > ((size_t)1 << 26)) return false;
  for (int v : c->rc_variant)
    if (rc_variant_tiled(v) || rc_variant_packed(v) || rc_variant_nib(v)) return false;
  const int cell = 1 << dist_cmin_shift(c->W, c->H);
  for (int q = 0; q < c->world; ++q) {
    int y0, y1;
    strip_rows(c->H, q, c->world, y0, y1);
    if (y0 % cell || y1 % cell || y1 <= y0) return false;
  }
  return true;
}

// A row-strip shard whose blur runs as k_blur_rows with the merge fused (power-of-two cascades the size of the
// screen, a dyadic radius, raylib's merge shader not asked for) writes cascadeBlurRT and the copied-back GI of the
// rows it merges only: those two textures then hold the own rows as well (out_buffers).
static bool gi_window_apply(const rc2dgi_ctx *c) {
  BlurTaps bt;
  return c->world > 1 && c->blur_radius > 0.0f && c->blur_path == 0 && c->sd.W == c->CW && c->sd.H == c->CH &&
         !c->linux_merge && blur_rows_plan(c->cd, c->blur_radius, &bt) >= 0;
}


// Banded cascade textures (row-strip shards with strip tables on the fused blur + merge, f32, no top-level variant
// 25, no chain or kept levels): a level's rows the shard computes are a band of every direction block
// (RadianceCascades.fs:131-139 keeps the taps block-local), so giRT1 / giRT2 hold only those bands (k_rc_level's RD
// marches and k_blur_rows map a row to its band row).
static bool gi_band_apply(const rc2dgi_ctx *c) {
  if (!c->cascade_band || !gi_window_apply(c) || !strip_tables_apply(c) || c->keep_levels || chain_active(c))
    return false;
  if (c->storage != RC2DGI_STORAGE_F32) return false;
  for (int v : c->rc_variant)
    if (v == 25) return false;
  return true;
}

// the shortest cyclic range of rows holding every row of r: first row, rows (0 rows: r is empty)
static void circ_band(const RowSet &r, int &b0, int &bn) {
  b0 = bn = 0;
  const int m = (int)r.iv.size();
  if (m == 0) return;
  int gap = -1, k0 = 0;
  for (int k = 0; k < m; ++k) {  // the largest gap between consecutive intervals (cyclically) is left out
    const int nx = k + 1 < m ? r.iv[k + 1].first : r.iv[0].first + r.n;
    if (nx - r.iv[k].second > gap) {
      gap = nx - r.iv[k].second;
      k0 = k;
    }
  }
  b0 = r.iv[(k0 + 1) % m].first;
  bn = r.n - gap;
}

// Rows giRT1 / giRT2 are allocated with.  k_rc_level stages the upper level's footprint of a tile, up to 18 rows for
// the 32-row tiles, with loads that are unconditional and wrap once (REPEAT): on a cascade of fewer rows than the
// footprint the rows past the second wrap are read (never used: they lie under probes the tile does not have) at
// row indices below the footprint's height.  The textures keep that many rows allocated, so those loads stay inside
// them (cascades of 8 rows: 32768 x 8 at cascade_count 3 with the 32-row tiles).  Columns wrap into the pitch padding.
// (gi_spare trades places with them only after a fused blur, which takes cascades of 16 rows and more: there the
// highest row read, 15, exists.)
static size_t gi_alloc_rows(size_t rows) { return std::max(rows, (size_t)18); }

// giRT1 / giRT2 for this frame's plan: the bands of the levels each one receives (level L: giRT1 when N-1-L is even,
// phase2_levels), or whole.  Before anything of the frame is enqueued (out_buffers).
static int gi_buffers(rc2dgi_ctx *c) {
  const bool gb = gi_band_apply(c);
  std::vector<int> b0(c->N, 0), bn(c->N, 0);
  size_t rows[2] = {(size_t)c->CH, (size_t)c->CH};
  if (gb) {
    const FramePlan plan = make_plan(c);
    rows[0] = rows[1] = 1;
    for (int L = 0; L < c->N; ++L) {
      circ_band(plan.level[L], b0[L], bn[L]);
      if (bn[L] <= 0) bn[L] = 1;  // (a level the shard computes no row of: one dummy row per block)
      size_t &r = rows[(c->N - 1 - L) & 1];
      r = std::max(r, (size_t)bn[L] << L);
    }
  }
  c->gb0 = b0;
  c->gbn = bn;
  if (c->gi1 && c->gi2 && gb == c->gband && rows[0] == c->gi_rows[0] && rows[1] == c->gi_rows[1]) {
    c->gband = gb;
    return RC2DGI_OK;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (float4 **b : {&c->gi1, &c->gi2}) {
    if (*b) HIPCHK(c, hipFree(*b));
    *b = nullptr;
  }
  c->gi_rows[0] = c->gi_rows[1] = 0;
  c->gband = false;
  HIPCHK(c, alloc(&c->gi1, gi_alloc_rows(rows[0]) * c->cd.pitch * gi_bytes(c)));
  HIPCHK(c, alloc(&c->gi2, gi_alloc_rows(rows[1]) * c->cd.pitch * gi_bytes(c)));
  c->gi_rows[0] = rows[0];
  c->gi_rows[1] = rows[1];
  c->gband = gb;
  return RC2DGI_OK;
}

// tempRT and the merged colorRT of a row-strip shard hold its own rows only (the merge writes nothing else; the
// kernels take the window's first row, launch_blur_rows / launch_merge m0): 2 x 16 B a texel of the strip instead of
// the screen; on the fused blur + merge (gi_window_apply) cascadeBlurRT and the copy-back texture too.  Unsharded:
// the whole screen.  Called when the shard is set and before every frame (the blur radius and path may change
// between frames), before anything of the frame is enqueued.
int out_buffers(rc2dgi_ctx *c) {
  int y0 = 0, y1 = c->H;
  if (c->world > 1) strip_rows(c->H, c->rank, c->world, y0, y1);
  const bool gw = gi_window_apply(c);
  if (int rc = gi_buffers(c)) return rc;
  if (c->temp && c->color_out && c->blur && c->gi_spare && y0 == c->ow0 && y1 == c->ow1 && gw == c->gwin)
    return RC2DGI_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (float4 **b : {&c->temp, &c->color_out, &c->blur, &c->gi_spare}) {
    if (*b) HIPCHK(c, hipFree(*b));
    *b = nullptr;
  }
  c->ow0 = c->ow1 = 0;
  c->gwin = false;
  const size_t n = (size_t)c->sd.pitch * (size_t)(y1 - y0 + 1);  // (+ the guard row k_blur_rows writes outside rows to)
  HIPCHK(c, alloc(&c->temp, n * sizeof(float4)));
  HIPCHK(c, alloc(&c->color_out, n * sizeof(float4)));
  // (gw: the cascade is the screen, one pitch)
  const size_t nc = gw ? n : (size_t)c->cd.pitch * c->CH;
  HIPCHK(c, alloc(&c->blur, nc * sizeof(float4)));
  HIPCHK(c, alloc(&c->gi_spare, nc * gi_bytes(c)));
  HIPCHK(c, hipMemsetAsync(c->blur, 0, nc * sizeof(float4), c->stream));  // (a fresh texture, as allocate())
  c->ow0 = y0;
  c->ow1 = y1;
  c->gwin = gw;
  return RC2DGI_OK;
}

// The distRT copies the schedule's variants read ("t" / "p" / "n") and the surface-palette tables (rc_pal),
// allocated when the schedule or the knobs are set (rc2dgi_set_tuning, rc2dgi_autotune with all = true,
// allocate), never inside a frame: hipMalloc may synchronise the device, and an out-of-memory then surfaces
// at the call that asked for the buffer instead of mid-enqueue (rc2dgi_do_group enqueues several devices).
int prepare_side_buffers(rc2dgi_ctx *c, bool all) {
  if (!c->dist) return RC2DGI_OK;  // not allocated yet (allocate() calls this again)
  bool tiled = all, packed = all, nib = all;
  for (int v : c->rc_variant) {
    tiled |= rc_variant_tiled(v);
    packed |= rc_variant_packed(v);
    nib |= rc_variant_nib(v);
  }
  // (the packed marches run on power-of-two screens of up to 16384 columns and rows only)
  const bool p2s = c->sd.powW && c->sd.powH && c->cd.powW && c->cd.powH && c->W <= 16384 && c->H <= 16384;
  if (tiled && !c->dist_t)
    HIPCHK(c, alloc(&c->dist_t, (size_t)((c->W + 7) / 8) * ((c->H + 7) / 8) * 64 * sizeof(unsigned short)));
  if (packed && p2s && !c->dist_p) HIPCHK(c, alloc(&c->dist_p, dist_packed_bytes(c->W, c->H)));
  if (nib && p2s && !c->dist_n) HIPCHK(c, alloc(&c->dist_n, dist_nib_bytes(c->W, c->H)));
  if (chain_active(c) && c->chain_bufs.empty()) {  // the chain's own level textures (levels 0 / 1 use giRT1 / 2)
    c->chain_bufs.assign(c->N, nullptr);
    for (int L = 2; L < c->N; ++L) {
      hipError_t e = alloc(&c->chain_bufs[L], (size_t)c->cd.pitch * c->CH * sizeof(float4));
      if (e != hipSuccess) {
        free_chain(c);
        return hip_fail(c, e, "cascade chain textures");
      }
    }
    c->chain = rc_chain_create();
    // one flag per 16x16 tile of every level, bounded by (CW/16 + 2^L)(CH/16 + 2^L) per level
    size_t nflags = 0;
    for (int L = 0; L < c->N; ++L)
      nflags += (size_t)(c->CW / 16 + (1 << L) + 1) * (size_t)(c->CH / 16 + (1 << L) + 1);
    const hipError_t e = rc_chain_reserve(c->chain, nflags);
    if (e != hipSuccess) {
      free_chain(c);
      return hip_fail(c, e, "cascade chain flags");
    }
  }
  const bool pal = c->rc_pal && shade_cmin_fused_ok(c->W, c->H, c->sd.pitch) &&
                   (size_t)c->sd.pitch * c->H <= ((size_t)1 << 26);
  if (pal && (!c->mfield || !c->cell_pal)) {
    hipError_t e = c->mfield ? hipSuccess : alloc(&c->mfield, (size_t)c->sd.pitch * c->H * sizeof(unsigned short));
    if (e == hipSuccess && !c->cell_pal)
      e = alloc(&c->cell_pal, (size_t)kCminDim * kCminDim * kCellPalStride * sizeof(float4));
    if (e != hipSuccess) {  // both or neither
      for (void *q : {(void *)c->mfield, (void *)c->cell_pal})
        if (q) (void)hipFree(q);
      c->mfield = nullptr;
      c->cell_pal = nullptr;
      return hip_fail(c, e, "surface palette tables");
    }
  }
  if (pal && !c->shade_list) {
    const size_t n = (2 + (size_t)kCminDim * kCminDim) * sizeof(unsigned);
    hipError_t e = alloc(&c->shade_list, n);
    if (e == hipSuccess) e = hipMemset(c->shade_list, 0, n);
    if (e != hipSuccess) {
      if (c->shade_list) (void)hipFree(c->shade_list);
      c->shade_list = nullptr;
      return hip_fail(c, e, "records pass cell list");
    }
  }
  if (jfa_tail_apply(c) && !c->jtail) HIPCHK(c, alloc(&c->jtail, (size_t)c->sd.pitch * c->H * sizeof(unsigned)));
  // the record texture (16 B a texel): not held by shards that run with strip tables (their hits derive records)
  const bool st = strip_tables_apply(c);
  if (st && c->shade) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipFree(c->shade));
    c->shade = nullptr;
  } else if (!st && !c->shade) {
    HIPCHK(c, alloc(&c->shade, (size_t)c->sd.pitch * c->H * sizeof(float4)));
  }
  return RC2DGI_OK;
}

// (re)allocate every render texture for the current W, H, N (RC2DGI.cs:79-98)
int allocate(rc2dgi_ctx *c) {
  free_buffers(c);
  derive_sizes(c->W, c->H, c->N, c->render_scale, c->CW, c->CH, c->S);
  const int sp = round_up(c->W, 64), cp = round_up(c->CW, 64);
  c->sd = ScreenDims{c->W, c->H, sp, is_pow2(c->W), is_pow2(c->H), rgba8(c)};
  c->cd = CascadeDims{c->CW, c->CH, cp, is_pow2(c->CW), is_pow2(c->CH), c->storage == RC2DGI_STORAGE_F16, rgba8(c)};
  const size_t ns = (size_t)sp * c->H, nc = (size_t)cp * c->CH;
  HIPCHK(c, alloc(&c->color_in, ns * sizeof(float4)));
  HIPCHK(c, alloc(&c->emissive, ns * sizeof(float4)));
  // (tempRT / merged colorRT: one guard row after the screen, which k_blur_rows' merge writes the rows outside the
  // held window into, out_buffers)
  HIPCHK(c, alloc(&c->temp, (ns + sp) * sizeof(float4)));
  HIPCHK(c, alloc(&c->color_out, (ns + sp) * sizeof(float4)));
  c->ow0 = 0;
  c->ow1 = c->H;
  c->gwin = false;
  c->strip = false;
  c->jwin_rows = (size_t)c->H;
  HIPCHK(c, alloc(&c->jump1, ns * sizeof(unsigned)));
  HIPCHK(c, alloc(&c->jump2, ns * sizeof(unsigned)));
  c->mpitch = ((c->W + 63) / 64) * 2;
  HIPCHK(c, alloc(&c->occ, (size_t)c->mpitch * c->H * sizeof(unsigned)));
  HIPCHK(c, alloc(&c->dist, ns * sizeof(unsigned short)));
  // (the re-laid-out distRT copies of the "t" / "p" / "n" variants: prepare_side_buffers, when a schedule reads them)
  HIPCHK(c, alloc(&c->shade, ns * sizeof(float4)));
  HIPCHK(c, alloc(&c->cmin, (size_t)kCminDim * kCminDim * sizeof(CminT)));
  HIPCHK(c, alloc(&c->hitc, (size_t)kCminDim * kCminDim));
  HIPCHK(c, alloc(&c->dclr, (size_t)kDirBins * kCminDim * kCminDim));
  {
    std::vector<int4> boxes((size_t)kDirBins * kCminDim);
    dir_clear_boxes(dist_cmin_shift(c->W, c->H), boxes.data());
    HIPCHK(c, alloc(&c->dboxes, boxes.size() * sizeof(int4)));
    HIPCHK(c, hipMemcpy(c->dboxes, boxes.data(), boxes.size() * sizeof(int4), hipMemcpyHostToDevice));
  }
  const size_t gsz = gi_bytes(c);  // giRT1 / giRT2 texel size (storage)
  HIPCHK(c, alloc(&c->gi1, gi_alloc_rows((size_t)c->CH) * cp * gsz));
  HIPCHK(c, alloc(&c->gi2, gi_alloc_rows((size_t)c->CH) * cp * gsz));
  c->gi_rows[0] = c->gi_rows[1] = (size_t)c->CH;
  c->gband = false;
  HIPCHK(c, alloc(&c->blur, nc * sizeof(float4)));
  HIPCHK(c, alloc(&c->gi_spare, nc * gsz));
  {  // texcoord table of the float-path JumpFlood (non-power-of-two screens)
    std::vector<float> t((size_t)c->W + c->H);
    tc_table(c->W, c->H, t.data());
    HIPCHK(c, alloc(&c->tc, t.size() * sizeof(float)));
    HIPCHK(c, hipMemcpy(c->tc, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
    c->tc_rcp_ok = tc_rcp_exact(c->W) && tc_rcp_exact(c->H);
  }
  if (c->N <= 10)  // (4^L values per level: at most 350 k float4)
    HIPCHK(c, alloc(&c->bconst, ((((size_t)1 << (2 * c->N)) - 1) / 3) * sizeof(float4)));
  c->alloff.clear();
  c->rdiv_x.assign(c->N, 0);
  c->rdiv_y.assign(c->N, 0);
  for (int L = 0; L < c->N; ++L) {
    c->rdiv_x[L] = !c->cd.powW && rc_div_exact(c->CW, L, L == c->N - 1);
    c->rdiv_y[L] = !c->cd.powH && rc_div_exact(c->CH, L, L == c->N - 1);
  }
  HIPCHK(c, alloc(&c->dirs, dir_table_len(c->N) * sizeof(float2)));
  HIPCHK(c, alloc(&c->dexit, dir_table_len(c->N) * sizeof(float4)));
  HIPCHK(c, alloc(&c->sky, ((size_t)4 << (2 * (c->N - 1))) * sizeof(float4)));
  // initial contents: ClearAllRTs (RC2DGI.cs:109) -> (0,0,0,1) is implied by the frame
  // itself; zero everything so never-written texels (cascadeBlurRT with blur off) read as a
  // fresh texture does.
  HIPCHK(c, hipMemsetAsync(c->color_in, 0, ns * sizeof(float4), c->stream));
  HIPCHK(c, hipMemsetAsync(c->emissive, 0, ns * sizeof(float4), c->stream));
  HIPCHK(c, hipMemsetAsync(c->blur, 0, nc * sizeof(float4), c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->dir_override.assign(c->N, {});
  c->tables_dirty = true;
  c->have_frame = c->frame_done = false;
  c->ev_level.resize(c->N + 1);
  tuning_level_defaults(*c, c->N);
  if (int rc = jfa_buffers(c)) return rc;
  if (int rc = prepare_side_buffers(c)) return rc;
  if (c->keep_levels) {
    c->level_bufs.assign(c->N, nullptr);
    for (auto &p : c->level_bufs) HIPCHK(c, alloc(&p, nc * gsz));
  }
  return RC2DGI_OK;
}

// correctly rounded tables for RadianceCascades.fs:117-121 and :48-57/:150-154
static void build_tables(const rc2dgi_ctx *c, std::vector<float2> &dirs, std::vector<float4> &dexit,
                  std::vector<float4> &sky) {
  dirs.resize(dir_table_len(c->N));
  for (int L = 0; L < c->N; ++L) {
    const int b = 1 << L, n = 4 * b * b;
    const size_t off = dir_table_offset(L);
    if (!c->dir_override[L].empty()) {
      for (int a = 0; a < n; ++a) dirs[off + a] = make_float2(c->dir_override[L][2 * a], c->dir_override[L][2 * a + 1]);
      continue;
    }
    const float angleStep = kTau / (float)(b * b * 4);
    for (int a = 0; a < n; ++a) {
      const float angle = ((float)a + 0.5f) * angleStep;
      dirs[off + a] = make_float2((float)std::cos((double)angle), (float)std::sin((double)angle));
    }
  }
  float aspx, aspy;
  rc_aspect(c->W, c->H, aspx, aspy);
  dexit.resize(dirs.size());
  for (size_t i = 0; i < dirs.size(); ++i) {
    float e[4];
    rc_exit_terms(dirs[i].x, dirs[i].y, aspx, aspy, e);
    dexit[i] = make_float4(e[0], e[1], e[2], e[3]);
  }
  const int b = 1 << (c->N - 1), n = 4 * b * b;
  sky.resize(n);
  if (!c->sky_override.empty()) {
    for (int a = 0; a < n; ++a)
      sky[a] = make_float4(c->sky_override[3 * a], c->sky_override[3 * a + 1], c->sky_override[3 * a + 2], 0.0f);
    return;
  }
  const float angleStep = kTau / (float)(b * b * 4);
  const float SSunS = 8.0f, ISSunS = 1.0f / 8.0f;
  for (int a = 0; a < n; ++a) {
    const float a0 = ((float)a + 0.5f) * angleStep;
    const float a1 = a0 + angleStep;
    const float ca1 = (float)std::cos((double)a1), ca0 = (float)std::cos((double)a0);
    const float sky_term = a1 - a0 - 0.5f * (ca1 - ca0);
    const float at0 = (float)std::atan((double)(SSunS * (c->sun_angle - a0)));
    const float at1 = (float)std::atan((double)(SSunS * (c->sun_angle - a1)));
    const float sun_term = at0 - at1;
    float v[3];
    for (int k = 0; k < 3; ++k) {
      float SI = c->sky_color[k] * sky_term;
      SI = SI + c->sun_color[k] * sun_term * ISSunS;
      float s = SI * 0.16f;
      s = s * c->sky_radiance;
      v[k] = (s / angleStep) * 2.0f;
    }
    sky[a] = make_float4(v[0], v[1], v[2], 0.0f);
  }
}

int upload_tables(rc2dgi_ctx *c) {
  if (!c->tables_dirty) return RC2DGI_OK;
  std::vector<float2> dirs;
  std::vector<float4> dexit, sky;
  build_tables(c, dirs, dexit, sky);
  // The directional miss proofs assume every direction of block bi lies in angular bin bi * kDirBins / 4^L
  // and has unit length (the clear distances are texels along the ray, converted to t).  True of the
  // library's own tables; a caller's table (rc2dgi_set_direction_table) is checked here, level by level,
  // with 1e-5 of slack (k_dir_clear's boxes carry a texel of margin: 1e-5 rad is 0.08 texels at 8192).
  c->dp_ok.assign(c->N, 0);
  for (int L = 0; L < c->N; ++L) {
    if ((1 << (2 * L)) < kDirBins) continue;
    const double PI2 = 6.283185307179586, half = 0.5 * PI2 / kDirBins;
    bool ok = true;
    const size_t off = dir_table_offset(L), n = (size_t)4 << (2 * L);
    for (size_t a = 0; a < n && ok; ++a) {
      const double x = dirs[off + a].x, y = dirs[off + a].y;
      const int j = (int)(((a / 4) * (size_t)kDirBins) >> (2 * L));
      const double center = PI2 * (j + 0.5) / kDirBins;
      const double d = std::remainder(std::atan2(y, x) - center, PI2);
      ok = std::fabs(d) <= half + 1e-5 && std::fabs(std::hypot(x, y) - 1.0) <= 1e-5;
    }
    c->dp_ok[L] = ok;
  }
  HIPCHK(c, hipMemcpyAsync(c->dirs, dirs.data(), dirs.size() * sizeof(float2), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->dexit, dexit.data(), dexit.size() * sizeof(float4), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->sky, sky.data(), sky.size() * sizeof(float4), hipMemcpyHostToDevice, c->stream));
  // the host vectors die here: make the pageable copies complete first
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->h_dirs = dirs;
  c->alloff.clear();  // (levels no ray samples: proven again with these directions)
  c->tables_dirty = false;
  return RC2DGI_OK;
}

static float half_to_float(uint16_t h) {  // exact
  const unsigned s = (h >> 15) & 1u, e = (h >> 10) & 31u, m = h & 1023u;
  float v;
  if (e == 0) v = std::ldexp((float)m, -24);
  else if (e == 31) v = m ? NAN : INFINITY;
  else v = std::ldexp((float)(m | 1024u), (int)e - 25);
  return s ? -v : v;
}

// a GI-format cascade texture -> float4 (CW x CH, tight); texels of RGBA8 storage read as k * (1/255).  The source
// holds rows [y0, y1) from its row 0 (a shard's strip-sized blur textures); the other rows read as NaN.
int fetch_gi(rc2dgi_ctx *c, const void *src, std::vector<float4> &img, size_t gsz, int y0, int y1) {
  if (y1 < 0) y1 = c->CH;
  const size_t nr = (size_t)(y1 - y0), off = (size_t)y0 * c->CW, nt = nr * c->CW;
  if (y0 > 0 || y1 < c->CH) std::memset(img.data(), 0xFF, img.size() * sizeof(float4));
  if (gsz == 16) {
    HIPCHK(c, hipMemcpy2D(img.data() + off, (size_t)c->CW * 16, src, (size_t)c->cd.pitch * 16, (size_t)c->CW * 16, nr,
                          hipMemcpyDeviceToHost));
    return RC2DGI_OK;
  }
  if (gsz == 4) {
    std::vector<uint8_t> b(nt * 4);
    HIPCHK(c, hipMemcpy2D(b.data(), (size_t)c->CW * 4, src, (size_t)c->cd.pitch * 4, (size_t)c->CW * 4, nr,
                          hipMemcpyDeviceToHost));
    for (size_t k = 0; k < nt; ++k)
      img[off + k] = make_float4((float)b[4 * k] * kInv255h, (float)b[4 * k + 1] * kInv255h,
                                 (float)b[4 * k + 2] * kInv255h, (float)b[4 * k + 3] * kInv255h);
    return RC2DGI_OK;
  }
  std::vector<uint16_t> h(nt * 4);
  HIPCHK(c, hipMemcpy2D(h.data(), (size_t)c->CW * 8, src, (size_t)c->cd.pitch * 8, (size_t)c->CW * 8, nr,
                        hipMemcpyDeviceToHost));
  for (size_t k = 0; k < nt; ++k)
    img[off + k] = make_float4(half_to_float(h[4 * k]), half_to_float(h[4 * k + 1]), half_to_float(h[4 * k + 2]),
                               half_to_float(h[4 * k + 3]));
  return RC2DGI_OK;
}

FramePlan make_plan(const rc2dgi_ctx *c) {
  return plan_frame(PlanInputs{c->W, c->H, c->CW, c->CH, c->S, c->N, c->blur_radius, c->rank, c->world});
}

}  // namespace rc2dgi
