// rc2dgi_frame.cpp -- the DoRC2DGI() orchestrator: pass order and ping-pong identities of RC2DGI.cs:267-406.
#include "rc2dgi_ctx.h"

namespace rc2dgi {

// phase 1: ScreenUV, JumpFlood, DistanceField (RC2DGI.cs:276-340), in three parts so that the
// JumpFlood exchange of row-strip shards can run between the steps: phase1_begin (ScreenUV and
// step 0), phase1_step (step t >= 1), phase1_end.
// JumpFlood ping-pong (RC2DGI.cs:287-326): step t writes jumpRT2 for even t, jumpRT1 for odd t.
static unsigned *jfa_out(rc2dgi_ctx *c, int t) { return (t & 1) ? c->jump1 : c->jump2; }

// how the float-path steps get their texcoords (launch_jfa_step tmode): tuning jfa_tab, tc_rcp only where exact
static int jfa_tmode(const rc2dgi_ctx *c) { return c->jfa_tab == 2 ? (c->tc_rcp_ok ? 2 : 1) : c->jfa_tab; }

int jfa_launch(rc2dgi_ctx *c, const FramePlan &plan, int t) {
  float ox[3], oy[3];
  jfa_offsets(c->W, c->H, t, ox, oy);  // vec2(x, y) * _Aspect.yx * _StepSize
  unsigned short *dist = t == c->S - 1 ? c->dist : nullptr;  // 3. DistanceField fused into the last step
  hipStream_t st = c->stream;
  JfaStepArgs a;  // (what the step's launches share; a row-strip shard leaves lds, small_rt and jrows off)
  a.first = t == 0;
  a.dist = dist;
  a.off_x = ox;
  a.off_y = oy;
  a.tc = c->tc;
  a.tmode = jfa_tmode(c);
  if (!c->strip) {
    // the first four steps in one kernel (k_jfa_coset): the ScreenUV mask -> J_3
    const int lat = (c->jfa_coset == 2 && c->W <= 4096) ? 32 : 16;  // (the float-key build of lat 32 spills)
    int cs = c->jfa_coset ? jfa_coset_steps(c->sd, c->S, lat) : 0;
    for (int q = 0; q < cs; ++q)
      if (!plan.jfa[q].is_full()) cs = 0;
    // the last nt steps in one kernel (k_jfa_tail), which writes J_{S-2} and J_{S-1} into the two ping-pong textures:
    // the step before it writes its result into a texture of its own (jtail) instead
    int nt = jfa_tail_apply(c) && c->jtail ? c->jfa_tail : 0;
    for (int q = c->S - nt; q < c->S; ++q)
      if (!plan.jfa[q].is_full()) nt = 0;
    if (cs > c->S - nt) nt = 0;
    auto out_of = [&](int q) { return (nt && q == c->S - nt - 1) ? c->jtail : jfa_out(c, q); };
    if (t < cs) {
      if (t == 0) HIPCHK(c, launch_jfa_coset(c->occ, c->mpitch, out_of(cs - 1), c->sd, st, lat));
      return RC2DGI_OK;
    }
    if (nt && t >= c->S - nt) {
      if (t == c->S - nt)
        HIPCHK(c, launch_jfa_tail(out_of(t - 1), jfa_out(c, c->S - 1), jfa_out(c, c->S - 2), c->dist, c->sd, c->S, nt, st));
      return RC2DGI_OK;
    }
    a.src = t == 0 ? c->occ : out_of(t - 1);
    a.src_pitch = t == 0 ? c->mpitch : c->sd.pitch;
    a.dst = out_of(t);
    a.lds = c->jfa_lds;
    a.small_rt = c->jfa_rt;
    a.jrows = c->jfa_rows;
    for (auto &r : plan.jfa[t].iv) {
      a.row0 = r.first;
      a.row1 = r.second;
      HIPCHK(c, launch_jfa_step(a, c->sd, st));
    }
    return RC2DGI_OK;
  }
  // row-strip shard: the own strip, into its window (global row y0 - m = local row 0)
  int y0, y1;
  strip_rows(c->H, c->rank, c->world, y0, y1);
  a.dst = jfa_out(c, t);
  a.row0 = y0;
  a.row1 = y1;
  a.dst_row0 = y0 - c->jx.m;
  if (t == 0) {
    a.src = c->occ;
    a.src_pitch = c->mpitch;
    HIPCHK(c, launch_jfa_step(a, c->sd, st));
    return RC2DGI_OK;
  }
  int buf[3], row0[3];
  jfa_window(c->jx, t, c->rank, buf, row0);
  JfaSrc win{};
  win.on = 1;
  for (int y = 0; y < 3; ++y) {
    win.base[y] = buf[y] == 0 ? jfa_out(c, t - 1) : c->jblk[buf[y] - 1];
    win.row0[y] = row0[y];
  }
  a.src_pitch = c->sd.pitch;  // (src stays nullptr: every tap row comes from the window)
  a.window = &win;
  HIPCHK(c, launch_jfa_step(a, c->sd, st));
  return RC2DGI_OK;
}

int phase1_begin(rc2dgi_ctx *c, const FramePlan &plan) {
  HIPCHK(c, hipSetDevice(c->device));
  int rc = upload_tables(c);
  if (rc != RC2DGI_OK) return rc;
  hipStream_t st = c->stream;
  const bool T = c->timing;
  if (c->poison) {  // debug: rows a (sharded) frame never writes read as NaN / far seeds / far distance
    const size_t ns = (size_t)c->sd.pitch * c->H, nc = (size_t)c->cd.pitch * c->CH;
    HIPCHK(c, hipMemsetAsync(c->jump1, 0xFF, (size_t)c->sd.pitch * c->jwin_rows * 4, st));
    HIPCHK(c, hipMemsetAsync(c->jump2, 0xFF, (size_t)c->sd.pitch * c->jwin_rows * 4, st));
    HIPCHK(c, hipMemsetAsync(c->occ, 0xFF, (size_t)c->mpitch * c->H * 4, st));
    HIPCHK(c, hipMemsetAsync(c->dist, 0xFF, ns * 2, st));
    const size_t nw = (size_t)c->sd.pitch * (size_t)(c->ow1 - c->ow0);  // (the own rows on a shard)
    HIPCHK(c, hipMemsetAsync(c->temp, 0xFF, nw * 16, st));
    HIPCHK(c, hipMemsetAsync(c->color_out, 0xFF, nw * 16, st));
    const size_t nb = c->gwin ? (size_t)c->cd.pitch * (size_t)(c->ow1 - c->ow0) : nc;  // (cascadeBlurRT, spare)
    for (int b = 0; b < 2; ++b)
      HIPCHK(c, hipMemsetAsync(b ? c->gi2 : c->gi1, 0xFF, c->gi_rows[b] * c->cd.pitch * gi_bytes(c), st));
    HIPCHK(c, hipMemsetAsync(c->gi_spare, 0xFF, nb * gi_bytes(c), st));
    for (float4 *b : c->chain_bufs)
      if (b) HIPCHK(c, hipMemsetAsync(b, 0xFF, nc * 16, st));
    HIPCHK(c, hipMemsetAsync(c->blur, 0xFF, nb * 16, st));
  }
  if (T) HIPCHK(c, hipEventRecord(c->ev[0], st));

  // 1. ScreenUV (RC2DGI.cs:276-285): occupancy mask; J0 itself is only materialised when a
  //    single JFA step leaves it visible in jumpRT1.  A row-strip shard computes the mask rows its
  //    step 0 taps (from the replicated colorRT).
  if (c->strip) {
    for (auto &r : jfa_mask_rows(c->W, c->H, c->rank, c->world).iv)
      HIPCHK(c, launch_occupancy(c->color_in, c->occ, c->mpitch, c->sd, st, r.first, r.second));
  } else {
    HIPCHK(c, launch_occupancy(c->color_in, c->occ, c->mpitch, c->sd, st));
  }
  if (c->S == 1) HIPCHK(c, launch_seeds_from_mask(c->occ, c->mpitch, c->jump1, c->sd, st));
  if (T) HIPCHK(c, hipEventRecord(c->ev[1], st));
  // 2. JumpFlood step 0 (from the mask)
  return jfa_launch(c, plan, 0);
}

int phase1_end(rc2dgi_ctx *c) {
  if (c->timing) HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
  return RC2DGI_OK;
}

// device pointer of row `row` of a JumpFlood exchange buffer (0 the window holding J_{t-1}, 1 / 2 blocks)
unsigned *jfa_xbuf(rc2dgi_ctx *c, int t, int buf, int row) {
  unsigned *b = buf == 0 ? jfa_out(c, t - 1) : c->jblk[buf - 1];
  return b + (size_t)row * c->sd.pitch;
}

// one phase 1 on a context with its own exchange (RCCL communicator) or none (unsharded)
static int do_phase1(rc2dgi_ctx *c, const FramePlan &plan) {
  int rc = phase1_begin(c, plan);
  for (int t = 1; rc == RC2DGI_OK && t < c->S; ++t) {
    if (c->strip) rc = jfa_exchange_rccl(c, t);
    if (rc == RC2DGI_OK) rc = jfa_launch(c, plan, t);
  }
  return rc == RC2DGI_OK ? phase1_end(c) : rc;
}

// phase 2: cascades, blur, merge (RC2DGI.cs:342-404), in two parts: the side pass (the march's records, bound
// table, palettes, march field and directional clear table) and the levels with blur and merge.  Row-strip shards
// with strip tables (strip_tables_apply) exchange the side tables of their cell rows in between (rc2dgi_do over
// RCCL, rc2dgi_do_group by device copies).
int phase2_side(rc2dgi_ctx *c, SidePass &f) {
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  // 4. radiance cascades N-1 .. 0 (RC2DGI.cs:342-362).  The "t" / "p" / "o" variants read re-laid-out
  // copies of distRT; building them is timed with the top level (it is RC work, not DistanceField's)
  // per-level events only in timing mode 1: each one idles the GPU ~5 us before the next level
  const bool LT = c->timing == 1;
  if (LT) HIPCHK(c, hipEventRecord(c->ev_level[c->N], st));
  bool tiled = false, packed = false, nib = false;
  for (int v : c->rc_variant) {
    tiled |= rc_variant_tiled(v);
    packed |= rc_variant_packed(v);
    nib |= rc_variant_nib(v);
  }
  // (the packed marches run on power-of-two screens of up to 16384 columns and rows only, the bound jfa_p2_taps
  // keeps; elsewhere their variants launch the plain-field march, and the copies would be built for nothing)
  const bool p2s = c->sd.powW && c->sd.powH && c->cd.powW && c->cd.powH && c->W <= 16384 && c->H <= 16384;
  // (the copies were allocated when the schedule was set: prepare_side_buffers; a frame never allocates)
  if ((tiled && !c->dist_t) || (packed && p2s && !c->dist_p) || (nib && p2s && !c->dist_n))
    return fail(c, RC2DGI_E_STATE, "distRT copy of the schedule not prepared");
  if (tiled) HIPCHK(c, launch_dist_tile(c->dist, c->sd.pitch, c->dist_t, c->W, c->H, st));
  if (packed && p2s) HIPCHK(c, launch_dist_pack(c->dist, c->sd.pitch, c->dist_p, c->W, c->H, st));
  if (nib && p2s) HIPCHK(c, launch_dist_nib(c->dist, c->sd.pitch, c->dist_n, c->W, c->H, st));
  const bool proofs = proofs_on(c);
  // the directional table only where some level reads it: a one-probe tile at a level with 4^L >= kDirBins,
  // directional proofs on there and the level's direction table binnable (dp_ok)
  bool mps = false;
  for (int L = 0; L < c->N; ++L)
    mps |= c->rc_mp[L] != 0 && !c->rc_noproof[L] && (1 << (2 * L)) >= kDirBins && rc_variant_one_probe(c->rc_variant[L]) &&
           L < (int)c->dp_ok.size() && c->dp_ok[L];
  mps = mps && proofs;
  // surface records and the bound table in one pass over distRT where its cells are >= 64 texels; with the
  // surface palettes also the march field the plain-field levels read (launch_shade_cmin)
  const bool fused = proofs && c->shade_fused && shade_cmin_fused_ok(c->W, c->H, c->sd.pitch);
  const bool pal = fused && c->rc_pal && (size_t)c->sd.pitch * c->H <= ((size_t)1 << 26);
  if (pal && (!c->mfield || !c->cell_pal)) return fail(c, RC2DGI_E_STATE, "surface palette tables not prepared");
  const bool stt = pal && strip_tables_apply(c);
  if (!stt && !c->shade) return fail(c, RC2DGI_E_STATE, "record texture not prepared");
  f.proofs = proofs;
  f.mps = mps;
  f.fused = fused;
  f.pal = pal;
  f.st = stt;
  c->st_last = stt;
  c->built_hitc = mps;
  c->built_cmin = proofs;
  c->built_dclr = mps;
  c->built_pal = pal;
  bool side = false, dc_merged = false;  // (k_dir_clear on the side stream / in k_shade_cells' launch)
  ShadeCminArgs a;
  a.dist = c->dist;
  a.color = c->color_in;
  a.emis = c->emissive;
  a.shade = stt ? nullptr : c->shade;
  a.reflectivity = c->reflectivity;
  a.cmin = c->cmin;
  a.hitc = mps ? c->hitc : nullptr;
  if (fused) {
    // (the split pass's parity advances only with the split passes themselves: k_shade_cells clears the other
    // parity's counter for the next one)
    const bool split = pal && c->shade_split && shade_split_ok(c->W, c->H);
    // split pass with directional proofs: k_dir_clear needs only the scan's hit flags, so it runs on the side
    // stream beside k_shade_cells (the few hundred workgroups of the hit cells leave most CUs idle); with strip
    // tables it waits for every shard's flags (phase2_levels)
    side = split && mps && !stt && c->side_overlap == 1 && c->side_stream && c->ev_fork && c->ev_join;
    // side_overlap 2: k_dir_clear's workgroups appended to k_shade_cells' grid instead (one launch, one stream)
    dc_merged = split && mps && !stt && c->side_overlap == 2;
    a.mf = pal ? c->mfield : nullptr;
    a.cpal = pal ? c->cell_pal : nullptr;
    a.list = split ? c->shade_list : nullptr;
    a.parity = split ? (int)(c->split_frames++ & 1u) : 0;
    a.after_scan = side ? c->ev_fork : nullptr;
    a.boxes = dc_merged ? c->dboxes : nullptr;
    a.dclr = dc_merged ? c->dclr : nullptr;
    if (stt) {  // (strip tables: the cell rows of the own strip)
      int y0, y1;
      strip_rows(c->H, c->rank, c->world, y0, y1);
      const int csh = dist_cmin_shift(c->W, c->H);
      a.cr0 = y0 >> csh;
      a.ncr = (y1 - y0) >> csh;
    }
    HIPCHK(c, launch_shade_cmin(a, c->sd, st));
  } else {
    HIPCHK(c, launch_shade(a, c->sd, st));
    if (proofs) HIPCHK(c, launch_dist_cmin(a, c->sd, st));
  }
  if (mps && side) {
    HIPCHK(c, hipStreamWaitEvent(c->side_stream, c->ev_fork, 0));
    HIPCHK(c, launch_dir_clear(c->hitc, c->dboxes, c->dclr, c->side_stream));
    HIPCHK(c, hipEventRecord(c->ev_join, c->side_stream));
    HIPCHK(c, hipStreamWaitEvent(st, c->ev_join, 0));
  } else if (mps && stt) {
    f.dclr_pending = true;
  } else if (mps && !dc_merged) {
    HIPCHK(c, launch_dir_clear(c->hitc, c->dboxes, c->dclr, st));
  }
  return RC2DGI_OK;
}

// the pieces of shard q's strip tables (strip_tables_apply): its rows of the march field, its cell rows of the bound
// table, hit flags and palettes -- each one contiguous run of its buffer
void strip_table_pieces(const rc2dgi_ctx *c, int q, StripPiece out[4]) {
  int y0, y1;
  strip_rows(c->H, q, c->world, y0, y1);
  const int csh = dist_cmin_shift(c->W, c->H);
  const size_t cr0 = (size_t)(y0 >> csh), ncr = (size_t)((y1 - y0) >> csh);
  out[0] = {(size_t)y0 * c->sd.pitch * sizeof(unsigned short), (size_t)(y1 - y0) * c->sd.pitch * sizeof(unsigned short)};
  out[1] = {cr0 * kCminDim * sizeof(CminT), ncr * kCminDim * sizeof(CminT)};
  out[2] = {cr0 * kCminDim, ncr * kCminDim};
  out[3] = {cr0 * kCminDim * kCellPalStride * sizeof(float4), ncr * kCminDim * kCellPalStride * sizeof(float4)};
}
char *strip_table_base(rc2dgi_ctx *c, int piece) {
  switch (piece) {
    case 0: return reinterpret_cast<char *>(c->mfield);
    case 1: return reinterpret_cast<char *>(c->cmin);
    case 2: return reinterpret_cast<char *>(c->hitc);
    default: return reinterpret_cast<char *>(c->cell_pal);
  }
}

// level L runs inside the chain launch of a chained frame (rc_chain 4: the top level too)
static bool in_chain_launch(const rc2dgi_ctx *c, int L) { return L < c->N - 1 || c->rc_chain == 4; }

// k_rc_level's arguments of level L, which merges with `upper` into `out` (chained: inside the chain launch)
static int level_args(rc2dgi_ctx *c, const SidePass &f, int L, bool chained, float4 *upper, float4 *out,
                      RcLevelArgs &a) {
  const bool proofs = f.proofs, mps = f.mps, pal = f.pal;
  a.upper = (L == c->N - 1) ? nullptr : upper;
  a.out = out;
  // (palettes: the one-probe tiles of the plain field, rc2dgi_rc.h PALC; level 0 shares its first sample; the
  // chain's levels are 16x16x1 tiles of the plain field)
  const int var = chained ? 0 : c->rc_variant[L];
  const bool plain = !rc_variant_tiled(var) && !rc_variant_packed(var) && !rc_variant_nib(var) &&
                     rc_variant_one_probe(var) && L > 0;
  // the march field: same samples, hits carry a palette entry (strip tables: every level marches on it -- the
  // shard holds distRT for its own rows only -- and hit records come from the palettes or the inputs)
  a.dist = (pal && (plain || f.st)) ? c->mfield : c->dist;
  a.cell_pal = (pal && plain) ? c->cell_pal : nullptr;
  a.shade = c->shade;
  if (f.st) {
    a.rec_color = c->color_in;
    a.rec_emis = c->emissive;
  }
  a.dirs = c->dirs + dir_table_offset(L);
  a.dexit = c->dexit + dir_table_offset(L);
  a.sky = c->sky;
  a.level = L;
  a.N = c->N;
  a.ray_range = c->ray_range;
  a.reflectivity = c->reflectivity;
  a.variant = c->rc_variant[L];
  a.order_code = c->rc_order[L];
  a.map_cache = &c->rc_maps;
  a.dist_tiled = c->dist_t;
  a.dist_packed = c->dist_p;
  a.dist_nib = c->dist_n;
  a.cmin = (proofs && !c->rc_noproof[L]) ? c->cmin : nullptr;
  a.dclr = (mps && c->rc_mp[L] && !c->rc_noproof[L] && L < (int)c->dp_ok.size() && c->dp_ok[L]) ? c->dclr : nullptr;
  // the screen-edge test pays where rays are long (t1 >= 1/8 of the screen: L4 / L5 at N = 6)
  a.cmin_screen = c->rc_skip == 3 || (c->rc_skip == 1 && rc_ray_end(L, c->N, c->ray_range) >= 0.125f);
  a.tail_k = c->rc_tail[L];
  a.wg_proof = c->rc_wgproof;
  a.div_x = c->rc_rdiv && c->rdiv_x[L];
  a.div_y = c->rc_rdiv && c->rdiv_y[L];
  if (c->gband) {  // banded cascade textures (gi_buffers)
    if (!f.st) return fail(c, RC2DGI_E_STATE, "banded cascade textures without strip tables");
    a.out_b0 = c->gb0[L];
    a.out_bn = c->gbn[L];
    if (L + 1 < c->N) {
      a.up_b0 = c->gb0[L + 1];
      a.up_bn = c->gbn[L + 1];
    }
  }
  return RC2DGI_OK;
}

// 5. blur + blended copy-back (RC2DGI.cs:367-387) into the spare texture, which then becomes
//    finalGI (buffer swap, same contents as blending in place); 6. merge + copy-back
//    (RC2DGI.cs:389-404), fused into the blur pass when the fixed-tap kernel applies and the
//    cascade matches the screen (its pass time is then reported under blur).
static int blur_and_merge(rc2dgi_ctx *c, const FramePlan &plan, float4 *&finalGI) {
  hipStream_t st = c->stream;
  const bool T = c->timing;
  bool merged = false;
  BlurArgs b;  // (filled once; the launches below differ in their rows, gi_in follows finalGI)
  b.gi_in = finalGI;
  b.blur_out = c->blur;
  b.gi_out = c->gi_spare;
  b.radius = c->blur_radius;
  b.color_in = c->color_in;
  b.temp = c->temp;
  b.color_out = c->color_out;
  b.m0 = c->ow0;
  b.m1 = c->ow1;
  auto rows = [&b](const std::pair<int, int> &r) -> const BlurArgs & {
    b.row0 = r.first;
    b.row1 = r.second;
    return b;
  };
  if (c->blur_radius > 0.0f) {
    bool fused = false;
    BlurTaps bt;
    const bool mrg = c->sd.W == c->CW && c->sd.H == c->CH && !c->linux_merge;
    // The fused kernels skip LINEAR taps of weight 0, an identity but for non-finite or huge neighbours
    // (absmax4, rc2dgi_blur.hip): they report such a value through odd_flag, and the frame is then redone tap by tap
    // on the device (launch_blur_exact below; one launch that returns at once otherwise).  A row-strip shard's fused
    // kernels stage whole tiles, rows it did not compute among them, so there a scan of its level-0 rows reports
    // (launch_blur_odd_rows) and its own rows are redone: the level-0 plan holds every row their redo reads, and a
    // shard whose rows hold no such value keeps the fused kernels' bits, which are the redo's there.
    const bool whole = c->world == 1 && !c->gwin && !c->gband;
    if (!c->odd_flag) {
      HIPCHK(c, alloc(&c->odd_flag, sizeof(unsigned)));
      HIPCHK(c, hipMemsetAsync(c->odd_flag, 0, sizeof(unsigned), st));
      c->odd_epoch = 0;
    }
    if (++c->odd_epoch == 0) c->odd_epoch = 1;  // (0: the cleared flag)
    unsigned *const flag = c->odd_flag;
    b.flag = whole ? flag : nullptr;
    b.epoch = c->odd_epoch;
    b.g0 = c->gband ? c->gb0[0] : 0;
    b.gn = c->gband ? c->gbn[0] : 0;
    // a fused kernel writes the copied-back GI into gi_spare, which then becomes finalGI: only when
    // every launch of it ran (a refused launch -- shapes it does not take -- falls back before any
    // launch ran, since the shapes are the same for every row interval)
    if (c->blur_path == 0 && blur_rows_plan(c->cd, c->blur_radius, &bt) >= 0) {
      bool ok = true;
      b.merge = mrg;
      for (auto &r : plan.blur.iv) ok = ok && launch_blur_rows(rows(r), c->sd, c->cd, st);
      if (!ok && plan.blur.iv.size() > 1) return fail(c, RC2DGI_E_HIP, "fixed-tap blur refused a row interval");
      fused = ok;
      merged = ok && mrg;
    }
    // (strip-sized cascadeBlurRT / copy-back texture: only the fused blur + merge writes them; out_buffers sized them
    // for this frame's settings)
    if (c->gwin && !merged) return fail(c, RC2DGI_E_STATE, "strip-sized blur textures without the fused blur + merge");
    if (!fused && c->blur_path <= 1 && blur_fused_ok(c->cd, c->blur_radius)) {
      bool ok = true;
      for (auto &r : plan.blur.iv) ok = ok && launch_blur_fused(rows(r), c->cd, st);
      if (!ok && plan.blur.iv.size() > 1) return fail(c, RC2DGI_E_HIP, "LDS-tiled blur refused a row interval");
      fused = ok;
    }
    if (fused) {
      HIPCHK(c, hipGetLastError());
      b.merge = merged;
      b.flag = flag;
      if (whole) {
        HIPCHK(c, launch_blur_exact(rows({0, -1}), c->sd, c->cd, st));
      } else {
        for (auto &r : plan.level[0].iv) HIPCHK(c, launch_blur_odd_rows(rows(r), c->cd, st));
        b.strip = c->gwin;
        if (merged)  // (the merge's outputs hold the own rows)
          HIPCHK(c, launch_blur_exact(rows({c->ow0, c->ow1}), c->sd, c->cd, st));
        else
          for (auto &r : plan.blur.iv) HIPCHK(c, launch_blur_exact(rows(r), c->sd, c->cd, st));
      }
      if (!c->gwin) std::swap(finalGI, c->gi_spare);  // (gwin: the final GI stays in the strip-sized gi_spare)
    } else {
      for (auto &r : plan.blur.iv) HIPCHK(c, launch_blur(rows(r), c->cd, st));
      for (auto &r : plan.blur.iv) HIPCHK(c, launch_blur_copyback(c->blur, finalGI, c->cd, st, r.first, r.second));
    }
  }
  if (T) HIPCHK(c, hipEventRecord(c->ev[4], st));
  b.gi_in = finalGI;
  if (!merged)
    for (auto &r : plan.merge.iv) HIPCHK(c, launch_merge(rows(r), c->sd, c->cd, st, c->linux_merge));
  if (T) HIPCHK(c, hipEventRecord(c->ev[5], st));
  return RC2DGI_OK;
}

int phase2_levels(rc2dgi_ctx *c, const FramePlan &plan, const SidePass &f) {
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const bool T = c->timing;
  const bool LT = c->timing == 1;
  if (f.dclr_pending) HIPCHK(c, launch_dir_clear(c->hitc, c->dboxes, c->dclr, st));
  bool gi1final = false;
  // The cascade chain (tuning rc_chain, rc2dgi_rc_chain.hip): the top level as usual, then levels N-2 .. 0 in one
  // launch of 16x16x1 tiles, each level into a texture of its own -- level 0 into giRT1 / giRT2 as the loop below
  // leaves it (N odd: giRT1), level 1 into the other, levels >= 2 into chain_bufs.
  const bool chain = chain_active(c) && c->chain && (int)c->chain_bufs.size() == c->N;
  std::vector<RcLevelArgs> chain_args;
  // levels no ray samples (rc_level_all_off): per-block values and a fill in place of the level's launch, from the top
  // down while every level above was one too (k_rc_block_const; f32 frames without the chain)
  const bool fill_on = c->rc_fill && c->bconst && !chain && c->storage == RC2DGI_STORAGE_F32 &&
                       c->h_dirs.size() == dir_table_len(c->N);
  if (fill_on && ((int)c->alloff.size() != c->N || c->alloff_rr != c->ray_range)) {
    c->alloff.assign(c->N, 0);
    for (int L = c->N - 1; L >= 0; --L) {
      c->alloff[L] = rc_level_all_off(c->sd, c->cd, c->N, L, c->ray_range, c->h_dirs.data() + dir_table_offset(L),
                                      c->rc_rdiv && c->rdiv_x[L], c->rc_rdiv && c->rdiv_y[L]);
      if (!c->alloff[L]) break;  // (only a run from the top is used)
    }
    c->alloff_rr = c->ray_range;
  }
  auto boff = [](int L) { return ((((size_t)1) << (2 * L)) - 1) / 3; };
  int filled = 0;
  float4 *const g0 = (c->N % 2) ? c->gi1 : c->gi2, *const g1 = (c->N % 2) ? c->gi2 : c->gi1;
  auto chain_out = [&](int L) { return L == 0 ? g0 : (L == 1 ? g1 : c->chain_bufs[L]); };
  for (int L = c->N - 1; L >= 0; --L) {
    float4 *srcGI = gi1final ? c->gi1 : c->gi2;
    float4 *dstGI = gi1final ? c->gi2 : c->gi1;
    if (chain) {
      srcGI = L + 1 < c->N ? chain_out(L + 1) : nullptr;
      dstGI = chain_out(L);
    }
    const bool chained = chain && in_chain_launch(c, L);
    if (LT && L + 1 < c->N && !(chain && in_chain_launch(c, L + 1))) HIPCHK(c, hipEventRecord(c->ev_level[L + 1], st));
    RcLevelArgs a;
    if (int rc = level_args(c, f, L, chained, srcGI, dstGI, a)) return rc;
    const bool top = L == c->N - 1;
    // below a filled level: merge with its block values instead of staging its texture (the 32x8x2 tiles)
    if (fill_on && !top && (filled >> (L + 1) & 1) && c->rc_variant[L] == 6 && c->sd.powW && c->sd.powH &&
        c->cd.powW && c->cd.powH && L > 0)
      a.upper_const = c->bconst + boff(L + 1);
    if (fill_on && c->alloff[L] && (top || (filled >> (L + 1) & 1))) {
      HIPCHK(c, launch_rc_block_const(top, top ? c->sky : c->bconst + boff(L + 1), c->bconst + boff(L), L, st));
      for (auto &r : plan.level[L].iv)  // (a row-strip shard: its rows, into the banded texture when banded)
        HIPCHK(c, launch_rc_fill(dstGI, c->bconst + boff(L), c->cd, L, st, r.first, r.second,
                                 c->gband ? c->gb0[L] : 0, c->gband ? c->gbn[L] : 0));
      filled |= 1 << L;
    } else if (chained) {
      chain_args.push_back(a);  // (whole levels: one process; rc_chain 4: the top level in the launch too)
    } else {
      for (auto &r : plan.level[L].iv) {
        a.p0 = r.first;
        a.p1 = r.second;
        HIPCHK(c, launch_rc_level(a, c->sd, c->cd, st));
      }
    }
    if (c->keep_levels && !chain)
      HIPCHK(c, hipMemcpyAsync(c->level_bufs[L], dstGI, (size_t)c->cd.pitch * c->CH * gi_bytes(c),
                               hipMemcpyDeviceToDevice, st));
    gi1final = !gi1final;
  }
  if (chain) {
    HIPCHK(c, launch_rc_chain(c->chain, chain_args.data(), (int)chain_args.size(), c->sd, c->cd,
                              c->rc_chain == 2 ? 32 : 1, st, c->rc_chain == 3, c->rc_chain_spin));
    // (per-level events: the whole chain counts as its first level, the levels below it as 0)
    if (LT)
      for (int L = c->N - (c->rc_chain == 4 ? 1 : 2); L >= 1; --L) HIPCHK(c, hipEventRecord(c->ev_level[L], st));
    if (c->keep_levels)
      for (int L = 0; L < c->N; ++L)
        HIPCHK(c, hipMemcpyAsync(c->level_bufs[L], chain_out(L), (size_t)c->cd.pitch * c->CH * gi_bytes(c),
                                 hipMemcpyDeviceToDevice, st));
  }
  c->fill_mask = filled;
  if (LT) HIPCHK(c, hipEventRecord(c->ev_level[0], st));
  if (T) HIPCHK(c, hipEventRecord(c->ev[3], st));
  float4 *&finalGI = gi1final ? c->gi1 : c->gi2;  // RC2DGI.cs:365
  c->final_gi = gi1final ? 1 : 2;
  if (int rc = blur_and_merge(c, plan, finalGI)) return rc;
  c->frame_done = true;
  c->have_frame = true;
  c->level_times = LT;
  return RC2DGI_OK;
}

// phase 2 of a context without an exchange in its middle (unsharded, or a shard without strip tables)
static int do_phase2(rc2dgi_ctx *c, const FramePlan &plan) {
  SidePass f;
  int rc = phase2_side(c, f);
  if (rc != RC2DGI_OK) return rc;
  if (f.st) return fail(c, RC2DGI_E_STATE, "strip tables exchange between the side pass and the levels");
  return phase2_levels(c, plan, f);
}

// distRT strip of shard q: device pointer and byte count (rows are contiguous, pitch-linear)
void dist_strip(const rc2dgi_ctx *c, int q, unsigned short **p, size_t *bytes) {
  int y0, y1;
  strip_rows(c->H, q, c->world, y0, y1);
  *p = c->dist + (size_t)y0 * c->sd.pitch;
  *bytes = (size_t)(y1 - y0) * c->sd.pitch * sizeof(unsigned short);
}

}  // namespace rc2dgi

extern "C" {

int rc2dgi_do(rc2dgi_ctx *c) {
  if (!c) return RC2DGI_E_ARG;
  RC2DGI_USABLE(c);
  if (int rc = check_chain(c)) return rc;  // (an earlier chained frame that has completed)
  if (c->world > 1 && !c->comm)
    return fail(c, RC2DGI_E_STATE, "sharded context: use rc2dgi_shard_connect, rc2dgi_do_group or rc2dgi_do_phase");
  if (int rc = out_buffers(c)) return rc;  // (the strip-sized outputs follow the blur settings)
  const FramePlan plan = make_plan(c);
  int rc = do_phase1(c, plan);
  if (rc != RC2DGI_OK) return rc;
  const bool stt = c->comm && strip_tables_apply(c);
  if (c->comm) {
    // every strip of distRT to every rank: one in-place broadcast per root; with strip tables only row 0 (the REPEAT
    // wrap of the last cell row's bound), the side tables' rows follow the side pass instead
    std::vector<Bcast> pieces;
    if (stt) pieces.push_back({c->dist, (size_t)c->sd.pitch * sizeof(unsigned short), 0});
    for (int q = 0; q < c->world && !stt; ++q) {
      unsigned short *p;
      size_t n;
      dist_strip(c, q, &p, &n);
      pieces.push_back({p, n, q});
    }
    if (int rc = broadcast_group(c, pieces, "ncclBroadcast")) return rc;
  }
  if (!stt) return do_phase2(c, plan);
  SidePass f;
  rc = phase2_side(c, f);
  if (rc != RC2DGI_OK) return rc;
  if (!f.st) return fail(c, RC2DGI_E_STATE, "strip tables: side pass disagrees");
  // the side tables' rows of every rank to every rank: four in-place broadcasts per root, one group
  std::vector<Bcast> pieces;
  for (int q = 0; q < c->world; ++q) {
    StripPiece pc[4];
    strip_table_pieces(c, q, pc);
    for (int i = 0; i < 4; ++i) pieces.push_back({strip_table_base(c, i) + pc[i].off, pc[i].bytes, q});
  }
  if (int rc = broadcast_group(c, pieces, "ncclBroadcast (strip tables)")) return rc;
  return phase2_levels(c, plan, f);
}

int rc2dgi_do_phase(rc2dgi_ctx *c, int phase) {
  if (!c) return RC2DGI_E_ARG;
  RC2DGI_USABLE(c);
  if (int rc = check_chain(c)) return rc;  // (an earlier chained frame that has completed)
  if (phase != 1 && phase != 2) return fail(c, RC2DGI_E_ARG, "phase is 1 or 2");
  if (phase == 1 && c->strip)
    return fail(c, RC2DGI_E_STATE,
                "phase 1 of a row-strip shard exchanges JumpFlood rows between its steps: use rc2dgi_do with a "
                "communicator, or rc2dgi_do_group");
  if (int rc = out_buffers(c)) return rc;
  const FramePlan plan = make_plan(c);
  return phase == 1 ? do_phase1(c, plan) : do_phase2(c, plan);
}

}  // extern "C"
