// rc2dgi_autotune.cpp -- rc2dgi_autotune: the per-level workgroup order and march variant, picked by timing
// whole frames on the uploaded scene.
#include "rc2dgi_ctx.h"

namespace {

// rc2dgi_autotune candidates (px, py, dg); the library falls back to tile-major per level where
// a candidate does not tile the grid
// (4th field: 1 oriented patches, px tiles along the chunk's mean ray direction, py across;
// 2 bands py tiles wide along the chunk's mean ray direction, rc_logical_order)
const int kOrderCandidates[][4] = {{0, 0, 0, 0},  {2, 2, 8, 0},  {4, 4, 4, 0},   {2, 4, 4, 0},  {2, 8, 8, 0},
                                   {2, 16, 16, 0}, {1, 16, 16, 0}, {1, 16, 32, 0}, {1, 32, 16, 0}, {1, 4, 64, 0},
                                   {2, 8, 16, 0},  {4, 8, 4, 0},   {1, 8, 8, 0},   {2, 2, 16, 0},  {4, 2, 32, 0},
                                   {1, 4, 16, 0},  {16, 1, 16, 1}, {16, 2, 8, 1},  {8, 2, 16, 1},  {16, 1, 32, 1},
                                   {8, 1, 32, 1},  {32, 1, 8, 1},  {8, 4, 8, 1},   {4, 2, 32, 1},  {1, 1, 16, 2},
                                   {1, 1, 32, 2},  {1, 2, 8, 2},   {1, 2, 16, 2},  {1, 4, 4, 2},   {1, 4, 8, 2},
                                   {1, 1, 8, 2},   {1, 2, 32, 2},  {1, 1, 4, 2},   {1, 2, 4, 2},   {1, 4, 2, 2},
                                   {1, 8, 4, 2},   {1, 1, 64, 2},  {1, 2, 64, 2},  {1, 1, 128, 2}, {1, 8, 8, 2},
                                   {1, 3, 8, 2},   {1, 6, 8, 2},   {1, 3, 16, 2},  {1, 6, 4, 2},   {1, 12, 4, 2},
                                   {1, 16, 2, 2},  {1, 3, 32, 2},  {1, 6, 16, 2},
                                   // round 4 (order grids, profiles/r04/ab/orders_grid*.txt)
                                   {1, 1, 4, 1},   {2, 32, 32, 0}, {8, 32, 4, 1},  {8, 2, 4, 0},   {8, 32, 64, 0},
                                   {1, 3, 2, 2}};

}  // namespace

extern "C" int rc2dgi_autotune(rc2dgi_ctx *c, int frames) {
  if (!c) return RC2DGI_E_ARG;
  RC2DGI_USABLE(c);
  if (c->world > 1) return fail(c, RC2DGI_E_STATE, "autotune an unsharded context (the orders carry over)");
  if (frames < 1) frames = 1;
  if (int rc = prepare_side_buffers(c, true)) return rc;  // every copy a candidate variant reads
  // the chain books its levels on its first level's event and ignores rc_variant below the top: the per-level
  // picks are made on separate launches, and the chain setting comes back afterwards (as the timing mode does)
  struct Restore {
    rc2dgi_ctx *c;
    int timing, chain;
    ~Restore() {
      c->timing = timing;
      c->rc_chain = chain;
    }
  } restore{c, c->timing, c->rc_chain};
  c->timing = 1;
  c->rc_chain = 0;
  const int nc = (int)(sizeof(kOrderCandidates) / sizeof(kOrderCandidates[0]));
  // march rolled / unrolled x linear / 8x8-tiled / packed / nibble-predicted distance field; 32x8 tiles
  // (x2 probes per lane); one probe per lane in 512- and 1024-lane workgroups
  // (RGBA16F / RGBA8 cascades build the 16x16x1 family and three low-level shapes: the other ids would time
  // the default kernel again)
  const int kVariantsF32[] = {0, 1, 3, 5, 6, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25};
  const int kVariantsOther[] = {0, 1, 3, 6, 13, 14, 15, 16, 17, 18, 19, 25};
  const bool f32 = c->storage == RC2DGI_STORAGE_F32;
  const int *kVariants = f32 ? kVariantsF32 : kVariantsOther;
  const int nv = f32 ? (int)(sizeof(kVariantsF32) / sizeof(int)) : (int)(sizeof(kVariantsOther) / sizeof(int));
  std::vector<float> best(c->N, 1e30f), bestp(c->N, 1e30f);
  std::vector<int> pick(c->rc_order), pickv(c->rc_variant);
  std::vector<int> pickp(c->rc_order), pickpv(c->rc_variant);  // the best of the variants that need no distRT copy
  // which distRT copy a variant reads (0: none, 1 tiled, 2 packed, 3 nibble): the copy is built once per frame and
  // timed with the top level, so the per-level picks below do not see it
  auto copy_kind = [](int v) { return rc_variant_tiled(v) ? 1 : rc_variant_packed(v) ? 2 : rc_variant_nib(v) ? 3 : 0; };
  // frames + 1 frames of the schedule set in the context (the first warms the caches for its orders): the minimum
  // of every level's time into mins, and of the RC pass (every level, the copies included) into *pass
  std::vector<float> lv(c->N), acc;
  auto measure = [&](std::vector<float> &mins, float *pass = nullptr) -> int {
    mins.assign(c->N, 1e30f);
    float m = 1e30f;
    for (int f = 0; f <= frames; ++f) {
      int rc = rc2dgi_do(c);
      if (rc == RC2DGI_OK) rc = rc2dgi_pass_times(c, nullptr, 0, lv.data(), c->N);
      if (rc != RC2DGI_OK) return rc;
      if (f == 0) continue;
      float t = 0.0f;
      for (int L = 0; L < c->N; ++L) {
        mins[L] = std::min(mins[L], lv[L]);
        t += lv[L];
      }
      m = std::min(m, t);
    }
    if (pass) *pass = m;
    return RC2DGI_OK;
  };
  // level L ran in t ms with this order and variant: the best, and the best copy-free, pick so far
  auto note = [&](int L, float t, int order, int variant) {
    if (t < best[L]) {
      best[L] = t;
      pick[L] = order;
      pickv[L] = variant;
    }
    if (copy_kind(variant) == 0 && t < bestp[L]) {
      bestp[L] = t;
      pickp[L] = order;
      pickpv[L] = variant;
    }
  };
  // per level the kTop fastest (time, order, variant) of stage 1, for the XCD interleave stage below
  constexpr int kTop = 4;
  struct Cand {
    float t;
    int order, variant;
  };
  std::vector<std::vector<Cand>> top(c->N);
  auto keep_top = [&](int L, float t, int o, int v) {
    auto &T = top[L];
    T.push_back({t, o, v});
    std::sort(T.begin(), T.end(), [](const Cand &a, const Cand &b) { return a.t < b.t; });
    if ((int)T.size() > kTop) T.pop_back();
  };
  for (int k = 0; k < nv * nc; ++k) {
    const int *o = kOrderCandidates[k % nc];
    c->rc_order.assign(c->N, order_code(o[0], o[1], o[2], o[3]));
    c->rc_variant.assign(c->N, kVariants[k / nc]);
    if (int rc = measure(acc)) return rc;
    for (int L = 0; L < c->N; ++L) {
      keep_top(L, acc[L], c->rc_order[L], c->rc_variant[L]);
      note(L, acc[L], c->rc_order[L], c->rc_variant[L]);
    }
  }
  // Stage 2, the XCD interleave (order code bits 26-30, rc2dgi_plan_wg_map): each level's kTop stage-1 picks with
  // chunks of 2^lc logical workgroups dealt round-robin to the XCDs.  A level's march cost follows the
  // occluders; a contiguous eighth of the order per XCD leaves the XCDs unevenly loaded (4096^2 N=6 demo:
  // L4 0.445 -> 0.389 ms, profiles/r05/ab/xcd_interleave_grid.jsonl).
  for (int rank = 0; rank < kTop; ++rank) {
    for (int lc = 1; lc <= 9; ++lc) {
      for (int L = 0; L < c->N; ++L) {
        const Cand &cd = top[L][std::min(rank, (int)top[L].size() - 1)];
        c->rc_order[L] = (cd.order & ~(31 << 26)) | (lc << 26);
        c->rc_variant[L] = cd.variant;
      }
      if (int rc = measure(acc)) return rc;
      for (int L = 0; L < c->N; ++L) note(L, acc[L], c->rc_order[L], c->rc_variant[L]);
    }
  }
  // the schedule's RC pass
  auto pass_ms = [&](const std::vector<int> &ord, const std::vector<int> &var, float *ms) -> int {
    c->rc_order = ord;
    c->rc_variant = var;
    return measure(acc, ms);
  };
  // a copy kind pays only if its levels gain more than the copy costs: try each kind's levels on their best
  // copy-free picks instead
  for (int kind = 1; kind <= 3; ++kind) {
    bool used = false;
    for (int L = 0; L < c->N; ++L) used |= copy_kind(pickv[L]) == kind;
    if (!used) continue;
    std::vector<int> o2(pick), v2(pickv);
    for (int L = 0; L < c->N; ++L)
      if (copy_kind(pickv[L]) == kind) {
        o2[L] = pickp[L];
        v2[L] = pickpv[L];
      }
    float t1 = 0.0f, t2 = 0.0f;
    int rc = pass_ms(pick, pickv, &t1);
    if (rc == RC2DGI_OK) rc = pass_ms(o2, v2, &t2);
    if (rc != RC2DGI_OK) return rc;
    if (t2 < t1) {
      pick = o2;
      pickv = v2;
    }
  }
  c->rc_order = pick;
  c->rc_variant = pickv;
  c->rc_maps.retain(pick);  // the maps of the candidates that lost are device memory for nothing
  return RC2DGI_OK;
}
