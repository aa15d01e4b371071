// rc2dgi_group.cpp -- row-strip shards: the RCCL exchanges of a context with a communicator, the
// in-process group frame (rc2dgi_do_group) and the shard / plan entry points of the C ABI.
#include <dlfcn.h>

#include <cstdlib>

#include "rc2dgi_ctx.h"

namespace {

// RCCL, resolved at first use (the single-GPU path never loads it).  In a process that already
// loaded RCCL (e.g. through torch.distributed) dlopen returns that same library.  RC2DGI_RCCL_LIB, read at that
// first use, names the library to open instead (a test transport: tests/fake_rccl.cpp); if it does not load or
// lacks a symbol the transport is unsupported -- never a fallback to librccl.
struct Rccl {
  decltype(&ncclGetUniqueId) get_unique_id = nullptr;
  decltype(&ncclCommInitRank) comm_init_rank = nullptr;
  decltype(&ncclCommDestroy) comm_destroy = nullptr;
  decltype(&ncclGroupStart) group_start = nullptr;
  decltype(&ncclGroupEnd) group_end = nullptr;
  decltype(&ncclBroadcast) broadcast = nullptr;
  decltype(&ncclSend) send = nullptr;
  decltype(&ncclRecv) recv = nullptr;
  decltype(&ncclGetErrorString) error_string = nullptr;
  bool ok = false;
};

const Rccl &rccl() {
  static Rccl r = [] {
    Rccl x;
    void *h = nullptr;
    if (const char *named = std::getenv("RC2DGI_RCCL_LIB"); named && *named) {
      h = dlopen(named, RTLD_NOW | RTLD_LOCAL);
    } else {
      h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
      if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    }
    if (!h) return x;
    x.get_unique_id = reinterpret_cast<decltype(x.get_unique_id)>(dlsym(h, "ncclGetUniqueId"));
    x.comm_init_rank = reinterpret_cast<decltype(x.comm_init_rank)>(dlsym(h, "ncclCommInitRank"));
    x.comm_destroy = reinterpret_cast<decltype(x.comm_destroy)>(dlsym(h, "ncclCommDestroy"));
    x.group_start = reinterpret_cast<decltype(x.group_start)>(dlsym(h, "ncclGroupStart"));
    x.group_end = reinterpret_cast<decltype(x.group_end)>(dlsym(h, "ncclGroupEnd"));
    x.broadcast = reinterpret_cast<decltype(x.broadcast)>(dlsym(h, "ncclBroadcast"));
    x.send = reinterpret_cast<decltype(x.send)>(dlsym(h, "ncclSend"));
    x.recv = reinterpret_cast<decltype(x.recv)>(dlsym(h, "ncclRecv"));
    x.error_string = reinterpret_cast<decltype(x.error_string)>(dlsym(h, "ncclGetErrorString"));
    x.ok = x.get_unique_id && x.comm_init_rank && x.comm_destroy && x.group_start && x.group_end && x.broadcast &&
           x.send && x.recv && x.error_string;
    return x;
  }();
  return r;
}

// device-to-device copies on a context's stream: gathered into launch_copy_batch launches where the pieces allow it
// (one device, 16-byte aligned), else one hipMemcpyAsync each; flush() before anything else is enqueued
struct Copier {
  rc2dgi_ctx *c;
  bool batch;
  CopyBatch b;
  Copier(rc2dgi_ctx *ctx, bool one_device) : c(ctx), batch(one_device) {}
  hipError_t add(void *dst, const void *src, size_t bytes) {
    if (bytes == 0) return hipSuccess;
    if (!batch || !copy_piece_ok(src, dst, bytes))
      return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream);
    if (b.n == kCopyBatchMax)
      if (hipError_t e = flush()) return e;
    b.p[b.n++] = CopyPiece{src, dst, bytes};
    return hipSuccess;
  }
  hipError_t flush() {
    const hipError_t e = launch_copy_batch(b, c->stream);
    b.n = 0;
    return e;
  }
};

}  // namespace

namespace rc2dgi {

// the JumpFlood exchange of step t over RCCL: every transfer this shard sends or receives as
// ncclSend / ncclRecv in one group on the context stream (rows of its own window to itself:
// device copies)
int jfa_exchange_rccl(rc2dgi_ctx *c, int t) {
  const Rccl &R = rccl();
  const size_t rowb = (size_t)c->sd.pitch * sizeof(unsigned);
  ncclResult_t e = R.group_start();
  hipError_t he = hipSuccess;  // (a failing self-copy still closes the group below)
  for (const JfaXfer &x : c->jx.steps[t].xfers) {
    if (e != ncclSuccess || he != hipSuccess) break;
    if (x.src == c->rank && x.dst == c->rank) {
      he = hipMemcpyAsync(jfa_xbuf(c, t, x.dst_buf, x.dst_row), jfa_xbuf(c, t, 0, x.src_row), x.rows * rowb,
                          hipMemcpyDeviceToDevice, c->stream);
    } else if (x.src == c->rank) {
      e = R.send(jfa_xbuf(c, t, 0, x.src_row), x.rows * rowb, ncclUint8, x.dst, c->comm, c->stream);
    } else if (x.dst == c->rank) {
      e = R.recv(jfa_xbuf(c, t, x.dst_buf, x.dst_row), x.rows * rowb, ncclUint8, x.src, c->comm, c->stream);
    }
  }
  const ncclResult_t e2 = R.group_end();
  if (e == ncclSuccess) e = e2;
  if (he != hipSuccess) return hip_fail(c, he, "hipMemcpyAsync (JumpFlood exchange, own rows)");
  if (e != ncclSuccess) return fail(c, RC2DGI_E_HIP, std::string("JumpFlood exchange: ") + R.error_string(e));
  return RC2DGI_OK;
}

int broadcast_group(rc2dgi_ctx *c, const std::vector<Bcast> &pieces, const char *what) {
  const Rccl &R = rccl();
  ncclResult_t e = R.group_start();
  for (const Bcast &b : pieces) {
    if (e != ncclSuccess) break;
    e = R.broadcast(b.p, b.p, b.bytes, ncclUint8, b.root, c->comm, c->stream);
  }
  const ncclResult_t e2 = R.group_end();
  if (e == ncclSuccess) e = e2;
  if (e != ncclSuccess) return fail(c, RC2DGI_E_HIP, std::string(what) + ": " + R.error_string(e));
  return RC2DGI_OK;
}

void drop_comm(rc2dgi_ctx *c) {
  if (c->comm && rccl().ok) (void)rccl().comm_destroy(c->comm);
  c->comm = nullptr;
}

}  // namespace rc2dgi

extern "C" {

int rc2dgi_do_group(rc2dgi_ctx **cs, int n) {
  if (!cs || n < 1) return RC2DGI_E_ARG;
  for (int k = 0; k < n; ++k) {
    if (!cs[k]) return RC2DGI_E_ARG;
    RC2DGI_USABLE(cs[k]);
    const rc2dgi_ctx *c = cs[k];
    if (c->rank != k || c->world != n || c->W != cs[0]->W || c->H != cs[0]->H || c->N != cs[0]->N ||
        c->CW != cs[0]->CW || c->CH != cs[0]->CH)
      return fail(cs[k], RC2DGI_E_ARG, "rc2dgi_do_group: context k must be shard k of n of one configuration");
  }
  for (int k = 0; k < n; ++k) {  // (the strip-sized outputs follow the blur settings; before anything is enqueued)
    HIPCHK(cs[k], hipSetDevice(cs[k]->device));
    if (int rc = out_buffers(cs[k])) return rc;
  }
  // the shards' exchange copies as batched copy kernels when every shard is on one device (in-process rehearsal),
  // else one hipMemcpyAsync each (Copier)
  bool one_device = true;
  for (int k = 1; k < n; ++k) one_device = one_device && cs[k]->device == cs[0]->device;
  // a peer may still be copying our previous distRT strip: wait for every peer's last frame
  for (int k = 0; k < n; ++k) {
    HIPCHK(cs[k], hipSetDevice(cs[k]->device));
    for (int q = 0; q < n; ++q)
      if (q != k) HIPCHK(cs[k], hipStreamWaitEvent(cs[k]->stream, cs[q]->ev_frame, 0));
  }
  // phase 1, step by step over the group: before step t every shard copies the rows of J_{t-1} it
  // receives (JumpFlood exchange plan) from their owners, after the owners' step t-1
  std::vector<FramePlan> plans;
  for (int k = 0; k < n; ++k) plans.push_back(make_plan(cs[k]));
  for (int k = 0; k < n; ++k) {
    int rc = phase1_begin(cs[k], plans[k]);
    if (rc != RC2DGI_OK) return rc;
    HIPCHK(cs[k], hipEventRecord(cs[k]->ev_jfa[0], cs[k]->stream));
  }
  for (int t = 1; t < cs[0]->S; ++t) {
    for (int k = 0; k < n; ++k) {
      rc2dgi_ctx *c = cs[k];
      HIPCHK(c, hipSetDevice(c->device));
      if (c->strip) {
        const size_t rowb = (size_t)c->sd.pitch * sizeof(unsigned);
        // step t overwrites J_{t-2} (ping-pong); the peers that copied rows of J_{t-2} from us before their
        // step t-1 did so on their own streams, so wait for those steps (the block partners change from step
        // to step, so they need not be the peers we receive from now); and the owners of the rows of J_{t-1}
        // we copy now must have finished their step t-1 (group_step_waits; tests/test_shard_plan.py)
        std::vector<int> readers, senders;
        group_step_waits(c->jx, k, t, readers, senders);
        for (int q : readers) HIPCHK(c, hipStreamWaitEvent(c->stream, cs[q]->ev_jfa[(t - 1) & 1], 0));
        for (int q : senders)
          if (std::find(readers.begin(), readers.end(), q) == readers.end())
            HIPCHK(c, hipStreamWaitEvent(c->stream, cs[q]->ev_jfa[(t - 1) & 1], 0));
        Copier cp(c, one_device);
        for (const JfaXfer &x : c->jx.steps[t].xfers) {
          if (x.dst != k) continue;
          HIPCHK(c, cp.add(jfa_xbuf(c, t, x.dst_buf, x.dst_row), jfa_xbuf(cs[x.src], t, 0, x.src_row), x.rows * rowb));
        }
        HIPCHK(c, cp.flush());
      }
      int rc = jfa_launch(c, plans[k], t);
      if (rc != RC2DGI_OK) return rc;
      HIPCHK(c, hipEventRecord(c->ev_jfa[t & 1], c->stream));
    }
  }
  for (int k = 0; k < n; ++k) {
    int rc = phase1_end(cs[k]);
    if (rc != RC2DGI_OK) return rc;
    HIPCHK(cs[k], hipEventRecord(cs[k]->ev_phase1, cs[k]->stream));
  }
  // strip tables (strip_tables_apply, the same on every shard of one configuration): no distRT exchange -- the last
  // shard only needs row 0 for the REPEAT wrap of its last cell row's bound (k_shade_scan / shade_cell)
  const bool stt = strip_tables_apply(cs[0]);
  for (int k = 0; k < n; ++k)
    if (strip_tables_apply(cs[k]) != stt)
      return fail(cs[k], RC2DGI_E_ARG, "rc2dgi_do_group: every shard must run with the same strip_tables setting");
  for (int k = 0; k < n; ++k) {
    rc2dgi_ctx *c = cs[k];
    HIPCHK(c, hipSetDevice(c->device));
    if (stt) {
      if (k == n - 1) {
        HIPCHK(c, hipStreamWaitEvent(c->stream, cs[0]->ev_phase1, 0));
        HIPCHK(c, hipMemcpyAsync(c->dist, cs[0]->dist, (size_t)c->sd.pitch * sizeof(unsigned short),
                                 hipMemcpyDeviceToDevice, c->stream));
      }
      continue;
    }
    for (int q = 0; q < n; ++q) {
      if (q == k) continue;
      HIPCHK(c, hipStreamWaitEvent(c->stream, cs[q]->ev_phase1, 0));
      unsigned short *src, *dst;
      size_t bytes;
      dist_strip(cs[q], q, &src, &bytes);
      dist_strip(c, q, &dst, &bytes);
      HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
    }
  }
  // phase 2 of a context overwrites nothing a peer still copies from (only distRT -- or, with strip tables, the
  // side tables' own rows -- is read, and a context's next frame waits for every peer's frame)
  std::vector<SidePass> sides(n);
  for (int k = 0; k < n; ++k) {
    int rc = phase2_side(cs[k], sides[k]);
    if (rc != RC2DGI_OK) return rc;
    if (sides[k].st != stt) return fail(cs[k], RC2DGI_E_STATE, "strip tables: shards disagree");
    HIPCHK(cs[k], hipEventRecord(cs[k]->ev_side, cs[k]->stream));
  }
  if (stt) {  // every shard's table rows to every other shard
    for (int k = 0; k < n; ++k) {
      rc2dgi_ctx *c = cs[k];
      HIPCHK(c, hipSetDevice(c->device));
      for (int q = 0; q < n; ++q)
        if (q != k) HIPCHK(c, hipStreamWaitEvent(c->stream, cs[q]->ev_side, 0));
      Copier cp(c, one_device);
      for (int q = 0; q < n; ++q) {
        if (q == k) continue;
        StripPiece pc[4];
        strip_table_pieces(c, q, pc);
        for (int i = 0; i < 4; ++i)
          HIPCHK(c, cp.add(strip_table_base(c, i) + pc[i].off, strip_table_base(cs[q], i) + pc[i].off, pc[i].bytes));
      }
      HIPCHK(c, cp.flush());
    }
  }
  for (int k = 0; k < n; ++k) {
    int rc = phase2_levels(cs[k], plans[k], sides[k]);
    if (rc != RC2DGI_OK) return rc;
    HIPCHK(cs[k], hipEventRecord(cs[k]->ev_frame, cs[k]->stream));
  }
  return RC2DGI_OK;
}

int rc2dgi_set_shard(rc2dgi_ctx *c, int rank, int world) {
  if (!c) return RC2DGI_E_ARG;
  if (world < 1 || rank < 0 || rank >= world || world > c->H)
    return fail(c, RC2DGI_E_ARG, "rank must be in [0, world), world in [1, H]");
  if ((world != c->world || rank != c->rank) && c->comm) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    drop_comm(c);
  }
  c->rank = rank;
  c->world = world;
  c->frame_done = c->have_frame = false;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int rc = jfa_buffers(c);  // strip windows (world > 1) or full-size jumpRT1 / jumpRT2
  if (rc == RC2DGI_OK) rc = out_buffers(c);  // tempRT / merged colorRT: the own rows
  if (rc != RC2DGI_OK) c->broken = true;
  if (rc == RC2DGI_OK) rc = prepare_side_buffers(c);  // (strip tables: no record texture)
  c->st_last = false;
  return rc;
}

int rc2dgi_shard_rows(rc2dgi_ctx *c, int *y0, int *y1) {
  if (!c || !y0 || !y1) return RC2DGI_E_ARG;
  strip_rows(c->H, c->rank, c->world, *y0, *y1);
  return RC2DGI_OK;
}

int rc2dgi_shard_unique_id(void *id, int nbytes) {
  if (!id || nbytes < (int)sizeof(ncclUniqueId)) return RC2DGI_E_ARG;
  const Rccl &R = rccl();
  if (!R.ok) return RC2DGI_E_UNSUPPORTED;
  ncclUniqueId u;
  if (R.get_unique_id(&u) != ncclSuccess) return RC2DGI_E_HIP;
  std::memcpy(id, &u, sizeof(u));
  return RC2DGI_OK;
}

int rc2dgi_shard_connect(rc2dgi_ctx *c, const void *id, int nbytes) {
  if (!c || !id || nbytes < (int)sizeof(ncclUniqueId)) return fail(c, RC2DGI_E_ARG, "bad unique id");
  const Rccl &R = rccl();
  if (!R.ok) return fail(c, RC2DGI_E_UNSUPPORTED, "librccl not found");
  HIPCHK(c, hipSetDevice(c->device));
  drop_comm(c);
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof(u));
  const ncclResult_t e = R.comm_init_rank(&c->comm, c->world, u, c->rank);
  if (e != ncclSuccess) {
    c->comm = nullptr;
    return fail(c, RC2DGI_E_HIP, std::string("ncclCommInitRank: ") + R.error_string(e));
  }
  return RC2DGI_OK;
}

int rc2dgi_plan_order(int code, int tiles_x, int tiles_y, int tile_w, int tile_h, int ngrp, int *tiles, int *groups,
                      int n) {
  if (tiles_x <= 0 || tiles_y <= 0 || tile_w <= 0 || tile_h <= 0 || ngrp <= 0 || n < 0 ||
      n > tiles_x * tiles_y * ngrp || (n && (!tiles || !groups)))
    return RC2DGI_E_ARG;
  return rc_order_plan(code, tiles_x, tiles_y, tile_w, tile_h, ngrp, tiles, groups, n);
}

int rc2dgi_plan_wg_map(int code, int tiles_x, int tiles_y, int tile_w, int tile_h, int ngrp, int *tiles, int *groups,
                      int n) {
  if (tiles_x <= 0 || tiles_y <= 0 || tile_w <= 0 || tile_h <= 0 || ngrp <= 0 || n < 0 ||
      n > tiles_x * tiles_y * ngrp || (n && (!tiles || !groups)))
    return RC2DGI_E_ARG;
  return rc_wg_map_plan(code, tiles_x, tiles_y, tile_w, tile_h, ngrp, tiles, groups, n);
}

int rc2dgi_plan_jfa_exchange(const rc2dgi_config *cfg, int world, int step, int *info, int *xfers, int max_xfers) {
  if (!cfg || !info || cfg->screen_width < 1 || cfg->screen_height < 1 || cfg->cascade_count < 1 ||
      cfg->cascade_count > 15 || !(cfg->render_scale > 0.0f) || world < 2 || world > cfg->screen_height ||
      max_xfers < 0 || (max_xfers > 0 && !xfers))
    return RC2DGI_E_ARG;
  int CW, CH, S;
  derive_sizes(cfg->screen_width, cfg->screen_height, cfg->cascade_count, cfg->render_scale, CW, CH, S);
  if (S < 2 || step < 1 || step >= S) return RC2DGI_E_ARG;
  const JfaExchange x = plan_jfa_exchange(cfg->screen_width, cfg->screen_height, S, world);
  const JfaExStep &st = x.steps[step];
  const int v[9] = {x.m, x.hmax, x.mg_max, st.halo, st.sh[0], st.sh[1], st.sh[2], st.mg, st.same_block};
  for (int k = 0; k < 9; ++k) info[k] = v[k];
  int n = 0;
  for (const JfaXfer &t : st.xfers) {
    if (n < max_xfers) {
      const int r[6] = {t.src, t.src_row, t.rows, t.dst, t.dst_buf, t.dst_row};
      for (int k = 0; k < 6; ++k) xfers[6 * n + k] = r[k];
    }
    ++n;
  }
  return n;
}

int rc2dgi_plan_group_waits(const rc2dgi_config *cfg, int world, int rank, int step, int *peers, int max_peers) {
  if (!cfg || cfg->screen_width < 1 || cfg->screen_height < 1 || world < 2 || rank < 0 || rank >= world ||
      world > cfg->screen_height || cfg->cascade_count < 1 || cfg->cascade_count > 15 || !(cfg->render_scale > 0.0f) ||
      max_peers < 0 || (max_peers > 0 && !peers))
    return RC2DGI_E_ARG;
  int CW, CH, S;
  derive_sizes(cfg->screen_width, cfg->screen_height, cfg->cascade_count, cfg->render_scale, CW, CH, S);
  if (S < 2 || step < 1 || step >= S) return RC2DGI_E_ARG;
  std::vector<int> readers, senders;
  group_step_waits(plan_jfa_exchange(cfg->screen_width, cfg->screen_height, S, world), rank, step, readers, senders);
  int n = 0;
  for (int q : readers) {
    if (n < max_peers) peers[n] = q;
    ++n;
  }
  for (int q : senders) {
    if (n < max_peers) peers[n] = -1 - q;  // senders as -1 - shard
    ++n;
  }
  return n;
}

int rc2dgi_plan_jfa_window(const rc2dgi_config *cfg, int rank, int world, int step, int *buf, int *row0) {
  if (!cfg || !buf || !row0 || cfg->screen_width < 1 || cfg->screen_height < 1 || world < 2 || rank < 0 ||
      rank >= world || world > cfg->screen_height || cfg->cascade_count < 1 || cfg->cascade_count > 15 || !(cfg->render_scale > 0.0f))
    return RC2DGI_E_ARG;
  int CW, CH, S;
  derive_sizes(cfg->screen_width, cfg->screen_height, cfg->cascade_count, cfg->render_scale, CW, CH, S);
  if (S < 2 || step < 1 || step >= S) return RC2DGI_E_ARG;
  jfa_window(plan_jfa_exchange(cfg->screen_width, cfg->screen_height, S, world), step, rank, buf, row0);
  return RC2DGI_OK;
}

int rc2dgi_plan_rows(const rc2dgi_config *cfg, float blur_radius, int rank, int world, int pass, int *intervals,
                     int max_intervals) {
  if (!cfg || cfg->screen_width <= 0 || cfg->screen_height <= 0 || cfg->cascade_count < 1 ||
      cfg->cascade_count > 15 || !(cfg->render_scale > 0.0f) || world < 1 || rank < 0 || rank >= world ||
      world > cfg->screen_height)
    return RC2DGI_E_ARG;
  int CW, CH, S;
  derive_sizes(cfg->screen_width, cfg->screen_height, cfg->cascade_count, cfg->render_scale, CW, CH, S);
  const FramePlan p =
      plan_frame(PlanInputs{cfg->screen_width, cfg->screen_height, CW, CH, S, cfg->cascade_count, blur_radius, rank, world});
  const RowSet *rs = nullptr;
  if (pass >= RC2DGI_PLAN_JFA && pass < RC2DGI_PLAN_JFA + S) rs = &p.jfa[pass - RC2DGI_PLAN_JFA];
  else if (pass >= RC2DGI_PLAN_LEVEL && pass < RC2DGI_PLAN_LEVEL + cfg->cascade_count) rs = &p.level[pass - RC2DGI_PLAN_LEVEL];
  else if (pass == RC2DGI_PLAN_BLUR) rs = &p.blur;
  else if (pass == RC2DGI_PLAN_MERGE) rs = &p.merge;
  else return RC2DGI_E_ARG;
  const int n = (int)rs->iv.size();
  for (int k = 0; k < n && k < max_intervals && intervals; ++k) {
    intervals[2 * k] = rs->iv[k].first;
    intervals[2 * k + 1] = rs->iv[k].second;
  }
  return n;
}

}  // extern "C"
