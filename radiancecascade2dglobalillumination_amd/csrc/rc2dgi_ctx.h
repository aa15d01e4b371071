// rc2dgi_ctx.h -- the context behind the C ABI (include/rc2dgi.h) and the helpers its host units share:
// rc2dgi_buffers.cpp (sizes, allocation, tables), rc2dgi_frame.cpp (the frame), rc2dgi_group.cpp (RCCL, sharded
// groups), rc2dgi_autotune.cpp, the accessory calls over rc2dgi_accessory.h -- rc2dgi_display.cpp (the display frame
// and its tone curves), rc2dgi_regions.cpp (region statistics, histograms and image reads, planned by
// rc2dgi_rectplan.cpp) and rc2dgi_points.cpp (samples and ray casts) -- and rc2dgi_capi.cpp (everything else of the
// ABI).
#pragma once
#include "../../include/rc2dgi.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <new>
#include <utility>
#include <string>
#include <vector>

#include "rc2dgi_kernels.h"
#include "rc2dgi_paint.h"
#include "rc2dgi_present.h"
#include "rc2dgi_query.h"
#include "rc2dgi_reduce.h"
#include "rc2dgi_hist.h"
#include "rc2dgi_read.h"
#include "rc2dgi_tone.h"
#include "rc2dgi_shard.h"
#include "rc2dgi_tuning.h"

using namespace rc2dgi;  // (the host units only: this header is not part of the public interface)

enum Pass { P_SCREENUV = 0, P_JFA, P_RC, P_BLUR, P_MERGE, P_TOTAL, P_COUNT };

inline bool is_pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }
inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

// (the tuning knobs: its Tuning base, rc2dgi_tuning.h)
struct rc2dgi_ctx : rc2dgi::Tuning {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t side_stream = nullptr;  // the directional table beside the split records pass (fork / join events)
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipStream_t stream = nullptr;
  // knobs (RC2DGI.cs:28-41, 66-68)
  int W = 0, H = 0, N = 0;
  float render_scale = 1.0f;
  int storage = RC2DGI_STORAGE_F32;
  bool linux_merge = false;  // RC2DGI_FLAG_LINUX_MERGE_FALLBACK: the merge pass runs raylib's default shader
  float ray_range = 2.0f;
  float sky_radiance = 1.0f, sky_color[3] = {0.5f, 0.6f, 0.8f}, sun_color[3] = {1.0f, 0.9f, 0.6f};
  float sun_angle = 0.3f, reflectivity = 0.0f, blur_radius = 1.5f;
  // derived sizes
  int CW = 0, CH = 0, S = 0;
  ScreenDims sd{};
  CascadeDims cd{};
  // device buffers (the reference's render textures)
  float4 *color_in = nullptr, *emissive = nullptr, *temp = nullptr, *color_out = nullptr;
  unsigned *jump1 = nullptr, *jump2 = nullptr;  // packed seeds (row-strip shards: their windows, see jx)
  // row-strip shards: the JumpFlood exchange plan, and the two block buffers of its long steps
  JfaExchange jx;
  bool strip = false;   // world > 1 and S >= 2: JumpFlood on strip windows with the exchange
  unsigned *jblk[2] = {nullptr, nullptr};
  size_t jwin_rows = 0;  // rows of a window (jump1 / jump2)
  unsigned *occ = nullptr;                      // ScreenUV occupancy mask
  int mpitch = 0;                               // mask row pitch (words)
  unsigned short *dist = nullptr;  // packUNorm16 q
  unsigned short *dist_t = nullptr;  // 8x8-tiled copy for the "t" RC variants
  uint4 *dist_p = nullptr;           // packed copy for the "p" RC variants (k_dist_pack)
  uint4 *dist_n = nullptr;           // nibble-predicted copy for the "n" RC variants (k_dist_nib)
  unsigned short *mfield = nullptr;  // march field of the surface palettes (tuning rc_pal, launch_shade_cmin)
  float4 *cell_pal = nullptr;        // kCminDim^2 cells x kCellPalStride palette entries
  unsigned *shade_list = nullptr;    // the split records pass's cell list (launch_shade_cmin, tuning shade_split)
  unsigned split_frames = 0;         // split records passes enqueued (their list counters alternate by this parity)
  // which side tables the last frame built (rc2dgi_download_table answers RC2DGI_E_STATE for the others)
  bool built_hitc = false, built_cmin = false, built_dclr = false, built_pal = false;
  float4 *shade = nullptr;           // surface records of the hittable texels (k_shade)
  CminT *cmin = nullptr;             // coarse lower bound of distRT for the march's exit proofs (k_dist_cmin)
  unsigned char *hitc = nullptr;     // per bound-table cell: holds a texel that passes the hit test
  unsigned char *dclr = nullptr;     // directional clear distances of the miss proofs (k_dir_clear)
  int4 *dboxes = nullptr;            // k_dir_clear's per-bin step boxes (dir_clear_boxes)
  float4 *gi1 = nullptr, *gi2 = nullptr, *blur = nullptr;
  float4 *gi_spare = nullptr;  // fused blur writes the copied-back final GI here, then swaps
  unsigned *odd_flag = nullptr;  // holds odd_epoch when a fused blur kernel of that frame (a shard: the scan of its
                                 // level-0 rows) met a value the skipped weight-0 taps are no identity for
                                 // (launch_blur_exact then redoes the frame, a shard its rows)
  unsigned odd_epoch = 0;
  float2 *dirs = nullptr;  // concatenated per level
  float4 *dexit = nullptr;  // screen-exit terms of dirs (rc_exit_terms), same layout
  float4 *sky = nullptr;
  // state
  bool tables_dirty = true;
  std::vector<std::vector<float>> dir_override;  // per level, empty = computed
  std::vector<float> sky_override;
  bool frame_done = false;   // colorRT holds the merged result
  bool have_frame = false;
  int final_gi = 1;
  bool level_times = false;  // the last frame recorded ev_level
  int timing = 0;  // rc2dgi_set_timing: 0 off, 1 pass and per-level events, 2 pass events only
  hipEvent_t ev[P_COUNT + 1] = {};
  std::vector<hipEvent_t> ev_level;  // N + 1
  std::vector<int> dp_ok;        // per level: its direction table fits k_dir_clear's bins (upload_tables)
  unsigned *jtail = nullptr;     // J_{S-jfa_tail-1}, which the fused tail reads (it writes both ping-pong textures)
  float *tc = nullptr;           // texcoords of the W columns and H rows (tc_table) for the float-path JumpFlood
  bool tc_rcp_ok = false;        // tc_rcp equals the division for every column and row (tc_rcp_exact)
  std::vector<unsigned char> rdiv_x, rdiv_y;  // per level: rc_div_exact on CW / CH (non-power-of-two cascades)
  float4 *bconst = nullptr;      // per-direction-block values of the levels no ray samples (k_rc_block_const), level L
                                 // from (4^L - 1) / 3 on
  std::vector<float2> h_dirs;    // the uploaded direction table (rc_level_all_off)
  std::vector<unsigned char> alloff;  // per level: rc_level_all_off, for ray range alloff_rr (cleared with the tables)
  float alloff_rr = -1.0f;
  int fill_mask = 0;             // levels the last frame filled
  bool keep_levels = false;
  std::vector<float4 *> level_bufs;  // debug copies of G_L
  RcChain *chain = nullptr;          // its argument block and readiness flags (rc2dgi_rc_chain.hip)
  std::vector<float4 *> chain_bufs;  // per level >= 2: its own G_L (the chain's levels overlap)
  // row-strip sharding
  RcMapCache rc_maps;  // host-built k_rc_level workgroup maps
  PaintBuffers paint_buf;  // rc2dgi_paint primitive setup
  PaintDevBuffers paint_dev;  // rc2dgi_paint_device's and rc2dgi_sprites_device's plan (paint_dev_plan of the screen
                              // and the "paint_plan" knob) and working memory: a fixed size for the plan, allocated
                              // at the first call of either
  unsigned *tilemap_cnt = nullptr;  // rc2dgi_tilemap_device's {drawn, refused} counters: 8 KiB (kTilemapCounterBytes), zero
                                    // between calls, allocated at the first call that has a status
  unsigned char *present_buf = nullptr;  // rc2dgi_compose's window image (RGBA8), grown on demand
  size_t present_cap = 0;
  unsigned char *query_in = nullptr, *query_out = nullptr;  // rc2dgi_sample / rc2dgi_raycast's points or rays and
  size_t query_in_cap = 0, query_out_cap = 0;               // their results, grown on demand
  unsigned char *reduce_buf = nullptr;  // rc2dgi_reduce's plan (work items, joins) and band partials of one batch: a
                                        // fixed size (reduce_bytes, rc2dgi_regions.cpp), allocated at the first call
  unsigned char *hist_buf = nullptr;    // rc2dgi_histogram's search tree of the edges, then one batch of work items:
                                        // a fixed size (hist_bytes, rc2dgi_regions.cpp), allocated at the first call
  unsigned char *read_buf = nullptr;    // rc2dgi_read's and rc2dgi_write's staged image rows: kReadChunkBytes
                                        // (rc2dgi_read.h), allocated at the first call of either
  std::vector<float> curve_host[RC2DGI_MAX_CURVES];  // rc2dgi_set_curve: slot s at [s - 1], 255 edges; empty: not set
  float *curves_dev = nullptr;          // the same as search trees (rc2dgi_tone.h), 256 words a slot; stored on the
                                        // context stream, allocated at the first rc2dgi_set_curve, kept to the end
  int rank = 0, world = 1;
  int ow0 = 0, ow1 = 0;  // screen rows tempRT / the merged colorRT hold (their row 0 = row ow0): [0, H), or a row-strip
                         // shard's own rows (out_buffers)
  bool gwin = false;     // cascadeBlurRT and the blur's copy-back texture (gi_spare) hold rows [ow0, ow1) too
                         // (a shard on the fused blur + merge, gi_window_apply); the copy-back then stays in
                         // gi_spare (no buffer swap) and is the frame's final GI
  bool gband = false;    // giRT1 / giRT2 banded (gi_band_apply): level L's texture holds, per block row, the gbn[L]
                         // block-local rows from gb0[L] on (cyclically) -- the rows the shard's plan computes
  std::vector<int> gb0, gbn;
  size_t gi_rows[2] = {0, 0};  // rows giRT1 / giRT2 hold (CH when whole)
  ncclComm_t comm = nullptr;
  hipEvent_t ev_phase1 = nullptr;   // end of phase 1 (group exchange)
  hipEvent_t ev_frame = nullptr;    // end of the last group frame (peers copy from our distRT)
  hipEvent_t ev_jfa[2] = {nullptr, nullptr};  // end of the last even / odd JFA step (group exchange)
  hipEvent_t ev_side = nullptr;     // end of the side pass (group exchange of the strip tables)
  bool st_last = false;             // the last frame ran with strip tables
  bool gi1final = false;            // phase 1 -> phase 2 state
  bool broken = false;              // a reallocation failed: the device buffers are gone (destroy it)
  std::string err;
};

namespace rc2dgi {

// giRT1 / giRT2 texel size of the context's storage
inline size_t gi_bytes(const rc2dgi_ctx *c) {
  return c->storage == RC2DGI_STORAGE_F16 ? 8 : (c->storage == RC2DGI_STORAGE_RGBA8_COMPAT ? 4 : 16);
}
inline bool rgba8(const rc2dgi_ctx *c) { return c->storage == RC2DGI_STORAGE_RGBA8_COMPAT; }
constexpr float kInv255h = 1.0f / 255.0f;  // an RGBA8 texel k reads as k * (1/255)

inline int fail(rc2dgi_ctx *c, int code, const std::string &msg) {
  if (c) c->err = msg;
  return code;
}

// a context whose reallocation failed holds freed / null device buffers: refuse to touch them
#define RC2DGI_USABLE(ctx)                                                                                   \
  do {                                                                                                       \
    if ((ctx)->broken)                                                                                       \
      return fail((ctx), RC2DGI_E_STATE, "the context lost its render textures (a reallocation failed): destroy it"); \
  } while (0)

inline int hip_fail(rc2dgi_ctx *c, hipError_t e, const char *what) {
  std::string m = std::string(what) + ": " + hipGetErrorString(e);
  return fail(c, e == hipErrorOutOfMemory ? RC2DGI_E_OOM : RC2DGI_E_HIP, m);
}

#define HIPCHK(ctx, expr)                                 \
  do {                                                    \
    hipError_t e_ = (expr);                               \
    if (e_ != hipSuccess) return hip_fail(ctx, e_, #expr); \
  } while (0)

template <class T>
hipError_t alloc(T **p, size_t bytes) {
  return hipMalloc(reinterpret_cast<void **>(p), bytes);
}

// ---- rc2dgi_buffers.cpp
void derive_sizes(int W, int H, int N, float rs, int &CW, int &CH, int &S);
unsigned timing_event_flags();
size_t dir_table_len(int N);
size_t dir_table_offset(int L);
void free_level_bufs(rc2dgi_ctx *c);
void free_chain(rc2dgi_ctx *c);
bool chain_active(const rc2dgi_ctx *c);
int check_chain(rc2dgi_ctx *c);
void free_buffers(rc2dgi_ctx *c);
int jfa_buffers(rc2dgi_ctx *c);
bool jfa_tail_apply(const rc2dgi_ctx *c);
bool proofs_on(const rc2dgi_ctx *c);
bool strip_tables_apply(const rc2dgi_ctx *c);
int out_buffers(rc2dgi_ctx *c);
int prepare_side_buffers(rc2dgi_ctx *c, bool all = false);
int allocate(rc2dgi_ctx *c);
int upload_tables(rc2dgi_ctx *c);
int fetch_gi(rc2dgi_ctx *c, const void *src, std::vector<float4> &img, size_t gsz, int y0 = 0, int y1 = -1);
FramePlan make_plan(const rc2dgi_ctx *c);

// ---- rc2dgi_frame.cpp
struct SidePass {
  bool proofs = false, mps = false, fused = false, pal = false;
  bool st = false;            // strip tables: own cell rows only; the exchange follows
  bool dclr_pending = false;  // k_dir_clear still to run (strip tables: it needs every shard's hit flags)
};
struct StripPiece {
  size_t off, bytes;
};
int jfa_launch(rc2dgi_ctx *c, const FramePlan &plan, int t);
int phase1_begin(rc2dgi_ctx *c, const FramePlan &plan);
int phase1_end(rc2dgi_ctx *c);
unsigned *jfa_xbuf(rc2dgi_ctx *c, int t, int buf, int row);
int phase2_side(rc2dgi_ctx *c, SidePass &f);
void strip_table_pieces(const rc2dgi_ctx *c, int q, StripPiece out[4]);
char *strip_table_base(rc2dgi_ctx *c, int piece);
int phase2_levels(rc2dgi_ctx *c, const FramePlan &plan, const SidePass &f);
void dist_strip(const rc2dgi_ctx *c, int q, unsigned short **p, size_t *bytes);

// ---- rc2dgi_group.cpp
int jfa_exchange_rccl(rc2dgi_ctx *c, int t);
// a group of in-place broadcasts on c->stream over the context's communicator (piece k from rank root[k])
struct Bcast {
  void *p;
  size_t bytes;
  int root;
};
int broadcast_group(rc2dgi_ctx *c, const std::vector<Bcast> &pieces, const char *what);
void drop_comm(rc2dgi_ctx *c);  // destroy the context's communicator, if any

}  // namespace rc2dgi
