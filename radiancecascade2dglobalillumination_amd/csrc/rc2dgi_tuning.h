// rc2dgi_tuning.h -- the tuning knobs (rc2dgi_set_tuning / rc2dgi_get_tuning, include/rc2dgi.h) as one table: the
// values, their keys and validity rules.  Free of HIP, so the knob contract is testable on a CPU
// (tests/sanitize/tuning_check.cpp).
#pragma once

#include <string>
#include <vector>

namespace rc2dgi {

// Every value a set_tuning key writes, with its default.  rc2dgi_ctx derives from it; the per-level vectors are sized
// (and defaulted) by the context's allocate().
struct Tuning {
  int strip_tables = 1;   // row-strip shards build the side tables of their own cell rows and exchange them
                          // (strip_tables_apply); 0: every shard builds them all
  int blur_path = 0;
  int poison = 0;         // 0xFF-fill intermediates before each frame
  int rc_skip = 1;        // march exit proofs 0 off, 1 auto (screens >= 2048), 2 interval only, 3 interval and screen edge
  int rc_wgproof = 1;     // workgroup-wide exit proof of the first samples
  int cascade_band = 1;   // band giRT1 / giRT2 where gi_band_apply allows (0: whole)
  int rc_fill = 1;        // levels no ray samples as per-block fills (0: their usual launch)
  int rc_rdiv = 1;        // exact reciprocal divisions on non-power-of-two cascades (0: IEEE divisions)
  int jfa_tab = 2;        // float-path texcoords 0 divided, 1 from tc, 2 by tc_rcp where exact (else from tc)
  int jfa_tail = 0;       // the last 2..4 steps in one kernel (k_jfa_tail; 0 off)
  int jfa_coset = 2;      // the first four (1) or five (2) steps in one kernel (k_jfa_coset)
  int shade_fused = 1;    // k_shade_cmin (records + bound table in one pass) where it applies
  int shade_split = 1;    // the records / palette pass split at the cells with hits
  int side_overlap = 2;   // k_dir_clear beside k_shade_cells -- 1: on the side stream (measured slower), 2: in its
                          // launch (default; 7 us less than 0)
  int jfa_lds = 0;        // LDS-staged taps for the short JumpFlood steps
  int jfa_rows = 0;       // consecutive rows per lane in the short steps (0 off, 4, 8)
  int jfa_rt = 1;         // rows per lane of the float-path steps on small screens (1, 2, 4)
  int rc_pal = 1;         // surface palettes on (where they apply: 4096^2 .. 8192^2 square screens)
  int rc_chain = 0;       // levels N-2 .. 0 in one launch (1; 2: unrolled march; 4: the top level too)
  int rc_chain_spin = 0;  // polls per wait (0 default; -1 diagnostic: all time out)
  int paint_plan = 0;     // the device painters' tile height and batch (paint_plan_code_ok; 0: by the screen size)
  std::vector<int> rc_variant;  // per level tile shape
  std::vector<int> rc_order;    // per level workgroup order px | py << 8 | dg << 16 (0 = tile-major)
  std::vector<int> rc_tail;     // per level: tail compaction after this many lockstep iterations
  std::vector<int> rc_mp;       // per level: directional miss proofs in the one-probe tiles
  std::vector<int> rc_noproof;  // per level: no bound table / exit proofs at this level
};

// rc_order code; mode: 0 patches, 1 oriented patches, 2 bands along the rays (rc_logical_order)
inline int order_code(int px, int py, int dg, int mode = 0) { return px | (py << 8) | (dg << 16) | (mode << 24); }

// paint_plan code: log2(tile_h) | (batch / 2048) << 8 with tile_h 4 .. 128 and batch 2048, 4096 or 8192 (0 is not a
// code: it asks for the plan the screen size gives, PaintDevPlan in rc2dgi_paint.h)
inline bool paint_plan_code_ok(int v) {
  const int th = v & 255, b = v >> 8;
  return v > 0 && th >= 2 && th <= 7 && (b == 1 || b == 2 || b == 4);
}

// the per-level vectors at N levels, every level at its default
void tuning_level_defaults(Tuning &t, int N);

// what the C ABI has to do on the device for a set (tuning_set's `effects`, or-ed)
enum TuningEffect : unsigned {
  kTuneSideStream = 1,   // side_overlap: value 1 needs the side stream and its fork / join events
  kTuneChain = 2,        // rc_chain: drain the stream before the value changes; 0 frees the chain
  kTuneAlloff = 4,       // rc_rdiv: the no-sample proofs (alloff) divide as the levels do -- prove them again
  kTuneSideBuffers = 8,  // prepare_side_buffers reads this knob
  kTunePaintPlan = 16,   // paint_plan: the plan must fit this screen; a changed plan drains the stream and frees the
                         // painters' working memory
};

// Set / get `key` on t (N levels; rc_variant takes 0 .. variant_count-1).  The only code that parses keys: a
// per-level key is "<name>_L<n>" with n all digits and below N.  false: *err holds the message, t is unchanged.
bool tuning_set(Tuning &t, int N, int variant_count, const char *key, int value, std::string *err, unsigned *effects);
bool tuning_get(const Tuning &t, int N, const char *key, int *value, std::string *err);

// the table's keys as the header documents them ("name", "name_L<n>")
std::vector<std::string> tuning_keys();

}  // namespace rc2dgi
