// rc2dgi_tuning.cpp -- the knob table and the two functions that read it (rc2dgi_tuning.h)
#include "rc2dgi_tuning.h"

#include <climits>
#include <cstring>

namespace rc2dgi {
namespace {

enum Kind { kScalar, kLevel, kLevelAll };  // "key" | "key_L<n>" only | "key_L<n>" and "key" (set-only: every level)

struct Knob {
  const char *key;
  Kind kind;
  int Tuning::*scalar;
  std::vector<int> Tuning::*levels;
  int lo, hi;      // accepted range (hi kVariants: variant_count - 1)
  unsigned holes;  // bit v: value v of the range is refused all the same
  bool norm;       // any value, stored as value != 0
  const char *msg;  // the range error
  unsigned effects;
  bool (*valid)(int) = nullptr;  // non-null: the values accepted besides 0, instead of the range
};

constexpr int kVariants = INT_MIN;
constexpr unsigned bit(int v) { return 1u << v; }
#ifdef RC2DGI_DIAG_CHAIN_TIGHT
constexpr unsigned kChainHoles = 0;  // (3: the timing-only in-block window)
#else
constexpr unsigned kChainHoles = bit(3);
#endif

#define S(name) #name, kScalar, &Tuning::name, nullptr
#define L(name, kind) #name, kind, nullptr, &Tuning::name
const Knob kKnobs[] = {
    {S(strip_tables), 0, 0, 0, true, "", kTuneSideBuffers},
    {L(rc_variant, kLevelAll), 0, kVariants, 0, false, "rc_variant out of range", kTuneSideBuffers},
    {S(blur_path), 0, 2, 0, false, "blur_path out of range", 0},
    {S(poison), 0, 0, 0, true, "", 0},
    {S(rc_skip), 0, 3, 0, false, "rc_skip is 0..3", kTuneSideBuffers},
    {S(rc_wgproof), 0, 0, 0, true, "", 0},
    {S(cascade_band), 0, 1, 0, false, "cascade_band is 0 or 1", 0},
    {S(rc_fill), 0, 1, 0, false, "rc_fill is 0 or 1", 0},
    {S(rc_rdiv), 0, 1, 0, false, "rc_rdiv is 0 or 1", kTuneAlloff},
    {S(jfa_tab), 0, 2, 0, false, "jfa_tab is 0, 1 or 2", 0},
    {S(jfa_tail), 0, 4, bit(1), false, "jfa_tail is 0 (off) or 2..4 steps", kTuneSideBuffers},
    {S(jfa_coset), 0, 2, 0, false, "jfa_coset is 0 (off), 1 (4 steps), 2 (5 steps)", 0},
    {S(shade_fused), 0, 0, 0, true, "", kTuneSideBuffers},
    {S(shade_split), 0, 0, 0, true, "", 0},
    {S(side_overlap), 0, 2, 0, false, "side_overlap is 0 (off), 1 (side stream), 2 (merged into k_shade_cells)",
     kTuneSideStream},
    {S(jfa_lds), 0, 0, 0, true, "", 0},
    {S(jfa_rows), 0, 8, 0xFFu & ~(bit(0) | bit(4)), false, "jfa_rows is 0, 4 or 8", 0},
    {S(jfa_rt), 1, 4, bit(3), false, "jfa_rt is 1, 2 or 4", 0},
    {L(rc_mp, kLevelAll), 0, 0, 0, true, "", 0},
    {L(rc_tail, kLevelAll), -1, 32, 0, false, "rc_tail is -1 (queue every ray) .. 0 (off) .. 32 lockstep iterations", 0},
    {S(rc_pal), 0, 0, 0, true, "", kTuneSideBuffers},
    {S(rc_chain), 0, 4, kChainHoles, false, "rc_chain is 0 (off), 1 (chain), 2 (unrolled march), 4 (with the top level)",
     kTuneChain | kTuneSideBuffers},
    {S(rc_chain_spin), -1, INT_MAX, 0, false, "rc_chain_spin is -1, 0 or a poll count", 0},
    {S(paint_plan), 0, 0, 0, false, "paint_plan is 0 or log2(tile_h) 2..7 | (batch / 2048 = 1, 2 or 4) << 8",
     kTunePaintPlan, paint_plan_code_ok},
    {L(rc_noproof, kLevel), 0, 0, 0, true, "", 0},
    {L(rc_order, kLevel), 0, INT_MAX, 0, false, "rc_order is px | py << 8 | dg << 16", 0},
};
#undef S
#undef L

// key -> its knob; *level: -1 for "name", n for "name_L<n>" (n all digits; saturates far above any level count)
const Knob *find_knob(const char *key, int *level) {
  const std::string k(key ? key : "");
  for (const Knob &d : kKnobs) {
    const size_t n = std::strlen(d.key);
    if (k.compare(0, n, d.key) != 0) continue;
    if (k.size() == n) {
      if (d.kind == kLevel) continue;
      *level = -1;
      return &d;
    }
    if (d.kind == kScalar || k.compare(n, 2, "_L") != 0 || k.size() == n + 2) continue;
    int v = 0;
    size_t i = n + 2;
    for (; i < k.size() && k[i] >= '0' && k[i] <= '9'; ++i) v = v < (1 << 20) ? v * 10 + (k[i] - '0') : v;
    if (i != k.size()) continue;
    *level = v;
    return &d;
  }
  return nullptr;
}

// a per-level key's level lies within the N levels (and the vector, which a context sizes to N)
bool level_ok(const Tuning &t, const Knob &d, int level, int N) {
  return level < 0 || (level < N && level < (int)(t.*(d.levels)).size());
}

bool refuse(std::string *err, const std::string &msg) {
  if (err) *err = msg;
  return false;
}

// measured default tile shape per level (profiles/, bench.py --sweep-rc): from level 3 up the
// gather-bound levels prefer the fully unrolled march ("16x16x1u")
int default_rc_variant(int level) { return level >= 3 ? 13 : 0; }

// default workgroup order per level (scripts/sweep_rc_order.py, profiles/r01/rc_order_*.json):
// from level 3 up, patches of 2 x 2 tiles x 8 direction blocks keep the distance-field
// footprint of an XCD's resident workgroups closer to its L2; below, tile-major
int default_rc_order(int level) { return level >= 3 ? order_code(2, 2, 8) : 0; }

// tail compaction default: rays still marching after kDefaultTail lockstep iterations finish one per lane
constexpr int kDefaultTail = 10;

}  // namespace

void tuning_level_defaults(Tuning &t, int N) {
  t.rc_variant.resize(N);
  t.rc_order.resize(N);
  for (int L = 0; L < N; ++L) {
    t.rc_variant[L] = default_rc_variant(L);
    t.rc_order[L] = default_rc_order(L);
  }
  t.rc_tail.assign(N, kDefaultTail);
  t.rc_mp.assign(N, 1);  // directional miss proofs wherever they apply (one-probe tiles, 4^L >= kDirBins)
  t.rc_noproof.assign(N, 0);
}

bool tuning_set(Tuning &t, int N, int variant_count, const char *key, int value, std::string *err, unsigned *effects) {
  if (effects) *effects = 0;
  int level = -1;
  const Knob *d = find_knob(key, &level);
  if (!d) return refuse(err, std::string("unknown tuning key ") + (key ? key : ""));
  if (d->valid) {
    if (value != 0 && !d->valid(value)) return refuse(err, d->msg);
  } else if (!d->norm) {
    const int hi = d->hi == kVariants ? variant_count - 1 : d->hi;
    if (value < d->lo || value > hi || (value >= 0 && value < 32 && (d->holes >> value & 1))) return refuse(err, d->msg);
  }
  if (!level_ok(t, *d, level, N)) return refuse(err, "level out of range");
  const int v = d->norm ? value != 0 : value;
  if (d->scalar) {
    t.*(d->scalar) = v;
  } else if (level < 0) {
    for (int &x : t.*(d->levels)) x = v;
  } else {
    (t.*(d->levels))[level] = v;
  }
  if (effects) *effects = d->effects;
  return true;
}

bool tuning_get(const Tuning &t, int N, const char *key, int *value, std::string *err) {
  int level = -1;
  const Knob *d = find_knob(key, &level);
  if (!d || (!d->scalar && level < 0))  // (the broadcast forms are set-only)
    return refuse(err, std::string("unknown tuning key ") + (key ? key : ""));
  if (!level_ok(t, *d, level, N)) return refuse(err, "level out of range");
  *value = d->scalar ? t.*(d->scalar) : (t.*(d->levels))[level];
  return true;
}

std::vector<std::string> tuning_keys() {
  std::vector<std::string> keys;
  for (const Knob &d : kKnobs) {
    if (d.kind != kLevel) keys.push_back(d.key);
    if (d.kind != kScalar) keys.push_back(std::string(d.key) + "_L<n>");
  }
  return keys;
}

}  // namespace rc2dgi
