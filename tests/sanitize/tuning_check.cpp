// The tuning knobs' contract (include/rc2dgi.h, "tuning knobs") against csrc/rc2dgi_tuning.cpp, under ASan / UBSan
// (tests/test_sanitize_cpu.py).  The table below restates the header's comment -- default, range, refused values,
// whether any value is taken as value != 0 -- independently of the library's own table.  --list prints that
// table's keys.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rc2dgi_tuning.h"

using namespace rc2dgi;

namespace {

constexpr int kVariantCount = 26;  // ("rc_variant" takes 0 .. rc_variant_count-1; any count serves here)
enum Kind { SCALAR, LEVEL, LEVEL_ALL };  // "key" | "key_L<n>" | "key_L<n>" and "key" for every level (set-only)

struct Spec {
  const char *key;
  Kind kind;
  int def_low, def_high;  // default (per-level knobs: of levels 0..2, of levels >= 3)
  int lo, hi;
  std::vector<int> holes;  // values inside lo..hi that are refused
  bool norm;               // every value accepted, stored as value != 0
};

const int kPatch228 = 2 | 2 << 8 | 8 << 16;  // px | py << 8 | dg << 16

// "paint_plan": 0 or log2(tile_h) | (batch / 2048) << 8, tile_h 4 .. 128, batch 2048, 4096 or 8192 -- every other value
// between the smallest code and the largest is refused
std::vector<int> paint_plan_holes() {
  std::vector<int> holes;
  for (int v = 1; v < (7 | 4 << 8); ++v) {
    const int th = v & 255, b = v >> 8;
    if (!(th >= 2 && th <= 7 && (b == 1 || b == 2 || b == 4))) holes.push_back(v);
  }
  return holes;
}
const Spec kSpecs[] = {
    {"strip_tables", SCALAR, 1, 1, 0, 1, {}, true},
    {"rc_variant", LEVEL_ALL, 0, 13, 0, kVariantCount - 1, {}, false},
    {"blur_path", SCALAR, 0, 0, 0, 2, {}, false},
    {"poison", SCALAR, 0, 0, 0, 1, {}, true},
    {"rc_skip", SCALAR, 1, 1, 0, 3, {}, false},
    {"rc_wgproof", SCALAR, 1, 1, 0, 1, {}, true},
    {"cascade_band", SCALAR, 1, 1, 0, 1, {}, false},
    {"rc_fill", SCALAR, 1, 1, 0, 1, {}, false},
    {"rc_rdiv", SCALAR, 1, 1, 0, 1, {}, false},
    {"jfa_tab", SCALAR, 2, 2, 0, 2, {}, false},
    {"jfa_tail", SCALAR, 0, 0, 0, 4, {1}, false},
    {"jfa_coset", SCALAR, 2, 2, 0, 2, {}, false},
    {"shade_fused", SCALAR, 1, 1, 0, 1, {}, true},
    {"shade_split", SCALAR, 1, 1, 0, 1, {}, true},
    {"side_overlap", SCALAR, 2, 2, 0, 2, {}, false},
    {"jfa_lds", SCALAR, 0, 0, 0, 1, {}, true},
    {"jfa_rows", SCALAR, 0, 0, 0, 8, {1, 2, 3, 5, 6, 7}, false},
    {"jfa_rt", SCALAR, 1, 1, 1, 4, {3}, false},
    {"rc_mp", LEVEL_ALL, 1, 1, 0, 1, {}, true},
    {"rc_tail", LEVEL_ALL, 10, 10, -1, 32, {}, false},
    {"rc_pal", SCALAR, 1, 1, 0, 1, {}, true},
    {"rc_chain", SCALAR, 0, 0, 0, 4, {3}, false},
    {"rc_chain_spin", SCALAR, 0, 0, -1, INT_MAX, {}, false},
    {"paint_plan", SCALAR, 0, 0, 0, 7 | 4 << 8, paint_plan_holes(), false},
    {"rc_noproof", LEVEL, 0, 0, 0, 1, {}, true},
    {"rc_order", LEVEL, 0, kPatch228, 0, INT_MAX, {}, false},
};

int failures = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      ++failures;                             \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);               \
      std::printf("\n");                      \
    }                                         \
  } while (0)

bool set(Tuning &t, int N, const std::string &k, int v, unsigned *fx = nullptr) {
  std::string err;
  const bool ok = tuning_set(t, N, kVariantCount, k.c_str(), v, &err, fx);
  CHECK(ok == err.empty(), "%s = %d: result %d with message '%s'", k.c_str(), v, (int)ok, err.c_str());
  return ok;
}

bool get(const Tuning &t, int N, const std::string &k, int *v) {
  std::string err;
  const bool ok = tuning_get(t, N, k.c_str(), v, &err);
  CHECK(ok == err.empty(), "get %s: result %d with message '%s'", k.c_str(), (int)ok, err.c_str());
  return ok;
}

// every value the table can report, for "nothing changed" comparisons
std::vector<int> snapshot(const Tuning &t, int N) {
  std::vector<int> s;
  for (const Spec &sp : kSpecs)
    for (int L = 0; L < (sp.kind == SCALAR ? 1 : N); ++L) {
      int v = INT_MIN;
      get(t, N, sp.kind == SCALAR ? sp.key : std::string(sp.key) + "_L" + std::to_string(L), &v);
      s.push_back(v);
    }
  return s;
}

void refused(Tuning &t, int N, const std::string &k, int v) {
  const std::vector<int> before = snapshot(t, N);
  unsigned fx = 99;
  CHECK(!set(t, N, k, v, &fx), "%s = %d accepted (N = %d)", k.c_str(), v, N);
  CHECK(fx == 0, "%s = %d refused with effects %u", k.c_str(), v, fx);
  CHECK(snapshot(t, N) == before, "%s = %d refused but a value changed (N = %d)", k.c_str(), v, N);
}

void round_trip(Tuning &t, int N, const Spec &sp, const std::string &k, int v) {
  int got = INT_MIN;
  CHECK(set(t, N, k, v), "%s = %d refused (N = %d)", k.c_str(), v, N);
  const int want = sp.norm ? v != 0 : v;
  CHECK(get(t, N, k, &got) && got == want, "%s = %d reads back %d (N = %d)", k.c_str(), v, got, N);
}

void check_values(Tuning &t, int N, const Spec &sp, const std::string &k) {
  if (sp.norm) {
    for (int v : {0, 1, 7, -3, INT_MIN, INT_MAX}) round_trip(t, N, sp, k, v);
    return;
  }
  std::vector<int> ok = {sp.lo, sp.hi};
  for (int h : sp.holes) {  // the neighbours of a refused value are boundaries too
    refused(t, N, k, h);
    ok.push_back(h - 1);
    ok.push_back(h + 1);
  }
  for (int v : ok) {
    bool hole = v < sp.lo || v > sp.hi;
    for (int h : sp.holes) hole = hole || h == v;
    if (!hole) round_trip(t, N, sp, k, v);
  }
  refused(t, N, k, sp.lo - 1);
  if (sp.hi != INT_MAX) refused(t, N, k, sp.hi + 1);
}

void check(int N) {
  Tuning fresh;
  tuning_level_defaults(fresh, N);
  for (const Spec &sp : kSpecs) {
    Tuning t = fresh;
    const std::string key = sp.key;
    int v = INT_MIN;
    if (sp.kind == SCALAR) {
      CHECK(get(t, N, key, &v) && v == sp.def_low, "%s: default %d", sp.key, v);
      check_values(t, N, sp, key);
      for (const char *sfx : {"_L0", "_L", "x", "_"}) {
        refused(t, N, key + sfx, sp.lo);
        CHECK(!get(t, N, key + sfx, &v), "get %s%s answered", sp.key, sfx);
      }
      continue;
    }
    for (int L = 0; L < N; ++L) {
      const std::string k = key + "_L" + std::to_string(L);
      CHECK(get(t, N, k, &v) && v == (L >= 3 ? sp.def_high : sp.def_low), "%s: default %d", k.c_str(), v);
    }
    check_values(t, N, sp, key + "_L0");
    check_values(t, N, sp, key + "_L" + std::to_string(N - 1));
    for (const std::string &sfx : {"_L" + std::to_string(N), std::string("_L-1"), std::string("_L"), std::string("_Lx"),
                                   std::string("_L1x"), std::string("_L0 "), std::string("_L+0"),
                                   std::string("_L99999999999999999999")}) {
      refused(t, N, key + sfx, sp.lo);
      CHECK(!get(t, N, key + sfx, &v), "get %s%s answered (N = %d)", sp.key, sfx.c_str(), N);
    }
    CHECK(!get(t, N, key, &v), "get %s answered: the every-level form is set-only", sp.key);
    if (sp.kind == LEVEL) {
      refused(t, N, key, sp.lo);
      continue;
    }
    t = fresh;
    const int all = sp.norm ? 0 : sp.hi;  // (differs from the default of every level)
    CHECK(set(t, N, key, all), "%s = %d refused", sp.key, all);
    for (int L = 0; L < N; ++L)
      CHECK(get(t, N, key + "_L" + std::to_string(L), &v) && v == all, "%s = %d left level %d at %d", sp.key, all, L, v);
    if (!sp.norm) refused(t, N, key, sp.lo - 1);
  }
  Tuning t = fresh;
  for (const char *k : {"", "_L0", "rc", "rc_variant_count", "rc_fill_levels", "RC_SKIP", "rc_skip ", "nonesuch"}) {
    int v;
    refused(t, N, k, 0);
    CHECK(!get(t, N, k, &v), "get '%s' answered", k);
  }
  // "paint_plan": a code with bits above its two fields is no code
  for (int v : {2 | 1 << 8 | 1 << 16, 2 | 256 << 8, 3 | 1 << 8 | 1 << 30, INT_MAX, INT_MIN}) refused(t, N, "paint_plan", v);
  // what the C ABI must do on the device after a set
  const struct {
    const char *key;
    int value;
    unsigned effects;
  } fx[] = {{"rc_chain", 1, kTuneChain | kTuneSideBuffers}, {"rc_chain", 0, kTuneChain | kTuneSideBuffers},
            {"rc_rdiv", 0, kTuneAlloff},                    {"side_overlap", 1, kTuneSideStream},
            {"rc_pal", 0, kTuneSideBuffers},                {"rc_variant", 1, kTuneSideBuffers},
            {"rc_variant_L0", 1, kTuneSideBuffers},         {"blur_path", 1, 0},
            {"rc_order_L0", 1, 0},                          {"rc_chain_spin", 5, 0},
            {"paint_plan", 3 | 2 << 8, kTunePaintPlan},     {"paint_plan", 0, kTunePaintPlan}};
  for (const auto &e : fx) {
    unsigned got = 99;
    CHECK(set(t, N, e.key, e.value, &got) && got == e.effects, "%s: effects %u, expected %u", e.key, got, e.effects);
  }
}

}  // namespace

int main(int argc, char **argv) {
  if (argc > 1 && !std::strcmp(argv[1], "--list")) {
    for (const std::string &k : tuning_keys()) std::printf("%s\n", k.c_str());
    return 0;
  }
  // the restatement and the table name the same keys
  std::vector<std::string> mine;
  for (const Spec &sp : kSpecs) {
    if (sp.kind != LEVEL) mine.push_back(sp.key);
    if (sp.kind != SCALAR) mine.push_back(std::string(sp.key) + "_L<n>");
  }
  std::vector<std::string> theirs = tuning_keys();
  std::sort(mine.begin(), mine.end());
  std::sort(theirs.begin(), theirs.end());
  CHECK(mine == theirs, "the table's keys differ from the header's");
  for (int N : {1, 2, 15}) check(N);
  std::printf("%s\n", failures ? "tuning_check: FAILED" : "tuning_check: ok");
  return failures ? 1 : 0;
}
