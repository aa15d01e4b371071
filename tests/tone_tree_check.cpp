// tone_tree_check.cpp -- host program for tests/test_tone_cpu.py: the level-order search tree of an edge table
// (csrc/rc2dgi_tone.h: tree_levels, tree_layout) descended as the kernels descend it, k = 2k + (T[k] <= v), against the
// linear scan of the header, for tables of every size around the powers of two up to 1023 edges -- random bit patterns,
// clustered values, repeats, +-inf, -0.0 beside +0.0 -- on the values within 2 bit patterns of every edge, on random
// bit patterns and on +-0, +-inf, the smallest subnormals and +-FLT_MAX.  Prints "checked N bad M"; exit status 1 when
// M != 0.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "rc2dgi_tone.h"

using namespace rc2dgi;

static int scan(const std::vector<float> &e, float v) {
  int n = 0;
  for (float x : e) n += x <= v ? 1 : 0;
  return n;
}

static int descend(const std::vector<float> &T, int levels, float v) {
  unsigned k = 1;
  for (int l = 0; l < levels; ++l) k = 2u * k + (T[k] <= v ? 1u : 0u);
  return (int)(k - (1u << levels));
}

static float from_bits(uint32_t b) {
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}

int main() {
  std::mt19937 rng(3);
  long bad = 0, total = 0;
  const int sizes[] = {1, 2, 3, 4, 7, 8, 9, 254, 255, 256, 511, 512, 1022, 1023};
  for (int m : sizes)
    for (int rep = 0; rep < 6; ++rep) {
      std::vector<float> e((size_t)m);
      for (float &x : e) {
        uint32_t b = rng();
        if (rep % 3 == 0) b = (b & 0x80000000u) | (0x3F000000u + (b & 0xFFFFFu));  // clustered around +-0.5 .. 0.53
        const float f = from_bits(b);
        x = f != f ? 0.0f : f;
      }
      if (rep & 1) {  // repeats, infinite ends, the two zeros side by side
        for (int i = 0; i < m; i += 3) e[(size_t)i] = e[(size_t)((i + 1) % m)];
        e[0] = -INFINITY;
        e[(size_t)m - 1] = INFINITY;
        if (m > 3) {
          e[1] = -0.0f;
          e[2] = 0.0f;
        }
      }
      std::sort(e.begin(), e.end());
      const int levels = tree_levels(m);
      if ((1 << levels) - 1 < m || (levels > 1 && (1 << (levels - 1)) - 1 >= m)) ++bad;
      std::vector<float> T((size_t)1 << levels);
      tree_layout(e.data(), m, levels, NAN, T.data());
      std::vector<float> vals;
      for (float x : e) {
        uint32_t b;
        std::memcpy(&b, &x, 4);
        for (int d = -2; d <= 2; ++d) {
          const float f = from_bits(b + (uint32_t)d);
          if (f == f) vals.push_back(f);
        }
      }
      for (int i = 0; i < 20000; ++i) {
        const float f = from_bits((uint32_t)rng());
        if (f == f) vals.push_back(f);
      }
      const float special[] = {0.0f, -0.0f, INFINITY, -INFINITY, 1e-45f, -1e-45f, 3.4028235e38f, -3.4028235e38f};
      for (float f : special) vals.push_back(f);
      for (float v : vals) {
        ++total;
        if (scan(e, v) != descend(T, levels, v)) ++bad;
      }
      if (descend(T, levels, NAN) != 0) ++bad;  // a NaN fails every comparison
    }
  std::printf("checked %ld bad %ld\n", total, bad);
  return bad != 0;
}
