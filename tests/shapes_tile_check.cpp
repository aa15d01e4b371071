// shapes_tile_check.cpp -- host check of k_shapes_bin's tile rejection (csrc/rc2dgi_tile_test.h), a stand-alone program
// built by tests/test_shapes_cpu.py with -fsanitize=address,undefined.  20000 pseudo-random snapped triangles -- a third
// small, a third across the target, a third with two vertices near +-2^21 pixels and an edge through the target -- are
// set up as paint_dev_emit sets them up (rc2dgi_paint_setup.h), binned on a 160 x 136 target with tiles of 64 x 4 and
// of 64 x 128 (partial tiles on both axes), and every tile the header's test rejects is walked centre by centre with
// the raster's coverage rule.  Exit 1 if a rejected tile holds a covered centre.  `--flip` takes the opposite corner in
// the test (the mistake the check exists to catch) and must make the program exit 1.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rc2dgi_tile_test.h"

namespace {

struct Edge {
  int a, b;
  long long c;
};
struct Tri {
  Edge e[3];
  unsigned incl;
};
struct Snap {
  long long x, y;
};

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
long long uniform(long long lo, long long hi) { return lo + (long long)(rnd() % (uint64_t)(hi - lo + 1)); }

long long floor_div(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// paint_dev_emit: false for a zero area; otherwise counter-clockwise, the three edges and the incl bits
bool setup(Snap s0, Snap s1, Snap s2, Tri &t) {
  const long long area = (s1.x - s0.x) * (s2.y - s0.y) - (s2.x - s0.x) * (s1.y - s0.y);
  if (area == 0) return false;
  if (area < 0) std::swap(s1, s2);
  const Snap s[3] = {s0, s1, s2};
  t.incl = 0;
  for (int e = 0; e < 3; ++e) {
    const Snap a = s[e], b = s[(e + 1) % 3];
    const long long dx = b.x - a.x, dy = b.y - a.y;
    t.e[e].a = (int)(-dy);
    t.e[e].b = (int)dx;
    t.e[e].c = dy * a.x - dx * a.y;
    if (dy < 0 || (dy == 0 && dx > 0)) t.incl |= 1u << e;
  }
  return true;
}

// paint_covered on one triangle
bool covered(const Tri &t, long long X, long long Y) {
  bool ok = true;
  for (int e = 0; e < 3; ++e) {
    const long long E = (long long)t.e[e].a * X + (long long)t.e[e].b * Y + t.e[e].c;
    ok = ok && (E > 0 || (E == 0 && ((t.incl >> e) & 1u)));
  }
  return ok;
}

// the header's test with the corner choice reversed: what a wrong sign in the kernel would compute
bool tri_out_flipped(const Tri &t, long long X0, long long Y0, long long X1, long long Y1) {
  bool out = false;
  for (int e = 0; e < 3; ++e) {
    const long long E = (long long)t.e[e].a * (t.e[e].a >= 0 ? X0 : X1) +
                        (long long)t.e[e].b * (t.e[e].b >= 0 ? Y0 : Y1) + t.e[e].c;
    out = out || E < 0 || (E == 0 && !((t.incl >> e) & 1u));
  }
  return out;
}

}  // namespace

int main(int argc, char **argv) {
  const bool flip = argc > 1 && std::strcmp(argv[1], "--flip") == 0;
  const int W = 160, H = 136, N = 20000;
  const long long FAR = (1LL << 21) * 256;  // 2^21 pixels in 1/256 pixel
  long long tiles = 0, kept = 0, kept_empty = 0, wrong = 0, drawn = 0;
  std::vector<unsigned char> cov((size_t)W * H);
  for (int k = 0; k < N; ++k) {
    Snap s[3];
    if (k % 3 == 0) {  // small: a few pixels to a few tens, anywhere around the target
      const long long cx = uniform(-20 * 256, (W + 20) * 256), cy = uniform(-20 * 256, (H + 20) * 256);
      const long long r = uniform(1, 30 * 256);
      for (Snap &v : s) v = Snap{cx + uniform(-r, r), cy + uniform(-r, r)};
    } else if (k % 3 == 1) {  // across the target; every fourth one a sliver
      for (Snap &v : s) v = Snap{uniform(-40 * 256, (W + 40) * 256), uniform(-40 * 256, (H + 40) * 256)};
      if (k % 4 == 0) s[2] = Snap{(s[0].x + s[1].x) / 2 + uniform(-200, 200), (s[0].y + s[1].y) / 2 + uniform(-200, 200)};
    } else {  // two vertices near +-2^21 pixels on a line through a point of the target, the third anywhere that far
      const long long px = uniform(0, W * 256), py = uniform(0, H * 256);
      const long long dx = uniform(-1000, 1000), dy = uniform(-1000, 1000);
      const long long m = std::max<long long>(1, std::max(dx < 0 ? -dx : dx, dy < 0 ? -dy : dy));
      const long long L0 = (FAR - (1 << 16)) / m, L1 = uniform(L0 / 2, L0);
      s[0] = Snap{px + dx * L0, py + dy * L0};
      s[1] = Snap{px - dx * L1, py - dy * L1};
      s[2] = Snap{uniform(-FAR + (1 << 16), FAR - (1 << 16)), uniform(-FAR + (1 << 16), FAR - (1 << 16))};
      if (k % 2 == 0) s[2] = Snap{px + uniform(-3000, 3000), py + uniform(-3000, 3000)};
    }
    Tri t;
    if (!setup(s[0], s[1], s[2], t)) continue;
    long long mnx = LLONG_MAX, mny = LLONG_MAX, mxx = LLONG_MIN, mxy = LLONG_MIN;
    for (const Snap &v : s) {
      mnx = std::min(mnx, v.x); mxx = std::max(mxx, v.x);
      mny = std::min(mny, v.y); mxy = std::max(mxy, v.y);
    }
    const int x0 = (int)std::max(0LL, -floor_div(-(mnx - 128), 256)), x1 = (int)std::min((long long)W - 1, floor_div(mxx - 128, 256));
    const int y0 = (int)std::max(0LL, -floor_div(-(mny - 128), 256)), y1 = (int)std::min((long long)H - 1, floor_div(mxy - 128, 256));
    if (x0 > x1 || y0 > y1) continue;
    ++drawn;
    for (int j = y0; j <= y1; ++j)
      for (int i = x0; i <= x1; ++i) cov[(size_t)j * W + i] = covered(t, 256LL * i + 128, 256LL * j + 128);
    for (int th_shift : {2, 7}) {
      for (int ty = y0 >> th_shift; ty <= (y1 >> th_shift); ++ty)
        for (int tx = x0 >> 6; tx <= (x1 >> 6); ++tx) {
          const int i0 = std::max(tx << 6, x0), i1 = std::min((tx << 6) + 63, x1);
          const int j0 = std::max(ty << th_shift, y0), j1 = std::min(((ty + 1) << th_shift) - 1, y1);
          const long long X0 = 256LL * i0 + 128, X1 = 256LL * i1 + 128, Y0 = 256LL * j0 + 128, Y1 = 256LL * j1 + 128;
          const bool out = flip ? tri_out_flipped(t, X0, Y0, X1, Y1) : rc2dgi::paint_tri_out(t, X0, Y0, X1, Y1);
          bool any = false;
          for (int j = j0; j <= j1 && !any; ++j)
            for (int i = i0; i <= i1 && !any; ++i) any = cov[(size_t)j * W + i] != 0;
          ++tiles;
          if (!out) ++kept;
          if (!out && !any) ++kept_empty;
          if (out && any) {
            if (wrong++ < 5)
              std::printf("WRONG: triangle %d, tile (%d, %d) of 64 x %d rejected with a covered centre\n", k, tx, ty,
                          1 << th_shift);
          }
        }
    }
  }
  std::printf("triangles drawn %lld, tiles in their boxes %lld, kept %lld (of them empty %lld), wrongly rejected %lld\n",
              drawn, tiles, kept, kept_empty, wrong);
  return wrong != 0 || drawn < N / 4 ? 1 : 0;
}
