// gradients_interp_check.cpp -- host check of k_gradients_raster's "which triangle" walk and interpolation
// (csrc/rc2dgi_gradient_interp.h), a stand-alone program built by tests/test_gradients_cpu.py with
// -fsanitize=address,undefined and -ffp-contract=off.  3000 pseudo-random shapes of two overlapping snapped triangles
// -- a third small, a third across the target, a third with two vertices near +-2^21 pixels and an edge through the
// target -- are set up as paint_dev_emit_t<true> sets them up (rc2dgi_paint_setup.h: the zero-area drop, the
// counter-clockwise swap, the colours tagged in listed order) and walked over pixel centres of a 32768 x 4 strip with
// the header's own functions.  At every covered centre: A = E_0 + E_1 + E_2 is positive and is twice the triangle's
// area (the same everywhere; UBSan watches the sums), the weights are finite, equal colours come back as q0 exactly,
// the triangle returned is the first that covers in listed order, and the colour lies within 2^-20 of the float64
// barycentric interpolation of the listed vertices' colours (sixteen half-ulps of 1.0: two conversions and a division
// a weight, two differences, two products and two sums a channel, all of magnitude at most about 1).  Exit 1 on any
// miss.  `--wrong` tags the colours after the swap instead of before it (the mistake the check exists to catch) and
// must make the program exit 1.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "rc2dgi_gradient_interp.h"

namespace {

struct Edge {
  int a, b;
  long long c;
};
struct Tri {
  Edge e[3];
  unsigned incl;
  unsigned pad[3];
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

// paint_dev_emit_t<true>: false for a zero area; otherwise counter-clockwise, the three edges, the incl bits, the tags
bool setup(Snap s0, Snap s1, Snap s2, unsigned q0, unsigned q1, unsigned q2, bool wrong, Tri &t, bool &swapped) {
  const long long area = (s1.x - s0.x) * (s2.y - s0.y) - (s2.x - s0.x) * (s1.y - s0.y);
  if (area == 0) return false;
  swapped = area < 0;
  if (swapped) std::swap(s1, s2);
  const Snap s[3] = {s0, s1, s2};
  t = Tri{};
  for (int e = 0; e < 3; ++e) {
    const Snap a = s[e], b = s[(e + 1) % 3];
    const long long dx = b.x - a.x, dy = b.y - a.y;
    t.e[e].a = (int)(-dy);
    t.e[e].b = (int)dx;
    t.e[e].c = dy * a.x - dx * a.y;
    if (dy < 0 || (dy == 0 && dx > 0)) t.incl |= 1u << e;
  }
  // --wrong: q0, q1, q2 go to the record's vertices as the swap left them, so q1 lands on the listed R2
  rc2dgi::grad_tag(t, wrong ? false : swapped, q0, q1, q2);
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

// twice the signed area of (a, b, p), in float64 from exact integers below 2^63 (an independent statement)
double cross(Snap a, Snap b, double px, double py) {
  return ((double)b.x - (double)a.x) * (py - (double)a.y) - ((double)b.y - (double)a.y) * (px - (double)a.x);
}

}  // namespace

int main(int argc, char **argv) {
  const bool wrong = argc > 1 && std::strcmp(argv[1], "--wrong") == 0;
  const int W = 32768, H = 4, N = 3000;
  const long long FAR = (1LL << 21) * 256;  // 2^21 pixels in 1/256 pixel
  long long centres = 0, covered_n = 0, swapped_n = 0, second_n = 0, bad = 0;
  double worst = 0.0;
  for (int k = 0; k < N; ++k) {
    Snap s[3];
    if (k % 3 == 0) {  // small: a few pixels to a few tens, anywhere along the strip
      const long long cx = uniform(-20 * 256, (W + 20) * 256LL), cy = uniform(-20 * 256, (H + 20) * 256);
      const long long r = uniform(1, 30 * 256);
      for (Snap &v : s) v = Snap{cx + uniform(-r, r), cy + uniform(-r, r)};
    } else if (k % 3 == 1) {  // across the strip
      for (Snap &v : s) v = Snap{uniform(-40 * 256, (W + 40) * 256LL), uniform(-400 * 256, (H + 400) * 256)};
    } else {  // two vertices near +-2^21 pixels on a line through a point of the target, the third near or far
      const long long px = uniform(0, W * 256LL), py = uniform(0, H * 256);
      const long long dx = uniform(-1000, 1000), dy = uniform(-1000, 1000);
      const long long m = std::max<long long>(1, std::max(dx < 0 ? -dx : dx, dy < 0 ? -dy : dy));
      const long long L0 = (FAR - (1LL << 24)) / m, L1 = uniform(L0 / 2, L0);
      s[0] = Snap{px + dx * L0, py + dy * L0};
      s[1] = Snap{px - dx * L1, py - dy * L1};
      s[2] = Snap{uniform(-FAR + (1 << 16), FAR - (1 << 16)), uniform(-FAR + (1 << 16), FAR - (1 << 16))};
      if (k % 2 == 0) s[2] = Snap{px + uniform(-300000, 300000), py + uniform(-300000, 300000)};
    }
    // the shape: the triangle and a second one that overlaps it (its third vertex moved), each with colours of its own
    Snap v[2][3] = {{s[0], s[1], s[2]}, {s[0], s[1], Snap{s[2].x + uniform(-2000, 2000), s[2].y + uniform(-2000, 2000)}}};
    unsigned q[2][3];
    for (auto &qq : q)
      for (unsigned &c : qq) c = (unsigned)rnd();
    Tri tris[2];
    int listed[2];  // slot -> index in listed order (a dropped triangle leaves no slot)
    Snap vs[2][3];
    bool sw[2] = {false, false};
    int nt = 0;
    long long mnx = LLONG_MAX, mny = LLONG_MAX, mxx = LLONG_MIN, mxy = LLONG_MIN;
    for (int t = 0; t < 2; ++t) {
      if (!setup(v[t][0], v[t][1], v[t][2], q[t][0], q[t][1], q[t][2], wrong, tris[nt], sw[nt])) continue;
      listed[nt] = t;
      for (int i = 0; i < 3; ++i) {
        vs[nt][i] = v[t][i];
        mnx = std::min(mnx, v[t][i].x); mxx = std::max(mxx, v[t][i].x);
        mny = std::min(mny, v[t][i].y); mxy = std::max(mxy, v[t][i].y);
      }
      ++nt;
    }
    if (nt == 0) continue;
    const int x0 = (int)std::max(0LL, -floor_div(-(mnx - 128), 256)), x1 = (int)std::min((long long)W - 1, floor_div(mxx - 128, 256));
    const int y0 = (int)std::max(0LL, -floor_div(-(mny - 128), 256)), y1 = (int)std::min((long long)H - 1, floor_div(mxy - 128, 256));
    if (x0 > x1 || y0 > y1) continue;
    const int step = std::max(1, (x1 - x0 + 1) / 512);
    for (int j = y0; j <= y1; ++j)
      for (int i = x0 + (int)uniform(0, step - 1); i <= x1; i += step) {
        const long long X = 256LL * i + 128, Y = 256LL * j + 128;
        ++centres;
        long long E[3];
        const int t = rc2dgi::grad_first_covering(tris, nt, X, Y, E);
        int first = -1;
        for (int u = 0; u < nt && first < 0; ++u)
          if (covered(tris[u], X, Y)) first = u;
        if (t != first) {
          if (bad++ < 5) std::printf("WRONG: shape %d centre (%d, %d): triangle %d returned, %d covers first\n", k, i, j, t, first);
          continue;
        }
        if (t < 0) continue;
        ++covered_n;
        if (sw[t]) ++swapped_n;
        if (listed[t] == 1) ++second_n;
        const Snap *R = vs[t];
        const long long A = E[0] + E[1] + E[2];
        long long area2 = (R[1].x - R[0].x) * (R[2].y - R[0].y) - (R[2].x - R[0].x) * (R[1].y - R[0].y);
        if (area2 < 0) area2 = -area2;
        float w1, w2;
        rc2dgi::grad_weights(E, w1, w2);
        bool ok = A > 0 && A == area2 && E[0] >= 0 && E[1] >= 0 && E[2] >= 0 && std::isfinite(w1) && std::isfinite(w2);
        // equal colours: q0 exactly
        Tri eq = tris[t];
        eq.pad[1] = eq.pad[2] = eq.pad[0];
        float flat[4], src[4];
        rc2dgi::grad_colour(eq, E, 1.0f, flat);
        for (int ch = 0; ch < 4; ++ch) ok = ok && flat[ch] == rc2dgi::grad_unorm(eq.pad[0], ch);
        // the colours of the listed vertices, interpolated in float64 with weights from the vertices themselves
        rc2dgi::grad_colour(tris[t], E, 1.0f, src);
        const double sgn = cross(R[0], R[1], (double)R[2].x, (double)R[2].y) < 0 ? -1.0 : 1.0;
        const double b0 = sgn * cross(R[1], R[2], (double)X, (double)Y), b1 = sgn * cross(R[2], R[0], (double)X, (double)Y),
                     b2 = sgn * cross(R[0], R[1], (double)X, (double)Y), bs = b0 + b1 + b2;
        const unsigned *qq = q[listed[t]];
        for (int ch = 0; ch < 4; ++ch) {
          const double c0 = ((qq[0] >> (8 * ch)) & 255u) / 255.0, c1 = ((qq[1] >> (8 * ch)) & 255u) / 255.0,
                       c2 = ((qq[2] >> (8 * ch)) & 255u) / 255.0;
          const double want = (b0 * c0 + b1 * c1 + b2 * c2) / bs, err = std::fabs((double)src[ch] - want);
          worst = std::max(worst, err);
          ok = ok && err < 0x1p-20;
        }
        if (!ok && bad++ < 5)
          std::printf("WRONG: shape %d centre (%d, %d) triangle %d%s: A %lld (area %lld) w1 %g w2 %g\n", k, i, j, listed[t],
                      sw[t] ? " (swapped)" : "", A, area2, (double)w1, (double)w2);
      }
  }
  std::printf("centres walked %lld, covered %lld (in a swapped triangle %lld, by the second triangle %lld), worst error "
              "%.3g, wrong %lld\n", centres, covered_n, swapped_n, second_n, worst, bad);
  return bad != 0 || covered_n < 100000 || swapped_n < covered_n / 8 || second_n == 0 ? 1 : 0;
}
