// rects_check.cpp -- TEST INFRASTRUCTURE.  The host's planning of the rectangle calls and of a view's geometry
// (csrc/rc2dgi_rectplan.cpp with the cut of csrc/rc2dgi_rects.h, which the kernels evaluate too) built with
// AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_sanitize_cpu.py).  Besides running clean it checks, with
// arithmetic of its own, what k_reduce_rows, k_reduce_bands, k_hist and the callers rest on:
//   - bands and blocks tile [0, h) once, in order, only the last one short, at most 4096 of them;
//   - a band is a power of two of rows and whole passes of 64 / lanes-a-row rows, a block whole passes of 256 / lanes;
//   - w * h and the row bounds stay inside int at 32768-texel axes;
//   - a batch holds at most 65536 items, a join's partials lie inside its batch and are numbered from 0, the bands of
//     a rectangle share a batch (the blocks of a histogram need not);
//   - an invalid rectangle is one w == 0 item of its record;
//   - the uploaded items are those the device derives from the inline descriptors of the same rectangles;
//   - rc2dgi_read's staged block is 1 .. h rows that fit the buffer, as many as do;
//   - a view's clip is view n window and its blit interior that minus the border, pixel by pixel.
#include <climits>
#include <cstdio>
#include <vector>

#include "rc2dgi_rectplan.h"

using namespace rc2dgi;

static int fails = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      if (fails < 50) {                  \
        std::printf("FAIL: " __VA_ARGS__); \
        std::printf("\n");               \
      }                                  \
      ++fails;                           \
    }                                    \
  } while (0)

static bool pow2(long long v) { return v > 0 && (v & (v - 1)) == 0; }

// lanes that hold a row of w texels, four a lane: the power of two >= w / 4 (k_reduce_rows, k_hist)
static int lanes_a_row(int w) {
  const int need = (w + 3) / 4;
  int lr = 1;
  while (lr < need) lr *= 2;
  return lr;
}

static bool valid_ref(const rc2dgi_rect &r, int tw, int th) {
  const long long x = r.x, y = r.y, w = r.w, h = r.h;
  return w > 0 && h > 0 && x >= 0 && y >= 0 && x + w <= tw && y + h <= th;
}

// ---- one shape: the band and block heights, and the items of every band and block
static void check_shape(int w, int h) {
  const rc2dgi_rect r{3, 5, w, h};
  const long long texels = (long long)w * h;
  for (int hist = 0; hist < 2; ++hist) {
    const char *what = hist ? "hist" : "reduce";
    const int rows = hist ? hist_block_rows(w, h) : reduce_band_rows(w, h);
    CHECK(rows >= 1, "%s %dx%d: %d rows", what, w, h, rows);
    if (rows < 1) continue;
    const long long nb = ((long long)h + rows - 1) / rows;
    CHECK(nb >= 1 && nb <= 4096, "%s %dx%d: %lld items", what, w, h, nb);
    if (!hist) {
      CHECK(pow2(rows), "reduce %dx%d: band of %d rows is no power of two", w, h, rows);
      if (w <= 256) CHECK(rows % (64 / lanes_a_row(w)) == 0, "reduce %dx%d: band of %d rows, %d lanes a row", w, h, rows, lanes_a_row(w));
    } else if (w <= 1024) {
      CHECK(rows % (256 / lanes_a_row(w)) == 0, "hist %dx%d: block of %d rows, %d lanes a row", w, h, rows, lanes_a_row(w));
    }
    RectDesc d;
    const int got = rect_desc(r, 3 + w, 5 + h, hist != 0, 11, 22, 7, d);
    CHECK(got == nb && d.x == 3 && d.y == 5 && d.w == w && d.h == h && d.rows == rows && d.item0 == 11 && d.part0 == 22 &&
              d.out == 7, "%s %dx%d: descriptor", what, w, h);
    long long at = 0;
    for (int b = 0; b < nb && b < 4096; ++b) {
      int x, y, iw, r0, r1;
      unsigned out, want_out;
      if (hist) {
        const HistItem it = hist_item_of(d, b);
        x = it.x, y = it.y, iw = it.w, r0 = it.r0, r1 = it.r1, out = it.out;
        want_out = 7u | (nb == 1 ? kHistSingle : 0u) | (b == 0 ? kHistFirst : 0u);
        CHECK(it.texels == texels, "hist %dx%d: texels %d", w, h, it.texels);
      } else {
        const ReduceItem it = reduce_item_of(d, b);
        x = it.x, y = it.y, iw = it.w, r0 = it.r0, r1 = it.r1, out = it.out;
        want_out = nb == 1 ? 7u | kReduceFinal : (unsigned)(22 + b);
      }
      CHECK(x == 3 && y == 5 && iw == w && out == want_out, "%s %dx%d item %d: fields", what, w, h, b);
      CHECK(r0 == at && r1 > r0 && r1 <= h, "%s %dx%d item %d: rows [%d, %d) after %lld", what, w, h, b, r0, r1, at);
      CHECK(r1 - r0 == rows || (b == nb - 1 && r1 - r0 < rows), "%s %dx%d item %d: %d rows of %d", what, w, h, b, r1 - r0, rows);
      at = r1;
    }
    CHECK(at == h, "%s %dx%d: the items end at row %lld", what, w, h, at);
    if (!hist && nb > 1) {
      const ReduceJoin j = reduce_join_of(d);
      CHECK(j.first == 22 && j.nb == nb && j.out == 7 && j.texels == texels, "reduce %dx%d: join", w, h);
    }
  }
}

static void check_shapes() {
  for (int w = 1; w <= 130; ++w)
    for (int h = 1; h <= 130; ++h) check_shape(w, h);
  const int edge_w[] = {254, 255, 256, 257, 258, 1022, 1023, 1024, 1025, 1026, 4096, 8192, 16385, 32767, 32768};
  const int edge_h[] = {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095,
                        4096, 4097, 16383, 16384, 16385, 32767, 32768};
  for (int w : edge_w)
    for (int h : edge_h) check_shape(w, h);
  for (int w = 1; w <= 130; ++w)
    for (int h : {32767, 32768}) {
      check_shape(w, h);
      check_shape(h, w);
    }
  // where the cap of 4096 bands starts to bind: 1024-row bands of 2^22 rows (no texture is that tall: the planner is
  // only asked for rectangles whose w * h fits an int, as those of a texture do)
  for (int w : {1, 2, 3, 4, 5, 64, 255, 256, 257})
    for (int dh = -2; dh <= 2; ++dh)
      for (int sh : {22, 23})
        if ((long long)w * ((1 << sh) + dh) <= INT_MAX) check_shape(w, (1 << sh) + dh);
  // and of 4096 blocks: 16384-row blocks of 2^26 rows
  for (int w : {1, 2, 4, 5})
    for (int dh = -2; dh <= 2; ++dh) check_shape(w, (1 << 26) + dh);
}

// ---- each kind of invalid rectangle
static void check_invalid() {
  const int tw = 200, th = 120;
  const rc2dgi_rect bad[] = {{0, 0, 0, 1}, {0, 0, 1, 0}, {0, 0, -1, 1}, {0, 0, 1, -3}, {-1, 0, 1, 1}, {0, -1, 1, 1},
                             {1, 0, tw, 1}, {0, 1, 1, th}, {tw, 0, 1, 1}, {0, th, 1, 1}, {tw - 4, 3, 5, 2}, {3, th - 4, 2, 5},
                             {INT_MAX, 0, 1, 1}, {0, INT_MAX, 1, 1}, {1, 0, INT_MAX, 1}, {0, 1, 1, INT_MAX},
                             {INT_MAX, INT_MAX, INT_MAX, INT_MAX}, {INT_MIN, 0, 1, 1}, {0, INT_MIN, 1, 1},
                             {0, 0, INT_MIN, 1}, {0, 0, 1, INT_MIN}};
  int k = 40;
  for (const rc2dgi_rect &r : bad) {
    ++k;
    CHECK(!valid_ref(r, tw, th) && !rect_valid(r, tw, th), "{%d, %d, %d, %d} is valid", r.x, r.y, r.w, r.h);
    for (int hist = 0; hist < 2; ++hist) {
      RectDesc d;
      CHECK(rect_desc(r, tw, th, hist != 0, 5, 6, k, d) == 1 && d.w == 0 && d.out == k && d.item0 == 5, "invalid descriptor %d", k);
      if (hist) {
        const HistItem it = hist_item_of(d, 0);
        CHECK(it.w == 0 && it.out == ((unsigned)k | kHistSingle | kHistFirst), "invalid hist item %d", k);
      } else {
        const ReduceItem it = reduce_item_of(d, 0);
        CHECK(it.w == 0 && it.out == ((unsigned)k | kReduceFinal), "invalid reduce item %d", k);
      }
    }
  }
  const rc2dgi_rect good[] = {{0, 0, tw, th}, {tw - 1, th - 1, 1, 1}, {tw - 5, 3, 5, 2}, {0, 0, 1, 1}};
  for (const rc2dgi_rect &r : good) CHECK(valid_ref(r, tw, th) && rect_valid(r, tw, th), "{%d, %d, %d, %d} is invalid", r.x, r.y, r.w, r.h);
}

// ---- lists: the batches against the inline descriptors of the same rectangles, four at a time
static std::vector<rc2dgi_rect> make_list(int n, int tw, int th) {
  std::vector<rc2dgi_rect> v;
  unsigned s = 12345u + (unsigned)n;
  auto rnd = [&](int m) {
    s = s * 1664525u + 1013904223u;
    return (int)((s >> 8) % (unsigned)m);
  };
  for (int k = 0; k < n; ++k) {
    rc2dgi_rect r{0, 0, 1 + rnd(40), 1 + rnd(40)};
    if (k % 11 == 3) r = rc2dgi_rect{0, 0, 2049 + rnd(3), 400 + rnd(700)};      // one-row bands: hundreds of them
    else if (k % 13 == 5) r = rc2dgi_rect{0, 0, 1 + rnd(300), 100 + rnd(2000)};  // a few bands or blocks
    r.x = rnd(tw - r.w + 1);
    r.y = rnd(th - r.h + 1);
    if (k % 7 == 2) {  // invalid, in one of the ways there are
      switch ((k / 7) % 6) {
        case 0: r.w = 0; break;
        case 1: r.h = -rnd(50); break;
        case 2: r.x = -1; break;
        case 3: r.x = tw - r.w + 1; break;
        case 4: r.y = th - r.h + 1; break;
        default: r.y = INT_MAX; break;
      }
    }
    v.push_back(r);
  }
  return v;
}

static void check_list(int n, bool hist) {
  const int tw = 4096, th = 4096, cap = 1 << 16;
  const char *what = hist ? "hist" : "reduce";
  const std::vector<rc2dgi_rect> rects = make_list(n, tw, th);
  // the cursor into what the device would derive: rectangle k, its band or block b
  int k = 0, b = 0, nb = 0, batches = 0, straddles = 0;
  long long total = 0, want_total = 0;
  RectInline inl{};
  RectDesc d{};
  auto enter = [&]() {  // the descriptor of rectangle k, from the inline plan of its group of four
    if (k % 4 == 0) {
      int items, parts;
      inl = rect_inline_plan(rects.data() + k, std::min(4, n - k), tw, th, hist, &items, &parts);
    }
    d = inl.d[k % 4];
    const bool ok = valid_ref(rects[k], tw, th);
    CHECK(ok == (d.w != 0), "%s list %d: rectangle %d validity", what, n, k);
    nb = ok ? (int)(((long long)d.h + d.rows - 1) / d.rows) : 1;
    CHECK(d.out == k % 4, "%s list %d: rectangle %d record", what, n, k);
    for (int i : {0, nb - 1}) {  // the lookup of the device finds this descriptor for its first and last item
      const RectDesc f = inline_desc(inl, d.item0 + i);
      CHECK(f.out == d.out && f.item0 == d.item0, "%s list %d: rectangle %d lookup", what, n, k);
    }
    b = 0;
  };
  for (int q = 0; q < n; ++q) {
    const rc2dgi_rect &r = rects[q];
    if (!valid_ref(r, tw, th)) want_total += 1;
    else {
      const int rows = hist ? hist_block_rows(r.w, r.h) : reduce_band_rows(r.w, r.h);
      want_total += (r.h + rows - 1) / rows;
    }
  }
  enter();
  const int rc = rect_batches(rects.data(), n, tw, th, hist, [&](const RectBatch &bt) -> int {
    ++batches;
    const size_t ni = hist ? bt.blocks.size() : bt.items.size();
    CHECK(ni >= 1 && ni <= (size_t)cap, "%s list %d: a batch of %zu items", what, n, ni);
    CHECK(hist ? bt.items.empty() && bt.joins.empty() && bt.parts == 0 : bt.blocks.empty(), "%s list %d: lists of the other call", what, n);
    if (b != 0) {
      ++straddles;
      CHECK(hist, "reduce list %d: rectangle %d straddles a batch", n, k);
    }
    int part = 0;
    size_t join = 0;
    for (size_t i = 0; i < ni; ++i) {
      CHECK(k < n, "%s list %d: more items than rectangles have", what, n);
      if (k >= n) return 0;
      if (hist) {
        const HistItem g = bt.blocks[i], e = hist_item_of(d, b);
        CHECK(g.x == e.x && g.y == e.y && g.w == e.w && g.r0 == e.r0 && g.r1 == e.r1 && g.texels == e.texels &&
                  g.out == (e.out - (unsigned)d.out + (unsigned)k), "hist list %d: rectangle %d block %d", n, k, b);
      } else {
        const ReduceItem g = bt.items[i], e = reduce_item_of(d, b);
        CHECK(g.x == e.x && g.y == e.y && g.w == e.w && g.r0 == e.r0 && g.r1 == e.r1, "reduce list %d: rectangle %d band %d", n, k, b);
        if (nb == 1) {
          CHECK((e.out & kReduceFinal) && g.out == ((unsigned)k | kReduceFinal), "reduce list %d: rectangle %d record", n, k);
        } else {
          CHECK(e.out == (unsigned)(d.part0 + b) && g.out == (unsigned)part, "reduce list %d: rectangle %d band %d partial %u", n, k, b, g.out);
          if (b == 0) {
            CHECK(join < bt.joins.size(), "reduce list %d: rectangle %d has no join", n, k);
            if (join < bt.joins.size()) {
              const ReduceJoin j = bt.joins[join++], ej = reduce_join_of(d);
              CHECK(j.first == part && j.nb == nb && j.nb == ej.nb && j.out == k && j.texels == ej.texels &&
                        j.texels == rects[k].w * rects[k].h && j.first + j.nb <= cap, "reduce list %d: join of rectangle %d", n, k);
            }
          }
          ++part;
        }
      }
      ++total;
      if (++b == nb && ++k < n) enter();
    }
    if (!hist) {
      CHECK(join == bt.joins.size() && part == bt.parts, "reduce list %d: %zu joins and %d partials, %zu and %d stated", n, join, part, bt.joins.size(), bt.parts);
      if (!bt.joins.empty()) CHECK(bt.joins[0].first == 0, "reduce list %d: the partials start at %d", n, bt.joins[0].first);
    }
    return 0;
  });
  CHECK(rc == 0 && k == n && total == want_total, "%s list %d: %lld of %lld items, %d of %d rectangles", what, n, total, want_total, k, n);
  const long long full = (want_total + cap - 1) / cap;  // the histogram fills every batch; the reduction may not
  CHECK(hist ? batches == full : batches >= full, "%s list %d: %d batches", what, n, batches);
  if (hist && want_total > 4ll * cap) CHECK(straddles > 0, "hist list %d: no rectangle straddles a batch", n);
  // a small list is one batch, and then the two plans agree to the last bit
  if (n <= kRectInline) {
    int items, parts;
    const RectInline all = rect_inline_plan(rects.data(), n, tw, th, hist, &items, &parts);
    CHECK(items == want_total && batches == 1, "%s list %d: %d inline items", what, n, items);
    rect_batches(rects.data(), n, tw, th, hist, [&](const RectBatch &bt) -> int {
      CHECK(bt.parts == parts, "%s list %d: %d inline partials", what, n, parts);
      for (int i = 0; i < items; ++i) {
        const RectDesc f = inline_desc(all, i);
        if (hist) {
          const HistItem g = bt.blocks[i], e = hist_item_of(f, i - f.item0);
          CHECK(g.x == e.x && g.y == e.y && g.w == e.w && g.r0 == e.r0 && g.r1 == e.r1 && g.texels == e.texels && g.out == e.out, "hist list %d: item %d", n, i);
        } else {
          const ReduceItem g = bt.items[i], e = reduce_item_of(f, i - f.item0);
          CHECK(g.x == e.x && g.y == e.y && g.w == e.w && g.r0 == e.r0 && g.r1 == e.r1 && g.out == e.out, "reduce list %d: item %d", n, i);
        }
      }
      return 0;
    });
  }
  // a status from the callback ends the walk
  int calls = 0;
  CHECK(rect_batches(rects.data(), n, tw, th, hist, [&](const RectBatch &) { return ++calls, 7; }) == 7 && calls == 1, "%s list %d: a failed flush", what, n);
}

// ---- the staged block of rc2dgi_read
static void check_read_blocks() {
  std::vector<int> widths;
  for (int w = 1; w <= 130; ++w) widths.push_back(w);
  for (int w : {255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 32767, 32768}) widths.push_back(w);
  for (int w : widths)
    for (int px : {4, 8, 16})
      for (int h : {1, 2, 3, 100, 4095, 4096, 4097, 32767, 32768}) {
        const size_t row = (size_t)w * px, sp = read_staged_pitch(row);
        const int block = read_block_rows(row, h);
        CHECK(sp % 16 == 0 && sp >= row && sp - row < 16, "read: pitch %zu of a row of %zu bytes", sp, row);
        CHECK(block >= 1 && block <= h && (size_t)block * sp <= kReadChunkBytes, "read %d x %d, %d bytes a pixel: block of %d rows", w, h, px, block);
        CHECK(block == h || (size_t)(block + 1) * sp > kReadChunkBytes, "read %d x %d, %d bytes a pixel: block of %d rows is short", w, h, px, block);
      }
}

// ---- a view against the window, pixel by pixel
static void check_view(int x, int y, int w, int h, int ow, int oh) {
  for (int border = 0; border < 2; ++border)
    for (int blit = 0; blit < 2; ++blit) {
      ViewClip v;
      const bool kept = clip_view(x, y, w, h, ow, oh, border, blit != 0, v);
      // bounding box and count of the pixels inside the view, and inside it without the border
      int n = 0, x0 = ow, x1 = 0, y0 = oh, y1 = 0, fn = 0, fx0 = ow, fx1 = 0, fy0 = oh, fy1 = 0;
      for (int py = 0; py < oh; ++py)
        for (int px = 0; px < ow; ++px) {
          const long long dx = (long long)px - x, dy = (long long)py - y;
          if (dx < 0 || dx >= w || dy < 0 || dy >= h) continue;
          ++n;
          x0 = std::min(x0, px), x1 = std::max(x1, px + 1), y0 = std::min(y0, py), y1 = std::max(y1, py + 1);
          if (dx < border || dx >= (long long)w - border || dy < border || dy >= (long long)h - border) continue;
          ++fn;
          fx0 = std::min(fx0, px), fx1 = std::max(fx1, px + 1), fy0 = std::min(fy0, py), fy1 = std::max(fy1, py + 1);
        }
      CHECK(kept == (n > 0), "view {%d, %d, %d, %d} in %d x %d: kept %d, %d pixels", x, y, w, h, ow, oh, (int)kept, n);
      if (!kept || n == 0) continue;
      CHECK(v.cx0 == x0 && v.cx1 == x1 && v.cy0 == y0 && v.cy1 == y1 && n == (x1 - x0) * (y1 - y0),
            "view {%d, %d, %d, %d} in %d x %d: clip [%d, %d) x [%d, %d)", x, y, w, h, ow, oh, v.cx0, v.cx1, v.cy0, v.cy1);
      const bool empty = v.fx0 >= v.fx1 || v.fy0 >= v.fy1;
      if (!blit) CHECK(v.fx0 == 0 && v.fx1 == 0 && v.fy0 == 0 && v.fy1 == 0, "view {%d, %d, %d, %d}: an interior without blit", x, y, w, h);
      else if (fn == 0) CHECK(empty, "view {%d, %d, %d, %d} in %d x %d border %d: interior [%d, %d) x [%d, %d) of no pixel", x, y, w, h, ow, oh, border, v.fx0, v.fx1, v.fy0, v.fy1);
      else
        CHECK(v.fx0 == fx0 && v.fx1 == fx1 && v.fy0 == fy0 && v.fy1 == fy1 && fn == (fx1 - fx0) * (fy1 - fy0),
              "view {%d, %d, %d, %d} in %d x %d border %d: interior [%d, %d) x [%d, %d)", x, y, w, h, ow, oh, border, v.fx0, v.fx1, v.fy0, v.fy1);
    }
}

static void check_views() {
  const int wins[][2] = {{1, 1}, {7, 5}, {40, 3}, {3, 40}, {40, 40}};
  for (auto &win : wins) {
    const int ow = win[0], oh = win[1];
    // origins left of, on, inside, on and right of each edge; sizes that fall short of, meet and pass the far edge
    const int xs[] = {INT_MIN, -100, -41, -2, -1, 0, 1, ow - 2, ow - 1, ow, ow + 3, INT_MAX};
    const int ys[] = {INT_MIN, -41, -1, 0, 1, oh - 1, oh, oh + 3, INT_MAX};
    const int ws[] = {1, 2, 3, ow - 1, ow, ow + 1, 41, 45, 100, INT_MAX};
    const int hs[] = {1, 2, 3, oh, oh + 1, 42, 100, INT_MAX};
    for (int x : xs)
      for (int w : ws)
        for (int y : ys)
          for (int h : hs)
            if (w >= 1 && h >= 1) check_view(x, y, w, h, ow, oh);
  }
}

int main() {
  check_shapes();
  check_invalid();
  for (int n : {1, 4, 5, 65535, 65536, 65537})
    for (int hist = 0; hist < 2; ++hist) check_list(n, hist != 0);
  check_read_blocks();
  check_views();
  std::printf("%s (%d failures)\n", fails ? "FAILED" : "OK", fails);
  return fails != 0;
}
