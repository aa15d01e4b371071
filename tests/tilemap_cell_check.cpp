// tilemap_cell_check.cpp -- host check of k_tilemap's cell logic (csrc/rc2dgi_tilemap_cell.h), a stand-alone program
// built by tests/test_tilemap_cpu.py with -fsanitize=address,undefined.  The kernel maps a screen pixel BACK to its
// cell and offset (a division) and a cell word to a tile (a division and two comparisons with host quotients); this
// program walks FORWARD in 64 bits -- every cell, every pixel of it, its screen position; every tile, its rectangle
// against the atlas -- and compares, at the extremes rc2dgi_tilemap_device admits:
//   axes      every pixel of a 32768-pixel axis (and a 200-pixel one), tile sizes 1, 3, 16, 32767, 32768, origins 0,
//             +-1, +-2^22 and some near a tile, grids of 0, 1, 7 and 32768 cells: the cell, the offset, the increment
//             k_tilemap's rows use, and the one counting pixel a visible cell;
//   decode    set_cols 1, 2, 31, 32768, margins and spacings 0, 1, 32768, the same tile sizes, the smallest atlas the
//             call admits and the largest, ids 0, 1, the last tile, one past it, the end of a set row and 0x0FFFFFFF
//             under all sixteen flag nibbles: the refusal decision and the source pixel at the tile's corners.
// `--late` refuses one tile too late (max_tx + 1): the mistake the check exists to catch; the program must exit 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rc2dgi_tilemap_cell.h"

namespace {

using rc2dgi::TilemapGeom;

long long g_checked = 0, g_wrong = 0;

void wrong(const char *what, long long a, long long b, long long c, long long d) {
  if (++g_wrong <= 10) printf("WRONG %s: %lld %lld %lld %lld\n", what, a, b, c, d);
}

// ---- one axis: `size` pixels, cell 0 at o, n cells of `tile` pixels
struct Owner {
  int cell, off;
};

void check_axis(int size, int o, int tile, int n) {
  std::vector<Owner> own((size_t)size, Owner{-1, -1});
  long long visible = 0;
  for (long long c = 0; c < n; ++c) {  // the forward walk, 64-bit
    const long long first = (long long)o + c * tile, last = first + tile - 1;
    if (last < 0) continue;
    if (first >= size) break;
    ++visible;
    for (long long i = first < 0 ? -first : 0; i < tile && first + i < size; ++i)
      own[(size_t)(first + i)] = Owner{(int)c, (int)i};
  }
  long long counted = 0;
  int cell = 0, off = 0, ncell = 0, noff = 0;
  bool nin = false;
  for (int P = 0; P < size; ++P) {
    const bool in = rc2dgi::tilemap_axis(P, o, tile, n, cell, off);
    nin = P == 0 ? rc2dgi::tilemap_axis(P, o, tile, n, ncell, noff) : rc2dgi::tilemap_axis_next(P, o, tile, n, ncell, noff);
    const Owner w = own[(size_t)P];
    ++g_checked;
    if (in != (w.cell >= 0) || (in && (cell != w.cell || off != w.off))) wrong("axis", P, o, tile, n);
    if (nin != in || (in && (ncell != cell || noff != off))) wrong("axis_next", P, o, tile, n);
    if (in && rc2dgi::tilemap_first_pixel(P, 1, off, 0)) ++counted;  // (the other axis: not a first pixel by position)
  }
  if (counted != visible) wrong("first pixels", counted, visible, o, tile);
}

// ---- the decode: tile set of set_cols columns in an AW x AH atlas
bool g_late = false;

void check_decode(int AW, int AH, int tw, int th, int set_cols, int margin, int spacing) {
  TilemapGeom m{};
  m.tile_w = tw, m.tile_h = th, m.set_cols = set_cols, m.margin = margin;
  m.step_x = tw + spacing, m.step_y = th + spacing;
  m.max_tx = rc2dgi::tilemap_max_tile(AW, margin, tw, spacing) + (g_late ? 1 : 0);
  m.max_ty = rc2dgi::tilemap_max_tile(AH, margin, th, spacing);
  // the last tile the atlas holds, by walking (64-bit): the largest tx, ty whose rectangle fits
  long long ltx = 0, lty = 0;
  while ((long long)margin + (ltx + 1) * ((long long)tw + spacing) + tw <= AW) ++ltx;
  while ((long long)margin + (lty + 1) * ((long long)th + spacing) + th <= AH) ++lty;
  const long long lx = ltx < set_cols - 1 ? ltx : set_cols - 1;
  const long long last = lty * set_cols + lx + 1;  // its id
  const long long ids[] = {0, 1, 2, last, last + 1, last + set_cols, (lty + 1) * (long long)set_cols,
                           (lty + 1) * (long long)set_cols + 1, (long long)set_cols, (long long)set_cols + 1,
                           0x0FFFFFFE, 0x0FFFFFFF};
  for (long long id : ids) {
    if (id < 0 || id > 0x0FFFFFFF) continue;
    for (unsigned nib = 0; nib < 16; ++nib) {
      const unsigned g = (unsigned)id | nib << 28;
      int tx = -1, ty = -1;
      const int kind = rc2dgi::tilemap_decode(g, m, tx, ty);
      int want = rc2dgi::TILE_DRAWN;
      long long wtx = 0, wty = 0;
      if (g == 0) want = rc2dgi::TILE_EMPTY;
      else if ((nib & 3u) != 0 || id == 0) want = rc2dgi::TILE_REFUSED;
      else {
        wtx = (id - 1) % set_cols, wty = (id - 1) / set_cols;
        const long long sx = margin + wtx * ((long long)tw + spacing), sy = margin + wty * ((long long)th + spacing);
        if (sx + tw > AW || sy + th > AH) want = rc2dgi::TILE_REFUSED;
      }
      ++g_checked;
      if (kind != want || (kind == rc2dgi::TILE_DRAWN && (tx != wtx || ty != wty))) {
        wrong("decode", g, set_cols, AW, tw);
        continue;
      }
      if (kind != rc2dgi::TILE_DRAWN) continue;
      const int offs_x[] = {0, 1 % tw, tw / 2, tw - 1}, offs_y[] = {0, 1 % th, th / 2, th - 1};
      for (int i : offs_x)
        for (int j : offs_y) {
          int u = -1, v = -1;
          rc2dgi::tilemap_source(g, m, tx, ty, i, j, u, v);
          const long long wu = margin + wtx * ((long long)tw + spacing) + ((nib & 8u) ? tw - 1 - i : i);
          const long long wv = margin + wty * ((long long)th + spacing) + ((nib & 4u) ? th - 1 - j : j);
          ++g_checked;
          if (u != wu || v != wv || u < 0 || u >= AW || v < 0 || v >= AH) wrong("source", g, u, v, AW);
        }
    }
  }
}

}  // namespace

int main(int argc, char **argv) {
  g_late = argc > 1 && !strcmp(argv[1], "--late");
  const int tiles[] = {1, 3, 16, 32767, 32768};
  const int lim = 1 << 22;
  for (int tile : tiles) {
    const int origins[] = {0, 1, -1, lim, -lim, -tile, -tile + 1, -tile - 1, 32767 - tile, 32768 - tile, 5 - 3 * tile};
    for (int o : origins) {
      if (o < -lim || o > lim) continue;
      for (int n : {0, 1, 7, 32768}) {
        check_axis(32768, o, tile, n);
        check_axis(200, o, tile, n);
      }
    }
  }
  // tile 1, 2^22 cells to the left: the last cells of the largest grid still fall short of the target
  check_axis(72, -lim, 1, 32768);
  const long long axes = g_checked;
  const int set_cols[] = {1, 2, 31, 32768}, pads[] = {0, 1, 32768};
  for (int tw : tiles)
    for (int th : {tiles[1], tiles[4], tw})
      for (int sc : set_cols)
        for (int margin : pads)
          for (int spacing : pads) {
            const int mw = margin + tw, mh = margin + th;  // the smallest atlas the call admits
            if (mw > 32768 || mh > 32768) continue;
            check_decode(mw, mh, tw, th, sc, margin, spacing);
            check_decode(32768, 32768, tw, th, sc, margin, spacing);
            check_decode(mw, 32768, tw, th, sc, margin, spacing);
          }
  printf("axis pixels checked %lld, words and source pixels checked %lld, wrong %lld\n", axes, g_checked - axes, g_wrong);
  return g_wrong ? 1 : 0;
}
