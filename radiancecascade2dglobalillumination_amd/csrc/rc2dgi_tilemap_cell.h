// rc2dgi_tilemap_cell.h -- the cell logic of rc2dgi_tilemap_device (include/rc2dgi.h): the decode of a
// cell word, the refusal test, and the map from a screen pixel to (cell, source pixel of the atlas).  Plain C++ with no
// HIP include, so that a host program calls the very text k_tilemap runs (tests/tilemap_cell_check.cpp).
//
// Ranges (rc2dgi_tilemap_device's argument checks): a screen coordinate P is 0 .. 32767 + a launch's padding, an origin
// |o| <= 2^22, a tile 1 .. 32768 pixels, cols and rows 0 .. 32768, set_cols 1 .. 32768, margin and spacing 0 .. 32768,
// the atlas at most 32768 pixels on an axis and margin + tile <= the atlas.  Every sum below stays inside an int:
// |P - o| < 2^23; a tile index that passed the refusal test has tx * (tile_w + spacing) <= AW - margin - tile_w.
#pragma once

#ifndef RC2DGI_TILEMAP_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define RC2DGI_TILEMAP_HD __host__ __device__
#else
#define RC2DGI_TILEMAP_HD
#endif
#endif

namespace rc2dgi {

// rc2dgi_tilemap, validated: what the kernel needs of it, with the two quotients of the refusal test
struct TilemapGeom {
  int cols, rows;
  int pitch;           // cell words from one row to the next (resolved: never 0)
  int tile_w, tile_h;
  int ox, oy;
  int set_cols;
  int margin;
  int step_x, step_y;  // tile_w + spacing, tile_h + spacing: from one tile of the set to the next
  int max_tx, max_ty;  // (AW - margin - tile_w) / step_x, (AH - margin - tile_h) / step_y: the last tile that fits
};

constexpr unsigned kTileFlipX = 0x80000000u, kTileFlipY = 0x40000000u, kTileUnsupported = 0x30000000u,
                   kTileIdMask = 0x0FFFFFFFu;
enum { TILE_EMPTY = 0, TILE_DRAWN = 1, TILE_REFUSED = 2 };

// the two quotients, as the header writes them (margin + tile <= A: nothing is negative)
RC2DGI_TILEMAP_HD inline int tilemap_max_tile(int A, int margin, int tile, int spacing) {
  return (A - margin - tile) / (tile + spacing);
}

// One axis of the map from a screen pixel to its cell: pixel P of an axis whose cell 0 begins at o, cells `tile`
// pixels long, n of them.  False: P is outside the grid on this axis.  One division; k_tilemap calls it once a lane
// for the column and once a wave for its first row.
RC2DGI_TILEMAP_HD inline bool tilemap_axis(int P, int o, int tile, int n, int &cell, int &off) {
  const int d = P - o;
  cell = 0;
  off = 0;
  if (d < 0) return false;
  cell = d / tile;
  off = d - cell * tile;
  return cell < n;
}

// The next pixel of the same axis, without a division (k_tilemap's rows): cell and off are what tilemap_axis or this
// function left for P1 - 1 and become those of P1.
RC2DGI_TILEMAP_HD inline bool tilemap_axis_next(int P1, int o, int tile, int n, int &cell, int &off) {
  const int d = P1 - o;
  if (d < 0) return false;
  if (d == 0) {
    cell = 0;
    off = 0;
  } else if (++off == tile) {
    off = 0;
    ++cell;
  }
  return cell < n;
}

// A cell word: TILE_EMPTY (g == 0), TILE_REFUSED, or TILE_DRAWN with the tile's column and row of the set.
RC2DGI_TILEMAP_HD inline int tilemap_decode(unsigned g, const TilemapGeom &m, int &tx, int &ty) {
  tx = 0;
  ty = 0;
  if (g == 0u) return TILE_EMPTY;
  const unsigned id = g & kTileIdMask;
  if ((g & kTileUnsupported) != 0u || id == 0u) return TILE_REFUSED;
  const unsigned t = id - 1u, q = t / (unsigned)m.set_cols, r = t - q * (unsigned)m.set_cols;
  if (r > (unsigned)m.max_tx || q > (unsigned)m.max_ty) return TILE_REFUSED;
  tx = (int)r;
  ty = (int)q;
  return TILE_DRAWN;
}

// The atlas pixel under offset (offx, offy) of a drawn cell (0 <= offx < tile_w, 0 <= offy < tile_h): inside the
// tile's rectangle, which the refusal test found inside the atlas.
RC2DGI_TILEMAP_HD inline void tilemap_source(unsigned g, const TilemapGeom &m, int tx, int ty, int offx, int offy,
                                             int &u, int &v) {
  u = m.margin + tx * m.step_x + ((g & kTileFlipX) ? m.tile_w - 1 - offx : offx);
  v = m.margin + ty * m.step_y + ((g & kTileFlipY) ? m.tile_h - 1 - offy : offy);
}

// Does this pixel count its cell?  The one at screen (max(dx, 0), max(dy, 0)): the cell's first visible pixel.
RC2DGI_TILEMAP_HD inline bool tilemap_first_pixel(int X, int Y, int offx, int offy) {
  return (offx == 0 || X == 0) && (offy == 0 || Y == 0);
}

}  // namespace rc2dgi
