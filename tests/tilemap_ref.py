"""numpy restatement of rc2dgi_tilemap_device as include/rc2dgi.h states it (written from the header, not from the
kernel): the cell word's decode, the refusal rule, the visible cells, the counts {drawn, refused}, and the header's
consequence -- the texture is what rc2dgi_sprites_device leaves for the list of the visible, non-empty, accepted cells,
which tests/sprites_ref.py restates.

A grid is a (rows, cols) array of 32-bit words (any integer dtype; read as uint32), row 0 the top row.  A map is the
dict `layer` makes: the arguments of the call beside the grid, the atlas and the target."""
import numpy as np

import sprites_ref as S

FLIP_X, FLIP_Y, DIAGONAL, HEXAGONAL, ID_MASK = 1 << 31, 1 << 30, 1 << 29, 1 << 28, (1 << 28) - 1
EMPTY, DRAWN, REFUSED = 0, 1, 2


def layer(tile, origin=(0, 0), set_cols=None, margin=0, spacing=0, tint=(255, 255, 255, 255), replace=False):
    return dict(tile=(int(tile[0]), int(tile[1])), origin=(int(origin[0]), int(origin[1])), set_cols=set_cols,
                margin=int(margin), spacing=int(spacing), tint=tuple(int(v) for v in tint), replace=bool(replace))


def tiled_set_cols(AW, tile_w, margin, spacing):
    """Tiled's columns of a tile set image"""
    return (AW - 2 * margin + spacing) // (tile_w + spacing)


def words_u32(cells):
    a = np.asarray(cells)
    return (a.astype(np.int64) & 0xFFFFFFFF).astype(np.int64)


def decode(g, AW, AH, m):
    """(kind, tx, ty) of cell words g (int64 arrays of any shape): EMPTY, DRAWN or REFUSED by the header's rule"""
    tw, th = m["tile"]
    margin, spacing = m["margin"], m["spacing"]
    set_cols = tiled_set_cols(AW, tw, margin, spacing) if m["set_cols"] is None else int(m["set_cols"])
    max_tx = (AW - margin - tw) // (tw + spacing)
    max_ty = (AH - margin - th) // (th + spacing)
    ident = g & ID_MASK
    t = ident - 1
    tx, ty = np.where(t >= 0, t % set_cols, 0), np.where(t >= 0, t // set_cols, 0)
    refused = ((g & (DIAGONAL | HEXAGONAL)) != 0) | (ident == 0) | (tx > max_tx) | (ty > max_ty)
    kind = np.where(g == 0, EMPTY, np.where(refused, REFUSED, DRAWN))
    return kind, tx, ty


def visible(m, rows, cols, W, H):
    """the inclusive ranges (c0, c1, r0, r1) of the cells with a pixel inside the W x H target (empty: c0 > c1 or
    r0 > r1), by the definition: dx + tile_w > 0, dx < W, dy + tile_h > 0, dy < H"""
    (tw, th), (ox, oy) = m["tile"], m["origin"]
    cs = [c for c in _candidates(ox, tw, cols, W) if ox + c * tw + tw > 0 and ox + c * tw < W]
    rs = [r for r in _candidates(oy, th, rows, H) if oy + r * th + th > 0 and oy + r * th < H]
    return (cs[0], cs[-1], rs[0], rs[-1]) if cs and rs else (0, -1, 0, -1)


def _candidates(o, tile, n, size):
    """a range of cell indices that holds every visible one (two to spare on either side), inside [0, n)"""
    lo, hi = (-o) // tile - 2, (size - o) // tile + 2
    return range(max(lo, 0), min(hi, n - 1) + 1)


def expand(cells, AW, AH, W, H, m):
    """((n, 8) int32 sprite words of the visible drawn cells in row-major order, [drawn, refused])"""
    g = words_u32(cells)
    rows, cols = g.shape
    c0, c1, r0, r1 = visible(m, rows, cols, W, H)
    if c0 > c1 or r0 > r1:
        return np.zeros((0, 8), np.int32), [0, 0]
    (tw, th), (ox, oy) = m["tile"], m["origin"]
    win = g[r0:r1 + 1, c0:c1 + 1]
    kind, tx, ty = decode(win, AW, AH, m)
    out = []
    for r, c in zip(*np.nonzero(kind == DRAWN)):
        w = int(win[r, c])
        flags = (S.FLIP_X if w & FLIP_X else 0) | (S.FLIP_Y if w & FLIP_Y else 0) | (S.REPLACE if m["replace"] else 0)
        out.append((m["margin"] + int(tx[r, c]) * (tw + m["spacing"]), m["margin"] + int(ty[r, c]) * (th + m["spacing"]),
                    tw, th, ox + (c0 + int(c)) * tw, oy + (r0 + int(r)) * th, m["tint"], flags))
    wd = S.words(out) if out else np.zeros((0, 8), np.int32)
    return wd, [int(np.count_nonzero(kind == DRAWN)), int(np.count_nonzero(kind == REFUSED))]


def draw(tex, atlas, cells, m, rgba8=False, clear=None):
    """(the texture after rc2dgi_tilemap_device, [drawn, refused]); tex is not changed"""
    AH, AW = np.asarray(atlas).shape[:2]
    H, W = np.asarray(tex).shape[:2]
    wd, status = expand(cells, AW, AH, W, H, m)
    assert S.accepted(wd, AW, AH).all(), "an accepted cell is an admissible sprite"
    return S.draw(tex, atlas, wd, rgba8, clear), status
