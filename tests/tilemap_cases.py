"""The maps the tile-map tests share (tests/test_tilemap_cpu.py expands them on the host, tests/test_gpu_tilemap.py draws
them): seeded grids of Tiled cell words and the edge maps of rc2dgi_tilemap_device -- every tile size class, origins
that put cell boundaries on columns 63 / 64 / 128 and one either side, negative origins, maps smaller than, much larger
than and wholly off the target, a pitched window, a set with margin and spacing -- each grid holding both flips, empty
cells and one cell of every refusal term."""
import numpy as np

import tilemap_ref as T

TINT = (255, 160, 90, 200)


def set_size(tile, cols, rows, margin=0, spacing=0):
    """(AW, AH) of a tile set image of cols x rows tiles, as Tiled lays it out"""
    return (2 * margin + cols * tile[0] + (cols - 1) * spacing, 2 * margin + rows * tile[1] + (rows - 1) * spacing)


def grid(rows, cols, ntiles, seed, empty=0.25):
    """(rows, cols) uint32 cell words: ids 1 .. ntiles with random flips, `empty` of them 0"""
    rng = np.random.default_rng(seed)
    g = rng.integers(1, ntiles + 1, (rows, cols)).astype(np.uint32)
    g |= rng.integers(0, 4, (rows, cols)).astype(np.uint32) << 30
    g[rng.random((rows, cols)) < empty] = 0
    return g


def spoil(g, ntiles, set_cols, max_tx, at):
    """one cell of each refusal term at the (r, c) of `at` (those inside the grid): bit 29, bit 28, an id one past the
    set, flag bits alone, and -- where the set has more columns than fit -- a column beyond max_tx"""
    words = [1 | T.DIAGONAL, 2 | T.HEXAGONAL | T.FLIP_X, ntiles + 1, T.FLIP_Y]
    if set_cols > max_tx + 1:
        words.append(max_tx + 2)  # t = max_tx + 1 < set_cols: tx = max_tx + 1
    for (r, c), w in zip(at, words):
        if r < g.shape[0] and c < g.shape[1]:
            g[r, c] = w
    return g


def case(name, W, H, tile, set_tiles, rows, cols, origin, seed, margin=0, spacing=0, extra_cols=0, window=None):
    """set_tiles: (columns, rows) of tiles in the atlas; extra_cols: set_cols is that much more than fits; window:
    (r0, c0, world_rows, world_cols) puts the grid into a larger world tensor (pitch_cells > cols)"""
    AW, AH = set_size(tile, set_tiles[0], set_tiles[1], margin, spacing)
    set_cols = None if not extra_cols else set_tiles[0] + extra_cols
    sc = set_tiles[0] + extra_cols
    ntiles = sc * set_tiles[1]
    g = grid(rows, cols, ntiles if not extra_cols else set_tiles[0], seed)
    m = T.layer(tile, origin, set_cols, margin, spacing, TINT)
    # the spoiled cells go where the target is (the first visible cells), so that they are counted
    c0, c1, r0, r1 = T.visible(m, rows, cols, W, H)
    if c0 <= c1 and r0 <= r1:
        at = [(r0 + k // 3, c0 + k % 3) for k in range(1, 6)]
        spoil(g, ntiles, sc, set_tiles[0] - 1, at)
        g[r0, c0] = 3 | T.FLIP_X | T.FLIP_Y  # the first visible cell is drawn in every case, turned half round
    return dict(name=name, W=W, H=H, AW=AW, AH=AH, cells=g, m=m, window=window)


def edge_cases():
    big, small = (200, 72), (64, 48)
    out = [
        case("1x1", *small, (1, 1), (9, 7), 60, 70, (-3, -2), 1),
        case("3x5", *small, (3, 5), (6, 4), 12, 30, (-4, 3), 2),
        case("16x16 boundary on 63", *big, (16, 16), (4, 3), 6, 14, (-1, -5), 3),
        case("16x16 boundary on 64 and 128", *big, (16, 16), (4, 3), 6, 14, (0, 0), 4),
        case("16x16 boundary on 65", *big, (16, 16), (4, 3), 6, 14, (1, 7), 5),
        case("7x64", *big, (7, 64), (5, 2), 3, 40, (-5, -30), 6),
        case("300x100 tile", *big, (300, 100), (2, 2), 2, 2, (-120, -20), 7),
        case("smaller than the target", *big, (16, 16), (4, 3), 2, 3, (20, 10), 8),
        case("much larger than the target", *small, (16, 16), (4, 3), 200, 300, (-2000, -1500), 9),
        case("off to the right", *small, (16, 16), (4, 3), 4, 4, (64, 0), 10),
        case("off to the left by one", *small, (16, 16), (4, 3), 4, 4, (-64, 5), 11),
        case("off below", *small, (16, 16), (4, 3), 4, 4, (3, 48), 12),
        case("off above, far", *small, (16, 16), (4, 3), 4, 4, (3, -(1 << 22)), 13),
        case("a window of a larger world", *big, (16, 16), (4, 3), 5, 9, (10, -3), 14, window=(3, 2, 11, 17)),
        case("margin 1, spacing 2", *big, (16, 16), (3, 2), 6, 14, (-7, -9), 15, margin=1, spacing=2),
        case("a set_cols beyond the atlas", *small, (16, 16), (4, 3), 4, 5, (-3, -3), 16, extra_cols=2),
        case("one pixel of one cell", *small, (16, 16), (4, 3), 1, 1, (63, 47), 17),
    ]
    return out


def narrowed_garbage(rows, cols, ntiles, seed):
    """seeded random words with the id reduced modulo twice the tile count and the four flag bits random: about one
    cell in eight is accepted (half the ids, a quarter of the flag nibbles)"""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 1 << 32, (rows, cols), dtype=np.uint64)
    return ((raw & 0xF0000000) | ((raw & 0x0FFFFFFF) % (2 * ntiles))).astype(np.uint32)


def raw_garbage(rows, cols, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 32, (rows, cols), dtype=np.uint64).astype(np.uint32)


GARBAGE = dict(W=200, H=72, tile=(16, 16), set_tiles=(4, 3), rows=7, cols=15, origin=(-9, -11))
