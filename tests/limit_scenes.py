"""Scenes for screens that are long and thin (one axis above 8192, the other a few texels), for
tests/test_limit_scenes_cpu.py and tests/test_gpu_limits.py.  scenes.random_scene sizes its shapes by min(W, H): on an
8-row screen its discs are below a texel and the frame is nearly the empty scene's.  Here walls cross the short axis at
positions along the long one, so that every cascade level hits something.  Every array is deterministic per
(W, H, seed)."""
import numpy as np

# positions along the long axis that always carry a wall (where they exist): either side of the JumpFlood key-mode and
# texcoord-table limits (4096, 8192), of the packed marches' gate (16384), and both ends of the screen
PINNED = (0, 4095, 4096, 8191, 8192, 8193, 16383, 16384, 16385)
WALL_EVERY = 96      # one random wall per this many texels of the long axis
EMISSIVE_SHARE = 3   # one wall in this many also emits


def wall_positions(L, rng):
    pos = {int(p) for p in rng.integers(0, L, max(1, L // WALL_EVERY))}
    pos.update(p for p in PINNED if p < L)
    pos.add(L - 1)
    return sorted(pos)


def wall_scene(W, H, seed):
    """(color, emissive) float32 (H, W, 4), channels k/255: one-texel walls across the short axis at wall_positions
    along the long axis.  A third of the walls span the short axis, the others a random part of it (the distance
    field then varies along the short axis too); every wall texel has its own random colour; one wall in three is
    also written, with colours of its own, into the emissive image.  Colour alpha is 1 everywhere, the emissive
    background (0, 0, 0, 0)."""
    rng = np.random.default_rng(seed)
    wide = W >= H
    L, S = (W, H) if wide else (H, W)
    col = np.zeros((L, S, 4), np.uint8)  # (long, short): transposed below for wide screens
    col[..., 3] = 255
    emi = np.zeros((L, S, 4), np.uint8)
    for p in wall_positions(L, rng):
        a, b = 0, S
        if rng.integers(0, 3) != 0 and S > 1:  # partial: [a, b) a proper part of the short axis
            a = int(rng.integers(0, S - 1))
            b = a + 1 + int(rng.integers(0, S - 1 - a)) if a > 0 else 1 + int(rng.integers(0, S - 1))
        col[p, a:b, :3] = rng.integers(1, 256, size=(b - a, 3))
        if rng.integers(0, EMISSIVE_SHARE) == 0:
            emi[p, a:b, :3] = rng.integers(1, 256, size=(b - a, 3))
            emi[p, a:b, 3] = 255
    if wide:
        col, emi = col.transpose(1, 0, 2), emi.transpose(1, 0, 2)
    to_f = lambda a: np.ascontiguousarray(a.astype(np.float32) / np.float32(255.0))  # noqa: E731
    return to_f(col), to_f(emi)


def wall_columns(dist, wide):
    """The positions along the long axis where distRT holds a wall texel (q == 0: the texel is its own seed)."""
    q0 = (dist[..., 0] == 0) & (dist[..., 1] == 0)
    return np.flatnonzero(q0.any(axis=0 if wide else 1))


# The thin shapes of tests/test_gpu_limits.py: (W, H, N, rayRange, seed).  rayRange and seed are chosen so that
# tests/test_limit_scenes_cpu.py holds (every cascade level differs from the empty scene's on >= 2 % of its texels).
THIN_SHAPES = [
    (32768, 8, 3, 8.0, 1),
    (8, 32768, 4, 8.0, 2),
    (16, 16384, 5, 8.0, 3),
    (16384, 16, 4, 8.0, 4),
    (16, 32768, 4, 8.0, 5),
    (32768, 16, 4, 8.0, 6),
    (20000, 12, 4, 8.0, 7),
    (12, 20000, 4, 8.0, 8),
    (32767, 6, 3, 8.0, 9),
    (12, 8200, 3, 8.0, 10),
]


def thin_case(W, H):
    """(N, rayRange, seed) of the thin shape W x H."""
    return next((n, rr, s) for (w, h, n, rr, s) in THIN_SHAPES if (w, h) == (W, H))
