"""CPU: the wall scenes of tests/limit_scenes.py give the thin screens of tests/test_gpu_limits.py something to hit.

A condition on the reference alone (the CPU oracle), not a measurement of the library: a GPU parity test on a frame
whose rays never hit anything would pass on the sky alone.  For every thin shape, with the rayRange and seed the GPU
tests use, every cascade level differs from the oracle's frame of scenes.empty on at least 2 % of its texels, and the
distance field holds walls at both ends of the long axis and at the positions 8192 and 16384.

Smallest per-level share the oracle reached (the top level each time), as run for this file:
  32768 x 8 N 3: 7.3 %    8 x 32768 N 4: 4.1 %    16 x 16384 N 5: 5.7 %   16384 x 16 N 4: 7.0 %
  16 x 32768 N 4: 7.1 %   32768 x 16 N 4: 7.0 %   20000 x 12 N 4: 5.7 %   12 x 20000 N 4: 5.5 %
  32767 x 6 N 3: 5.5 %    12 x 8200 N 3: 7.1 %
with occluders on 0.53 to 0.63 % of the texels."""
import numpy as np
import pytest

import oracle
from limit_scenes import PINNED, THIN_SHAPES, wall_columns, wall_positions, wall_scene

MIN_SHARE = 0.02


@pytest.mark.parametrize("W,H,N,rr,seed", THIN_SHAPES)
def test_every_level_of_a_thin_shape_hits_walls(W, H, N, rr, seed):
    from radiancecascade2dglobalillumination_amd import scenes

    p = oracle.Params(W=W, H=H, N=N, ray_range=rr)
    color, emis = wall_scene(W, H, seed)
    fr = oracle.frame(p, color, emis, keep_levels=True)
    fe = oracle.frame(p, *scenes.empty(W, H), keep_levels=True)
    shares = [float(np.any(a != b, axis=-1).mean()) for a, b in zip(fr.gi_levels, fe.gi_levels)]
    print(f"{W}x{H} N={N} rayRange={rr}: smallest per-level share {min(shares):.4f} ({[round(s, 4) for s in shares]})")
    for L, s in enumerate(shares):
        assert s >= MIN_SHARE, f"level {L}: {s:.4%} of the texels differ from the empty scene's"
    # the boundary walls reach the distance field
    long_axis = max(W, H)
    cols = set(wall_columns(fr.dist, W >= H).tolist())
    for pos in (0, 8192, 16384, long_axis - 1):
        if pos < long_axis:
            assert pos in cols, f"no wall at {pos} in distRT"


@pytest.mark.parametrize("W,H", [(32768, 8), (8, 32768), (12, 8200)])
def test_wall_scene_is_as_described(W, H):
    seed = 3
    color, emis = wall_scene(W, H, seed)
    again = wall_scene(W, H, seed)
    assert np.array_equal(color, again[0]) and np.array_equal(emis, again[1])  # deterministic
    wide = W >= H
    L, S = max(W, H), min(W, H)
    occ = np.any(color[..., :3] > 0, axis=-1)
    along = occ.sum(axis=0 if wide else 1)  # wall texels per position of the long axis
    pos = np.flatnonzero(along)
    assert pos.tolist() == wall_positions(L, np.random.default_rng(seed))
    for q in PINNED + (L - 1,):
        if q < L:
            assert along[q] > 0, q
    assert L // 96 <= len(pos) <= L // 96 + len(PINNED) + 1
    assert np.any(along[pos] == S) and np.any(along[pos] < S)  # full and partial walls
    lit = np.any(emis[..., :3] > 0, axis=-1)
    assert not np.any(lit & ~occ)  # only walls emit
    n_lit = np.count_nonzero(lit.any(axis=0 if wide else 1))
    assert 0.2 * len(pos) <= n_lit <= 0.5 * len(pos)  # about a third
    k255 = np.arange(256, dtype=np.float32) / np.float32(255)
    assert np.isin(color, k255).all() and np.isin(emis, k255).all()
    assert np.all(color[..., 3] == 1)
    assert len(np.unique(color[occ][:, :3], axis=0)) > 0.9 * occ.sum()  # every wall texel its own colour
