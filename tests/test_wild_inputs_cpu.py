"""No GPU: the inputs of tests/wild_inputs.py do reach the arithmetic they are meant for, on the oracle alone --
so that the GPU tests built on them (test_gpu_inputs.py, test_gpu_live.py) cannot pass vacuously.  For every
(size, seed, storage) of the parity matrix and the small cases beside it: every output finite, every class of
wild_scene among the hittable texels, most merged colorRT texels translucent; an RGBA16F case that saturates at
65504 and one that stores half subnormals."""
import numpy as np
import pytest

import oracle
import wild_inputs as wi

# the matrix, the schedules' size, the small shard case, the live contexts' sizes (200 x 120 is in the matrix; the
# 4096^2 frames count their classes on the GPU, on their own distRT: the oracle's whole frame takes too long here)
SIZES = wi.MATRIX_SIZES + [(256, 192, 5, 1.0), (200, 122, 3, 1.0), (256, 256, 6, 1.0), (1200, 900, 6, 1.0)]
_frames = {}


def frame_of(W, H, N, rs, storage):
    """One oracle frame per case, shared by the tests below and left unchanged."""
    key = (W, H, N, rs, storage)
    if key not in _frames:
        color, emis = wi.matrix_inputs(W, H, storage)
        fr = oracle.frame(wi.matrix_params(W, H, N, rs, storage), color, emis, keep_levels=True)
        _frames[key] = (color, emis, fr)
    return _frames[key]


def textures(fr):
    return [fr.color_out, fr.temp, fr.jump1, fr.jump2, fr.dist, fr.gi1, fr.gi2, fr.blur] + list(fr.gi_levels)


@pytest.mark.parametrize("storage", wi.STORAGES)
@pytest.mark.parametrize("W,H,N,rs", SIZES)
def test_outputs_are_finite_and_mostly_translucent(W, H, N, rs, storage):
    _, _, fr = frame_of(W, H, N, rs, storage)
    for k, t in enumerate(textures(fr)):
        assert np.isfinite(t).all(), f"texture {k} holds a non-finite value"
    share = float(np.mean(fr.color_out[..., 3] != 1))
    assert share >= 0.40, f"only {share:.1%} of the merged colorRT texels have alpha != 1"


@pytest.mark.parametrize("W,H,N,rs", [s for s in SIZES if s[0] * s[1] >= wi.CENSUS_MIN_TEXELS])
def test_every_class_is_hit(W, H, N, rs):
    """>= 8 hittable texels of every class of both tables, in the float inputs (RGBA8 texels have no such classes).
    17 x 5 is left out: its 85 texels cannot hold 12 classes of 8."""
    color, emis, fr = frame_of(W, H, N, rs, "f32")
    cen = wi.census(color, emis, fr.dist)
    for table, names in (("color", wi.COLOR_CLASSES), ("emis", wi.EMIS_CLASSES)):
        for name in names:
            assert cen[table][name] >= 8, f"{W}x{H} seed {wi.SEEDS[(W, H)]}: {table} class {name}: {cen}"
    # the record rule's edges, counted with the rule itself
    rec = wi.records(color, emis, wi.REFLECTIVITY)[wi.hittable(fr.dist)]
    assert np.count_nonzero(rec[:, 3] == 1) >= 8 and np.count_nonzero(rec[:, 3] != 1) >= 8


def test_wild_scene_is_deterministic_and_as_described():
    a, b = wi.wild_scene(96, 80, 3), wi.wild_scene(96, 80, 3)
    assert wi.bits_equal(a[0], b[0]) and wi.bits_equal(a[1], b[1])
    color, emis = a
    assert np.isfinite(color).all() and np.isfinite(emis).all()
    assert set(np.unique(color[..., 3]).tolist()) == set(wi.ALPHAS.tolist())
    bg = np.all(color[..., :3].view(np.uint32) == wi.BACKGROUND.view(np.uint32), -1)
    assert 0.1 < bg.mean() < 0.25 and not np.any(color[bg][:, :3] > 0)
    # in range, as_rgba8 is oracle.from_u8(oracle.to_u8(.))
    x = np.linspace(0, 1, 4001, dtype=np.float32)
    assert wi.bits_equal(wi.as_rgba8(x), oracle.from_u8(oracle.to_u8(x)))
    assert wi.as_rgba8(np.float32([1.5, -0.25])).tolist() == oracle.from_u8(np.uint8([126, 192])).tolist()
    assert not wi.bits_equal(np.float32([0.0]), np.float32([-0.0])) and wi.bits_equal(np.float32([-0.0]), np.float32([-0.0]))


def test_a_half_case_saturates():
    hits = []
    for (W, H, N, rs) in wi.MATRIX_SIZES:
        _, _, fr = frame_of(W, H, N, rs, "f16")
        hits.append(any(np.any(np.abs(g) == wi.HALF_MAX) for g in fr.gi_levels))
    assert any(hits), "no RGBA16F case stores 65504"
    # and the f32 frames of the same inputs go beyond it: the saturation is the store's, not the scene's
    _, _, fr = frame_of(*wi.MATRIX_SIZES[hits.index(True)], "f32")
    assert max(float(np.abs(g).max()) for g in fr.gi_levels) > wi.HALF_MAX


def faint_frame():
    f = wi.FAINT
    color, emis = wi.faint_scene(f["W"], f["H"], f["seed"])
    p = oracle.Params(W=f["W"], H=f["H"], N=f["N"], sky_radiance=f["sky_radiance"], gi_f16=True,
                      reflectivity=wi.REFLECTIVITY)
    return p, color, emis


def test_the_faint_case_stores_half_subnormals():
    p, color, emis = faint_frame()
    fr = oracle.frame(p, color, emis, keep_levels=True)
    counts = []
    for g in fr.gi_levels:
        a = np.abs(g[..., :3])
        counts.append(int(np.count_nonzero((a > 0) & (a < wi.HALF_MIN_NORMAL))))
    assert max(counts) >= 100, counts
