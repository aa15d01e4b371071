"""GPU: row-strip shards (rc2dgi_do_group) on thin strips and under every level schedule, bit for bit against the
unsharded frame.

The row window a shard adds to the kernels -- p0 / p1 in the level kernels, row0 / row1 / m0 / m1 in blur and merge,
strip windows and block buffers in JumpFlood -- is run here where test_gpu_shard.py does not take it: strips of one
to four rows (every JumpFlood step a block step, block requests gathered from several owners, strip-sized textures of
one row under 32-row tiles), every tile variant, proof, workgroup order and blur path on windows that start at odd
rows and cut the last tile, block fills on an unbanded shard, three storage formats throughout.
tests/test_shard_edges_cpu.py shows with the host-only planners that the shapes (tests/shard_edge_cases.py) reach
those paths.

Reference: the unsharded context on its default schedule (shard_compare.whole_frame), itself compared once a shape
with oracle.frame on color, temp, dist, final_gi and every level.  Shards run with poison 1: a row that was not
computed reads as NaN.  Every comparison is on the 32-bit patterns; there is no tolerance.
"""
import numpy as np
import pytest

import oracle
import wild_inputs as wi
from shard_compare import assert_shard_levels, assert_shard_matches_whole, bits, level_rows, whole_frame
from shard_edge_cases import FILL, ORDER_CODES, STORAGES, SWEEPS, THIN, thin_id

pytestmark = pytest.mark.gpu

E_STATE = -6


@pytest.fixture(scope="module")
def R():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from radiancecascade2dglobalillumination_amd import rc2dgi

    return rc2dgi


# ---------------------------------------------------------------- the reference, computed once a shape and shared
_REF = {}


def reference(R, W, H, N, rr, rs, blur, storage, seed, linux_merge=False):
    """(color, emissive, whole_frame with levels) of a shape, the unsharded frame checked against the oracle; never
    written to afterwards."""
    key = (W, H, N, rr, rs, blur, storage, seed, linux_merge)
    if key not in _REF:
        from radiancecascade2dglobalillumination_amd import scenes

        color, emis = scenes.random_scene(W, H, seed)
        want = whole_frame(R, W, H, N, rr, rs, blur, color, emis, storage, keep_levels=True,
                           linux_merge_fallback=linux_merge)
        p = oracle.Params(W=W, H=H, N=N, ray_range=rr, render_scale=rs, blur_radius=blur, gi_f16=storage == "f16",
                          rgba8=storage == "rgba8", linux_merge=linux_merge)
        fr = oracle.frame(p, color, emis, keep_levels=True)
        what = f"unsharded {W}x{H} N={N} rs={rs} blur={blur} {storage}"
        for k, o in (("color", fr.color_out), ("temp", fr.temp), ("dist", fr.dist), ("final_gi", fr.gi_final)):
            assert np.array_equal(want[k], o), f"{what}: {k} differs from the oracle's"
        for L in range(N):
            assert np.array_equal(want["levels"][L], fr.gi_levels[L]), f"{what}: level {L} differs from the oracle's"
        for a in list(want.values()):
            for t in (a if isinstance(a, list) else [a]):
                if isinstance(t, np.ndarray):
                    t.setflags(write=False)
        _REF[key] = (color, emis, want)
    return _REF[key]


def make_shards(R, W, H, N, rr, rs, blur, world, color, emis, storage="f32", linux_merge=False, uniforms=None):
    ctxs = []
    for k in range(world):
        c = R.RC2DGI(W, H, cascade_count=N, render_scale=rs, ray_range=rr, storage=storage,
                     linux_merge_fallback=linux_merge)
        ctxs.append(c)
        c.set_shader_value("_BlurRadius", blur)
        for name, value in (uniforms or {}).items():
            c.set_shader_value(name, value)
        c.set_shard(k, world)
        c.set_keep_levels(True)
        c.set_tuning("poison", 1)
        c.upload("color", color)
        c.upload("emissive", emis)
    return ctxs


def close_all(ctxs):
    for c in ctxs:
        c.close()


def group_frame(R, ctxs):
    R.do_group(ctxs)
    for c in ctxs:
        c.sync()


def level_keys(c, key):
    """The keys `key` reads back through: itself, or (a key that sets every level at once cannot be read) its
    per-level keys"""
    try:
        c.get_tuning(key)
        return [key]
    except RuntimeError:  # (RC2DGIError: E_ARG, the key cannot be read)
        return [f"{key}_L{L}" for L in range(c.cascade_count)]


def set_all(ctxs, key, value):
    for c in ctxs:
        c.set_tuning(key, value)
        assert all(c.get_tuning(k) == value for k in level_keys(c, key)), key


def fused_blur_merge(W, H, rs, blur, storage="f32", linux_merge=False, blur_path=0):
    """Whether a shard of this shape runs the fixed-tap blur with the merge fused, on strip-sized textures: power-of-two
    cascades the size of the screen from 64 x 32 up, not RGBA8, a dyadic radius below 3, raylib's merge shader,
    blur_path 0."""
    pow2 = (W & (W - 1)) == 0 and (H & (H - 1)) == 0 and W >= 64 and H >= 32
    return int(pow2 and rs == 1.0 and storage != "rgba8" and blur in (0.5, 1.0, 1.5, 2.0, 2.5) and not linux_merge
               and blur_path == 0)


def check_group(ctxs, want, W, H, N, rs, blur, sized, what):
    world = len(ctxs)
    for k, c in enumerate(ctxs):
        try:
            assert_shard_levels(c, want["levels"], W, H, N, blur, k, world, rs)
            assert_shard_matches_whole(c, want, W, H, blur, expect_strip_tables=False, strip_sized=sized)
        except AssertionError as e:
            raise AssertionError(f"{what}: {e}") from None


# ---------------------------------------------------------------- thin strips
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("case", THIN, ids=thin_id)
def test_thin_strips_match_the_whole_frame(R, case, storage):
    """Strips of one to four rows, two frames each (the second checks the cross-frame ordering of the exchange): the
    merged rows, the JumpFlood rows, distRT, the blur textures' own rows and every level on its planned rows."""
    W, H, N, rr, rs, blur, world, linux = case[:8]
    color, emis, want = reference(R, W, H, N, rr, rs, blur, storage, seed=41, linux_merge=linux)
    sized = fused_blur_merge(W, H, rs, blur, storage, linux)
    if (W, H, rs, blur, linux) == (128, 64, 1.0, 1.5, False) and storage != "rgba8":
        assert sized == 1  # the fused case: BLUR / FINAL_GI of one or two rows
    if linux:
        assert sized == 0  # (no strip-sized textures without the fused merge)
    ctxs = make_shards(R, W, H, N, rr, rs, blur, world, color, emis, storage, linux)
    try:
        for frame in range(2):
            group_frame(R, ctxs)
            check_group(ctxs, want, W, H, N, rs, blur, sized, f"{thin_id(case)} {storage} frame {frame}")
    finally:
        close_all(ctxs)


# ---------------------------------------------------------------- level schedules under a row window
def sweep_id(s):
    return f"{s.W}x{s.H}-N{s.N}-w{s.world}"


def sweep_shards(R, s, storage):
    W, H, N, rr, blur, world = s
    color, emis, want = reference(R, W, H, N, rr, 1.0, blur, storage, seed=42)
    return make_shards(R, W, H, N, rr, 1.0, blur, world, color, emis, storage), want


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("s", SWEEPS, ids=sweep_id)
def test_every_rc_variant_under_a_row_window(R, s, storage):
    """Every tile variant on every level of three shards: the levels on their planned rows and the merged rows equal
    the unsharded frame on its default schedule (results do not depend on the variant)."""
    W, H, N, _rr, blur, _world = s
    ctxs, want = sweep_shards(R, s, storage)
    sized = fused_blur_merge(W, H, 1.0, blur, storage)
    try:
        nv = ctxs[0].get_tuning("rc_variant_count")
        assert nv == 26
        for v in range(nv):
            for c in ctxs:
                c.set_tuning("rc_variant", v)
                assert c.get_tuning(f"rc_variant_L{N - 1}") == v and c.get_tuning("rc_variant_L0") == v
            for frame in range(2 if v == 0 else 1):
                group_frame(R, ctxs)
                check_group(ctxs, want, W, H, N, 1.0, blur, sized, f"{sweep_id(s)} {storage} variant {v}")
    finally:
        close_all(ctxs)


def knob_frames(s, group):
    """[(what, [(key, value), ...])] of one sweep group: the settings of a frame on top of the defaults"""
    N = s.N
    if group == "proofs":
        out = [(f"rc_skip {v}", [("rc_skip", v)]) for v in (0, 1, 2, 3)]
        for skip in (1, 3):  # (the default leaves the proofs off at these sizes: every knob of theirs also with them on)
            base = [("rc_skip", skip)]
            out += [(f"rc_skip {skip} rc_mp {v}", base + [("rc_mp", v)]) for v in (0, 1)]
            out += [(f"rc_skip {skip} rc_tail {v}", base + [("rc_tail", v)]) for v in (-1, 0, 10)]
            out += [(f"rc_skip {skip} rc_wgproof {v}", base + [("rc_wgproof", v)]) for v in (0, 1)]
            out += [(f"rc_skip {skip} rc_noproof_L{L}", base + [(f"rc_noproof_L{L}", 1)]) for L in range(N)]
        return out
    if group == "paths":
        out = [(f"blur_path {v}", [("blur_path", v)]) for v in (0, 1, 2)]
        out += [(f"jfa_tab {v}", [("jfa_tab", v)]) for v in (0, 1, 2)]
        if (s.W, s.H) == (333, 200):
            out += [(f"rc_rdiv {v}", [("rc_rdiv", v)]) for v in (0, 1)]
        return out
    if group == "orders":
        return [(f"rc_order {code:#x}", [(f"rc_order_L{L}", code) for L in range(N)]) for code in ORDER_CODES]
    assert group == "ignored"  # knobs a shard leaves off by design: they set, read back and change nothing
    return [(f"{k} {v}", [(k, v)]) for k, v in (("rc_chain", 1), ("jfa_lds", 1), ("jfa_rows", 4), ("jfa_rows", 8),
                                                 ("jfa_rt", 2), ("jfa_rt", 4), ("jfa_coset", 0), ("jfa_coset", 1),
                                                 ("jfa_tail", 2), ("jfa_tail", 3), ("jfa_tail", 4))]


@pytest.mark.parametrize("group", ["proofs", "paths", "orders", "ignored"])
@pytest.mark.parametrize("s", SWEEPS, ids=sweep_id)
def test_knob_sweeps_under_a_row_window(R, s, group):
    """The proofs, blur paths, JumpFlood texcoord modes and workgroup orders on f32 shards, each setting on top of the
    defaults and read back; then the defaults again."""
    W, H, N, _rr, blur, _world = s
    ctxs, want = sweep_shards(R, s, "f32")
    try:
        for what, settings in knob_frames(s, group) + [("defaults again", [])]:
            defaults = [(r, ctxs[0].get_tuning(r)) for k, _ in settings for r in level_keys(ctxs[0], k)]
            for k, v in settings:
                set_all(ctxs, k, v)
            path = dict(settings).get("blur_path", 0)
            group_frame(R, ctxs)
            check_group(ctxs, want, W, H, N, 1.0, blur, fused_blur_merge(W, H, 1.0, blur, blur_path=path),
                        f"{sweep_id(s)} {what}")
            if what.startswith("rc_chain"):
                assert all(c.get_tuning("rc_chain_timeouts") == 0 for c in ctxs)
            for k, v in defaults:
                set_all(ctxs, k, v)
    finally:
        close_all(ctxs)


def test_autotune_on_a_shard_is_refused(R):
    """rc2dgi_autotune times whole frames: on a shard it is RC2DGI_E_STATE, and the next group frame is right."""
    s = SWEEPS[0]
    W, H, N, _rr, blur, _world = s
    ctxs, want = sweep_shards(R, s, "f32")
    try:
        orders = [ctxs[0].get_tuning(f"rc_order_L{L}") for L in range(N)]
        for c in ctxs:
            with pytest.raises(R.RC2DGIError) as e:
                c.autotune(1)
            assert e.value.code == E_STATE
        assert [ctxs[0].get_tuning(f"rc_order_L{L}") for L in range(N)] == orders
        group_frame(R, ctxs)
        check_group(ctxs, want, W, H, N, 1.0, blur, fused_blur_merge(W, H, 1.0, blur), "after autotune")
    finally:
        close_all(ctxs)


def test_the_comparisons_are_not_vacuous(R):
    """One flipped bit in a planned row of one level, or in an own row of colorRT, is noticed; and a shard's level
    texture holds NaN (the poison) on rows outside its plan, so the planned rows are what the shard computed."""
    s = SWEEPS[0]
    W, H, N, _rr, blur, world = s
    ctxs, want = sweep_shards(R, s, "f32")
    try:
        group_frame(R, ctxs)
        check_group(ctxs, want, W, H, N, 1.0, blur, 1, "unchanged reference")
        k, L = 1, 2
        rows = level_rows(R, W, H, N, blur, k, world, 1.0, L, H)
        got = ctxs[k].download_level(L)
        outside = np.setdiff1d(np.arange(H), rows)
        assert len(outside) > 0 and np.isnan(got[outside]).any(), "no poisoned row outside the plan"
        assert not np.isnan(got[rows]).any()
        levels = [a.copy() for a in want["levels"]]
        levels[L][rows[-1], W - 1, 2] = np.nextafter(levels[L][rows[-1], W - 1, 2], np.float32(np.inf))
        with pytest.raises(AssertionError, match=f"level {L}: 1 values differ"):
            assert_shard_levels(ctxs[k], levels, W, H, N, blur, k, world, 1.0)
        y0, y1 = ctxs[k].shard_rows()
        flipped = dict(want, color=want["color"].copy())
        flipped["color"][y1 - 1, 0, 0] = np.nextafter(flipped["color"][y1 - 1, 0, 0], np.float32(-np.inf))
        with pytest.raises(AssertionError, match="color: 1 values differ"):
            assert_shard_matches_whole(ctxs[k], flipped, W, H, blur, expect_strip_tables=False, strip_sized=1)
    finally:
        close_all(ctxs)


# ---------------------------------------------------------------- filled levels on an unbanded shard
@pytest.mark.parametrize("fill,below", [(1, 13), (1, 6), (0, 13)])
def test_block_fills_on_an_unbanded_shard(R, fill, below):
    """512^2, N = 8, rayRange 64: the top levels' rays start off screen and launch_rc_fill writes the shard's rows of
    them into whole (unbanded) cascade textures; rc_fill 0 marches the same levels under the row window.  below: the
    variant of level 5, the level under the fills (13: the default; 6: the 32 x 8 x 2 tiles, which merge with the
    filled level's block values instead of staging its texture)."""
    W, H, N, rr, blur, world = FILL
    color, emis, want = reference(R, W, H, N, rr, 1.0, blur, "f32", seed=43)
    assert want["rc_fill_levels"] == 0b11000000, bin(want["rc_fill_levels"])
    ctxs = make_shards(R, W, H, N, rr, 1.0, blur, world, color, emis)
    try:
        set_all(ctxs, "rc_fill", fill)
        set_all(ctxs, "rc_variant_L5", below)
        for frame in range(2):
            group_frame(R, ctxs)
            for c in ctxs:
                assert c.get_tuning("cascade_banded") == 0
                assert c.get_tuning("rc_fill_levels") == (want["rc_fill_levels"] if fill else 0)
            check_group(ctxs, want, W, H, N, 1.0, blur, 1, f"rc_fill {fill} frame {frame}")
    finally:
        close_all(ctxs)


# ---------------------------------------------------------------- odd radiance: a shard redoes its rows as the whole frame
ODD_SHAPES = [(128, 128, 4, 1.0), (256, 256, 4, 0.5)]  # fused and strip-sized; the fused blur, the merge on its own
ODD_WORLD = 4
# planted: NaN and infinities in records that rays hit.  huge: test_gpu_inputs.py's, every input finite, the emission
# scaled by 1e33.  overflow: the same scaled by 3.3e33, every input still finite, where G_0 itself overflows.
ODD_KINDS = ("planted", "huge", "overflow")


def odd_inputs(W, H, kind):
    from test_gpu_inputs import plant_non_finite

    color, emis = wi.wild_scene(W, H, wi.SEEDS[(128, 128)])
    if kind == "planted":
        plant_non_finite(color, emis)
    else:
        emis[..., :3] *= np.float32(1e33 if kind == "huge" else 3.3e33)
        assert np.isfinite(emis).all() and np.isfinite(color).all()
    return color, emis


def dilate2(mask):
    """Texels within a Chebyshev distance of 2 of a set texel, with REPEAT wrap"""
    out = np.zeros_like(mask)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            out |= np.roll(np.roll(mask, dy, 0), dx, 1)
    return out


def linear_footprint(n_dst, n_src):
    """The two source texels (wrapped) a LINEAR sample at the centre of each of n_dst texels reads on an axis of n_src"""
    f = np.floor((np.arange(n_dst) + 0.5) * (n_src / n_dst) - 0.5).astype(np.int64)
    return f % n_src, (f + 1) % n_src


def sampled_rows(y0, y1, H, CH):
    """The cascade rows (wrapped) whose blur / final_gi a shard is compared on: its own rows when the cascade is the
    screen (all it holds on strip-sized textures), else the rows the LINEAR samples of its merged rows read."""
    if CH == H:
        return np.arange(y0, y1)
    lo = int(np.floor((y0 + 0.5) * (CH / H) - 0.5))
    hi = int(np.floor((y1 - 0.5) * (CH / H) - 0.5)) + 1
    return np.arange(lo, hi + 1) % CH


_ODD = {}


def odd_run(R, W, H, N, rs, kind):
    """Two group frames of ODD_WORLD shards on an odd input against the whole frame, run once a case and shared by
    the tests below.  JumpFlood, distRT and the levels are asserted here (bit-equal on the own / planned rows).
    Returns (records, shards with a NaN of the whole frame's final_gi in their rows); a record counts, for one frame,
    shard and texture of blur / final_gi (on the cascade rows the shard's merged rows sample) and temp / color (own
    rows):
      off_nan   values whose bits differ although the whole frame's value is no NaN
      differ    texels with a value that is no NaN where the whole frame's is NaN
      far       those of them further than 2 texels (Chebyshev, REPEAT wrap) from a texel whose level 0, blur or
                final_gi is non-finite in the whole frame; for a screen texture over a coarser cascade the distance
                is taken in cascade texels from the texel's LINEAR footprint
      unequal   values whose bits differ at all, a NaN's sign and payload included"""
    key = (W, H, N, rs, kind)
    if key in _ODD:
        return _ODD[key]
    uniforms = {"_Reflectivity": wi.REFLECTIVITY}
    color, emis = odd_inputs(W, H, kind)
    want = whole_frame(R, W, H, N, 2.0, rs, 1.5, color, emis, keep_levels=True, uniforms=uniforms)
    CH, CW = want["final_gi"].shape[:2]
    g0 = want["levels"][0]
    bad = ~(np.isfinite(g0).all(-1) & np.isfinite(want["blur"]).all(-1) & np.isfinite(want["final_gi"]).all(-1))
    near = dilate2(bad)  # (cascade texels)
    fy, fx = linear_footprint(H, CH), linear_footprint(W, CW)
    fin_nan = np.isnan(want["final_gi"]).any(-1)
    near_screen = np.zeros((H, W), bool)
    for ry in fy:
        for rx in fx:
            near_screen |= near[ry][:, rx]
    if (CW, CH) == (W, H):
        near_screen = near
    if kind == "huge":
        assert np.isfinite(g0).all() and np.count_nonzero(np.abs(g0) >= 2.0 ** 30) >= 100
        assert not bad.any()
    ctxs = make_shards(R, W, H, N, 2.0, rs, 1.5, ODD_WORLD, color, emis, uniforms=uniforms)
    records, hit = [], 0
    try:
        assert all(c.get_tuning("blur_strip_sized") == int(rs == 1.0) for c in ctxs)
        for frame in range(2):
            group_frame(R, ctxs)
            for k, c in enumerate(ctxs):
                y0, y1 = c.shard_rows()
                what = f"{kind} {W}x{H} rs {rs} shard {k} frame {frame}"
                for name in ("jump1", "jump2", "dist"):
                    got = c.download(name)[y0:y1]
                    assert np.array_equal(bits(got), bits(want[name][y0:y1])), f"{what}: {name}"
                for L in range(N):
                    rows = level_rows(R, W, H, N, 1.5, k, ODD_WORLD, rs, L, CH)
                    got = c.download_level(L)[rows]
                    assert np.array_equal(bits(got), bits(want["levels"][L][rows])), f"{what}: level {L}"
                crow = sampled_rows(y0, y1, H, CH)
                hit += int(frame == 0 and fin_nan[crow].any())
                for name in ("blur", "final_gi", "temp", "color"):
                    screen = name in ("temp", "color")
                    rows = np.arange(y0, y1) if screen else crow
                    got, ref = c.download(name)[rows], want[name][rows]
                    off = ~np.isnan(ref) & (bits(got) != bits(ref))
                    differ = (np.isnan(ref) & ~np.isnan(got)).any(-1)
                    allowed = (near_screen if screen else near)[rows]
                    rec = dict(what=what, name=name, off_nan=int(off.sum()), differ=int(differ.sum()),
                               far=int((differ & ~allowed).sum()), unequal=int((bits(got) != bits(ref)).sum()))
                    records.append(rec)
                    print(f"{what}: {name}: off_nan {rec['off_nan']} differ {rec['differ']} far {rec['far']} "
                          f"unequal {rec['unequal']}")
    finally:
        close_all(ctxs)
    _ODD[key] = (records, hit)
    return _ODD[key]


@pytest.mark.parametrize("kind", ODD_KINDS)
@pytest.mark.parametrize("W,H,N,rs", ODD_SHAPES)
def test_shards_on_odd_radiance(R, W, H, N, rs, kind):
    """Non-finite radiance, and finite G_0 values of 2^30 and more: the fused blur kernels' skipped weight-0 taps are
    an identity on finite values and 0 * NaN = NaN otherwise, so the unsharded frame is redone tap by tap
    (k_blur_exact).  Asked of every shard, on its own rows and planned level rows:
      - JumpFlood, distRT and every level are bit-equal to the whole frame;
      - in blur, final_gi, temp and color the shard's bits equal the whole frame's wherever that is not NaN;
      - where they differ (the whole frame NaN, the shard not) the texel lies within a Chebyshev distance of 2, with
        REPEAT wrap, of a texel whose level 0, blur or final_gi is non-finite in the whole frame (odd_run: far).
    Reference side.  planted, overflow: the whole frame's final_gi holds NaN in the rows of at least two shards.  huge:
    G_0 is all finite with at least 100 values >= 2^30 -- and then the whole frame is finite: the oracle shows no
    uniform scale with finite G_0 and a NaN after it (finite up to 2.8e33 at 128^2 and 2.6e33 at 256^2 x 0.5, G_0
    overflows from 2.9e33 and 2.7e33), so on this input the rule asks the shard for the whole frame's bits everywhere;
    `overflow` is the nearest input with a NaN, at the price of a non-finite G_0.

    A shard that kept the fused kernels' values missed the second point: merge.fs takes min(colour + GI, 1), and
    min(NaN, 1) is 1, so where the whole frame's final GI is NaN its tempRT / colorRT hold alpha * 1 -- no NaN -- and
    the shard, its final GI finite there, held min(colour + GI, 1) (planted, 256^2 at renderScale 0.5, shard 0: 4
    values each of temp and color).  A shard now redoes its rows as the whole frame does (the same
    kernel on the same G_0 rows), so the last assertion asks for more than the rule: every bit equal, NaNs too."""
    records, hit = odd_run(R, W, H, N, rs, kind)
    if kind != "huge":
        assert hit >= 2, f"the whole frame's final_gi holds NaN in the rows of {hit} shards"
    broke = [r for r in records if r["off_nan"] or r["far"]]
    assert not broke, "; ".join(f"{r['what']} {r['name']}: {r['off_nan']} values differ where the whole frame is no "
                                f"NaN, {r['far']} of {r['differ']} differing texels far from a non-finite value"
                                for r in broke)
    broke = [r for r in records if r["unequal"]]
    assert not broke, "; ".join(f"{r['what']} {r['name']}: {r['unequal']} values differ in bits" for r in broke)
