"""GPU: frames on inputs outside the class of scenes.py (tests/wild_inputs.py: translucent colour, HDR, negative,
denormal and signed-zero albedo and emission, a non-zero background that is no occluder), bit for bit against
oracle.frame on the same arrays -- the blended stores, the hit-record rule at its edges, the occupancy test, the
RGBA16F store over the whole half range, and where non-finite records end up.  tests/test_wild_inputs_cpu.py
shows on the oracle alone that these inputs reach what they are meant for.

Every comparison is on the 32-bit patterns (wild_inputs.bits_equal): -0.0 is not +0.0.
"""
import ctypes

import numpy as np
import pytest

import oracle
import wild_inputs as wi
from shard_compare import assert_shard_matches_whole, whole_frame

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from radiancecascade2dglobalillumination_amd import rc2dgi

    return rc2dgi


def storage_of(p):
    return "rgba8" if p.rgba8 else ("f16" if p.gi_f16 else "f32")


def make_ctx(R, p, **kw):
    ctx = R.RC2DGI(p.W, p.H, cascade_count=p.N, render_scale=p.render_scale, ray_range=p.ray_range,
                   storage=storage_of(p), linux_merge_fallback=p.linux_merge, **kw)
    ctx.set_shader_value("_SkyRadiance", p.sky_radiance)
    ctx.set_shader_value("_SkyColor", p.sky_color)
    ctx.set_shader_value("_SunColor", p.sun_color)
    ctx.set_shader_value("_SunAngle", p.sun_angle)
    ctx.set_shader_value("_Reflectivity", p.reflectivity)
    ctx.set_shader_value("_BlurRadius", p.blur_radius)
    ctx.set_keep_levels(True)
    return ctx


def frame_vs_oracle(R, p, color, emis, what):
    want = wi.oracle_textures(oracle.frame(p, color, emis, keep_levels=True))
    ctx = make_ctx(R, p)
    ctx.frame(color, emis)
    ctx.sync()
    got = wi.download_all(ctx, levels=p.N)
    ctx.close()
    wi.assert_bits(got, want, what)


# ---------------------------------------------------------------- parity matrix
@pytest.mark.parametrize("storage", wi.STORAGES)
@pytest.mark.parametrize("W,H,N,rs", wi.MATRIX_SIZES)
def test_wild_scene_matches_oracle(R, W, H, N, rs, storage):
    """128^2: the fused blur + merge; 96 x 80: separate passes; 200 x 120 at renderScale 0.5: cascades coarser
    than the screen; 17 x 5: ragged.  _Reflectivity 0.6, so albedo hits merge the upper level."""
    color, emis = wi.matrix_inputs(W, H, storage)
    frame_vs_oracle(R, wi.matrix_params(W, H, N, rs, storage), color, emis, f"{W}x{H} {storage}")


@pytest.mark.parametrize("reflectivity", [-0.0, 1.5])
def test_wild_scene_reflectivity_edges(R, reflectivity):
    """_Reflectivity -0.0: `radiance.a != 0` is false on albedo hits (and the records hold the sign bit); 1.5: the
    interval alphas leave [0, 1]."""
    W, H, N, rs = wi.MATRIX_SIZES[0]
    color, emis = wi.matrix_inputs(W, H, "f32")
    frame_vs_oracle(R, wi.matrix_params(W, H, N, rs, "f32", reflectivity), color, emis, f"reflectivity {reflectivity}")


def test_faint_scene_half_subnormal_stores(R):
    """The faint scene under a dark sky, RGBA16F: levels 1-3 store hundreds of half subnormals
    (test_wild_inputs_cpu.py counts them)."""
    f = wi.FAINT
    color, emis = wi.faint_scene(f["W"], f["H"], f["seed"])
    p = oracle.Params(W=f["W"], H=f["H"], N=f["N"], sky_radiance=f["sky_radiance"], gi_f16=True,
                      reflectivity=wi.REFLECTIVITY)
    frame_vs_oracle(R, p, color, emis, "faint f16")


# ---------------------------------------------------------------- schedules on wild records
SCHED = (256, 192, 5)


@pytest.fixture(scope="module")
def sched_scene():
    W, H, _ = SCHED
    return wi.wild_scene(W, H, wi.SEEDS[(W, H)])


def test_level_schedules_on_wild_records(R, sched_scene):
    """Tile variants x exit proofs x miss proofs on one context: every level of every schedule."""
    W, H, N = SCHED
    color, emis = sched_scene
    p = oracle.Params(W=W, H=H, N=N, reflectivity=wi.REFLECTIVITY)
    fr = oracle.frame(p, color, emis, keep_levels=True)
    ctx = make_ctx(R, p)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    for v in (0, 3, 6, 13, 18, 19):
        ctx.set_tuning("rc_variant", v)
        for skip in (0, 2):
            ctx.set_tuning("rc_skip", skip)
            for mp in (0, 1):
                ctx.set_tuning("rc_mp", mp)
                ctx.do_rc2dgi()
                ctx.sync()
                for L in range(N):
                    g = ctx.download_level(L)
                    assert wi.bits_equal(g, fr.gi_levels[L]), \
                        f"variant {v} rc_skip {skip} rc_mp {mp} level {L}: {wi.bits_differ(g, fr.gi_levels[L])}"
    ctx.close()


def test_blur_paths_on_wild_records(R, sched_scene):
    """blur_path 0, 1, 2 at a dyadic radius, a non-dyadic one and one beyond the fixed taps: the whole frame."""
    W, H, N = SCHED
    color, emis = sched_scene
    p = oracle.Params(W=W, H=H, N=N, reflectivity=wi.REFLECTIVITY)
    ctx = make_ctx(R, p)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    for radius in (1.5, 1.37, 3.0):
        p.blur_radius = radius
        want = wi.oracle_textures(oracle.frame(p, color, emis, keep_levels=True))
        ctx.set_shader_value("_BlurRadius", radius)
        for path in (0, 1, 2):
            ctx.set_tuning("blur_path", path)
            ctx.do_rc2dgi()
            ctx.sync()
            wi.assert_bits(wi.download_all(ctx, levels=N), want, f"_BlurRadius {radius} blur_path {path}")
    ctx.close()


def test_linux_merge_fallback_on_translucent_colour(R, sched_scene):
    """RC2DGI_FLAG_LINUX_MERGE_FALLBACK: the merge source is the colour texel itself, translucent here."""
    W, H, N = SCHED
    color, emis = sched_scene
    p = oracle.Params(W=W, H=H, N=N, reflectivity=wi.REFLECTIVITY, linux_merge=True)
    frame_vs_oracle(R, p, color, emis, "linux merge fallback")


# ---------------------------------------------------------------- the side pass at its smallest size
@pytest.fixture(scope="module")
def big_scene():
    W = H = 4096
    color, emis = wi.wild_scene(W, H, wi.SEEDS[(W, H)])
    return wi.signed_zero_pairs(color), emis


def test_side_pass_on_wild_records(R, big_scene):
    """4096^2, N = 6 (palettes, the split and fused records pass): rc_pal 1 against 0, shade_split and shade_fused 0
    against 1, on every level and output; the palette entries against the record rule restated in numpy, in bits
    (records equal as floats and different in bits lie side by side: wild_inputs.signed_zero_pairs); 48 sampled rows
    of every level against oracle.rc_level fed the frame's own upper level and distRT."""
    W = H = 4096
    N = 6
    color, emis = big_scene
    p = oracle.Params(W=W, H=H, N=N, reflectivity=wi.REFLECTIVITY)
    ctx = make_ctx(R, p)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    outs = ("color", "temp", "dist", "blur", "final_gi")

    def render():
        ctx.do_rc2dgi()
        ctx.sync()
        got = {k: ctx.download(k) for k in outs}
        got.update({f"L{L}": ctx.download_level(L) for L in range(N)})
        return got

    assert ctx.get_tuning("rc_pal") == 1 and ctx.get_tuning("shade_split") == 1 and ctx.get_tuning("shade_fused") == 1
    base = render()
    # the inputs reach every class here too (on the frame's own distRT, itself compared below through the levels)
    cen = wi.census(color, emis, base["dist"])
    assert min(cen["emis"].values()) >= 8 and min(cen["color"].values()) >= 8, cen
    # palette entries: the records, in bits
    hit = wi.hittable(base["dist"])
    C = W // 64
    m = ctx.download_table("mfield")[:, :W].astype(np.uint32)
    assert m[hit].max(initial=0) <= 15
    rec = wi.records(color, emis, wi.REFLECTIVITY)
    pal = ctx.download_table("cellpal")
    ys, xs = np.nonzero(hit & (m < 15))
    assert len(ys) > 1000
    got = pal[ys // C, xs // C, m[ys, xs]]
    bad = np.any(got.view(np.uint32) != rec[ys, xs].view(np.uint32), -1)
    assert not bad.any(), f"{int(bad.sum())} of {len(ys)} palette entries are not their texel's record"
    neg0 = np.signbit(rec[ys, xs][:, 1]) & (rec[ys, xs][:, 1] == 0)
    assert np.count_nonzero(neg0) >= 8  # (-0.0 records took entries of their own)
    for knob in ("rc_pal", "shade_split", "shade_fused"):
        ctx.set_tuning(knob, 0)
        assert ctx.get_tuning(knob) == 0
        wi.assert_bits(render(), base, f"{knob} 0")
        ctx.set_tuning(knob, 1)
    ctx.close()
    # every level on 48 sampled rows (as test_headline_4096_n6_every_pass does)
    dirs, sky = oracle.dir_tables(p), oracle.sky_table(p)
    rows = np.linspace(0, H - 1, 48).astype(int)
    offs = [(((1 << (2 * L)) - 1) // 3) * 4 for L in range(N)]
    for L in range(N - 1, -1, -1):
        upper = base[f"L{L + 1}"] if L < N - 1 else None
        out = np.zeros_like(base["L0"])
        for r in rows:
            oracle.rc_level(p, L, upper, color, emis, base["dist"], out, np.ascontiguousarray(dirs[offs[L]:]), sky,
                            int(r), int(r) + 1)
        assert wi.bits_equal(base[f"L{L}"][rows], out[rows]), \
            f"level {L}: {wi.bits_differ(base[f'L{L}'][rows], out[rows])} values differ from the oracle's"
    bl = oracle.blur(base["L0"], p.blur_radius)
    assert wi.bits_equal(base["blur"], bl)
    fin = oracle.blur_copyback(bl, base["L0"])
    assert wi.bits_equal(base["final_gi"], fin)
    temp, col = oracle.merge(color, fin)
    assert wi.bits_equal(base["temp"], temp) and wi.bits_equal(base["color"], col)


# ---------------------------------------------------------------- shards
def group_vs_whole(R, W, H, N, color, emis, world, strip_tables):
    want = whole_frame(R, W, H, N, 2.0, 1.0, 1.5, color, emis)
    ctxs = []
    for k in range(world):
        c = R.RC2DGI(W, H, cascade_count=N, ray_range=2.0)
        c.set_shader_value("_BlurRadius", 1.5)
        c.set_shard(k, world)
        c.set_tuning("poison", 1)
        c.upload("color", color)
        c.upload("emissive", emis)
        ctxs.append(c)
    R.do_group(ctxs)
    for c in ctxs:
        c.sync()
    for c in ctxs:
        assert_shard_matches_whole(c, want, W, H, 1.5, expect_strip_tables=strip_tables)
        y0, y1 = c.shard_rows()
        for k in ("color", "temp"):  # (shard_compare compares values: here the bits too)
            assert wi.bits_equal(c.download(k)[y0:y1], want[k][y0:y1]), f"shard {(y0, y1)} {k}: bits"
    for c in ctxs:
        c.close()


def test_group_shards_on_wild_scene(R):
    W, H = 200, 122
    color, emis = wi.wild_scene(W, H, wi.SEEDS[(W, H)])
    group_vs_whole(R, W, H, 3, color, emis, 2, strip_tables=False)


def test_strip_table_shards_on_wild_scene(R, big_scene):
    """Strip tables: the palettes and the record-free derive_record path carry the wild records."""
    color, emis = big_scene
    group_vs_whole(R, 4096, 4096, 6, color, emis, 2, strip_tables=True)


# ---------------------------------------------------------------- the RGBA16F store
def half_sweep():
    """About 2000 floats: every half binade edge and its f32 neighbours, the half-subnormal grid, the ends of the
    half range and of fp32, both signs, zeros and infinities."""
    f = np.float32
    v = []
    for e in range(-26, 18):  # half subnormals from 2^-24, normals 2^-14 .. 2^15, 65504 < 2^16
        b = f(2.0) ** f(e)
        for k in (0, 1, 4):
            v += [b * (f(1) + f(k) * f(2.0 ** -23)), b * (f(1) - f(k) * f(2.0 ** -24))]
        for frac in (3, 1023):  # a half mantissa step and its f32 neighbours
            h = b * (f(1) + f(frac) / f(1024))
            v += [h, np.nextafter(h, f(np.inf)), np.nextafter(h, f(0)), h * (f(1) + f(2.0 ** -21))]
    for k in list(range(0, 32)) + [255, 256, 511, 1023, 1024]:  # the half-subnormal grid, k * 2^-24
        g = f(k) * f(2.0 ** -24)
        v += [g, g + f(2.0 ** -26), g + f(3 * 2.0 ** -26), g + f(2.0 ** -25)]
    v += [f(65504), f(65519.996), f(65520), f(65535), f(65536), f(1e5), np.finfo(f).max, np.finfo(f).tiny,
          f(1e-45), f(6.103515625e-05), np.nextafter(f(6.103515625e-05), f(0)), f(np.inf), f(0)]
    rng = np.random.default_rng(16)
    v += list((f(2.0) ** rng.uniform(-27, 17, 150).astype(f)).astype(f))
    # random values of at most 16 significant bits: the restated sum is exact for these
    r16 = (rng.integers(1 << 15, 1 << 16, 80).astype(f) * (f(2.0) ** rng.integers(-42, 2, 80).astype(f))).astype(f)
    v += list(r16)
    v = np.array(v, f)
    return np.concatenate([v, -v])


def level0_of_constant_sky(x):
    """What the level pass hands to the store when all four rays of a probe miss into a sky of x
    (RadianceCascades.fs:96-161): radiance 0 + x, summed four times with weight 0.25, blended with alpha 1 over
    the cleared texture -- in fp32, restated here."""
    f = np.float32
    with np.errstate(all="ignore"):
        r = (f(0) + x).astype(f)
        acc = np.zeros_like(x)
        for _ in range(4):
            acc = (acc + (r * f(0.25)).astype(f)).astype(f)
        return ((acc * f(1)).astype(f) + f(0) * f(0)).astype(f)


def test_half_store_rounds_toward_zero(R):
    """GiF16::pack against orc_half_rtz over the half range: N = 1 on an empty 2 x 2 screen with a sky table of
    one colour, so G_0 = (x, y, z, 1) wherever the four-term sum returns x exactly (computed, and such values
    only are kept)."""
    x = half_sweep()
    keep = level0_of_constant_sky(x).view(np.uint32) == x.view(np.uint32)
    x = x[keep]
    assert len(x) >= 1500, len(x)
    a = np.abs(x)
    assert np.count_nonzero((a > 0) & (a < wi.HALF_MIN_NORMAL)) >= 200 and np.count_nonzero(a > wi.HALF_MAX) >= 10
    assert np.isinf(x).sum() == 2
    rtz = oracle.lib().orc_half_rtz
    want = np.array([rtz(ctypes.c_float(float(t))) for t in x], np.float32)
    assert np.count_nonzero(want != x) >= 500  # (most of the sweep is not a half: the store has to round)
    pad = (-len(x)) % 3
    xs = np.concatenate([x, np.zeros(pad, np.float32)]).reshape(-1, 3)
    ws = np.concatenate([want, np.zeros(pad, np.float32)]).reshape(-1, 3)
    from radiancecascade2dglobalillumination_amd import scenes

    color, emis = scenes.empty(2, 2)
    ctx = R.RC2DGI(2, 2, cascade_count=1, storage="f16")
    ctx.set_shader_value("_BlurRadius", 0.0)
    ctx.set_keep_levels(True)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    bad = []
    for t, w in zip(xs, ws):
        ctx.set_sky_table(np.tile(t, (4, 1)))
        ctx.do_rc2dgi()
        ctx.sync()
        g = ctx.download_level(0)
        expect = np.broadcast_to(np.concatenate([w, np.float32([1.0])]), g.shape)
        if not wi.bits_equal(g, expect):
            bad.append((t.tolist(), g[0, 0].tolist(), w.tolist()))
    ctx.close()
    assert not bad, f"{len(bad)} of {len(xs)} stores differ from orc_half_rtz, first (in, got, want): {bad[:3]}"


# ---------------------------------------------------------------- non-finite records
def plant_non_finite(color, emis):
    """NaN, +inf and -inf into one emissive or albedo channel of 24 texels on occluder edges (in place)."""
    occ = np.any(color[..., :3] > 0, -1)
    pos = np.all(color[..., :3] > 0, -1)  # (stays an occluder whatever one channel becomes)
    edge = np.zeros_like(occ)
    edge[1:-1, 1:-1] = ~(occ[:-2, 1:-1] & occ[2:, 1:-1] & occ[1:-1, :-2] & occ[1:-1, 2:])
    ys, xs = np.nonzero(pos & edge)
    assert len(ys) >= 24
    pick = np.linspace(0, len(ys) - 1, 24).astype(int)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    plant = [("e", 0, nan), ("e", 1, inf), ("e", 2, -inf), ("c", 1, nan), ("c", 2, inf), ("c", 1, -inf)]
    for n, k in enumerate(pick):
        img, ch, val = plant[n % len(plant)]
        (emis if img == "e" else color)[ys[k], xs[k], ch] = val


@pytest.mark.parametrize("kind", ["planted", "huge"])
@pytest.mark.parametrize("W,H,N,rs", [(128, 128, 4, 1.0), (256, 256, 4, 0.5)])
def test_non_finite_values_end_up_where_the_oracle_puts_them(R, W, H, N, rs, kind):
    """f32; 128^2: the blur fused with the merge; 256^2 at renderScale 0.5: the fused blur, the merge on its own.
    planted: NaN, +inf and -inf in records that rays hit.  huge: every input finite, the emission scaled by 1e33,
    so G_0 holds finite values far beyond 2^30 (where the fused blur kernels stop trusting their skipped weight-0
    taps and the frame is redone tap by tap).  With every blur_path: the JumpFlood textures and the distance
    field are bit-equal; in every other texture the NaN, the +inf and the -inf values sit where the oracle's do and
    every finite value is bit-equal.  NaN payloads are not compared."""
    color, emis = wi.wild_scene(W, H, wi.SEEDS[(128, 128)])
    if kind == "planted":
        plant_non_finite(color, emis)
    else:
        emis[..., :3] *= np.float32(1e33)
        assert np.isfinite(emis).all()
    p = wi.matrix_params(W, H, N, rs, "f32")
    want = wi.oracle_textures(oracle.frame(p, color, emis, keep_levels=True))
    if kind == "planted":
        for test in (np.isnan, np.isposinf, np.isneginf):
            assert any(test(want[k]).any() for k in want), test  # (the values are hit and travel)
    else:
        g0 = np.abs(want["L0"])
        assert np.isfinite(g0).all() and np.count_nonzero(g0 >= 2.0 ** 30) >= 100
    ctx = make_ctx(R, p)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    for path in (0, 1, 2):
        ctx.set_tuning("blur_path", path)
        ctx.do_rc2dgi()
        ctx.sync()
        got = wi.download_all(ctx, levels=N)
        what = f"{kind} blur_path {path}"
        wi.assert_bits(got, want, what, names=("jump1", "jump2", "dist"))
        for k in want:
            a, b = got[k], want[k]
            assert np.array_equal(np.isnan(a), np.isnan(b)), \
                f"{what} {k}: NaN at {np.count_nonzero(np.isnan(a) != np.isnan(b))} other values than the oracle's"
            assert np.array_equal(np.isposinf(a), np.isposinf(b)) and np.array_equal(np.isneginf(a), np.isneginf(b)), \
                f"{what} {k}: infinities differ"
            fin = np.isfinite(b)
            assert np.array_equal(a[fin].view(np.uint32), b[fin].view(np.uint32)), \
                f"{what} {k}: {np.count_nonzero(a[fin].view(np.uint32) != b[fin].view(np.uint32))} finite values differ"
    ctx.close()
