"""GPU: parity of the HIP DoRC2DGI() (through the C ABI) with the reference and the oracle.

Bar (BASELINE.json north_star):
* with the transcendental tables the reference's GL implementation used (captured from
  llvmpipe into tests/golden), the HIP pipeline reproduces the reference shaders'
  render textures bit-for-bit at power-of-two sizes (where llvmpipe's interpolated
  texture coordinates are exactly (i+0.5)/n);
* with its own correctly rounded tables it matches the CPU oracle bit-for-bit; the
  written tolerance everywhere is max relative error <= 1e-4 (denominator
  max(|ref|, 1e-3)) and the tests also report/require exact equality where stated;
* at the headline size (4096^2, N=6) every cascade level, the JFA/distance field, blur
  and merge are checked against the oracle on the HIP pipeline's own inputs.
"""
import numpy as np
import pytest

import oracle
from conftest import load_fixture, manifest, params_of, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-4
SCREEN = ("color", "jump1", "jump2", "dist", "temp")
CASCADE = ("gi1", "gi2", "blur")


@pytest.fixture(scope="module")
def RC2DGI():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from radiancecascade2dglobalillumination_amd import RC2DGI as cls

    return cls


def set_uniforms(ctx, p):
    ctx.set_shader_value("_SkyRadiance", p.sky_radiance)
    ctx.set_shader_value("_SkyColor", p.sky_color)
    ctx.set_shader_value("_SunColor", p.sun_color)
    ctx.set_shader_value("_SunAngle", p.sun_angle)
    ctx.set_shader_value("_Reflectivity", p.reflectivity)
    ctx.set_shader_value("_BlurRadius", p.blur_radius)


def storage_of(p):
    return "rgba8" if p.rgba8 else ("f16" if p.gi_f16 else "f32")


def mode_params(storage):
    """oracle.Params keywords of a storage mode"""
    return dict(gi_f16=storage == "f16", rgba8=storage == "rgba8")


def run_hip(RC2DGI, p, color, emis, dir_tabs=None, sky=None, keep_levels=False):
    ctx = RC2DGI(p.W, p.H, cascade_count=p.N, render_scale=p.render_scale, ray_range=p.ray_range,
                 storage=storage_of(p), linux_merge_fallback=p.linux_merge)
    set_uniforms(ctx, p)
    if dir_tabs is not None:
        off = 0
        for L in range(p.N):
            n = 4 << (2 * L)
            ctx.set_direction_table(L, dir_tabs[off:off + n])
            off += n
    if sky is not None:
        ctx.set_sky_table(sky)
    if keep_levels:
        ctx.set_keep_levels(True)
    ctx.frame(color, emis)
    ctx.sync()
    out = {k: ctx.download(k) for k in SCREEN + CASCADE}
    out["final_gi"] = ctx.download("final_gi")
    out["_final"] = ctx.final_gi
    if keep_levels:
        for L in range(p.N):
            out[f"gi_L{L}"] = ctx.download_level(L)
    ctx.close()
    return out


def oracle_dict(fr):
    d = dict(color=fr.color_out, jump1=fr.jump1, jump2=fr.jump2, dist=fr.dist, temp=fr.temp, gi1=fr.gi1, gi2=fr.gi2,
             blur=fr.blur, final_gi=fr.gi_final)
    for L, g in enumerate(fr.gi_levels):
        d[f"gi_L{L}"] = g
    return d


def assert_parity(got, want, names, exact=True, what=""):
    for n in names:
        a, b = got[n], want[n]
        assert a.shape == b.shape, (what, n, a.shape, b.shape)
        r = rel_err(a, b)
        assert r.max() <= TOL, f"{what}:{n}: max rel err {r.max():.3e} ({np.mean(r > TOL):.4%} texels over)"
        if exact:
            mism = np.count_nonzero(a != b)
            assert mism == 0, f"{what}:{n}: {mism} texels not bit-identical (max rel {r.max():.2e})"


# ---------------------------------------------------------------- golden fixtures
@pytest.mark.parametrize("name", [m["name"] for m in manifest()])
def test_fixture_with_reference_tables(RC2DGI, name):
    m = next(x for x in manifest() if x["name"] == name)
    fx = load_fixture(name)
    p = params_of(m)
    got = run_hip(RC2DGI, p, fx["color"], fx["emissive"], fx["dir_tables"], fx["sky_table"], keep_levels=True)
    assert got["_final"] == m["final_gi"]
    names = ["color", "jump1", "jump2", "dist", "temp", "gi1", "gi2", "final_gi"] + [f"gi_L{L}" for L in range(p.N)]
    if p.blur_radius > 0:
        names.append("blur")
    pow2 = (p.W & (p.W - 1)) == 0 and (p.H & (p.H - 1)) == 0
    if pow2:
        # the reference shaders' own outputs, bit for bit (RGBA8 fixtures: the texels)
        alias = {"color": "color_out", "final_gi": "gi_final"}
        want = {k: fx[alias.get(k, k)] for k in names}
        if p.rgba8:
            got = {k: oracle.to_u8(got[k]) for k in names}
            for k in names:
                assert np.array_equal(got[k], want[k]), f"{name} vs llvmpipe:{k}: {np.count_nonzero(got[k] != want[k])}"
            return
        assert_parity(got, want, names, exact=True, what=name + " vs llvmpipe")
    else:
        # llvmpipe interpolates fragTexCoord to within 1 ulp of (i+0.5)/n here; compare with the
        # oracle on exact texture coordinates and the reference's transcendental tables
        fr = oracle.frame(p, fx["color"], fx["emissive"], dir_tabs=fx["dir_tables"], sky_tab=fx["sky_table"],
                          keep_levels=True)
        assert_parity(got, oracle_dict(fr), names, exact=True, what=name + " vs oracle(ref tables)")


@pytest.mark.parametrize("name", [m["name"] for m in manifest()])
def test_fixture_own_tables_vs_oracle(RC2DGI, name):
    m = next(x for x in manifest() if x["name"] == name)
    fx = load_fixture(name)
    p = params_of(m)
    got = run_hip(RC2DGI, p, fx["color"], fx["emissive"], keep_levels=True)
    fr = oracle.frame(p, fx["color"], fx["emissive"], keep_levels=True)
    names = ["color", "jump1", "jump2", "dist", "temp", "gi1", "gi2", "final_gi"] + [f"gi_L{L}" for L in range(p.N)]
    assert_parity(got, oracle_dict(fr), names, exact=True, what=name)
    # and the product stays within the reference's own branch-flip noise
    if p.rgba8:  # in bytes: an ulp of cos/sin occasionally crosses a byte boundary
        for n, g in (("final_gi", "gi_final"), ("color", "color_out")):
            d = np.abs(oracle.to_u8(got[n]).astype(int) - fx[g])
            assert np.mean(d == 0) >= 0.995 and d.max() <= 2, n
        return
    for n, g in (("final_gi", "gi_final"), ("color", "color_out")):
        r = rel_err(got[n], fx[g])
        assert np.mean(r <= TOL) >= 0.995 and np.abs(got[n] - fx[g]).max() <= 5e-3, n


# ---------------------------------------------------------------- random scenes and edge cases
CONFIGS = [
    # W, H, N, rayRange, renderScale, uniform overrides, scene
    (64, 64, 2, 8.0, 1.0, {}, "rand:11"),
    (1, 1, 1, 2.0, 1.0, {}, "rand:12"),            # smallest screen: S = 1 JFA step, CW = 2
    (3, 2, 1, 2.0, 1.0, {}, "full"),               # every texel an occluder
    (17, 5, 2, 2.0, 1.0, {}, "rand:13"),           # ragged, non-power-of-two both axes
    (256, 256, 5, 3.0, 1.0, {}, "demo"),
    (333, 200, 4, 2.0, 0.5, {}, "rand:14"),        # renderScale < 1: cascades coarser than screen
    (200, 120, 3, 2.0, 1.7, {}, "rand:15"),        # renderScale > 1
    (160, 96, 3, 4.0, 1.0, dict(reflectivity=1.0), "rand:16"),
    (128, 128, 3, 2.0, 1.0, dict(blur_radius=0.0), "rand:17"),
    (128, 64, 4, 64.0, 1.0, dict(blur_radius=5.0, sun_angle=3.0), "rand:18"),
    (512, 512, 8, 64.0, 1.0, {}, "rand:19"),       # C2-style knobs, top levels start off-screen
    (300, 300, 6, 2.0, 1.0, dict(sky_radiance=0.0), "empty"),
    # giRT1/2 as RGBA16F (RC2DGI_STORAGE_F16)
    (256, 256, 5, 3.0, 1.0, dict(gi_f16=True), "demo"),
    (333, 200, 4, 2.0, 0.5, dict(gi_f16=True, blur_radius=1.37), "rand:41"),
    (128, 128, 3, 2.0, 1.0, dict(gi_f16=True, blur_radius=0.0, reflectivity=0.7), "rand:42"),
    # every render texture RGBA8 (RC2DGI_STORAGE_RGBA8_COMPAT): float inputs quantized on upload
    (256, 256, 5, 3.0, 1.0, dict(rgba8=True), "demo"),
    (333, 200, 4, 2.0, 0.5, dict(rgba8=True, blur_radius=1.37), "rand:61"),
    (128, 128, 3, 2.0, 1.0, dict(rgba8=True, blur_radius=0.0, reflectivity=0.7), "rand:62"),
    (17, 5, 2, 2.0, 1.0, dict(rgba8=True), "rand:63"),
    (1, 1, 1, 2.0, 1.0, dict(rgba8=True), "rand:64"),
    (512, 512, 8, 64.0, 1.0, dict(rgba8=True, blur_radius=2.5), "rand:65"),
    (1200, 900, 6, 2.0, 1.0, dict(rgba8=True), "demo"),  # the reference app itself (C1 knobs)
]


def make_scene(spec, W, H):
    from radiancecascade2dglobalillumination_amd import scenes

    if spec == "demo":
        return scenes.demo(W, H)
    if spec == "empty":
        return scenes.empty(W, H)
    if spec == "full":
        c = np.ones((H, W, 4), np.float32)
        e = np.zeros((H, W, 4), np.float32)
        e[0, 0] = (1, 0.5, 0.25, 1)
        return c, e
    return scenes.random_scene(W, H, int(spec.split(":")[1]))


@pytest.mark.parametrize("W,H,N,rr,rs,over,scene", CONFIGS)
def test_random_configs_vs_oracle(RC2DGI, W, H, N, rr, rs, over, scene):
    p = oracle.Params(W=W, H=H, N=N, ray_range=rr, render_scale=rs, **over)
    color, emis = make_scene(scene, W, H)
    got = run_hip(RC2DGI, p, color, emis, keep_levels=True)
    fr = oracle.frame(p, color, emis, keep_levels=True)
    names = ["color", "jump1", "jump2", "dist", "temp", "gi1", "gi2", "final_gi"] + [f"gi_L{L}" for L in range(N)]
    if p.blur_radius > 0:
        names.append("blur")
    assert_parity(got, oracle_dict(fr), names, exact=True, what=f"{W}x{H} N={N}")


# ---------------------------------------------------------------- headline size
def test_headline_4096_n6_every_pass(RC2DGI):
    """4096^2, cascadeCount=6, rayRange=2 (the metric's configuration).  JFA + DF over the
    whole frame; every cascade level on 48 sampled rows (the oracle level pass fed the
    HIP pipeline's own G_{L+1} and distRT); blur, copy-back and merge over the whole frame."""
    W = H = 4096
    N = 6
    from radiancecascade2dglobalillumination_amd import scenes

    p = oracle.Params(W=W, H=H, N=N, ray_range=2.0)
    color, emis = scenes.demo(W, H)
    got = run_hip(RC2DGI, p, color, emis, keep_levels=True)
    # JFA + distance field, whole frame
    mx = max(W, H)
    j = oracle.screen_uv(color)
    step = np.float32(1.0)
    for _ in range(12):
        step = np.float32(step * np.float32(0.5))
        j = oracle.jfa_step(j, float(step), float(np.float32(W) / mx), float(np.float32(H) / mx))
    assert np.array_equal(got["jump1"], j), "final JFA state"
    assert np.array_equal(got["dist"], oracle.distance_field(j)), "distance field"
    # cascade levels on sampled rows
    dirs = oracle.dir_tables(p)
    sky = oracle.sky_table(p)
    rows = np.linspace(0, H - 1, 48).astype(int)
    off = 0
    offs = []
    for L in range(N):
        offs.append(off)
        off += 4 << (2 * L)
    for L in range(N - 1, -1, -1):
        upper = got[f"gi_L{L + 1}"] if L < N - 1 else None
        out = np.zeros_like(got["gi_L0"])
        for r in rows:
            oracle.rc_level(p, L, upper, color, emis, got["dist"], out, np.ascontiguousarray(dirs[offs[L]:]), sky,
                            int(r), int(r) + 1)
        a, b = got[f"gi_L{L}"][rows], out[rows]
        assert rel_err(a, b).max() <= TOL and np.count_nonzero(a != b) == 0, f"level {L}"
    # blur + copy-back + merge, whole frame
    g0 = got["gi_L0"]
    bl = oracle.blur(g0, p.blur_radius)
    assert np.array_equal(got["blur"], bl)
    fin = oracle.blur_copyback(bl, g0)
    assert np.array_equal(got["final_gi"], fin)
    temp, col = oracle.merge(color, fin)
    assert np.array_equal(got["temp"], temp) and np.array_equal(got["color"], col)


# ---------------------------------------------------------------- API behaviour
def test_uniform_api_and_errors(RC2DGI):
    from radiancecascade2dglobalillumination_amd import RC2DGIError

    ctx = RC2DGI(64, 48, cascade_count=3)
    ctx.sun_angle = 1.25
    ctx.sky_color = (0.1, 0.2, 0.3)
    assert ctx.sun_angle == pytest.approx(1.25)
    assert ctx.sky_color == pytest.approx((0.1, 0.2, 0.3))
    for bad in ("_Nope", "_StepSize", "_Aspect", "_CascadeLevel", "_CascadeResolution", "_Resolution"):
        with pytest.raises(RC2DGIError) as e:
            ctx.set_shader_value(bad, 1.0)
        assert e.value.code == -2
    with pytest.raises(RC2DGIError):
        ctx.set_shader_value("_SkyColor", 1.0)  # wrong component count
    assert ctx.cascade_resolution == (64, 48) and ctx.jfa_steps == 6 and ctx.final_gi == 1
    ctx.close()


def test_cascade_count_change_reallocates(RC2DGI):
    W, H = 96, 80
    color, emis = make_scene("rand:21", W, H)
    ctx = RC2DGI(W, H, cascade_count=2)
    ctx.frame(color, emis)
    ctx.cascade_count = 4
    assert ctx.cascade_resolution == (96, 80) and ctx.final_gi == 2
    ctx.do_rc2dgi()  # inputs survive the reallocation
    ctx.sync()
    fr = oracle.frame(oracle.Params(W=W, H=H, N=4), color, emis)
    assert np.array_equal(ctx.download("final_gi"), fr.gi_final)
    assert np.array_equal(ctx.download("color"), fr.color_out)
    ctx.close()


def test_frames_are_repeatable_and_uint8_io(RC2DGI):
    W, H = 120, 90
    color, emis = make_scene("rand:22", W, H)
    ctx = RC2DGI(W, H, cascade_count=3)
    ctx.frame(color, emis)
    ctx.sync()
    first = ctx.download("color")
    assert np.array_equal(ctx.download("color"), first)
    # RGBA8 upload of the same k/255 scene gives identical results
    ctx.frame((color * 255).round().astype(np.uint8), (emis * 255).round().astype(np.uint8))
    ctx.do_rc2dgi()  # a second frame without a new upload repeats the frame exactly
    ctx.sync()
    assert np.array_equal(ctx.download("color"), first)
    u8 = ctx.download("color", dtype=np.uint8)
    assert np.array_equal(u8, np.rint(np.clip(first, 0, 1) * 255).astype(np.uint8))
    ctx.close()


def test_device_resident_upload_matches_host(RC2DGI):
    import torch

    W, H = 128, 128
    color, emis = make_scene("rand:23", W, H)
    a = RC2DGI(W, H, cascade_count=3)
    a.frame(color, emis)
    a.sync()
    b = RC2DGI(W, H, cascade_count=3)
    tc, te = torch.from_numpy(color).cuda(), torch.from_numpy(emis).cuda()
    torch.cuda.synchronize()
    b.upload("color", tc)
    b.upload("emissive", te)
    b.do_rc2dgi()
    b.sync()
    for k in ("color", "final_gi", "dist"):
        assert np.array_equal(a.download(k), b.download(k)), k
    a.close()
    b.close()


def test_concurrent_contexts(RC2DGI):
    cfgs = [(64, 64, 2), (100, 60, 3), (256, 128, 5)]
    ctxs, refs = [], []
    for i, (W, H, N) in enumerate(cfgs):
        color, emis = make_scene(f"rand:{30 + i}", W, H)
        c = RC2DGI(W, H, cascade_count=N)
        c.upload("color", color)
        c.upload("emissive", emis)
        ctxs.append(c)
        refs.append(oracle.frame(oracle.Params(W=W, H=H, N=N), color, emis))
    for _ in range(2):
        for c in ctxs:
            c.do_rc2dgi()  # interleaved on independent streams
    for c, fr in zip(ctxs, refs):
        c.sync()
        assert np.array_equal(c.download("color"), fr.color_out)
        c.close()


def test_timing_reports_passes(RC2DGI):
    W, H = 256, 256
    color, emis = make_scene("demo", W, H)
    ctx = RC2DGI(W, H, cascade_count=4)
    ctx.set_timing(True)
    ctx.frame(color, emis)
    t = ctx.pass_times(levels=4)
    assert t["total"] > 0 and all(v >= 0 for k, v in t.items() if k != "levels")
    assert len(t["levels"]) == 4 and sum(t["levels"]) <= t["rc"] * 1.01 + 0.05
    # mode 2: pass events only (no per-level events, which idle the GPU between levels)
    ctx.set_timing(2)
    ctx.frame(color, emis)
    t2 = ctx.pass_times()
    assert t2["rc"] > 0 and t2["total"] >= t2["rc"]
    with pytest.raises(RuntimeError):
        ctx.pass_times(levels=4)
    ctx.set_timing(True)
    ctx.frame(color, emis)
    assert len(ctx.pass_times(levels=4)["levels"]) == 4
    ctx.close()


@pytest.mark.parametrize("W,H,N,rr,scene", [(256, 192, 5, 2.0, "rand:40"), (333, 200, 4, 8.0, "demo"),
                                            (512, 512, 6, 2.0, "demo")])
@pytest.mark.parametrize("storage", ["f32", "f16", "rgba8"])
def test_every_rc_variant_is_bit_identical(RC2DGI, W, H, N, rr, scene, storage):
    """The tile-shape tuning knob changes the schedule only, never a result."""
    color, emis = make_scene(scene, W, H)
    fr = oracle.frame(oracle.Params(W=W, H=H, N=N, ray_range=rr, **mode_params(storage)), color, emis,
                      keep_levels=True)
    ctx = RC2DGI(W, H, cascade_count=N, ray_range=rr, storage=storage)
    ctx.set_keep_levels(True)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    variants = range(ctx.get_tuning("rc_variant_count")) if storage == "f32" else (0, 1, 3, 6, 13, 14, 15, 16, 17, 18, 19)
    for v in variants:
        ctx.set_tuning("rc_variant", v)
        for rep in range(2):  # twice: a schedule must also be deterministic run to run
            ctx.do_rc2dgi()
            ctx.sync()
            for L in range(N):
                g = ctx.download_level(L)
                assert np.array_equal(g, fr.gi_levels[L]), \
                    f"variant {v} run {rep} level {L}: {np.count_nonzero(g != fr.gi_levels[L])}"
    ctx.close()


def speckled_scene(W, H, seed=7):
    """The demo scene with every occluder and emitter texel given its own random k/255 colour: far more
    than kCellPal distinct hit records per bound-table cell (the palettes overflow, hits read shade)."""
    from radiancecascade2dglobalillumination_amd import scenes

    color, emis = (np.array(a, np.float32, order="C") for a in scenes.demo(W, H))
    rng = np.random.default_rng(seed)
    for img in (color, emis):
        m = np.any(img[..., :3] > 0, axis=-1)
        img[m, :3] = rng.integers(1, 256, size=(int(m.sum()), 3)).astype(np.float32) / np.float32(255)
    return color, emis


@pytest.mark.parametrize("scene", ["demo", "speckled", "rand:43"])
def test_surface_palettes_are_bit_identical(RC2DGI, scene):
    """rc_pal (per-cell surface palettes and the march field, launch_shade_cmin; the one-probe tiles of the
    plain field read a hit's record from its cell's palette) against the same frame without: every level
    and every output texture bit for bit, at 4096^2 N=6 (the fused records pass needs cells of >= 64
    texels), with the one-probe variants at L1-L5 (256-, 512- and 1024-lane tiles); the speckled scene
    overflows the palettes."""
    W = H = 4096
    N = 6
    color, emis = speckled_scene(W, H) if scene == "speckled" else make_scene(scene, W, H)
    ctx = RC2DGI(W, H, cascade_count=N, ray_range=2.0)
    ctx.set_keep_levels(True)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    for v in (0, 13, 20, 22, 24, 25):  # (22 / 24: 1024-lane tiles, two waves per direction; 25: k_rc_top at L5)
        for L in range(1, N):
            ctx.set_tuning(f"rc_variant_L{L}", v)
        want = {}
        for pal in (0, 1):
            ctx.set_tuning("rc_pal", pal)
            assert ctx.get_tuning("rc_pal") == pal
            ctx.do_rc2dgi()
            ctx.sync()
            got = {f"L{L}": ctx.download_level(L) for L in range(N)}
            got.update({k: ctx.download(k) for k in ("color", "temp", "final_gi")})
            if pal == 0:
                want = got
            else:
                for k in got:
                    assert np.array_equal(got[k], want[k]), \
                        f"{scene} variant {v} {k}: {np.count_nonzero(got[k] != want[k])} differ with palettes"
    ctx.close()


@pytest.mark.parametrize("W,H,rs,radius", [
    (128, 128, 1.0, 1.5),    # fixed taps (F=1), merge fused
    (256, 128, 1.0, 2.5),    # F=2
    (128, 64, 1.0, 1.0),     # integral radius: a0 = -F
    (64, 64, 1.0, 0.5),      # F=0
    (512, 64, 1.0, 2.99609375),  # largest dyadic radius below 3
    (128, 128, 1.0, 1.37),   # not dyadic: LDS-tiled general kernel
    (128, 128, 1.0, 3.0),    # F=3: beyond the fixed-tap kernels
    (256, 256, 0.5, 1.5),    # cascade 128^2 != screen: fixed taps, separate merge
    (200, 120, 1.0, 1.5),    # non-power-of-two: separate passes only
])
@pytest.mark.parametrize("storage", ["f32", "f16", "rgba8"])
def test_every_blur_path_matches_oracle(RC2DGI, W, H, rs, radius, storage):
    """blur_path 0 (fixed taps + fused merge), 1 (LDS tile), 2 (separate passes): same bits
    (RGBA8 runs the separate passes whatever the knob says)."""
    p = oracle.Params(W=W, H=H, N=3, ray_range=4.0, render_scale=rs, blur_radius=radius, **mode_params(storage))
    color, emis = make_scene("rand:51", W, H)
    fr = oracle_dict(oracle.frame(p, color, emis))
    ctx = RC2DGI(W, H, cascade_count=3, render_scale=rs, ray_range=4.0, storage=storage)
    set_uniforms(ctx, p)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    for path in (0, 1, 2):
        ctx.set_tuning("blur_path", path)
        assert ctx.get_tuning("blur_path") == path
        ctx.do_rc2dgi()
        ctx.sync()
        got = {k: ctx.download(k) for k in ("color", "temp", "gi1", "gi2", "blur", "final_gi")}
        assert_parity(got, fr, list(got), exact=True, what=f"blur_path {path}")
    ctx.close()


def test_rc_orders_and_autotune_are_bit_identical(RC2DGI):
    """Workgroup orders (tuning rc_order_L<n>, autotune) change the schedule only."""
    W, H, N = 512, 512, 6
    color, emis = make_scene("demo", W, H)
    fr = oracle.frame(oracle.Params(W=W, H=H, N=N, ray_range=2.0), color, emis, keep_levels=True)
    ctx = RC2DGI(W, H, cascade_count=N, ray_range=2.0)
    ctx.set_keep_levels(True)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    codes = [0, 2 | 2 << 8 | 8 << 16, 4 | 4 << 8 | 4 << 16, 1 | 16 << 8 | 16 << 16, 2 | 3 << 8 | 5 << 16]
    for code in codes:  # the last does not tile any grid: tile-major fallback
        for L in range(N):
            ctx.set_tuning(f"rc_order_L{L}", code)
        ctx.do_rc2dgi()
        ctx.sync()
        for L in range(N):
            assert np.array_equal(ctx.download_level(L), fr.gi_levels[L]), f"order {code:#x} level {L}"
    picked = ctx.autotune(1)
    assert len(picked) == N
    ctx.do_rc2dgi()
    ctx.sync()
    assert np.array_equal(ctx.download("color"), fr.color_out)
    ctx.close()


@pytest.mark.parametrize("storage,W,N", [("f16", 512, 6), ("f32", 512, 6), ("rgba8", 512, 6), ("f16", 1024, 6),
                                         ("f32", 256, 4)])
@pytest.mark.parametrize("variant", [16, 17, 18, 19])
def test_packed_fields_first_in_fresh_context(RC2DGI, storage, W, N, variant):
    """The packed (16 unrolled, 18 rolled) and nibble-predicted (17 unrolled, 19 rolled)
    distance-field marches as the first and only schedule of a fresh context (the context must
    build its packed field itself), at sizes where many samples escape to the 16-bit field, three
    frames: every level bit-exact every time (the round-1 failure of the rolled form)."""
    color, emis = make_scene("demo", W, W)
    fr = oracle.frame(oracle.Params(W=W, H=W, N=N, ray_range=2.0, **mode_params(storage)), color, emis,
                      keep_levels=True)
    ctx = RC2DGI(W, W, cascade_count=N, ray_range=2.0, storage=storage)
    ctx.set_keep_levels(True)
    ctx.set_tuning("rc_variant", variant)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    for rep in range(3):
        ctx.do_rc2dgi()
        ctx.sync()
        for L in range(N):
            g = ctx.download_level(L)
            assert np.array_equal(g, fr.gi_levels[L]), \
                f"run {rep} level {L}: {np.count_nonzero(np.any(g != fr.gi_levels[L], axis=-1))} texels differ"
    ctx.close()


@pytest.mark.parametrize("W,H,N,rr,rs,scene", [(333, 200, 4, 8.0, 1.0, "demo"), (512, 512, 6, 2.0, 1.0, "demo"),
                                               (256, 128, 5, 64.0, 1.0, "rand:12"), (256, 256, 4, 2.0, 0.5, "rand:3"),
                                               (17, 5, 2, 8.0, 1.0, "rand:9"), (1024, 1024, 6, 2.0, 1.0, "rand:5")])
def test_exit_proofs_and_tail_are_bit_identical(RC2DGI, W, H, N, rr, rs, scene):
    """The march's exit proofs (tuning rc_skip: 0 off, 1 auto, 2 interval only, 3 interval and
    screen edge; k_dist_cmin's coarse lower bound) skip only samples whose outcome is already
    decided, and tail compaction (rc_tail: rays still marching after that many lockstep iterations
    finish one per lane) only moves rays between lanes: every level is bit-exact with each
    setting, in every tile variant family."""
    color, emis = make_scene(scene, W, H)
    fr = oracle.frame(oracle.Params(W=W, H=H, N=N, ray_range=rr, render_scale=rs), color, emis, keep_levels=True)
    ctx = RC2DGI(W, H, cascade_count=N, ray_range=rr, render_scale=rs)
    ctx.set_keep_levels(True)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    for v in (0, 3, 6, 9, 13, 18, 19):
        ctx.set_tuning("rc_variant", v)
        for skip, tail in ((0, 0), (1, 0), (2, 1), (3, 3), (1, 2), (0, 5), (1, 31)):
            ctx.set_tuning("rc_skip", skip)
            ctx.set_tuning("rc_tail", tail)
            assert ctx.get_tuning("rc_skip") == skip and ctx.get_tuning(f"rc_tail_L{N - 1}") == tail
            ctx.do_rc2dgi()
            ctx.sync()
            for L in range(N):
                g = ctx.download_level(L)
                assert np.array_equal(g, fr.gi_levels[L]), \
                    f"variant {v} rc_skip {skip} rc_tail {tail} level {L}: {np.count_nonzero(g != fr.gi_levels[L])}"
    ctx.close()


@pytest.mark.parametrize("W,H,N,storage", [(256, 256, 4, "f32"), (1024, 1024, 5, "f32"), (512, 512, 4, "rgba8"),
                                           (512, 256, 4, "f32"), (4096, 4096, 6, "f32")])
def test_jfa_lds_staging_is_bit_identical(RC2DGI, W, H, N, storage):
    """The LDS-staged taps of the short JumpFlood steps (tuning jfa_lds) load the same seeds: every
    JFA output and the distance field are unchanged (non-square screens keep the plain kernel)."""
    color, emis = make_scene("demo", W, H)
    ctx = RC2DGI(W, H, cascade_count=N, ray_range=2.0, storage=storage)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    ctx.set_tuning("jfa_coset", 0)  # the per-step kernels (the fused long steps are tested below)
    out = {}
    for lds in (0, 1):
        ctx.set_tuning("jfa_lds", lds)
        assert ctx.get_tuning("jfa_lds") == lds
        ctx.do_rc2dgi()
        ctx.sync()
        out[lds] = {k: ctx.download(k) for k in ("jump1", "jump2", "dist", "color")}
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), f"{k}: {np.count_nonzero(out[0][k] != out[1][k])}"
    ctx.close()


@pytest.mark.parametrize("W,H,N,storage", [(256, 256, 4, "f32"), (1024, 1024, 5, "f32"), (512, 512, 4, "rgba8"),
                                           (512, 256, 4, "f32"), (4096, 4096, 6, "f32"), (8192, 8192, 8, "f32")])
@pytest.mark.parametrize("scene", ["demo", "rand:61"])
def test_jfa_rows_short_steps_are_bit_identical(RC2DGI, W, H, N, storage, scene):
    """The short isotropic JumpFlood steps with consecutive rows per lane (tuning jfa_rows 4 / 8: k_jfa_rows, each
    tap row loaded once) pick the same seeds: jumpRT1 / jumpRT2, the distance field (fused into the last step) and
    the frame are unchanged, with poisoned intermediates; non-square (float keys) and RGBA8 screens keep k_jfa_p2."""
    color, emis = make_scene(scene, W, H)
    ctx = RC2DGI(W, H, cascade_count=N, ray_range=2.0, storage=storage)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    out = {}
    for jr in (0, 4, 8):
        ctx.set_tuning("jfa_rows", jr)
        assert ctx.get_tuning("jfa_rows") == jr
        ctx.set_tuning("poison", 1)
        ctx.do_rc2dgi()
        ctx.sync()
        out[jr] = {k: ctx.download(k) for k in ("jump1", "jump2", "dist", "color")}
    for jr in (4, 8):
        for k in out[0]:
            assert np.array_equal(out[0][k].view(np.uint8), out[jr][k].view(np.uint8)), \
                f"jfa_rows {jr} {k}: {np.count_nonzero(out[0][k] != out[jr][k])}"
    ctx.close()


@pytest.mark.parametrize("W,H,N,rr,filled", [(4096, 4096, 8, 64.0, 0b11000000), (512, 512, 8, 64.0, 0b11000000),
                                             (1000, 700, 6, 64.0, None), (256, 256, 5, 2.0, 0), (300, 300, 6, 200.0, None)])
@pytest.mark.parametrize("scene", ["demo", "rand:65"])
def test_rc_levels_no_ray_samples_as_block_fills(RC2DGI, W, H, N, rr, filled, scene):
    """Levels whose every ray starts off screen (rc_level_all_off, on the host: the whole-workgroup far test with
    each block's extreme probes) are written as per-direction-block values (k_rc_block_const: k_rc_level's merge
    expressions, from the sky or the upper level's block values) and a fill (tuning rc_fill, on by default): every
    level, render texture and the frame are unchanged.  C2's knobs (rayRange 64, N = 8) fill levels 6 and 7."""
    color, emis = make_scene(scene, W, H)
    ctx = RC2DGI(W, H, cascade_count=N, ray_range=rr)
    ctx.set_keep_levels(True)
    if N == 8:  # (the level below the fills on 32x8x2 tiles: it merges with their block values, k_rc_level UC)
        ctx.set_tuning("rc_variant_L5", 6)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    out = {}
    for fl in (0, 1):
        ctx.set_tuning("rc_fill", fl)
        ctx.set_tuning("poison", 1)
        ctx.do_rc2dgi()
        ctx.sync()
        if fl and filled is not None:
            assert ctx.get_tuning("rc_fill_levels") == filled
        if fl and filled is None:
            assert ctx.get_tuning("rc_fill_levels") != 0  # (the top levels of these start off screen)
        out[fl] = {k: ctx.download(k) for k in ("color", "temp", "gi1", "gi2", "final_gi")}
        out[fl].update({f"L{L}": ctx.download_level(L) for L in range(N)})
    for k in out[0]:
        assert np.array_equal(out[0][k].view(np.uint8), out[1][k].view(np.uint8)), \
            f"rc_fill {k}: {np.count_nonzero(out[0][k] != out[1][k])}"
    ctx.close()


@pytest.mark.parametrize("W,H,N,rr,rs", [(1200, 900, 6, 2.0, 1.0), (200, 120, 3, 2.0, 1.0), (333, 200, 4, 2.0, 0.5),
                                         (320, 256, 5, 8.0, 1.7), (1000, 700, 5, 64.0, 1.0)])
@pytest.mark.parametrize("chain", [0, 1])
def test_rc_reciprocal_divisions_are_bit_identical(RC2DGI, W, H, N, rr, rs, chain):
    """Non-power-of-two cascades: the levels' divisions by the cascade resolution as x * (1/n) plus one fused
    correction, where the host proved that equal to the IEEE quotient for every numerator of the level (tuning
    rc_rdiv, on by default): every render texture and cascade level is unchanged, with and without the cascade
    chain.  At C1 (1216 x 960 cascades) every level takes them."""
    color, emis = make_scene("rand:64", W, H)
    ctx = RC2DGI(W, H, cascade_count=N, ray_range=rr, render_scale=rs)
    ctx.set_keep_levels(True)
    if chain:
        ctx.set_tuning("rc_chain", 1)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    if (W, H, rs) == (1200, 900, 1.0):
        assert ctx.get_tuning("rc_rdiv_levels") == (1 << N) - 1
    out = {}
    for rd in (0, 1):
        ctx.set_tuning("rc_rdiv", rd)
        ctx.set_tuning("poison", 1)
        ctx.do_rc2dgi()
        ctx.sync()
        out[rd] = {k: ctx.download(k) for k in ("color", "temp", "gi1", "gi2", "final_gi")}
        out[rd].update({f"L{L}": ctx.download_level(L) for L in range(N)})
    for k in out[0]:
        assert np.array_equal(out[0][k].view(np.uint8), out[1][k].view(np.uint8)), \
            f"rc_rdiv {k}: {np.count_nonzero(out[0][k] != out[1][k])}"
    ctx.close()


@pytest.mark.parametrize("W,H,N,rs", [(1200, 900, 6, 1.0), (200, 120, 3, 1.0), (320, 256, 4, 0.5), (96, 4000, 4, 1.0),
                                      (4000, 96, 4, 1.0), (6000, 2000, 4, 1.0), (8188, 8, 3, 1.0), (8, 8188, 3, 1.0)])
@pytest.mark.parametrize("scene", ["demo", "rand:63"])
def test_jfa_texcoord_table_is_bit_identical(RC2DGI, W, H, N, rs, scene):
    """The float-path JumpFlood steps (non-power-of-two screens) take every fragTexCoord from the context's table of
    (i + 0.5) / n (tuning jfa_tab 1) or from x * (1/n) with one fused correction, proven equal to the division for
    every index on the host (jfa_tab 2, the default) instead of dividing per tap: jumpRT1 / jumpRT2, the distance
    field and the frame are unchanged, poisoned intermediates.  6000 x 2000 is the largest case inside the table
    (W + H <= 8192); the thin 8188 x 8 and 8 x 8188 screens (W + H = 8196) are over its limit, where jfa_tab 1 divides
    per tap -- those two are also compared with the oracle, so the fallback is checked against something other than
    itself."""
    color, emis = make_scene(scene, W, H)
    ctx = RC2DGI(W, H, cascade_count=N, ray_range=2.0, render_scale=rs)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    out = {}
    for tab in (0, 1, 2):
        ctx.set_tuning("jfa_tab", tab)
        assert ctx.get_tuning("jfa_tab") == tab
        ctx.set_tuning("poison", 1)
        ctx.do_rc2dgi()
        ctx.sync()
        out[tab] = {k: ctx.download(k) for k in ("jump1", "jump2", "dist", "color")}
    for tab in (1, 2):
        for k in out[0]:
            assert np.array_equal(out[0][k].view(np.uint8), out[tab][k].view(np.uint8)), \
                f"jfa_tab {tab} {k}: {np.count_nonzero(out[0][k] != out[tab][k])}"
    ctx.close()
    if W + H > 8192:
        ref = oracle_dict(oracle.frame(oracle.Params(W=W, H=H, N=N, ray_range=2.0, render_scale=rs), color, emis))
        for tab in (0, 1, 2):
            for k in out[tab]:
                assert np.array_equal(out[tab][k].view(np.uint8), ref[k].view(np.uint8)), \
                    f"jfa_tab {tab} {k} vs the oracle: {np.count_nonzero(out[tab][k] != ref[k])}"


@pytest.mark.parametrize("W,H,N,storage", [(64, 64, 3, "f32"), (128, 128, 3, "f32"), (256, 256, 4, "f32"),
                                           (1024, 1024, 5, "f32"), (4096, 4096, 6, "f32"), (512, 256, 4, "f32"),
                                           (512, 512, 4, "rgba8"), (8192, 8192, 8, "f32")])
@pytest.mark.parametrize("scene", ["demo", "rand:62", "empty", "full"])
def test_jfa_tail_steps_are_bit_identical(RC2DGI, W, H, N, storage, scene):
    """The last two to four JumpFlood steps in one kernel (tuning jfa_tail: k_jfa_tail, the tile and the ring the
    steps reach staged in LDS once, J_{S-2} / J_{S-1} / the distance field written) leave the same jumpRT1 / jumpRT2,
    distance field and frame as the per-step kernels, with poisoned intermediates, over two frames; on an empty
    screen (no seed anywhere) and a full one (every texel a seed) too; 8192^2 takes the hybrid keys.  Screens it does
    not take (non-square, RGBA8) are unchanged."""
    color, emis = make_scene(scene, W, H)
    ctx = RC2DGI(W, H, cascade_count=N, ray_range=2.0, storage=storage)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    out = {}
    for nt in (0, 2, 3, 4):
        ctx.set_tuning("jfa_tail", nt)
        assert ctx.get_tuning("jfa_tail") == nt
        ctx.set_tuning("poison", 1)
        for _ in range(2):
            ctx.do_rc2dgi()
        ctx.sync()
        out[nt] = {k: ctx.download(k) for k in ("jump1", "jump2", "dist", "color")}
    for nt in (2, 3, 4):
        for k in out[0]:
            assert np.array_equal(out[0][k].view(np.uint8), out[nt][k].view(np.uint8)), \
                f"jfa_tail {nt} {k}: {np.count_nonzero(out[0][k] != out[nt][k])}"
    with pytest.raises(Exception):
        ctx.set_tuning("jfa_tail", 1)
    ctx.close()


@pytest.mark.parametrize("W,H,N,storage", [(256, 256, 4, "f32"), (512, 512, 4, "f32"), (1024, 1024, 5, "f32"),
                                           (512, 256, 4, "f32"), (512, 512, 4, "rgba8"), (4096, 4096, 6, "f32"),
                                           (8192, 8192, 8, "f32")])
def test_jfa_coset_long_steps_are_bit_identical(RC2DGI, W, H, N, storage):
    """The first four JumpFlood steps in one kernel (k_jfa_coset, tuning jfa_coset: square power-of-two
    screens >= 512, the residues modulo W/16 as 16 x 16 tori in LDS) leave the same jumpRT1 / jumpRT2,
    distance field and frame as the per-step kernels: integer keys (<= 4096), float keys (8192^2);
    screens it does not take (256^2, non-square, RGBA8) are unchanged."""
    color, emis = make_scene("demo", W, H)
    ctx = RC2DGI(W, H, cascade_count=N, ray_range=2.0, storage=storage)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    out = {}
    for on in (0, 1, 2):  # 2: the first five steps (32 x 32 tori, integer keys; float keys take the 4-step kernel)
        ctx.set_tuning("jfa_coset", on)
        assert ctx.get_tuning("jfa_coset") == on
        ctx.set_tuning("poison", 1)
        ctx.do_rc2dgi()
        ctx.sync()
        out[on] = {k: ctx.download(k) for k in ("jump1", "jump2", "dist", "color")}
    for on in (1, 2):
        for k in out[0]:
            assert np.array_equal(out[0][k], out[on][k]), f"jfa_coset={on} {k}: {np.count_nonzero(out[0][k] != out[on][k])}"
    ctx.close()


@pytest.mark.parametrize("W,H,N,storage", [(1200, 900, 6, "f32"), (333, 200, 4, "f32"), (640, 360, 5, "rgba8")])
def test_jfa_rows_per_lane_are_bit_identical(RC2DGI, W, H, N, storage):
    """The float-path JumpFlood steps of small screens with 1, 2 or 4 rows per lane (tuning jfa_rt) leave the
    same jumpRT1 / jumpRT2, distance field and frame."""
    color, emis = make_scene("demo", W, H)
    ctx = RC2DGI(W, H, cascade_count=N, ray_range=2.0, storage=storage)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    out = {}
    for rt in (1, 2, 4):
        ctx.set_tuning("jfa_rt", rt)
        assert ctx.get_tuning("jfa_rt") == rt
        ctx.set_tuning("poison", 1)
        ctx.do_rc2dgi()
        ctx.sync()
        out[rt] = {k: ctx.download(k) for k in ("jump1", "jump2", "dist", "color")}
    for rt in (2, 4):
        for k in out[1]:
            assert np.array_equal(out[1][k], out[rt][k]), f"jfa_rt={rt} {k}: {np.count_nonzero(out[1][k] != out[rt][k])}"
    ctx.close()


@pytest.mark.parametrize("W,H,N,rr,scene", [(1200, 900, 6, 2.0, "demo"), (1024, 1024, 6, 2.0, "demo"),
                                             (333, 200, 4, 8.0, "rand:44"), (4096, 4096, 6, 2.0, "demo")])
def test_cascade_chain_is_bit_identical(RC2DGI, W, H, N, rr, scene):
    """The cascade chain (tuning rc_chain, rc2dgi_rc_chain.hip: levels N-2 .. 0 in one launch, a workgroup
    waiting on the readiness flags of the upper tiles under its footprint, sc1 hand-off) leaves every level G_L,
    giRT1 / giRT2 and the frame as the level-by-level launches, over two consecutive frames (the flags carry
    the frame's epoch), rolled and unrolled march, the top level in the launch or before it, with no workgroup
    timing out."""
    color, emis = make_scene(scene, W, H)
    ctx = RC2DGI(W, H, cascade_count=N, ray_range=rr)
    ctx.set_keep_levels(True)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    out = {}
    for on in (0, 1, 2, 4):  # 4: the top level in the launch too
        ctx.set_tuning("rc_chain", on)
        assert ctx.get_tuning("rc_chain") == on
        ctx.set_tuning("poison", 1)
        for frame in range(2):
            ctx.do_rc2dgi()
            ctx.sync()
            assert ctx.get_tuning("rc_chain_timeouts") == 0
            out[on, frame] = {k: ctx.download(k) for k in ("gi1", "gi2", "color")}
            out[on, frame].update({f"G{L}": ctx.download_level(L) for L in range(N)})
    for on in (1, 2, 4):
        for frame in range(2):
            for k in out[0, frame]:
                a, b = out[0, frame][k], out[on, frame][k]
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), \
                    f"rc_chain={on} frame {frame} {k}: {np.count_nonzero(a != b)}"
    ctx.close()


@pytest.mark.parametrize("report", ["sync", "download", "do", "download_level", "do_phase"])
def test_cascade_chain_timeout_is_an_error(RC2DGI, report):
    """A chain workgroup that stops waiting merges upper tiles that were not written, so the frame is wrong: the
    next rc2dgi_sync / rc2dgi_download / rc2dgi_download_level / rc2dgi_do / rc2dgi_do_phase returns
    RC2DGI_E_DEVICE (-7), names the chain, and the context falls back to one launch per level -- the following
    frame is bit-identical to the unchained one.  (rc2dgi_compose: tests/test_present_gpu.py covers the display.)
    The diagnostic knob rc_chain_spin -1 makes every wait time out at once (the product bound is 2^20 polls)."""
    from radiancecascade2dglobalillumination_amd import RC2DGIError

    W, H, N = 1200, 900, 6  # C1, where the committed schedule turns the chain on
    color, emis = make_scene("demo", W, H)
    ctx = RC2DGI(W, H, cascade_count=N, ray_range=2.0)
    if report == "download_level":  # (the kept levels of a chained frame are the chain's own stores)
        ctx.set_keep_levels(True)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    ctx.do_rc2dgi()
    want = ctx.download("color")
    ctx.set_tuning("rc_chain", 1)
    ctx.set_tuning("rc_chain_spin", -1)
    ctx.do_rc2dgi()
    with pytest.raises(RC2DGIError) as ei:
        if report == "sync":
            ctx.sync()
        elif report == "download":
            ctx.download("color")
        elif report == "download_level":
            ctx.download_level(0)
        else:  # (the frame has completed; rc2dgi_do / rc2dgi_do_phase themselves do not synchronise)
            import torch

            torch.cuda.synchronize()
            if report == "do":
                ctx.do_rc2dgi()
            else:
                ctx.do_phase(1)
    assert ei.value.code == -7 and "cascade chain" in str(ei.value)
    assert ctx.get_tuning("rc_chain") == 0  # the fallback
    assert ctx.get_tuning("rc_chain_timeouts") > 0
    ctx.set_tuning("rc_chain_spin", 0)
    ctx.do_rc2dgi()
    ctx.sync()  # no stale report
    got = ctx.download("color")
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    ctx.close()


@pytest.mark.parametrize("scene", ["demo", "speckled", "rand:45"])
def test_shade_split_is_bit_identical(RC2DGI, scene):
    """The records / palette pass split at the cells holding a hittable texel (tuning shade_split: k_shade_scan
    over every cell, k_shade_cells over the listed ones, the list counters alternating frame to frame) gives
    the frames, every level, the bound table and hit flags of the one-kernel pass, over three frames."""
    W = H = 4096
    color, emis = speckled_scene(W, H) if scene == "speckled" else make_scene(scene, W, H)
    ctx = RC2DGI(W, H, cascade_count=6, ray_range=2.0)
    ctx.set_keep_levels(True)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    out = {}
    # 2: split, k_dir_clear on the side stream; 3: split, k_dir_clear's workgroups in k_shade_cells' launch
    for split in (0, 1, 2, 3):
        ctx.set_tuning("shade_split", min(split, 1))
        ctx.set_tuning("side_overlap", max(split - 1, 0))
        assert ctx.get_tuning("shade_split") == min(split, 1)
        assert ctx.get_tuning("side_overlap") == max(split - 1, 0)
        for frame in range(3):
            ctx.do_rc2dgi()
            ctx.sync()
            out[split, frame] = {"color": ctx.download("color"), "hitc": ctx.download_table("hitc"),
                                 "cmin": ctx.download_table("cmin"), "dclr": ctx.download_table("dclr")}
            out[split, frame].update({f"G{L}": ctx.download_level(L) for L in range(6)})
    for split in (1, 2, 3):
        for frame in range(3):
            for k in out[0, frame]:
                a, b = out[0, frame][k], out[split, frame][k]
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), \
                    f"split {split} frame {frame} {k}: {np.count_nonzero(a != b)}"
    ctx.close()


@pytest.mark.parametrize("W,H,N", [(4096, 4096, 6), (8192, 8192, 8)])
def test_shade_cmin_fused_is_bit_identical(RC2DGI, W, H, N):
    """k_shade_cmin (surface records + the proofs' bound table and hit flags in one pass over distRT,
    tuning shade_fused) gives the same frame as k_shade + k_dist_cmin: every level at 4096^2, the merged
    colorRT at 8192^2."""
    color, emis = make_scene("demo", W, H)
    ctx = RC2DGI(W, H, cascade_count=N, ray_range=2.0)
    ctx.set_keep_levels(W <= 4096)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    out = {}
    for on in (0, 1):
        ctx.set_tuning("shade_fused", on)
        assert ctx.get_tuning("shade_fused") == on
        ctx.do_rc2dgi()
        ctx.sync()
        out[on] = {"color": ctx.download("color")}
        if W <= 4096:
            out[on].update({f"G{L}": ctx.download_level(L) for L in range(N)})
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), f"{k}: {np.count_nonzero(out[0][k] != out[1][k])}"
    ctx.close()


@pytest.mark.parametrize("W,H,N", [(256, 256, 4), (512, 256, 4), (240, 180, 3)])
def test_degenerate_direction_tables(RC2DGI, W, H, N):
    """Direction tables with exact zero components, unit axes, components below the exit table's
    2^-100 guard (csrc/rc2dgi_kernels.h rc_exit_terms), denormals and tiny ones: an ended ray holds
    t = +inf, so a zero component makes its position NaN (rejected by the screen test), and the
    screen-exit term of a vanishing component must never prove an exit.  Every level is bit-exact
    with the oracle under every exit-proof setting."""
    color, emis = make_scene("demo", W, H)
    specials = np.array([[1, 0], [0, 1], [-1, 0], [0, -1], [1e-35, 1], [-1e-40, -1], [1, 1e-38], [-1, -2e-7],
                         [0.6, -0.8], [-0.0, 1], [1, -0.0], [0.7071068, 0.7071068]], np.float32)
    rng = np.random.default_rng(11)
    tabs = []
    for L in range(N):
        n = 4 << (2 * L)
        tabs.append(specials[rng.integers(0, len(specials), n)])
    dir_tabs = np.concatenate(tabs).astype(np.float32)  # (directions, 2) as the fixtures hold them
    p = oracle.Params(W=W, H=H, N=N, ray_range=2.0)
    fr = oracle.frame(p, color, emis, dir_tabs=dir_tabs, keep_levels=True)
    ctx = RC2DGI(W, H, cascade_count=N, ray_range=2.0)
    ctx.set_keep_levels(True)
    off = 0
    for L in range(N):
        n = 4 << (2 * L)
        ctx.set_direction_table(L, dir_tabs[off:off + n])
        off += n
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    for v in (0, 6, 13):
        ctx.set_tuning("rc_variant", v)
        for skip in (0, 2, 3):
            ctx.set_tuning("rc_skip", skip)
            ctx.do_rc2dgi()
            ctx.sync()
            for L in range(N):
                g = ctx.download_level(L)
                assert np.array_equal(g, fr.gi_levels[L]), \
                    f"variant {v} rc_skip {skip} level {L}: {np.count_nonzero(g != fr.gi_levels[L])}"
    ctx.close()


def test_linux_merge_fallback_at_the_fused_blur_size(RC2DGI):
    """RC2DGI_FLAG_LINUX_MERGE_FALLBACK (SURVEY A.8, RC2DGI.cs:62) where the merge is otherwise fused into
    the blur kernel (cascade = screen size, power of two): colorRT / tempRT get no GI, finalGI unchanged,
    vs the oracle's linux_merge mode; the same context without the flag adds the GI."""
    from radiancecascade2dglobalillumination_amd import scenes

    W = H = 256
    color, emis = scenes.demo(W, H)
    for flag in (True, False):
        p = oracle.Params(W=W, H=H, N=4, ray_range=2.0, linux_merge=flag)
        fr = oracle.frame(p, color, emis)
        ctx = RC2DGI(W, H, cascade_count=4, ray_range=2.0, linux_merge_fallback=flag)
        ctx.frame(color, emis)
        ctx.sync()
        for k, w in (("temp", fr.temp), ("color", fr.color_out), ("final_gi", fr.gi_final)):
            g = ctx.download(k)
            assert np.array_equal(g, w), f"linux_merge={flag} {k}: {np.count_nonzero(g != w)} differ"
        ctx.close()


@pytest.mark.parametrize("W,H,N,rr,rs,scene,storage", [
    (512, 512, 6, 2.0, 1.0, "demo", "f32"), (333, 200, 4, 8.0, 1.0, "demo", "f32"),
    (256, 128, 5, 64.0, 1.0, "rand:12", "f32"), (256, 256, 4, 2.0, 0.5, "rand:3", "f16"),
    (17, 5, 2, 8.0, 1.0, "rand:9", "f32"), (1024, 1024, 6, 2.0, 1.0, "rand:5", "f32"),
    (512, 512, 6, 2.0, 1.0, "rand:6", "rgba8"), (2048, 2048, 6, 2.0, 1.0, "demo", "f32"),
    (64, 64, 3, 2.0, 1.0, "empty", "f32"), (512, 512, 8, 64.0, 1.0, "rand:19", "f32"),
    (640, 384, 5, 2.0, 1.0, "demo", "f32"), (512, 512, 5, 2.0, 1.0, "full", "f32")])
def test_miss_proofs_are_bit_identical(RC2DGI, W, H, N, rr, rs, scene, storage):
    """Directional miss proofs (tuning rc_mp: a sample from which no later sample of the ray can pass the
    hit test ends the ray unread -- k_dist_cmin's hit cells incl. the REPEAT wrap, k_dir_clear's clear
    distances per angular bin) with every tail setting (-1: every unproved ray queued at once, 0 off, 10
    the default) in the one-probe tile variants, and the variants without them (the flag must leave
    those alone): every level bit-exact vs the oracle (RadianceCascades.fs:60-92: a miss returns
    (0,0,0,1) however it ends)."""
    color, emis = make_scene(scene, W, H)
    if storage == "rgba8":
        color, emis = oracle.from_u8(np.rint(np.clip(color, 0, 1) * 255)), oracle.from_u8(np.rint(np.clip(emis, 0, 1) * 255))
    fr = oracle.frame(oracle.Params(W=W, H=H, N=N, ray_range=rr, render_scale=rs, **mode_params(storage)), color, emis,
                      keep_levels=True)
    ctx = RC2DGI(W, H, cascade_count=N, ray_range=rr, render_scale=rs, storage=storage)
    ctx.set_keep_levels(True)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    ctx.set_tuning("rc_skip", 2)  # bound tables at every size
    ctx.set_tuning("rc_mp", 1)
    for v in (0, 3, 4, 13, 18, 19, 6):
        ctx.set_tuning("rc_variant", v)
        for tail in (-1, 0, 10):
            ctx.set_tuning("rc_tail", tail)
            ctx.do_rc2dgi()
            ctx.sync()
            for L in range(N):
                g = ctx.download_level(L)
                assert np.array_equal(g, fr.gi_levels[L]), \
                    f"variant {v} tail {tail} level {L}: {np.count_nonzero(np.any(g != fr.gi_levels[L], axis=-1))} differ"
    ctx.close()


def dir_clear_cpu(hitc, boxes):
    """k_dir_clear restated (rc2dgi_side.hip): per angular bin j and cell (cy, cx) of the 64 x 64 grid, the
    first step s whose box (boxes[j, s] = x0, x1, y0, y1 cell offsets, clipped to the grid) holds a hit cell,
    if that comes before the first step whose box leaves the grid (vertically: the row's first such step;
    sideways: the cell's), else 255."""
    D = hitc.shape[0]
    P = np.zeros((D + 1, D + 1), np.int64)
    P[1:, 1:] = hitc.astype(np.int64).cumsum(0).cumsum(1)
    out = np.full((boxes.shape[0], D, D), 255, np.uint8)
    cx = np.arange(D)[:, None]
    for j in range(boxes.shape[0]):
        B = boxes[j].astype(np.int64)
        x0 = np.maximum(0, cx + B[None, :, 0])
        x1 = np.minimum(D - 1, cx + B[None, :, 1])
        xoff = x0 > x1  # (cells, steps)
        for cy in range(D):
            ly0 = np.maximum(0, cy + B[:, 2])
            ly1 = np.minimum(D - 1, cy + B[:, 3])
            voff = ly0 > ly1
            nsteps = int(np.argmax(voff)) if voff.any() else B.shape[0]
            a0, a1 = np.minimum(ly0, D - 1), np.maximum(ly1, 0)
            c0, c1 = np.clip(x0, 0, D - 1), np.clip(x1, 0, D - 1)
            s = (P[a1[None, :] + 1, c1 + 1] - P[a0[None, :], c1 + 1] - P[a1[None, :] + 1, c0] + P[a0[None, :], c0])
            hit = (s > 0) & ~xoff & ~voff[None, :]
            first_hit = np.where(hit.any(1), hit.argmax(1), B.shape[0])
            first_off = np.minimum(nsteps, np.where(xoff.any(1), xoff.argmax(1), B.shape[0]))
            out[j, cy] = np.where(first_hit < first_off, first_hit, 255)
    return out


@pytest.mark.parametrize("scene", ["demo", "speckled"])
def test_side_tables_match_their_restatement(RC2DGI, scene):
    """The march's side tables of a 4096^2 frame against CPU restatements from the frame's own distRT and
    inputs: the hit-cell flags and bound table (k_shade_cmin: REPEAT-wrap texels in the last cell row /
    column), the directional clear steps (k_dir_clear, on the downloaded hit flags and the host's step boxes),
    and the surface palettes: the march field equals distRT wherever the hit test fails, holds a palette entry
    (or 15: none) where it passes, and every entry used holds exactly that texel's record (emission with alpha
    1, else albedo with _Reflectivity)."""
    W = H = 4096
    color, emis = speckled_scene(W, H) if scene == "speckled" else make_scene(scene, W, H)
    ctx = RC2DGI(W, H, cascade_count=6, ray_range=2.0)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    assert ctx.get_tuning("rc_pal") == 1
    ctx.do_rc2dgi()
    ctx.sync()
    d = ctx.download("dist")  # RGBA: R, G = the bytes of q (packUNorm16)
    q = (np.rint(d[..., 0] * 255).astype(np.uint32) << 8) | np.rint(d[..., 1] * 255).astype(np.uint32)
    hittable = q <= 65  # decode_dist(q) < 0.001 (exhaustive: tests/test_kernels_cpu.py)
    C = W // 64
    qe = np.concatenate([q, q[:, :1]], 1)
    qe = np.concatenate([qe, qe[:1, :]], 0)  # REPEAT wrap onto column / row 0
    cmin_q = np.full((64, 64), 0xFFFF, np.uint32)
    for cy in range(64):
        for cx in range(64):
            y1 = (cy + 1) * C + (1 if cy == 63 else 0)
            x1 = (cx + 1) * C + (1 if cx == 63 else 0)
            cmin_q[cy, cx] = qe[cy * C:y1, cx * C:x1].min()
    hitc = (cmin_q <= 65).astype(np.uint8)
    assert np.array_equal(ctx.download_table("hitc"), hitc)
    dmin = (cmin_q.astype(np.float64) / 65535).astype(np.float32)
    want_cmin = np.where(cmin_q <= 65, 0, np.minimum(np.floor(dmin * np.float32(512)), 255)).astype(np.uint8)
    assert np.array_equal(ctx.download_table("cmin"), want_cmin)
    assert np.array_equal(ctx.download_table("dclr"), dir_clear_cpu(hitc, ctx.download_table("dboxes")))
    m = ctx.download_table("mfield")[:, :W].astype(np.uint32)
    assert np.array_equal(m[~hittable], q[~hittable])
    assert m[hittable].max(initial=0) <= 15
    e, c = emis[..., :3], color[..., :3]
    lit = np.sqrt(e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1] + e[..., 2] * e[..., 2]) > 0
    rec = np.where(lit[..., None], np.concatenate([e, np.ones_like(e[..., :1])], -1),
                   np.concatenate([c, np.zeros_like(c[..., :1])], -1))  # _Reflectivity 0
    pal = ctx.download_table("cellpal")
    ys, xs = np.nonzero(hittable & (m < 15))
    got = pal[ys // C, xs // C, m[ys, xs]]
    assert np.array_equal(got.view(np.uint32), rec[ys, xs].view(np.uint32))
    if scene == "speckled":
        assert np.count_nonzero(hittable & (m == 15)) > 0  # palettes overflowed: those hits read shade
    # a table the last frame did not build is RC2DGI_E_STATE (the buffers outlive the knob that built them)
    from radiancecascade2dglobalillumination_amd import RC2DGIError
    ctx.set_tuning("rc_pal", 0)
    ctx.do_rc2dgi()
    ctx.sync()
    for name in ("mfield", "cellpal"):
        with pytest.raises(RC2DGIError) as ei:
            ctx.download_table(name)
        assert ei.value.code == -6, name
    ctx.download_table("dclr")  # (still built: directional proofs stay on)
    ctx.close()


def knobs_round_trip(RC2DGI, W, H, N, storage, skip=()):
    """Set every settable key (tests/knob_cases.py) to a non-default value, read it back, put every key back to the
    default a fresh context reports, and render: the frame must equal a fresh context's bit for bit -- no set leaves
    a trace (a stale no-sample proof, side buffers not prepared again, a chain not freed)."""
    from knob_cases import KNOB_CASES

    color, emis = make_scene("rand:40", W, H)

    def render(ctx):
        ctx.frame(color, emis)
        ctx.sync()
        return {k: ctx.download(k) for k in ("color", "final_gi", "dist")}

    keys = [k for k, _ in KNOB_CASES]

    def readable(k):
        """the keys that read what setting k writes (the every-level form is set-only: its levels, one by one)"""
        per_level = k.endswith("_L<n>") or k + "_L<n>" in keys
        return [f"{k.replace('_L<n>', '')}_L{L}" for L in range(N)] if per_level else [k]

    fresh = RC2DGI(W, H, cascade_count=N, storage=storage)
    defaults = {name: fresh.get_tuning(name) for k in keys for name in readable(k)}
    want = render(fresh)
    fresh.close()
    ctx = RC2DGI(W, H, cascade_count=N, storage=storage)
    for k, v in KNOB_CASES:
        if (k, v) in skip:
            continue
        assert all(defaults[name] != v for name in readable(k)), f"{k} = {v} is a default"
        name = k.replace("<n>", str(N - 1))
        ctx.set_tuning(name, v)
        for r in ([name] if k.endswith("_L<n>") else readable(k)):
            assert ctx.get_tuning(r) == v, f"{name} = {v}: {r} reads {ctx.get_tuning(r)}"
    for name, d in defaults.items():
        ctx.set_tuning(name, d)
        assert ctx.get_tuning(name) == d, name
    got = render(ctx)
    ctx.close()
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), f"{k}: {np.count_nonzero(got[k] != want[k])} values differ"


def test_knobs_round_trip_and_leave_no_trace(RC2DGI):
    knobs_round_trip(RC2DGI, 256, 192, 4, "f32")


def test_knobs_round_trip_and_leave_no_trace_rgba8(RC2DGI):
    # (tile shape 5 is an f32 kernel: RGBA8 cascades build 0, 1, 3, 6, 13 .. 19, test_every_rc_variant_is_bit_identical)
    knobs_round_trip(RC2DGI, 64, 64, 2, "rgba8", skip={("rc_variant_L<n>", 5)})
