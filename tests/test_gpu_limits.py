"""GPU: frames at the largest screens and deepest cascades the ABI admits, bit for bit against the CPU oracle.

rc2dgi_create takes screens up to 32768 on either axis and cascade_count up to 15; the rest of the suite stops at
8192 and N = 8.  The code changes path at sizes in between -- the JumpFlood key mode (4096, 16384), the integer-tap
gate (16384 on both axes), the texcoord table (W + H <= 8192), the no-seed value one above the coordinate 32767, the
packed marches' gate, the 16-bit tile fields of the workgroup map, tables of 4^N entries, two-digit level keys -- and
each case below names the gate it is there for.  Thin screens (tests/limit_scenes.py) keep the oracle at half a
second; every comparison is exact equality with oracle.frame(..., keep_levels=True), no tolerance.

Not covered here (admitted by rc2dgi_create, not verified): cascade_count 13 to 15, and square screens above 8192
against a whole-frame oracle."""
import numpy as np
import pytest

import oracle
from limit_scenes import thin_case, wall_scene
from shard_compare import assert_shard_matches_whole, whole_frame
from test_gpu_parity import RC2DGI  # noqa: F401  (the module's fixture)
from test_gpu_parity import (CASCADE, SCREEN, assert_parity, knobs_round_trip, make_scene, mode_params, oracle_dict,
                             run_hip)

pytestmark = pytest.mark.gpu

E_ARG = -1


def frame_names(N):
    return list(SCREEN + CASCADE) + ["final_gi"] + [f"gi_L{L}" for L in range(N)]


# ---------------------------------------------------------------- the oracle's frames, computed once and shared
_THIN = {}


def thin_reference(W, H, storage="f32"):
    """(params, color, emissive, the oracle's textures) of thin shape W x H; never written to afterwards"""
    key = (W, H, storage)
    if key not in _THIN:
        N, rr, seed = thin_case(W, H)
        p = oracle.Params(W=W, H=H, N=N, ray_range=rr, **mode_params(storage))
        color, emis = wall_scene(W, H, seed)
        want = oracle_dict(oracle.frame(p, color, emis, keep_levels=True))
        for a in want.values():
            a.setflags(write=False)
        _THIN[key] = (p, color, emis, want)
    return _THIN[key]


_SQUARE = {}


def square_reference(W, N, rr, storage="f32", scene="rand:71"):
    key = (W, N, rr, storage, scene)
    if key not in _SQUARE:
        p = oracle.Params(W=W, H=W, N=N, ray_range=rr, **mode_params(storage))
        color, emis = make_scene(scene, W, W)
        want = oracle_dict(oracle.frame(p, color, emis, keep_levels=True))
        for a in want.values():
            a.setflags(write=False)
        _SQUARE[key] = (p, color, emis, want)
    return _SQUARE[key]


def context_of(RC2DGI, p, color, emis, storage="f32"):
    ctx = RC2DGI(p.W, p.H, cascade_count=p.N, render_scale=p.render_scale, ray_range=p.ray_range, storage=storage)
    ctx.set_keep_levels(True)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    return ctx


def render(ctx, N):
    ctx.do_rc2dgi()
    ctx.sync()
    out = {k: ctx.download(k) for k in SCREEN + CASCADE}
    out["final_gi"] = ctx.download("final_gi")
    for L in range(N):
        out[f"gi_L{L}"] = ctx.download_level(L)
    return out


def assert_levels(ctx, want, N, what):
    for L in range(N):
        g = ctx.download_level(L)
        assert np.array_equal(g, want[f"gi_L{L}"]), f"{what} level {L}: {np.count_nonzero(g != want[f'gi_L{L}'])}"


# ---------------------------------------------------------------- thin screens with an axis above 8192
THIN_PARITY = [
    # W, H, storage: the gate the shape is there for
    (32768, 8, "f32"),     # power of two above the integer-tap and packed gates (W > 16384): float JumpFlood steps,
                           # 15 steps with offsets up to 16384, seed column 32767 one below the no-seed value
    (8, 32768, "f32"),     # the same transposed: seed rows up to 32767, 8192 workgroup rows
    (16, 16384, "f32"),    # power of two inside every 16384 gate, H on it: integer taps with float keys (non-square)
    (16384, 16, "f32"),    # the same with W on the gate: the lattice order's one-row grid
    (16, 32768, "f32"),    # W <= 16384 and H = 32768: the integer taps refuse it, the packed marches now do too
    (20000, 12, "f32"),    # not a power of two, W + H above the texcoord table: x * (1/n) texcoords or divisions
    (12, 20000, "f32"),    # the same transposed
    (32767, 6, "f32"),     # W not a power of two while CW = 32768 is: cascade wider than the screen, at the limit
    (12, 8200, "f32"),     # just over the texcoord table's limit (W + H = 8212) on the other axis
    (32768, 8, "f16"),
    (32768, 8, "rgba8"),   # unorm8 seed uv: 32768 columns share 255 values of u
    (8, 32768, "rgba8"),
    (20000, 12, "rgba8"),
]


@pytest.mark.parametrize("W,H,storage", THIN_PARITY)
def test_thin_screens_match_the_oracle(RC2DGI, W, H, storage):
    p, color, emis, want = thin_reference(W, H, storage)
    got = run_hip(RC2DGI, p, color, emis, keep_levels=True)
    assert_parity(got, want, frame_names(p.N), exact=True, what=f"{W}x{H} N={p.N} {storage}")


# one context per shape: both sides of the packed marches' gate (16 x 16384 takes them, 16 x 32768 and 32768 x 16
# fall back to the plain field), and a non-power-of-two screen above the texcoord table
SCHEDULE_SHAPES = [(16, 16384), (16, 32768), (32768, 16), (20000, 12)]


# (32768 x 8: a cascade of 8 rows, fewer than the 18-row upper footprint the 32-row tiles stage)
@pytest.mark.parametrize("W,H", SCHEDULE_SHAPES + [(32768, 8)])
def test_every_rc_variant_on_thin_screens(RC2DGI, W, H):
    """Every tile variant, twice each (a schedule is also deterministic), against the oracle's levels: the tiled,
    packed, nibble and packed-field variants 14 .. 19 included, which fall back to the plain field without a word
    where the screen is outside their gate."""
    p, color, emis, want = thin_reference(W, H)
    ctx = context_of(RC2DGI, p, color, emis)
    for v in range(ctx.get_tuning("rc_variant_count")):
        ctx.set_tuning("rc_variant", v)
        assert ctx.get_tuning(f"rc_variant_L{p.N - 1}") == v
        for rep in range(2):
            ctx.do_rc2dgi()
            ctx.sync()
            assert_levels(ctx, want, p.N, f"{W}x{H} variant {v} run {rep}")
    ctx.close()


KNOB_SWEEPS = [("jfa_tab", (0, 1, 2)), ("jfa_rt", (1, 2, 4)), ("rc_rdiv", (0, 1)), ("rc_skip", (0, 1, 2, 3)),
               ("blur_path", (0, 1, 2)), ("rc_fill", (0, 1)), ("rc_chain", (0, 1))]


@pytest.mark.parametrize("W,H", SCHEDULE_SHAPES)
def test_knob_sweeps_on_thin_screens(RC2DGI, W, H):
    """Each knob swept with the others at their defaults, every frame against the oracle (never against the default
    schedule).  Where the header says a knob applies at some sizes only (jfa_tab 1 needs W + H <= 8192, jfa_rt small
    non-power-of-two screens, blur_path 0 power-of-two cascades of 64 x 32 and up, rc_rdiv non-power-of-two
    cascades), the set succeeds, reads back, and the frame is still the oracle's: a silent fallback."""
    p, color, emis, want = thin_reference(W, H)
    ctx = context_of(RC2DGI, p, color, emis)
    defaults = {k: ctx.get_tuning(k) for k, _ in KNOB_SWEEPS}
    names = frame_names(p.N)
    for key, values in KNOB_SWEEPS:
        for v in values:
            ctx.set_tuning(key, v)
            assert ctx.get_tuning(key) == v
            ctx.set_tuning("poison", 1)
            got = render(ctx, p.N)
            assert_parity(got, want, names, exact=True, what=f"{W}x{H} {key}={v}")
            if key == "rc_chain":
                assert ctx.get_tuning("rc_chain_timeouts") == 0
        ctx.set_tuning(key, defaults[key])
    ctx.close()


def test_row_strips_of_a_16_x_32768_screen(RC2DGI):
    """16 x 32768, N = 4 in 4 row strips through rc2dgi_do_group: every shard's own rows equal the unsharded
    frame's (the strip windows of the float-path JumpFlood with rows up to 32767)."""
    from radiancecascade2dglobalillumination_amd import rc2dgi as R

    W, H, world, blur = 16, 32768, 4, 1.5
    p, color, emis, ref = thin_reference(W, H)
    want = whole_frame(R, W, H, p.N, p.ray_range, 1.0, blur, color, emis)
    for k in ("color", "temp", "dist"):  # (the unsharded frame itself is the oracle's)
        assert np.array_equal(want[k], ref[k]), k
    ctxs = []
    for k in range(world):
        c = R.RC2DGI(W, H, cascade_count=p.N, ray_range=p.ray_range)
        c.set_shader_value("_BlurRadius", blur)
        c.set_shard(k, world)
        c.set_tuning("poison", 1)
        c.upload("color", color)
        c.upload("emissive", emis)
        ctxs.append(c)
    R.do_group(ctxs)
    for c in ctxs:
        c.sync()
    for c in ctxs:
        assert_shard_matches_whole(c, want, W, H, blur, expect_strip_tables=False)
        c.close()


# ---------------------------------------------------------------- cascade resolution above 32768
@pytest.mark.parametrize("W,H,N,rs", [(32768, 8, 3, 1.5),    # CW = 49152
                                      (8, 32768, 4, 2.0),    # CH = 65536
                                      (32767, 6, 3, 1.001),  # CW = 32800: the first multiple of 8 over the limit
                                      (20000, 12, 4, 1e6)])  # sizes past the int range
def test_cascades_wider_than_32768_are_refused(RC2DGI, W, H, N, rs):
    """rc2dgi_create refuses a configuration whose cascade textures would exceed 32768 texels on an axis
    (include/rc2dgi.h, render_scale) with RC2DGI_E_ARG: never a frame that is silently wrong or faults."""
    from radiancecascade2dglobalillumination_amd import RC2DGIError

    with pytest.raises(RC2DGIError) as ei:
        RC2DGI(W, H, cascade_count=N, render_scale=rs)
    assert ei.value.code == E_ARG


def test_cascade_count_cannot_widen_the_cascades_past_32768(RC2DGI):
    """The cascade resolution is the scaled screen rounded up to a multiple of 2^N, and 32768 is one for every N the
    ABI takes: a context that was created cannot be pushed over by _CascadeCount.  32760 x 6 has CW = 32760 at N = 3
    and the limit itself, 32768, at N = 4: the set succeeds and the frame is the oracle's at the new count."""
    W, H, rr = 32760, 6, 8.0
    color, emis = wall_scene(W, H, 11)
    p3 = oracle.Params(W=W, H=H, N=3, ray_range=rr)
    p4 = oracle.Params(W=W, H=H, N=4, ray_range=rr)
    assert oracle.dims(p3)[:2] == (32760, 8) and oracle.dims(p4)[:2] == (32768, 16)
    ctx = context_of(RC2DGI, p3, color, emis)
    assert ctx.cascade_resolution == (32760, 8)
    ctx.cascade_count = 4
    assert ctx.cascade_resolution == (32768, 16)
    want = oracle_dict(oracle.frame(p4, color, emis, keep_levels=True))
    assert_parity(render(ctx, 4), want, frame_names(4), exact=True, what="32760x6 after _CascadeCount 4")
    ctx.close()


# ---------------------------------------------------------------- deep cascades
@pytest.mark.parametrize("W,N,rr,storage", [
    (256, 8, 2.0, "f32"),    # CW = 2^N: the top level's blocks are 2 x 2 probes, the merge clamp one point
    (256, 8, 2.0, "f16"),
    (256, 8, 2.0, "rgba8"),
    (64, 9, 2.0, "f32"),     # CW = 512, eight times the screen: the merge samples a cascade finer than the screen
    (512, 9, 2.0, "f32"),    # 4^9-entry tables, every level marches
    (512, 9, 64.0, "f32"),   # the top levels start off screen: block fills
    (2048, 11, 2.0, "f32"),  # no block-constant table (N > 10), _L10
])
def test_deep_cascades_match_the_oracle(RC2DGI, W, N, rr, storage):
    p, color, emis, want = square_reference(W, N, rr, storage)
    ctx = context_of(RC2DGI, p, color, emis, storage)
    if N == 11:  # the two-digit level keys, non-default, read back
        for key, v in (("rc_variant_L10", 3), ("rc_order_L10", 4 | 4 << 8 | 4 << 16), ("rc_tail_L10", 3),
                       ("rc_mp_L10", 0), ("rc_noproof_L10", 1)):
            ctx.set_tuning(key, v)
            assert ctx.get_tuning(key) == v, key
    got = render(ctx, N)
    if rr == 64.0:
        filled = ctx.get_tuning("rc_fill_levels")
        assert filled != 0 and filled >> (N - 1) == 1, f"rc_fill_levels {filled:#b}"
    ctx.close()
    assert_parity(got, want, frame_names(N), exact=True, what=f"{W}^2 N={N} rayRange={rr} {storage}")


def test_two_digit_level_keys_at_1024_n10(RC2DGI):
    """1024^2, N = 10: per-level keys of level 9 set to non-default values and read back, the frame bit-exact; a key
    of level 10 is RC2DGI_E_ARG and changes nothing."""
    from radiancecascade2dglobalillumination_amd import RC2DGIError

    W, N = 1024, 10
    p, color, emis, want = square_reference(W, N, 2.0)
    ctx = context_of(RC2DGI, p, color, emis)
    sets = (("rc_variant_L9", 3), ("rc_order_L9", 4 | 4 << 8 | 4 << 16), ("rc_tail_L9", 3), ("rc_mp_L9", 0),
            ("rc_noproof_L9", 1))
    for key, v in sets:
        assert ctx.get_tuning(key) != v, f"{key} = {v} is the default"
        ctx.set_tuning(key, v)
        assert ctx.get_tuning(key) == v, key
    for key in ("rc_variant_L10", "rc_order_L10", "rc_tail_L10", "rc_mp_L10", "rc_noproof_L10"):
        with pytest.raises(RC2DGIError) as ei:
            ctx.set_tuning(key, 1)
        assert ei.value.code == E_ARG, key
    for key, v in sets:
        assert ctx.get_tuning(key) == v, key
    got = render(ctx, N)
    ctx.close()
    assert_parity(got, want, frame_names(N), exact=True, what="1024^2 N=10")


@pytest.mark.parametrize("group", ["variants 0-8", "variants 9-17", "variants 18-25", "chain"])
def test_schedules_at_512_n9(RC2DGI, group):
    """512^2, N = 9 (top-level blocks of 2 x 2 probes, 4^8 direction blocks): every tile variant twice, and the
    cascade chain (1, 2, and 4 with the top level in the launch), against the oracle's levels."""
    W, N = 512, 9
    p, color, emis, want = square_reference(W, N, 2.0)
    ctx = context_of(RC2DGI, p, color, emis)
    if group == "chain":
        for on in (1, 2, 4):
            ctx.set_tuning("rc_chain", on)
            assert ctx.get_tuning("rc_chain") == on
            ctx.set_tuning("poison", 1)
            for frame in range(2):
                got = render(ctx, N)
                assert ctx.get_tuning("rc_chain_timeouts") == 0
                assert_parity(got, want, frame_names(N), exact=True, what=f"rc_chain {on} frame {frame}")
    else:
        nv = ctx.get_tuning("rc_variant_count")
        assert nv == 26  # (the three groups cover every variant)
        lo = {"variants 0-8": 0, "variants 9-17": 9, "variants 18-25": 18}[group]
        for v in range(lo, min(lo + 9, nv)):
            ctx.set_tuning("rc_variant", v)
            for rep in range(2):
                ctx.do_rc2dgi()
                ctx.sync()
                assert_levels(ctx, want, N, f"variant {v} run {rep}")
    ctx.close()


def test_knobs_round_trip_at_n9(RC2DGI):
    knobs_round_trip(RC2DGI, 256, 256, 9, "f32")


def test_4096_n12_every_pass(RC2DGI):
    """4096^2, cascadeCount = 12 (the deepest cascade a 4096^2 screen has whole 2 x 2 blocks for; 4^12-entry sky
    table, 22 M directions), as test_headline_4096_n6_every_pass: JumpFlood and the distance field over the whole
    frame; every level on 16 spread rows (the oracle's level pass fed the device's own upper level and distRT);
    blur, copy-back and merge over the whole frame."""
    from radiancecascade2dglobalillumination_amd import scenes

    W = H = 4096
    N = 12
    p = oracle.Params(W=W, H=H, N=N, ray_range=2.0)
    color, emis = scenes.demo(W, H)
    ctx = context_of(RC2DGI, p, color, emis)
    ctx.do_rc2dgi()
    ctx.sync()
    j = oracle.screen_uv(color)
    step = np.float32(1.0)
    for _ in range(12):
        step = np.float32(step * np.float32(0.5))
        j = oracle.jfa_step(j, float(step), 1.0, 1.0)
    assert np.array_equal(ctx.download("jump1"), j), "final JFA state"
    dist = ctx.download("dist")
    assert np.array_equal(dist, oracle.distance_field(j)), "distance field"
    del j
    dirs = oracle.dir_tables(p)
    sky = oracle.sky_table(p)
    rows = np.linspace(0, H - 1, 16).astype(int)
    offs = np.concatenate([[0], np.cumsum([4 << (2 * L) for L in range(N)])])
    upper = None
    out = np.zeros((H, W, 4), np.float32)
    for L in range(N - 1, -1, -1):
        g = ctx.download_level(L)
        tab = np.ascontiguousarray(dirs[offs[L]:offs[L + 1]])
        for r in rows:
            oracle.rc_level(p, L, upper, color, emis, dist, out, tab, sky, int(r), int(r) + 1)
        assert np.array_equal(g[rows], out[rows]), f"level {L}: {np.count_nonzero(g[rows] != out[rows])}"
        upper = g
    del dirs, sky, out
    bl = oracle.blur(upper, p.blur_radius)  # (upper: level 0)
    assert np.array_equal(ctx.download("blur"), bl)
    fin = oracle.blur_copyback(bl, upper)
    assert np.array_equal(ctx.download("final_gi"), fin)
    temp, col = oracle.merge(color, fin)
    assert np.array_equal(ctx.download("temp"), temp) and np.array_equal(ctx.download("color"), col)
    ctx.close()


# ---------------------------------------------------------------- the accessory calls at the far end of a wide texture
# Each against `download` of the same texture through the reference restatements (tests/read_ref.c, reduce_ref.c,
# tone_ref.c, query_ref.c), on the 32768 x 8 f32 context after a frame: the planners' "w <= 32768" at w = 32768.
FAR_RECTS = [(32760, 0, 8, 8), (0, 0, 32768, 1)]  # the last 8 columns; one whole row of the widest texture
FAR_TEXTURES = ["color", "final_gi"]  # a screen texture and a cascade texture, both 32768 x 8


@pytest.fixture(scope="module")
def wide_ctx(RC2DGI):
    p, color, emis, _ = thin_reference(32768, 8)
    ctx = context_of(RC2DGI, p, color, emis)
    ctx.do_rc2dgi()
    ctx.sync()
    assert ctx.cascade_resolution == (32768, 8)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("name", FAR_TEXTURES)
def test_read_at_the_far_end_of_a_wide_texture(wide_ctx, tmp_path_factory, name):
    from test_read_cpu import build_read_ref, ref_image
    from test_read_gpu import same_image

    ref_lib = build_read_ref(tmp_path_factory)
    tex = wide_ctx.download(name)
    assert tex.shape == (8, 32768, 4)
    for rect in FAR_RECTS:
        for dtype in (np.float32, np.float16, np.uint8):
            for flip in (False, True):
                got = wide_ctx.read(name, rect, dtype=dtype, flip=flip)
                what = f"{name} {rect} {np.dtype(dtype).name} flip {flip}"
                same_image(got, ref_image(ref_lib, tex, rect, dtype, flip), what)
        x, y, w, h = rect
        assert np.array_equal(wide_ctx.read(name, rect), tex[y:y + h, x:x + w])


@pytest.mark.parametrize("name", FAR_TEXTURES)
def test_reduce_and_histogram_at_the_far_end_of_a_wide_texture(wide_ctx, tmp_path_factory, name):
    from test_reduce_cpu import build_reduce_ref, ref_reduce
    from test_reduce_gpu import same
    from test_tone_cpu import build_tone_ref, log_table, ref_hist, tone_curves
    from test_tone_gpu import CHANNELS, same_records

    tex = wide_ctx.download(name)
    rects = np.asarray(FAR_RECTS, np.int32)
    want = ref_reduce(build_reduce_ref(tmp_path_factory), tex, rects)
    same(wide_ctx.reduce(name, rects), want, f"reduce {name}", rects)
    tone = build_tone_ref(tmp_path_factory)
    q8 = tone_curves()["q8"]
    for tname, edges, ch in (("q8", q8, "luma"), ("log", log_table(), "r"), ("q8", q8, "a")):
        got = wide_ctx.histogram(name, edges, ch, rects)
        want = ref_hist(tone, tex, CHANNELS.index(ch), rects, edges)
        same_records(got, want, f"histogram {name} {tname} {ch}", rects)
        assert got[0, 1] == 64 and got[1, 1] == 32768  # (texels counted)


@pytest.mark.parametrize("name", FAR_TEXTURES + ["dist", "jump1"])
def test_samples_across_the_seam_of_a_wide_texture(wide_ctx, tmp_path_factory, name):
    """POINT and LINEAR samples at the centres of texels 0, 1, 32766 and 32767 of every row (LINEAR at a centre has
    weight 0 on its neighbour), and half a texel either side of them, where the REPEAT wrap crosses the seam."""
    from test_query_cpu import build_query_ref, ref_sample
    from test_query_gpu import LINEAR, LINEAR_RTS, POINT, same

    ref_lib = build_query_ref(tmp_path_factory)
    tex = wide_ctx.download(name)
    nx, ny = 32768, 8
    cols = np.float32([0, 1, 32766, 32767])
    us = np.concatenate([(cols + np.float32(0.5)) / np.float32(nx), cols / np.float32(nx),
                         (cols + np.float32(1.0)) / np.float32(nx)]).astype(np.float32)
    vs = ((np.arange(ny, dtype=np.float32) + np.float32(0.5)) / np.float32(ny)).astype(np.float32)
    uv = np.ascontiguousarray(np.stack(np.broadcast_arrays(us[None, :], vs[:, None]), -1).reshape(-1, 2), np.float32)
    for filt, mode in ((POINT, 0), (LINEAR, 1)):
        if filt == LINEAR and name not in LINEAR_RTS:  # (the packed screen textures are sampled as the display does)
            continue
        got = wide_ctx.sample(name, uv, filt)
        same(got, ref_sample(ref_lib, tex, uv, mode), f"{name} filter {filt}")
    # the texel centres themselves are the download
    centre = wide_ctx.sample(name, uv[:4], POINT)
    assert np.array_equal(centre, tex[0, [0, 1, 32766, 32767]])


def test_compose_a_view_as_wide_as_the_widest_window(wide_ctx, tmp_path_factory):
    """One view of the final GI at 1:1 into a 32768 x 8 window, the widest rc2dgi_compose takes."""
    from test_tone_cpu import build_tone_ref
    from test_tone_gpu import Downloads, reference, same_image

    views = [("final_gi", 0, 0, 32768, 8, 0, (0, 0, 0, 0))]
    got = wide_ctx.compose([v[:6] for v in views], size=(32768, 8))
    want = reference(build_tone_ref(tmp_path_factory), Downloads(wide_ctx), views, None, (32768, 8))
    same_image(got, want, "final_gi at 1:1")
