"""GPU: one context over many frames, as the reference runs (the scene repainted every frame, RC2DGI.cs:224-264; the
uniforms moved by sliders, RC2DGI.cs:189-221).  Between the frames of a timeline the script changes the scene, every
uniform, the pinned tables, cascadeCount, the debug and timing modes and the upload format; after every frame each
render texture and kept level is compared with oracle.frame of that frame's parameters and inputs alone, in bits --
whatever the context keeps from earlier frames (the no-sample proofs keyed on _RayRange, the tables' dirty flag,
the spare texture the blur swaps, the split records pass's alternating counters, the chain's epoch flags, the
palettes) must not show.
"""
import numpy as np
import pytest

import oracle
import wild_inputs as wi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from radiancecascade2dglobalillumination_amd import rc2dgi

    return rc2dgi


def scene_of(spec, W, H):
    from radiancecascade2dglobalillumination_amd import scenes

    kind, arg = spec
    if kind == "demo":
        return scenes.demo(W, H, arg)
    if kind == "wild":
        return wi.wild_scene(W, H, wi.SEEDS[(W, H)] if arg is None else arg)
    if kind == "rand":
        return scenes.random_scene(W, H, arg)
    return scenes.empty(W, H)


def custom_tables(p):
    """Tables no context computes itself: every direction's (cos, sin) swapped (unit vectors still), a random sky."""
    dirs = np.ascontiguousarray(oracle.dir_tables(p)[:, ::-1])
    sky = np.random.default_rng(p.N).random((4 << (2 * (p.N - 1)), 3)).astype(np.float32) * np.float32(2.0)
    return dirs, sky


# One step per frame: the state changes applied before it (everything else stays as the frame before left it).
# scene: ("demo", t) | ("wild", seed; None: the size's seed of wild_inputs.SEEDS, whose census the CPU file checks) |
# ("empty", 0); u8: upload as RGBA8 bytes (a k/255 scene); dirs / sky: pin the
# custom tables (True) or give them back (False); keep: set_keep_levels; timing: set_timing mode.
TIMELINE = [
    dict(scene=("demo", 3.0)),
    dict(scene=("demo", 3.5), reflectivity=0.7, sun_angle=1.9),
    # (_RayRange on its own, both ways: a sky uniform or a table in the same step would rebuild the tables and with
    # them the no-sample proofs, whatever their _RayRange key says)
    dict(scene=("demo", 7.0), ray_range=200.0),
    dict(scene=("wild", None), ray_range=2.0),
    dict(scene=("empty", 0), blur_radius=0.0, sky_radiance=0.25, sky_color=(0.9, 0.2, 0.1), timing=1),
    dict(blur_radius=1.37),
    dict(scene=("demo", 3.0), blur_radius=3.0, dirs=True, timing=2, sun_angle=-0.4),
    dict(dirs=False, sky=True, blur_radius=1.5, N=-1),
    dict(sky=False, N=+1, keep=False, timing=0, sky_radiance=1.75),
    dict(scene=("demo", 3.5), u8=True, keep=True, sky_color=(0.5, 0.6, 0.8), reflectivity=0.0),
    dict(scene=("wild", None), u8=False, reflectivity=0.7, sun_angle=0.3),
    # (_RayRange both ways once more, after cascadeCount reallocated the cascades and the chain's textures)
    dict(ray_range=200.0),
    dict(ray_range=2.0),
]


def run_timeline(R, W, H, N, tuning=(), chain=False):
    p = oracle.Params(W=W, H=H, N=N)
    ctx = R.RC2DGI(W, H, cascade_count=N, ray_range=p.ray_range)
    for k, v in tuning:
        ctx.set_tuning(k, v)
    ctx.set_keep_levels(True)
    keep, dirs, sky, color, emis = True, None, None, None, None
    for n, step in enumerate(TIMELINE):
        what = f"{W}x{H} frame {n} {step}"
        for key, name in (("ray_range", "_RayRange"), ("reflectivity", "_Reflectivity"), ("sun_angle", "_SunAngle"),
                          ("sky_color", "_SkyColor"), ("sky_radiance", "_SkyRadiance"), ("blur_radius", "_BlurRadius")):
            if key in step:
                setattr(p, key, step[key])
                ctx.set_shader_value(name, step[key])
        def pin_dirs(tab):
            off = 0
            for L in range(p.N):
                cnt = 4 << (2 * L)
                ctx.set_direction_table(L, None if tab is None else tab[off:off + cnt])
                off += cnt
            return tab

        # (the pinned tables are per cascadeCount: given back before it changes, pinned after)
        if step.get("dirs") is False:
            dirs = pin_dirs(None)
        if step.get("sky") is False:
            sky = None
            ctx.set_sky_table(None)
        if "N" in step:
            assert dirs is None and sky is None
            p.N += step["N"]
            ctx.cascade_count = p.N
        if step.get("dirs"):
            dirs = pin_dirs(custom_tables(p)[0])
        if step.get("sky"):
            sky = custom_tables(p)[1]
            ctx.set_sky_table(sky)
        if "keep" in step:
            keep = step["keep"]
            ctx.set_keep_levels(keep)
        if "timing" in step:
            ctx.set_timing(step["timing"])
        if "scene" in step:
            color, emis = scene_of(step["scene"], W, H)
            if step.get("u8"):
                c8, e8 = (np.rint(a * 255).astype(np.uint8) for a in (color, emis))
                ctx.upload("color", c8)
                ctx.upload("emissive", e8)
                color, emis = (a.astype(np.float32) / np.float32(255) for a in (c8, e8))
            else:
                ctx.upload("color", color)
                ctx.upload("emissive", emis)
        ctx.do_rc2dgi()
        ctx.sync()
        blur = p.blur_radius > 0
        fr = oracle.frame(p, color, emis, dir_tabs=dirs, sky_tab=sky, keep_levels=keep)
        assert ctx.final_gi == fr.final_gi, what
        wi.assert_bits(wi.download_all(ctx, levels=p.N if keep else 0, blur=blur), wi.oracle_textures(fr, blur=blur), what)
        # which path ran: without the chain the no-sample proofs follow _RayRange both ways, and the levels they
        # cover are fills; a chained frame never fills, so no fill at _RayRange 200 shows that the chain ran there --
        # one launch per level (a quiet fallback) would have filled
        fills = ctx.get_tuning("rc_fill_levels")
        if chain:
            assert ctx.get_tuning("rc_chain") == 1 and ctx.get_tuning("rc_chain_timeouts") == 0, what
            assert fills == 0, f"{what}: rc_fill_levels {fills:#x} on a chained frame"
        else:
            assert (fills != 0) == (p.ray_range == 200.0), f"{what}: rc_fill_levels {fills:#x}"
        if ctx.get_tuning("rc_chain") == 0 and "timing" in step and step["timing"]:
            t = ctx.pass_times(levels=p.N if step["timing"] == 1 else 0)
            assert t["total"] > 0, what
    assert n + 1 >= 8
    ctx.close()


def test_live_context_256(R):
    """256^2, N = 6: power-of-two, the fused blur + merge and its spare-texture swap."""
    run_timeline(R, 256, 256, 6)


def test_live_context_200x120(R):
    """200 x 120, N = 3: float JumpFlood keys, separate blur and merge passes."""
    run_timeline(R, 200, 120, 3)


def test_live_context_1200x900_chained(R):
    """The reference's own size with the cascade chain (its epoch flags carry over the frames, the chain's textures
    are reallocated with cascadeCount)."""
    run_timeline(R, 1200, 900, 6, tuning=(("rc_chain", 1),), chain=True)


def test_live_context_4096_default_schedule(R):
    """4096^2, N = 6 on the default schedule (palettes, the split records pass with its alternating list counters,
    no strips), four frames with the scene and _Reflectivity changing: each frame equals a fresh context given that
    frame alone, on every level and output; the third (the wild scene) also equals the oracle on 48 sampled rows of
    every level."""
    W = H = 4096
    N = 6
    steps = [(("demo", 3.0), 0.0), (("demo", 7.0), 0.7), (("wild", wi.SEEDS[(W, H)]), 0.6), (("rand", 46), 0.2)]
    outs = ("color", "temp", "dist", "blur", "final_gi")

    def grab(c):
        got = {k: c.download(k) for k in outs}
        got.update({f"L{L}": c.download_level(L) for L in range(N)})
        return got

    live = R.RC2DGI(W, H, cascade_count=N)
    live.set_keep_levels(True)
    for n, (spec, refl) in enumerate(steps):
        color, emis = scene_of(spec, W, H)
        live.set_shader_value("_Reflectivity", refl)
        live.frame(color, emis)
        live.sync()
        got = grab(live)
        fresh = R.RC2DGI(W, H, cascade_count=N)
        fresh.set_keep_levels(True)
        fresh.set_shader_value("_Reflectivity", refl)
        fresh.frame(color, emis)
        fresh.sync()
        want = grab(fresh)
        fresh.close()
        wi.assert_bits(got, want, f"frame {n} {spec} against a fresh context")
        del want
        if spec[0] == "wild":
            p = oracle.Params(W=W, H=H, N=N, reflectivity=refl)
            dirs, sky = oracle.dir_tables(p), oracle.sky_table(p)
            rows = np.linspace(0, H - 1, 48).astype(int)
            offs = [(((1 << (2 * L)) - 1) // 3) * 4 for L in range(N)]
            for L in range(N - 1, -1, -1):
                upper = got[f"L{L + 1}"] if L < N - 1 else None
                out = np.zeros_like(got["L0"])
                for r in rows:
                    oracle.rc_level(p, L, upper, color, emis, got["dist"], out, np.ascontiguousarray(dirs[offs[L]:]),
                                    sky, int(r), int(r) + 1)
                assert wi.bits_equal(got[f"L{L}"][rows], out[rows]), f"frame {n} level {L} against the oracle"
    live.close()
