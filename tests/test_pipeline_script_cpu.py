"""CPU: the script of tests/pipeline_script.py can tell its frames apart, on the oracle alone -- consecutive steps
differ in FINAL_GI and in the merged COLOR (step 5 repeats step 4 and equals it in bits), step 3 puts non-finite values
into level 0 on f32 and f16 and step 4 takes them out again, and the three curves tone slot 1 holds in turn give
different bytes for the same captures.  These are conditions on the script: where one fails, the script changes."""
import numpy as np
import pytest

import pipeline_script as ps
from test_tone_cpu import build_tone_ref, ref_bin
from test_write_cpu import build_write_ref

# the shapes test_gpu_pipeline.py runs an oracle frame at: (a) and (b), (c) the chain, (e) set_stream
SHAPES = [(256, 256, 4), (128, 128, 3), (200, 120, 3)]
STORAGES = ["f32", "f16", "rgba8"]


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return build_write_ref(tmp_path_factory)


@pytest.fixture(scope="module")
def tone_lib(tmp_path_factory):
    return build_tone_ref(tmp_path_factory)


def test_the_script_has_the_six_steps_and_every_change_comes_from_an_image(ref_lib):
    s = ps.build(ref_lib, 128, 128, 3)
    assert [st.index for st in s.steps] == [0, 1, 2, 3, 4, 5]
    kinds = [[(c.kind, c.which, c.img.dtype.name, c.flip, c.blend) for c in st.changes] for st in s.steps]
    assert kinds == [[("upload", "color", "float32", False, False), ("upload", "emissive", "float32", False, False)],
                     [("write", "emissive", "float32", True, False)], [("write", "color", "float16", False, True)],
                     [("write", "emissive", "float32", False, False)], [("write", "emissive", "float32", False, False)], []]
    assert s.steps[1].changes[0].img.shape == (16, 24, 4)
    assert [st.params.ray_range for st in s.steps] == [2.0, 2.0, 200.0, 200.0, 2.0, 2.0]
    assert [st.params.reflectivity for st in s.steps] == [0.0, 0.7, 0.7, 0.7, 0.7, 0.7]
    assert [st.params.blur_radius for st in s.steps] == [1.5, 1.5, 1.5, 1.5, 1.0, 1.0]
    assert [st.curve_name for st in s.steps] == ["q8", "q8", "gamma", "gamma", "reinhard", "reinhard"]
    assert [st.curve is not None for st in s.steps] == [True, False, True, False, True, False]
    odd, fin = s.steps[3].changes[0].img, s.steps[4].changes[0].img
    assert np.isnan(odd).any() and np.isposinf(odd).any() and np.isfinite(fin).all()
    assert s.steps[3].changes[0].rect == s.steps[4].changes[0].rect
    assert len(s.reduce_rects) == 3 and len(s.hist_rects) == 2 and len(s.hist_edges) == 15
    assert s.uv.shape == (256, 2) and s.rays.shape == (64, 6)
    # a subset applies its own changes only: without step 2 no image was blended into COLOR
    sub = ps.build(ref_lib, 128, 128, 3, steps=(0, 1, 4))
    assert [st.index for st in sub.steps] == [0, 1, 4]
    assert ps.same_bits(sub.steps[2].color, sub.steps[0].color) and ps.differ(s.steps[4].color, s.steps[0].color)
    assert ps.differ(sub.steps[2].emis, sub.steps[1].emis)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("W,H,N", SHAPES)
def test_consecutive_frames_differ_and_the_repeat_does_not(ref_lib, W, H, N, storage):
    s = ps.build(ref_lib, W, H, N, storage)
    fr = ps.frames(s)
    for a, b, st in zip(fr, fr[1:], s.steps[1:]):
        what = f"{W}x{H} {storage} step {st.index} against the step before"
        if st.index == 5:
            for k in ("gi_final", "color_out", "blur", "dist"):
                assert ps.same_bits(getattr(a, k), getattr(b, k)), f"{what}: {k}"
            continue
        assert ps.differ(a.gi_final, b.gi_final), f"{what}: FINAL_GI"
        assert ps.differ(a.color_out, b.color_out), f"{what}: the merged COLOR"
    # the blended image is a new occluder: the distance field changes with step 2 and with it alone
    assert [ps.differ(a.dist, b.dist) for a, b in zip(fr, fr[1:])] == [False, True, False, False, False]
    # the crop of DIST the script reads sees it
    x, y, w, h = s.dist_crop
    assert ps.differ(fr[1].dist[y:y + h, x:x + w], fr[2].dist[y:y + h, x:x + w])


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("W,H,N", SHAPES)
def test_step_3_alone_holds_non_finite_values_in_level_0(ref_lib, W, H, N, storage):
    s = ps.build(ref_lib, W, H, N, storage)
    fr = ps.frames(s)
    odd = [int(np.count_nonzero(~np.isfinite(f.gi_levels[0]))) for f in fr]
    if storage == "rgba8":  # (the storage quantises the patch: NaN and +inf become bytes)
        assert odd == [0] * 6
        return
    assert odd[3] >= 1 and odd[:3] == [0, 0, 0] and odd[4:] == [0, 0], odd
    assert not np.isfinite(fr[3].gi_final).all() and np.isfinite(fr[4].gi_final).all()


def test_tone_bytes_is_the_reference_bin(ref_lib, tone_lib):
    rng = np.random.default_rng(3)
    v = np.concatenate([rng.uniform(-0.5, 3.0, 200), [0.0, -0.0, 1.0, np.inf, -np.inf, np.nan]]).astype(np.float32)
    for name, e in ps.curves().items():
        for x in (1.0, 2.0):
            want = [ref_bin(tone_lib, e, np.float32(t) * np.float32(x)) for t in v]
            assert ps.tone_bytes(e, v, x).tolist() == want, (name, x)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("W,H,N", SHAPES)
def test_the_three_curves_tone_the_captures_differently(ref_lib, W, H, N, storage):
    """every step whose frame follows a set_curve, through the curve it should see and through the one it replaced;
    step 3 too, through the curve that comes next"""
    s = ps.build(ref_lib, W, H, N, storage)
    fr = ps.frames(s)
    cv = ps.curves()
    for n, right, wrong in ((2, "gamma", "q8"), (3, "gamma", "reinhard"), (4, "reinhard", "gamma")):
        assert s.steps[n].curve_name == right
        for k, x in (("color_out", 1.0), ("gi_final", 2.0)):  # (the window's view and a thumbnail)
            tex = np.nan_to_num(getattr(fr[n], k)[..., :3], nan=0.0, posinf=0.0, neginf=0.0)
            a, b = ps.tone_bytes(cv[right], tex, x), ps.tone_bytes(cv[wrong], tex, x)
            assert np.count_nonzero(a != b) >= tex.size // 100, f"{W}x{H} {storage} step {n} {k}: {right} against {wrong}"
