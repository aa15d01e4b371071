"""GPU: an image written into a rectangle of an input texture on the device (rc2dgi_write / rc2dgi_write_device,
include/rc2dgi.h) against rc2dgi_upload of the same image, tests/write_ref.c over the `download` of the texture, the
8-bit blend formula of the header and rc2dgi_paint.  Every comparison is exact: floats bit for bit, a NaN equal to any
NaN.  The textures are read back before a frame (COLOR is then the input) unless a case says otherwise."""
import ctypes

import numpy as np
import pytest

from shard_compare import assert_shard_matches_whole, whole_frame
from shard_edge_cases import THIN
from test_read_cpu import same_halves
from test_read_gpu import read_chunk_bytes
from test_reduce_cpu import INT_MAX
from test_write_cpu import (DTYPE_FORMAT, FMT_RGBA8, FMT_RGBA16F, FMT_RGBA32F, WRITE_BLEND, WRITE_FLIP, blend_pairs,
                            build_write_ref, every_half, ref_quant, ref_widen, ref_write, same_floats)

pytestmark = pytest.mark.gpu

f32, f16, u16, u32 = np.float32, np.float16, np.uint16, np.uint32
STORAGES = ["f32", "f16", "rgba8"]
DTYPES = [np.float32, np.float16, np.uint8]
E_ARG = -1
PAD = 0xA5
W0, H0 = 96, 80


@pytest.fixture(scope="module")
def R():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from radiancecascade2dglobalillumination_amd import rc2dgi

    return rc2dgi


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return build_write_ref(tmp_path_factory)


def assert_same(got, want, what):
    if not same_floats(got, want):
        ng, nw = np.isnan(got), np.isnan(want)
        bad = np.argwhere((got.view(u32) != want.view(u32)) & ~(ng & nw))
        raise AssertionError(f"{what}: {len(bad)} values differ, first at {bad[:4].tolist()}: "
                             f"{[(float(got[tuple(k)]), float(want[tuple(k)])) for k in bad[:4]]}")


def to_device(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def write_either(ctx, device, which, img, rect=None, flip=False, blend=False):
    """RC2DGI.write of a numpy image through the host variant, or of its copy on the GPU through the device variant"""
    if device:
        t = to_device(img)
        ctx.write(which, t, rect, flip, blend)
        ctx.sync()
    else:
        ctx.write(which, img, rect, flip, blend)


def pattern(W, H):
    """distinct per texel and channel, exact in every storage's float4 input and far from any image's values"""
    return (np.arange(H * W * 4, dtype=f32).reshape(H, W, 4) + f32(1000.5)).astype(f32)


def wild_images():
    """(color, emissive) of tests/wild_inputs.py at 96 x 80 with NaN, +-inf, -0.0, subnormals and values outside [0, 1]"""
    from test_gpu_inputs import plant_non_finite
    from wild_inputs import SEEDS, wild_scene

    color, emis = wild_scene(W0, H0, SEEDS[(W0, H0)])
    plant_non_finite(color, emis)
    color[3, 5] = [-0.0, 1e-45, -3e-39, 0.5]
    emis[4, 6] = [-0.0, 1e-45, -3e-39, 7.0]
    for a in (color, emis):
        assert np.isnan(a).any() and np.isposinf(a).any() and np.isneginf(a).any() and np.signbit(a[a == 0]).any()
        assert ((a != 0) & (np.abs(a) < f32(1.1754944e-38))).any() and (a > 1).any() and (a < 0).any()
    return color, emis


def byte_image(W, H, seed):
    """(H, W, 4) uint8 holding all 256 bytes in every channel"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    for c in range(4):
        img[:3, :, c].reshape(-1)[:256] = rng.permutation(256).astype(np.uint8)
        assert len(set(img[..., c].reshape(-1).tolist())) == 256
    return img


# ------------------------------------------------------------------ 1: a write of the whole texture is the upload
@pytest.fixture(scope="module", params=STORAGES)
def small(R, request):
    ctx = R.RC2DGI(W0, H0, cascade_count=2, render_scale=0.5, storage=request.param)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("which", ["color", "emissive"])
@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=lambda d: np.dtype(d).name)
def test_whole_texture_write_leaves_the_bits_of_the_upload(R, small, dtype, which):
    ctx = small
    color, emis = wild_images()
    img = byte_image(W0, H0, 11 if which == "color" else 12) if dtype == np.uint8 else (color if which == "color" else emis)
    ctx.upload(which, img)
    want = ctx.download(which)
    for device in (False, True):
        ctx.upload(which, pattern(W0, H0))
        assert not same_floats(ctx.download(which), want)
        write_either(ctx, device, which, img)
        assert_same(ctx.download(which), want, f"{ctx.storage} {which} {'device' if device else 'host'}")
        # through the C call with a null rectangle and a tight pitch given in bytes
        ctx.upload(which, pattern(W0, H0))
        if device:
            t = to_device(img)
            rc = ctx._L.rc2dgi_write_device(ctx._h, R.RT[which], None, DTYPE_FORMAT[np.dtype(dtype).name], 0,
                                            ctypes.c_void_p(t.data_ptr()), W0 * 4 * img.itemsize)
            ctx.sync()
        else:
            rc = ctx._L.rc2dgi_write(ctx._h, R.RT[which], None, DTYPE_FORMAT[np.dtype(dtype).name], 0,
                                     ctypes.c_void_p(img.ctypes.data), 0)
        assert rc == 0
        assert_same(ctx.download(which), want, f"{ctx.storage} {which} C call")


@pytest.mark.parametrize("storage", STORAGES)
def test_a_frame_after_the_write_is_the_frame_after_the_upload(R, storage):
    color, emis = wild_images()
    outs = []
    for mode in ("upload", "host", "device"):
        ctx = R.RC2DGI(W0, H0, cascade_count=2, render_scale=0.5, storage=storage)
        if mode == "upload":
            ctx.upload("color", color)
            ctx.upload("emissive", emis)
        else:
            write_either(ctx, mode == "device", "color", color)
            write_either(ctx, mode == "device", "emissive", emis)
        ctx.do_rc2dgi()
        ctx.sync()
        outs.append((ctx.download("final_gi"), ctx.download("color")))
        ctx.close()
    for gi, col in outs[1:]:
        assert_same(gi, outs[0][0], storage + " FINAL_GI")
        assert_same(col, outs[0][1], storage + " merged COLOR")


# ------------------------------------------------------------------ 2: halves
@pytest.mark.parametrize("storage", ["f32", "rgba8"])
def test_every_half_is_widened_exactly(R, ref_lib, storage):
    ctx = R.RC2DGI(128, 128, cascade_count=1, storage=storage)
    h = every_half().view(f16)
    with np.errstate(invalid="ignore"):
        wide = h.astype(f32)
    assert same_floats(ref_widen(ref_lib, h.view(u16)), wide)
    want = ref_quant(ref_lib, wide) if storage == "rgba8" else wide
    for device in (False, True):
        ctx.upload("color", pattern(128, 128))
        write_either(ctx, device, "color", h)
        assert_same(ctx.download("color"), want, f"{storage} {'device' if device else 'host'}")
        ctx.upload("color", pattern(128, 128))
        write_either(ctx, device, "color", h, flip=True)
        assert_same(ctx.download("color"), want[::-1], f"{storage} flipped")
    ctx.close()


def test_read_write_read_of_halves_is_the_identity(R):
    from radiancecascade2dglobalillumination_amd import scenes

    ctx = R.RC2DGI(128, 128, cascade_count=3, storage="f32")
    ctx.frame(*scenes.demo(128, 128))
    ctx.sync()
    assert ctx.cascade_resolution == (128, 128)
    gi = ctx.read("final_gi", dtype=f16)
    assert len(np.unique(gi.view(u16))) > 100, "a frame's FINAL_GI, not a constant"
    for flip in (False, True):
        ctx.write("emissive", gi, flip=flip)
        back = ctx.read("emissive", dtype=f16, flip=flip)
        assert same_halves(back.view(u16), gi.view(u16))
        assert_same(ctx.download("emissive"), (gi[::-1] if flip else gi).astype(f32), "the texels are the widened halves")
    ctx.close()


# ------------------------------------------------------------------ 3: placement
def placement_rects(tw, th):
    rects = [(x, 5 + x, w, 1 + (w + x) % 5) for w in range(1, 10) for x in range(4)]  # heights 1 .. 5
    assert {r[3] for r in rects} == {1, 2, 3, 4, 5}
    rects += [(0, 0, 1, 1), (tw - 1, 0, 1, 1), (0, th - 1, 1, 1), (tw - 1, th - 1, 1, 1)]  # the four corners
    rects += [(0, th - 1, tw, 1), (tw - 1, 0, 1, th), (0, 7, tw, 2), (tw - 9, th - 4, 9, 4), (0, 0, tw, th)]
    return rects


def random_image(rng, w, h, dtype):
    if dtype == np.uint8:
        return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    v = (rng.standard_normal((h, w, 4)) * 4).astype(f32)
    return v.astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_placement_writes_the_rectangle_and_nothing_else(R, ref_lib, dtype):
    ctx = R.RC2DGI(W0, H0, cascade_count=2, storage="f32")
    rng = np.random.default_rng(21)
    model = pattern(W0, H0)
    ctx.upload("color", model)
    for rect in placement_rects(W0, H0):
        for flip in (False, True):
            for device in (False, True):
                img = random_image(rng, rect[2], rect[3], dtype)
                before = model
                model = ref_write(ref_lib, model, img, rect, flip)
                x, y, w, h = rect
                crop = img[::-1] if flip else img
                if dtype == np.float32:  # (the reference's placement, restated: the crop, and the rest untouched)
                    inside = np.zeros((H0, W0), bool)
                    inside[y:y + h, x:x + w] = True
                    assert np.array_equal(model[y:y + h, x:x + w].view(u32), crop.view(u32))
                    assert np.array_equal(model[~inside].view(u32), before[~inside].view(u32))
                write_either(ctx, device, "color", img, rect, flip)
                assert_same(ctx.download("color"), model, f"{rect} flip {flip} {'device' if device else 'host'}")
    ctx.close()


# ------------------------------------------------------------------ 4: source addressing
def pad_texel_bits(ref_lib, dtype):
    """the float bits a channel would get from padding bytes (0xA5)"""
    if dtype == np.float32:
        return 0xA5A5A5A5
    if dtype == np.float16:
        return int(ref_widen(ref_lib, np.array([0xA5A5], u16)).view(u32)[0])
    return int((f32(0xA5) / f32(255)).view(u32))


def image_without_pad(rng, w, h, dtype):
    img = random_image(rng, w, h, dtype)
    if dtype == np.uint8:
        img[img == PAD] = 0x5A
    elif dtype == np.float16:
        img.view(u16)[img.view(u16) == 0xA5A5] = 0
    return img


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_source_pitch_alignment_and_padding(R, ref_lib, dtype):
    import torch

    ctx = R.RC2DGI(W0, H0, cascade_count=2, storage="f32")
    rng = np.random.default_rng(31)
    px = 4 * np.dtype(dtype).itemsize
    bad = pad_texel_bits(ref_lib, dtype)
    tdt = {np.float32: torch.float32, np.float16: torch.float16, np.uint8: torch.uint8}[dtype]
    for rect in [(3, 2, 37, 11), (0, 0, W0, H0), (1, 70, 95, 10), (5, 5, 1, 7)]:
        x, y, w, h = rect
        for flip in (False, True):
            img = image_without_pad(rng, w, h, dtype)
            want = ref_write(ref_lib, pattern(W0, H0), img, rect, flip)
            assert not (want.view(u32) == bad).any()
            # the device variant: one pixel past a 256-byte boundary, rows one pixel longer than w
            pitch = (w + 1) * px
            raw = np.full(256 + px + pitch * h + 256, PAD, np.uint8)
            dev = torch.full((len(raw) + 256,), PAD, dtype=torch.uint8, device="cuda")
            start = (-dev.data_ptr()) % 256 + px
            for j in range(h):
                raw[start + j * pitch:start + j * pitch + w * px] = img[j].reshape(-1).view(np.uint8)
            dev[:len(raw)] = torch.from_numpy(raw).to("cuda")
            torch.cuda.synchronize()
            ctx.upload("color", pattern(W0, H0))
            r = R._rect_array([rect])
            rc = ctx._L.rc2dgi_write_device(ctx._h, 0, r.ctypes.data_as(ctypes.c_void_p), DTYPE_FORMAT[np.dtype(dtype).name],
                                            WRITE_FLIP if flip else 0, ctypes.c_void_p(dev.data_ptr() + start), pitch)
            assert rc == 0, ctx._L.rc2dgi_last_error(ctx._h)
            ctx.sync()
            got = ctx.download("color")
            assert_same(got, want, f"device {rect} flip {flip}")
            assert not (got.view(u32) == bad).any(), "padding reached the texture"
            # a strided view of a larger tensor through RC2DGI.write
            wide = np.empty((h, w + 3, 4), dtype)
            wide.view(np.uint8)[:] = PAD
            wide[:, 2:2 + w] = img
            big = to_device(wide)
            view = big[:, 2:2 + w]
            assert big.dtype == tdt and view.stride(0) == (w + 3) * 4 and view.data_ptr() == big.data_ptr() + 2 * px
            torch.cuda.synchronize()
            ctx.upload("color", pattern(W0, H0))
            ctx.write("color", view, rect, flip=flip)
            ctx.sync()
            got = ctx.download("color")
            assert_same(got, want, f"strided view {rect} flip {flip}")
            assert not (got.view(u32) == bad).any(), "padding reached the texture"
            # the host variant has no alignment rule: an odd address, an odd pitch
            pitch = w * px + 3
            buf = np.full(1 + pitch * h + 5, PAD, np.uint8)
            for j in range(h):
                buf[1 + j * pitch:1 + j * pitch + w * px] = img[j].reshape(-1).view(np.uint8)
            assert buf.ctypes.data % 2 == 0 and pitch % 2 == 1
            ctx.upload("color", pattern(W0, H0))
            rc = ctx._L.rc2dgi_write(ctx._h, 0, r.ctypes.data_as(ctypes.c_void_p), DTYPE_FORMAT[np.dtype(dtype).name],
                                     WRITE_FLIP if flip else 0, ctypes.c_void_p(buf.ctypes.data + 1), pitch)
            assert rc == 0, ctx._L.rc2dgi_last_error(ctx._h)
            got = ctx.download("color")
            assert_same(got, want, f"host {rect} flip {flip}")
            assert not (got.view(u32) == bad).any(), "padding reached the texture"
            # ... and a numpy view with padded rows through RC2DGI.write
            ctx.upload("color", pattern(W0, H0))
            ctx.write("color", wide[:, 2:2 + w], rect, flip=flip)
            assert_same(ctx.download("color"), want, f"numpy view {rect} flip {flip}")
    with pytest.raises(ValueError):
        ctx.write("color", np.zeros((3, 4, 4), f32), (0, 0, 5, 3))
    with pytest.raises(TypeError):
        ctx.write("color", np.zeros((3, 4, 4), np.int32), (0, 0, 4, 3))
    with pytest.raises(ValueError):
        ctx.write("color", torch.zeros((3, 4, 4), device="cuda"), (0, 0, 4, 4))
    with pytest.raises(TypeError):
        ctx.write("color", torch.zeros((3, 4, 4), dtype=torch.int32, device="cuda"), (0, 0, 4, 3))
    with pytest.raises(TypeError):
        ctx.write("color", torch.zeros((3, 4, 4)), (0, 0, 4, 3))  # a tensor that is not on the GPU
    ctx.close()


# ------------------------------------------------------------------ 5: the blend
def test_float_blend_on_ordinary_and_non_finite_alphas(R, ref_lib):
    src, dst = blend_pairs()
    n = 35
    assert len(src) == n * n
    rect = (3, 5, n, n)
    tex = pattern(W0, H0)
    tex[5:5 + n, 3:3 + n] = dst.reshape(n, n, 4)
    img = src.reshape(n, n, 4)
    assert set(np.nan_to_num(img[..., 3], nan=-7.0, posinf=-8.0).reshape(-1).tolist()) == {0.0, 1.0, 0.5, 2.0, -1.0, -7.0, -8.0}
    ctx = R.RC2DGI(W0, H0, cascade_count=2, storage="f32")
    for flip in (False, True):
        want = ref_write(ref_lib, tex, img, rect, flip, blend=True)
        assert np.isnan(want).any() and not same_floats(want, ref_write(ref_lib, tex, img, rect, flip))
        for device in (False, True):
            ctx.upload("color", tex)
            write_either(ctx, device, "color", img, rect, flip, blend=True)
            assert_same(ctx.download("color"), want, f"flip {flip} {'device' if device else 'host'}")
    # a half image blends as its widening does
    with np.errstate(over="ignore", invalid="ignore"):
        h = img.astype(f16)
    want = ref_write(ref_lib, tex, h.astype(f32), rect, blend=True)
    ctx.upload("emissive", tex)
    ctx.write("emissive", h, rect, blend=True)
    assert_same(ctx.download("emissive"), want, "RGBA16F blended")
    ctx.close()


def test_8_bit_blend_of_every_source_and_alpha(R, ref_lib):
    """rgba8 storage: pixel (s, a) of a 256 x 256 RGBA8 image is (s, s, s, a), over destinations of a few fixed byte
    quadruples, against min(255, mul8(s8, a8) + mul8(d8, 255 - a8))"""
    s = np.arange(256, dtype=np.int64)[None, :, None]
    a = np.arange(256, dtype=np.int64)[:, None, None]
    img = np.empty((256, 256, 4), np.uint8)
    img[..., :3] = np.broadcast_to(s, (256, 256, 3))
    img[..., 3] = np.broadcast_to(a[..., 0], (256, 256))
    quads = np.array([[0, 255, 128, 255], [1, 254, 127, 0], [37, 200, 91, 128], [255, 0, 64, 77], [16, 17, 250, 254]],
                     np.uint8)
    yy, xx = np.mgrid[0:256, 0:256]
    dst = quads[(xx + 3 * yy) % len(quads)]
    mul8 = lambda p, q: (p * q * 257 + 32768) >> 16  # noqa: E731
    src8 = img.astype(np.int64)
    want8 = np.minimum(255, mul8(src8, a) + mul8(dst.astype(np.int64), 255 - a)).astype(np.uint8)
    ctx = R.RC2DGI(256, 256, cascade_count=1, storage="rgba8")
    inv = f32(1) / f32(255)
    for device in (False, True):
        ctx.upload("color", dst)
        tex = ctx.download("color")
        assert np.array_equal(tex.view(u32), (dst.astype(f32) * inv).astype(f32).view(u32))
        write_either(ctx, device, "color", img, blend=True)
        assert np.array_equal(ctx.download("color", np.uint8), want8)
        got = ctx.download("color")
        assert np.array_equal(got.view(u32), (want8.astype(f32) * inv).astype(f32).view(u32))
        assert_same(got, ref_write(ref_lib, tex, img, blend=True, u8=True), "write_ref.c")
    # a float image into RGBA8 storage is quantized first: out-of-range and non-finite values and alphas
    srcf, dstf = blend_pairs()
    n = 35
    tex = ctx.download("color")
    imgf = srcf.reshape(n, n, 4)
    want = ref_write(ref_lib, tex, imgf, (7, 9, n, n), flip=True, blend=True, u8=True)
    ctx.write("color", imgf, (7, 9, n, n), flip=True, blend=True)
    assert_same(ctx.download("color"), want, "float image, 8-bit blend")
    ctx.close()


@pytest.mark.parametrize("storage", ["f32", "rgba8"])
@pytest.mark.parametrize("colour", [(200, 100, 50, 255), (90, 220, 13, 97)], ids=["opaque", "translucent"])
def test_blend_of_a_constant_image_is_the_paint_of_that_rectangle(R, storage, colour):
    from radiancecascade2dglobalillumination_amd import scenes

    base = scenes.demo(W0, H0)[0]
    px, py, pw, ph = 7, 11, 30, 9  # DrawRectangle(7, 11, 30, 9, colour), screen coordinates (y down)
    rect = (px, H0 - py - ph, pw, ph)  # GL rows
    ctx = R.RC2DGI(W0, H0, cascade_count=2, storage=storage)
    ctx.upload("color", base)
    start = ctx.download("color")
    ctx.paint("color", [(0, px, py, pw, ph) + colour])
    painted = ctx.download("color")
    changed = np.any(painted.view(u32) != start.view(u32), -1)
    ys, xs = np.nonzero(changed)
    assert changed.any() and xs.min() >= rect[0] and xs.max() < rect[0] + pw and ys.min() >= rect[1] and ys.max() < rect[1] + ph
    img = np.broadcast_to((f32(colour) * (f32(1) / f32(255))).astype(f32), (ph, pw, 4)).copy()
    for device in (False, True):
        for flip in (False, True):
            ctx.upload("color", base)
            write_either(ctx, device, "color", img, rect, flip, blend=True)
            assert_same(ctx.download("color"), painted, f"{storage} {colour} {'device' if device else 'host'}")
    ctx.close()


# ------------------------------------------------------------------ 6: more than one staging block
def test_a_host_image_larger_than_the_staging_goes_in_blocks(R, ref_lib):
    W, H = 1200, 900
    chunk = read_chunk_bytes()
    per = chunk // (W * 16)
    assert W * H * 16 == 17280000 and -(-H // per) == 3 and H % per != 0, "three blocks, the last one short"
    ctx = R.RC2DGI(W, H, cascade_count=1, storage="f32")
    rng = np.random.default_rng(5)
    dst = rng.standard_normal((H, W, 4)).astype(f32)
    img = rng.standard_normal((H, W, 4)).astype(f32)
    img[..., 3] = rng.choice(f32([0.0, 1.0, 0.5, 0.25, 1.5, 0.3]), (H, W))
    img[..., 0] = np.arange(H, dtype=f32)[:, None]  # (the row, so that a misplaced block shows)
    ctx.upload("color", dst)
    ctx.write("color", img, flip=True, blend=True)
    assert_same(ctx.download("color"), ref_write(ref_lib, dst, img, None, True, True), "flipped and blended")
    ctx.write("color", img)
    assert_same(ctx.download("color"), img, "replaced")
    ctx.close()


# ------------------------------------------------------------------ 7: ordering and state
def test_device_write_is_ordered_between_the_frames_around_it(R, ref_lib):
    from radiancecascade2dglobalillumination_amd import scenes

    W, H, N = 200, 160, 3
    color, emis = scenes.demo(W, H)
    rng = np.random.default_rng(9)
    rect = (40, 30, 64, 48)
    ec = np.zeros((48, 64, 4), f32)
    ec[..., :3] = rng.random((48, 64, 3)).astype(f32) * 3
    ec[..., 3] = 1
    cc = rng.random((48, 64, 4)).astype(f32)
    color2 = ref_write(ref_lib, color, cc, rect)
    emis2 = ref_write(ref_lib, emis, ec, rect, flip=True)

    def outputs(c):
        return {k: c.download(k) for k in ("final_gi", "color", "dist")}

    plain = R.RC2DGI(W, H, cascade_count=N)
    plain.frame(color, emis)
    plain.sync()
    old = outputs(plain)
    plain.close()
    plain = R.RC2DGI(W, H, cascade_count=N)  # the written input from the start
    plain.frame(color2, emis2)
    plain.sync()
    new = outputs(plain)
    plain.close()
    assert not same_floats(old["final_gi"], new["final_gi"]), "the written input changes the frame"

    ctx = R.RC2DGI(W, H, cascade_count=N)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    tc, te = to_device(cc), to_device(ec)
    ctx.do_rc2dgi()
    ctx.write("color", tc, rect)  # no sync between the frame and the writes
    ctx.write("emissive", te, rect, flip=True)
    assert_same(ctx.download("color"), color2, "COLOR reads as the input again")
    ctx.sync()
    for k in ("final_gi", "dist"):
        assert_same(ctx.download(k), old[k], f"the frame enqueued before the write: {k}")
    ctx.do_rc2dgi()
    ctx.sync()
    got = outputs(ctx)
    for k in got:
        assert_same(got[k], new[k], f"the frame enqueued after the write: {k}")
    # after a frame, a partial write to COLOR makes COLOR read as the old input plus the rectangle
    assert_same(ctx.download("color"), new["color"], "the merged output")
    patch = rng.random((5, 9, 4)).astype(f32)
    ctx.write("color", patch, (1, 2, 9, 5))
    assert_same(ctx.download("color"), ref_write(ref_lib, color2, patch, (1, 2, 9, 5)), "the old input plus the rectangle")
    ctx.close()


# ------------------------------------------------------------------ 8: errors
def test_errors_leave_a_valid_context_and_an_untouched_texture(R, ref_lib):
    import torch

    ctx = R.RC2DGI(W0, H0, cascade_count=2, storage="f32")
    L, h = ctx._L, ctx._h
    tex = {"color": pattern(W0, H0), "emissive": pattern(W0, H0) + f32(0.25)}
    for k, v in tex.items():
        ctx.upload(k, v)
    host = np.zeros(W0 * H0 * 16 + 64, np.uint8)
    dev = torch.zeros((W0 * H0 * 16 + 64,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert dev.data_ptr() % 16 == 0
    hp = lambda off=0: ctypes.c_void_p(host.ctypes.data + off)  # noqa: E731
    dp = lambda off=0: ctypes.c_void_p(dev.data_ptr() + off)  # noqa: E731
    rp = lambda r: R._rect_array([r]).ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    ok = (3, 5, 17, 9)

    def refused(code):
        """the call failed as documented, said why, wrote nothing, and the context still works"""
        assert code == E_ARG, code
        assert L.rc2dgi_last_error(h), "no message"
        ctx.sync()
        for k, v in tex.items():
            assert np.array_equal(ctx.download(k).view(u32), v.view(u32)), "a refused call wrote"

    both = ((L.rc2dgi_write, hp), (L.rc2dgi_write_device, dp))
    for fn, p in both:
        refused(fn(h, 0, rp(ok), FMT_RGBA32F, 0, None, 0))  # a null source
        for which in (-1, 2, 7, 9, 10):
            refused(fn(h, which, rp(ok), FMT_RGBA32F, 0, p(), 0))
        for fmt in (3, -1):
            refused(fn(h, 0, rp(ok), fmt, 0, p(), 0))
        for flags in (4, 7, -1, 8 | WRITE_BLEND):
            refused(fn(h, 1, rp(ok), FMT_RGBA32F, flags, p(), 0))
        for r in [(0, 0, 0, 1), (0, 0, 1, 0), (0, 0, -3, 1), (0, 0, 1, -INT_MAX - 1), (-1, 0, 1, 1), (0, -1, 1, 1),
                  (W0 - 16, 0, 17, 1), (0, H0 - 8, 1, 9), (INT_MAX, 0, 1, 1), (0, INT_MAX, 1, 1), (0, 0, INT_MAX, 1),
                  (1, 1, INT_MAX, INT_MAX), (W0, 0, 1, 1), (0, H0, 1, 1)]:
            refused(fn(h, 0, rp(r), FMT_RGBA8, 0, p(), 0))
        for fmt, px in ((FMT_RGBA32F, 16), (FMT_RGBA16F, 8), (FMT_RGBA8, 4)):
            refused(fn(h, 0, rp(ok), fmt, 0, p(), 17 * px - px))  # a pitch one pixel short
            refused(fn(h, 0, None, fmt, 0, p(), W0 * px - px))
    refused(L.rc2dgi_write(h, 0, rp(ok), FMT_RGBA8, 0, hp(), 17 * 4 - 1))  # a pitch one byte short
    for fmt, px in ((FMT_RGBA32F, 16), (FMT_RGBA16F, 8), (FMT_RGBA8, 4)):
        for off in (1, 2, px // 2, px - 1):
            refused(L.rc2dgi_write_device(h, 0, rp(ok), fmt, 0, dp(off), 0))  # a misaligned pointer
        for extra in (1, 2, px // 2, px + 1):
            refused(L.rc2dgi_write_device(h, 0, rp(ok), fmt, 0, dp(), 17 * px + extra))  # a misaligned pitch
    # the order of the checks: the first one that fails names the error
    for fn, p in both:
        assert fn(h, 9, rp((0, 0, 0, 0)), 3, 4, p(), 1) == E_ARG and b"inputs" in L.rc2dgi_last_error(h)
        assert fn(h, 0, rp((0, 0, 0, 0)), 3, 4, p(), 1) == E_ARG and b"format" in L.rc2dgi_last_error(h)
        assert fn(h, 0, rp((0, 0, 0, 0)), 1, 4, p(), 1) == E_ARG and b"flag" in L.rc2dgi_last_error(h)
        assert fn(h, 0, rp((0, 0, 0, 0)), 1, 0, p(), 1) == E_ARG and b"rectangle" in L.rc2dgi_last_error(h)
        assert fn(h, 0, rp(ok), 1, 0, p(), 1) == E_ARG and b"pitch" in L.rc2dgi_last_error(h)
    assert L.rc2dgi_write_device(h, 0, rp(ok), 1, 0, dp(4), 17 * 16 + 4) == E_ARG and b"multiples" in L.rc2dgi_last_error(h)
    # what is allowed: the loosest alignment of each format
    for fmt, px, dt in ((FMT_RGBA32F, 16, f32), (FMT_RGBA16F, 8, f16), (FMT_RGBA8, 4, np.uint8)):
        assert L.rc2dgi_write_device(h, 1, rp(ok), fmt, 0, dp(px), 17 * px + px) == 0
        ctx.sync()
        zeros = np.zeros((9, 17, 4), dt)
        assert_same(ctx.download("emissive"), ref_write(ref_lib, tex["emissive"], zeros, ok), "zeros written")
        ctx.upload("emissive", tex["emissive"])
    # upload still knows two formats
    img = np.zeros((H0, W0, 4), f32)
    assert L.rc2dgi_upload(h, 0, img.ctypes.data_as(ctypes.c_void_p), 0, FMT_RGBA16F) == E_ARG
    assert L.rc2dgi_upload_device(h, 0, dp(), 0, FMT_RGBA16F) == E_ARG
    refused(E_ARG)
    # the Python binding hands the library's refusal on
    with pytest.raises(R.RC2DGIError) as ei:
        ctx.write("final_gi", np.zeros((ctx.cascade_resolution[1], ctx.cascade_resolution[0], 4), f32))
    assert ei.value.code == E_ARG
    refused(E_ARG)
    ctx.close()


# ------------------------------------------------------------------ 9: row-strip shards
def test_two_shards_written_alike_match_the_unsharded_frame(R, ref_lib):
    from radiancecascade2dglobalillumination_amd import scenes

    t = THIN[2]
    W, H, N, rr, rs, blur = t.W, t.H, t.N, t.rr, t.rs, t.blur
    assert (W, H, N, rs, blur) == (128, 64, 4, 1.0, 1.5)
    color, emis = scenes.random_scene(W, H, 3)
    rng = np.random.default_rng(17)
    rect = (20, H // 2 - 9, 50, 18)  # crosses the boundary between the two strips
    ce = np.zeros((18, 50, 4), f32)
    ce[..., :3] = (rng.random((18, 50, 3)) < 0.2) * rng.random((18, 50, 3)) * 2
    ce[..., 3] = 1
    cc = (rng.random((18, 50, 4)) < 0.5).astype(f32)
    color2 = ref_write(ref_lib, color, cc, rect, flip=True)
    emis2 = ref_write(ref_lib, emis, ce, rect)
    want = whole_frame(R, W, H, N, rr, rs, blur, color2, emis2)
    base = whole_frame(R, W, H, N, rr, rs, blur, color, emis)
    assert not np.array_equal(base["final_gi"], want["final_gi"]), "the written rectangle changes the frame"
    ctxs = []
    for k in range(2):
        c = R.RC2DGI(W, H, cascade_count=N, render_scale=rs, ray_range=rr)
        c.set_shader_value("_BlurRadius", blur)
        c.set_shard(k, 2)
        c.set_tuning("poison", 1)
        c.upload("color", color)
        c.upload("emissive", emis)
        ctxs.append(c)
    y0, y1 = ctxs[0].shard_rows()
    assert y0 < rect[1] + rect[3] and rect[1] < y1 < rect[1] + rect[3], "the rectangle lies on both strips"
    for k, c in enumerate(ctxs):  # one rank through the host variant, one through the device variant
        write_either(c, k == 1, "color", cc, rect, flip=True)
        write_either(c, k == 1, "emissive", ce, rect)
        assert_same(c.download("emissive"), emis2, f"rank {k}: the input is whole on every rank")
    R.do_group(ctxs)
    for c in ctxs:
        c.sync()
    for c in ctxs:
        assert_shard_matches_whole(c, want, W, H, blur, expect_strip_tables=False)
    for c in ctxs:
        c.close()
