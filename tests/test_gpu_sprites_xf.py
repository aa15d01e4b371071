"""GPU: rc2dgi_sprites_xf_device -- a device-resident list of scaled, rotated, sheared or mirrored sprites drawn from
one atlas image -- bit for bit (NaNs as one pattern) against the merged code (rc2dgi_sprites_device on the same context:
identity lists and mirrors), against numpy directly (whole upscales are np.repeat, quarter turns np.rot90) and against
the numpy restatement of the header (tests/sprites_xf_ref.py), POINT and LINEAR, every atlas format in every storage:
seeded arbitrary transforms, sprites over and off every edge, one over the whole target, one source pixel blown up, one
thinner than a pixel, 70 over one pixel in both orders, centres exactly on an edge, a pitched atlas, non-finite texels;
more than two batches and two forced plans; the device count and status words; garbage; the working memory shared with
the other two list calls; a device-only loop through a frame; the stream order behind a busy device; a shard; the
argument errors.  The consequences used in the first two groups are asserted of the restatement alone in
tests/test_sprites_xf_cpu.py.  Targets 64 x 48 and 200 x 150 (no multiple of a 64 x 4 tile, columns 63 / 64 / 128 and
the tile rows crossed) and a 37 x 29 atlas."""
import ctypes
import math
import time

import numpy as np
import pytest

import sprites_ref as S1
import sprites_xf_ref as S
from oracle import paint_ref
from test_gpu_sprites import (AH, AW, SENTINEL, WHITE, atlas_np, base_texture, differing, prim_words, prims, rand_tint,
                              texture, to_dev)

pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32
TARGETS = [(64, 48), (200, 150)]
FMTS = ["uint8", "float16", "float32"]
STORAGES = ["f32", "f16", "rgba8"]


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def R(torch):
    from radiancecascade2dglobalillumination_amd import rc2dgi

    return rc2dgi


# ------------------------------------------------------------------ calls and comparisons
def draw(torch, ctx, which, atlas_t, wd, clear=None, count=None):
    """sprites_xf_device of (n, 12) words; returns the status words"""
    t = torch.from_numpy(np.ascontiguousarray(wd, np.int32).reshape(-1, 12)).to("cuda")
    status = torch.full((2,), -77, dtype=torch.int32, device="cuda")
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device="cuda")
    ctx.sprites_xf_device(which, atlas_t, t, clear, cnt, status)
    ctx.sync()
    return status.cpu().numpy().tolist()


def draw1(torch, ctx, which, atlas_t, wd, clear=None):
    """sprites_device (the 1:1 call) of (n, 8) words"""
    t = torch.from_numpy(np.ascontiguousarray(wd, np.int32).reshape(-1, 8)).to("cuda")
    status = torch.full((2,), -77, dtype=torch.int32, device="cuda")
    ctx.sprites_device(which, atlas_t, t, clear, None, status)
    ctx.sync()
    return status.cpu().numpy().tolist()


def bits(x):
    """what is compared: the bytes of an 8-bit texture, the words of a float one with every NaN as one pattern"""
    if x.dtype == np.uint8:
        return x
    v = np.ascontiguousarray(x, f32).view(u32).copy()
    v[np.isnan(x)] = 0x7FC00000
    return v


def same(got, want):
    return np.array_equal(bits(got), bits(want))


def ident(sx, sy, w, h, x, y, tint=WHITE, flags=0):
    return (sx, sy, w, h, x, y, w, 0, 0, h, tint, flags)


def placed(sx, sy, w, h, cx, cy, deg, kx, ky, tint, flags, shear=0.0, mirror=False):
    """the record of a source rectangle scaled by (kx, ky), sheared, turned by `deg` (clockwise, y down) and, with
    `mirror`, reversed along its own u axis, its centre on (cx, cy)"""
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    ax, ay = c * w * kx, s * w * kx
    bx, by = -s * h * ky + shear * ax, c * h * ky + shear * ay
    if mirror:
        ax, ay = -ax, -ay
    return (sx, sy, w, h, cx - (ax + bx) / 2, cy - (ay + by) / 2, ax, ay, bx, by, tint, flags)


def general_list(W, H, seed, linear):
    """About 170 tinted sprites, blended and replacing, on a W x H target from the 37 x 29 atlas: seeded arbitrary A, B
    (odd angles, scales 3.7 and 0.3, shear, negative determinants), sprites over each edge and corner and wholly off
    each side (adjacent and far), two over the whole target, one source pixel blown up over it, two thinner than a
    pixel, 70 over one pixel, centres exactly on an edge (half-integer px), edges on columns 63 / 64 / 128 and on the
    tile rows; in a seeded order."""
    rng = np.random.default_rng(seed)
    lin = S.LINEAR if linear else 0
    P = []

    def src(w=None, h=None):
        w = int(rng.integers(1, 21)) if w is None else w
        h = int(rng.integers(1, 16)) if h is None else h
        return int(rng.integers(0, AW - w + 1)), int(rng.integers(0, AH - h + 1)), w, h

    def add(rect, cx, cy, deg, kx, ky, **kw):
        P.append(placed(*rect, cx, cy, deg, kx, ky, rand_tint(rng), lin | (S.REPLACE if len(P) % 3 == 0 else 0), **kw))

    angles = [7.0, 33.0, 61.5, 89.0, 123.0, 180.5, 211.0, 299.0, 347.3]
    for k in range(45):
        kx, ky = [(3.7, 3.7), (0.3, 0.3), (1.0, 1.0), (3.7, 0.3), (1.3, 2.1)][k % 5]
        add(src(), float(rng.uniform(0, W)), float(rng.uniform(0, H)), angles[k % 9] + k, kx, ky,
            shear=(0.0, 0.4, -0.7)[k % 3], mirror=k % 4 == 1)
    for cx, cy in ((-2, H / 2), (W + 1, H / 3), (W / 2, -3), (W / 3, H + 2), (0, 0), (W, H), (W, 0), (0, H)):  # over
        add(src(12, 9), cx, cy, 33.0, 1.5, 1.5)
        add(src(12, 9), cx, cy, -20.0, 0.8, 2.0, mirror=True)
    for cx, cy in ((-60, 5), (W + 60, 5), (5, -60), (5, H + 60), (-9, H / 2), (W + 9, H / 2), (W / 2, -9), (W / 2, H + 9),
                   (-1e5, 3), (3, 1e5)):  # off the target, far and adjacent (the adjacent ones' boxes still meet it)
        add(src(10, 10), cx, cy, 45.0, 1.0, 1.0)
    P.append((0, 0, AW, AH, -3.0, -2.0, W + 6.0, 0.0, 0.0, H + 5.0, rand_tint(rng), lin))      # the whole target
    add((0, 0, AW, AH), W / 2, H / 2, 30.0, 2.0 * W / AW, 2.0 * H / AH)                          # and turned
    P.append((5, 7, 1, 1, -1.0, -1.0, W + 4.0, 3.0, -2.0, H + 4.0, rand_tint(rng), lin))        # one source pixel
    add(src(20, 1), W / 2, H / 2, 18.0, 2.0, 0.4)                                                # thinner than a pixel
    P.append((3, 3, 2, 25, 17.4, 2.0, 0.3, 0.0, 0.0, H - 6.0, rand_tint(rng), lin | S.REPLACE))  # (and upright)
    px, py = min(W - 2, 37) + 0.5, min(H - 2, 5) + 0.5
    for k in range(70):  # more than 64 over one pixel: the walk crosses the mask's word boundaries
        add(src(1 + k % 3, 1 + k % 2), px + (k % 5 - 2) * 0.2, py + (k % 3 - 1) * 0.3, 13.0 * k, 1.0 + k % 4, 1.0 + k % 3)
    for x, w in ((10.5, 8.0), (20.5, -8.0), (31.5, 3.0)):  # a == 0 exactly on a column of centres, a == 1 on another
        P.append(src(4, 3) + (x, 3.0, w, 0.0, 0.0, 6.0, rand_tint(rng), lin | S.REPLACE))
        P.append(src(4, 3) + (3.0, x + 9, 0.0, w, -6.0, 0.0, rand_tint(rng), lin))
    for x in (63, 64, 128):
        if x < W:
            add(src(9, 5), x + 4.5, 9.5, 3.0, 1.0, 1.0)   # its first column about x
            add(src(9, 5), x - 4.5, 16.5, -3.0, 1.0, 1.0)  # its last column about x
    for y in (4, 8, H - 4, H - 8):
        add(src(11, 6), 30.0, y + 3.0, 2.0, 1.0, 1.0)
        add(src(11, 6), 41.0, y - 3.0, -2.0, 1.0, 1.0)
    order = rng.permutation(len(P))
    return [P[k] for k in order]


_refs = {}


def restated(key, make):
    """a restatement computed once and shared (F32 and F16 storage hold the same input texels); never written to"""
    if key not in _refs:
        _refs[key] = make()
        _refs[key].setflags(write=False)
    return _refs[key]


# ------------------------------------------------------------------ 1. against the merged code
def one_to_one_list(W, H, n, seed, flags):
    """n tinted 1:1 sprites, 1 x 1 up to 37 x 29, inside the target, over its edges and off it"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        w = int(rng.integers(1, AW + 1)) if k > 3 else (1, AW)[k % 2]
        h = int(rng.integers(1, AH + 1)) if k > 3 else (1, AH)[k // 2]
        out.append((int(rng.integers(0, AW - w + 1)), int(rng.integers(0, AH - h + 1)), w, h,
                    int(rng.integers(-w - 2, W + 3)), int(rng.integers(-h - 2, H + 3)), rand_tint(rng), flags))
    return out


@pytest.mark.parametrize("replace", [False, True], ids=["blend", "replace"])
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("fmt", FMTS)
def test_identity_lists_equal_sprites_device(R, torch, fmt, storage, replace):
    """A = (w, 0), B = (0, h), integer P, POINT: the bits rc2dgi_sprites_device leaves, on the same context"""
    W, H = (200, 150) if replace else (64, 48)
    a = atlas_np(fmt)
    at = to_dev(torch, a, 6 if replace else 0)
    P = one_to_one_list(W, H, 200, 11, S.REPLACE if replace else 0)
    u8 = storage == "rgba8"
    ctx = R.RC2DGI(W, H, cascade_count=2, storage=storage)
    ctx.upload("emissive", base_texture(W, H))
    start = texture(ctx, "emissive", u8)
    assert draw1(torch, ctx, "emissive", at, S1.words(P)) == [200, 0]
    want = texture(ctx, "emissive", u8)
    ctx.upload("emissive", base_texture(W, H))
    assert draw(torch, ctx, "emissive", at, S.words([ident(*p) for p in P])) == [200, 0]
    got = texture(ctx, "emissive", u8)
    assert same(got, want), differing(got, want)
    assert not np.array_equal(want, start), "the sprites changed the texture"
    ctx.close()


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("fmt", FMTS)
def test_mirrors_equal_the_flip_sprites(R, torch, fmt, storage):
    W, H = 200, 150
    a = atlas_np(fmt)
    at = to_dev(torch, a)
    u8 = storage == "rgba8"
    P1, PX = [], []
    for k, (sx, sy, w, h, x, y, tint, flags) in enumerate(one_to_one_list(W, H, 120, 12, 0)):
        flags = S.REPLACE if k % 3 == 0 else 0
        if k % 2:
            P1.append((sx, sy, w, h, x, y, tint, flags | S1.FLIP_X))
            PX.append((sx, sy, w, h, x + w, y, -w, 0, 0, h, tint, flags))
        else:
            P1.append((sx, sy, w, h, x, y, tint, flags | S1.FLIP_X | S1.FLIP_Y))
            PX.append((sx, sy, w, h, x + w, y + h, -w, 0, 0, -h, tint, flags))
    ctx = R.RC2DGI(W, H, cascade_count=2, storage=storage)
    ctx.upload("color", base_texture(W, H))
    assert draw1(torch, ctx, "color", at, S1.words(P1)) == [120, 0]
    want = texture(ctx, "color", u8)
    ctx.upload("color", base_texture(W, H))
    assert draw(torch, ctx, "color", at, S.words(PX)) == [120, 0]
    got = texture(ctx, "color", u8)
    assert same(got, want), differing(got, want)
    ctx.close()


# ------------------------------------------------------------------ 2. against numpy directly
@pytest.mark.parametrize("W,H", TARGETS)
def test_whole_upscales_equal_np_repeat(R, torch, W, H):
    a = atlas_np("float32")
    at = to_dev(torch, a)
    rng = np.random.default_rng(15)
    want = np.zeros((H, W, 4), f32)  # screen rows (y down); the texture is its vertical mirror
    P = []
    for k in range(1, 8):
        for m in range(1, 8):
            w, h = int(rng.integers(1, 7)), int(rng.integers(1, 6))
            sx, sy = int(rng.integers(0, AW - w + 1)), int(rng.integers(0, AH - h + 1))
            x, y = int(rng.integers(0, W - k * w + 1)), int(rng.integers(0, H - m * h + 1))
            P.append((sx, sy, w, h, x, y, k * w, 0, 0, m * h, WHITE, S.REPLACE))
            want[y:y + m * h, x:x + k * w] = np.repeat(np.repeat(a[sy:sy + h, sx:sx + w], m, axis=0), k, axis=1)
    ctx = R.RC2DGI(W, H, cascade_count=2)
    assert draw(torch, ctx, "emissive", at, S.words(P), (0, 0, 0, 0)) == [49, 0]
    got = ctx.download("emissive")
    assert np.array_equal(got.view(u32), want[::-1].view(u32)), differing(got, want[::-1])
    ctx.close()


@pytest.mark.parametrize("W,H", TARGETS)
def test_quarter_turns_equal_np_rot90(R, torch, W, H):
    a = atlas_np("float32")
    at = to_dev(torch, a)
    rng = np.random.default_rng(16)
    want = np.zeros((H, W, 4), f32)
    P = []
    for k in range(60):
        w, h = (int(rng.integers(1, AW + 1)), int(rng.integers(1, AH + 1))) if k > 3 else ((1, AW)[k % 2], (1, AH)[k // 2])
        sx, sy = int(rng.integers(0, AW - w + 1)), int(rng.integers(0, AH - h + 1))
        sub = a[sy:sy + h, sx:sx + w]
        turns = k % 4  # quarter turns clockwise of the sub-image, placed with its top-left pixel at (x, y)
        tw, th = (h, w) if turns % 2 else (w, h)
        x, y = int(rng.integers(0, W - tw + 1)), int(rng.integers(0, H - th + 1))
        p, A, B = [((x, y), (w, 0), (0, h)), ((x + h, y), (0, w), (-h, 0)), ((x + w, y + h), (-w, 0), (0, -h)),
                   ((x, y + w), (0, -w), (h, 0))][turns]
        P.append((sx, sy, w, h) + p + A + B + (WHITE, S.REPLACE))
        want[y:y + th, x:x + tw] = np.rot90(sub, -turns)
    ctx = R.RC2DGI(W, H, cascade_count=2)
    assert draw(torch, ctx, "color", at, S.words(P), (0, 0, 0, 0)) == [60, 0]
    got = ctx.download("color")
    assert np.array_equal(got.view(u32), want[::-1].view(u32)), differing(got, want[::-1])
    ctx.close()


# ------------------------------------------------------------------ 3. against the restatement
CLEAR = (9, 8, 7, 200)


@pytest.mark.parametrize("clear", [None, CLEAR], ids=["noclear", "clear"])
@pytest.mark.parametrize("linear", [False, True], ids=["point", "linear"])
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("W,H", TARGETS)
def test_general_lists_in_both_orders(R, torch, W, H, fmt, storage, linear, clear):
    a = atlas_np(fmt)
    at = to_dev(torch, a, 6)  # (a pitched view)
    P = general_list(W, H, 21, linear)
    u8 = storage == "rgba8"
    ctx = R.RC2DGI(W, H, cascade_count=2, storage=storage)
    outs = []
    for reverse in (False, True):
        ctx.upload("color", base_texture(W, H))
        start = texture(ctx, "color", u8)
        wd = S.words(P[::-1] if reverse else P)
        assert draw(torch, ctx, "color", at, wd, clear) == [len(P), 0]
        got = texture(ctx, "color", u8)
        want = restated((W, H, fmt, u8, linear, clear, reverse), lambda: S.draw(start, a, wd, u8, clear))
        assert same(got, want), f"{W}x{H} {storage} {fmt} reversed={reverse}: {differing(got, want)}"
        outs.append(got)
    assert not np.array_equal(outs[0], outs[1]), "the two orders give different textures: the order is kept"
    ctx.close()


@pytest.mark.parametrize("linear", [False, True], ids=["point", "linear"])
@pytest.mark.parametrize("storage", ["f32", "rgba8"])
def test_non_finite_texels_propagate_by_ieee_rules(R, torch, storage, linear):
    W, H = 64, 48
    a = atlas_np("float32")
    nan, inf = f32(np.nan), f32(np.inf)
    a[2, 3] = [nan, 0.5, 0.5, 0.5]
    a[2, 4] = [0.5, 0.5, 0.5, nan]
    a[3, 3] = [inf, -inf, 0.25, 0.5]
    a[3, 4] = [0.25, 0.5, 0.75, inf]
    a[4, 3] = [0.25, 0.5, 0.75, -inf]
    a[4, 4] = [inf, inf, inf, 0.0]
    a[5, 3] = [-inf, nan, inf, 1.0]
    at = to_dev(torch, a)
    lin = S.LINEAR if linear else 0
    P = []
    for k, (tint, flags) in enumerate([(WHITE, 0), (WHITE, 4), ((0, 128, 255, 255), 0), ((255, 255, 255, 0), 0),
                                       ((0, 0, 0, 0), 4), ((128, 0, 255, 128), 0)]):
        P.append(placed(1, 1, 8, 8, 8.0 + 9 * k, 12.0, 20.0 * k, 1.2, 1.2, tint, flags | lin))    # apart
        P.append(placed(2, 2, 4, 4, 20.0 + 2 * k, 34.0 + k, 31.0 * k, 2.5, 2.5, tint, flags | lin))  # over each other
    wd = S.words(P)
    u8 = storage == "rgba8"
    ctx = R.RC2DGI(W, H, cascade_count=2, storage=storage)
    ctx.upload("emissive", base_texture(W, H))
    start = texture(ctx, "emissive", u8)
    assert draw(torch, ctx, "emissive", at, wd) == [len(P), 0]
    got, want = texture(ctx, "emissive", u8), S.draw(start, a, wd, u8)
    if not u8:
        assert np.isnan(want).any() and np.isinf(want).any()
    assert same(got, want), f"{np.count_nonzero(bits(got) != bits(want))} words differ"
    ctx.close()


# ------------------------------------------------------------------ 4. batches and plans
def small_list(n, W, H, seed):
    """n small sprites (a few pixels each, POINT and LINEAR, blended and replacing) as words, seeded; their centres lie
    above screen row 10 or below row 40 and none reaches further than 9 pixels, so rows 20 .. 30 stay untouched"""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0, 2 * np.pi, n)
    k = rng.uniform(0.5, 3.0, n)
    wd = np.zeros((n, 12), np.int32)
    wd[:, 2:4] = rng.integers(1, 4, (n, 2))
    wd[:, 0] = rng.integers(0, AW - 3, n)
    wd[:, 1] = rng.integers(0, AH - 3, n)
    cx = rng.uniform(-3, W + 3, n)
    cy = np.where(rng.integers(0, 2, n) == 0, rng.uniform(-3, 10, n), rng.uniform(40, H + 3, n))
    fl = np.zeros((n, 6), np.float64)
    fl[:, 2], fl[:, 3] = np.cos(ang) * k * wd[:, 2], np.sin(ang) * k * wd[:, 2]
    fl[:, 4], fl[:, 5] = -np.sin(ang) * k * wd[:, 3], np.cos(ang) * k * wd[:, 3]
    fl[:, 0], fl[:, 1] = cx - (fl[:, 2] + fl[:, 4]) / 2, cy - (fl[:, 3] + fl[:, 5]) / 2
    wd[:, 4:10] = fl.astype(f32).view(np.int32)
    wd[:, 10] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(u32).view(np.int32)
    wd[:, 11] = rng.integers(0, 4, n) * 4
    return wd


def test_more_than_two_batches_keep_the_order_and_leave_the_masks_clean(R, torch):
    """paint_plan tile 8, batch 2048 on 64 x 48: 2 * 2048 + 70 sprites are three batches"""
    W, H = 64, 48
    a = atlas_np("uint8")
    at = to_dev(torch, a)
    ctx = R.RC2DGI(W, H, cascade_count=2)
    ctx.set_tuning("paint_plan", 3 | 1 << 8)
    batch = ctx.get_tuning("paint_batch")
    assert (ctx.get_tuning("paint_tile_h"), batch) == (8, 2048)
    n = 2 * batch + 70
    wd = small_list(n, W, H, 8)
    for b in (batch, 2 * batch):  # half-transparent sprites straddling each batch boundary, over the same pixels
        for k in range(b - 3, b + 3):
            wd[k] = S.words([(3, 3, 3, 3, 20.0 + (k - b), 24.0, 3, 0, 0, 3, (200, 90, 40, 128), 0)])[0]
    assert S.accepted(wd, AW, AH).all()
    ctx.upload("color", base_texture(W, H))
    start = ctx.download("color")
    assert draw(torch, ctx, "color", at, wd, (5, 5, 5, 255)) == [n, 0]
    got, want = ctx.download("color"), S.draw(start, a, wd, False, (5, 5, 5, 255))
    assert same(got, want), differing(got, want)
    # (the sprites at a batch boundary matter to the result: nothing else touches their rows, and without the first of
    # the next batch those rows differ)
    near = wd[batch - 3:batch + 3]
    assert not np.array_equal(S.draw(start, a, near, False), S.draw(start, a, np.delete(near, 3, axis=0), False))
    only = S.draw(start, a, np.concatenate([near, wd[2 * batch - 3:2 * batch + 3]]), False, (5, 5, 5, 255))
    rows = slice(H - 1 - 26, H - 23)  # screen rows 24 .. 26 in GL order
    assert np.array_equal(want[rows], only[rows]) and (only[rows] != f32(5) / f32(255)).any()
    # a following call finds the masks clean: a short list draws itself alone
    short = wd[5:25]
    assert draw(torch, ctx, "color", at, short) == [20, 0]
    got2, want2 = ctx.download("color"), S.draw(want, a, short, False)
    assert same(got2, want2), differing(got2, want2)
    ctx.close()


@pytest.mark.parametrize("linear", [False, True], ids=["point", "linear"])
def test_a_plan_of_tall_tiles_and_a_batch_of_4096(R, torch, linear):
    W, H = 200, 150
    a = atlas_np("uint8")
    at = to_dev(torch, a, 6)
    ctx = R.RC2DGI(W, H, cascade_count=2)
    ctx.set_tuning("paint_plan", 7 | 2 << 8)
    assert (ctx.get_tuning("paint_tile_h"), ctx.get_tuning("paint_batch")) == (128, 4096)
    wd = S.words(general_list(W, H, 21, linear))
    ctx.upload("color", base_texture(W, H))
    start = ctx.download("color")
    assert draw(torch, ctx, "color", at, wd) == [len(wd), 0]
    got = ctx.download("color")
    want = restated((W, H, "uint8", False, linear, None, False), lambda: S.draw(start, a, wd, False))
    assert same(got, want), differing(got, want)
    ctx.close()


# ------------------------------------------------------------------ 5. the device count and the status words
def nine(W, H, seed=3, flags=None):
    rng = np.random.default_rng(seed)
    P = []
    for k in range(9):
        w, h = int(rng.integers(4, 31)), int(rng.integers(4, 21))
        P.append(placed(int(rng.integers(0, AW - w + 1)), int(rng.integers(0, AH - h + 1)), w, h,
                        float(rng.uniform(0, W)), float(rng.uniform(0, H)), float(rng.uniform(0, 360)),
                        float(rng.uniform(0.4, 2.5)), float(rng.uniform(0.4, 2.5)), rand_tint(rng),
                        (k % 4) * 4 if flags is None else flags, mirror=k % 2 == 1))
    return P


@pytest.mark.parametrize("storage", ["f32", "rgba8"])
def test_count_and_status_words(R, torch, storage):
    W, H, n = 64, 48, 9
    a = atlas_np("float16")
    at = to_dev(torch, a)
    wd = S.words(nine(W, H))
    u8 = storage == "rgba8"
    clear = (20, 30, 40, 255)
    ctx = R.RC2DGI(W, H, cascade_count=2, storage=storage)
    ctx.upload("color", base_texture(W, H))
    start = texture(ctx, "color", u8)
    for count, m in [(-5, 0), (0, 0), (n - 1, n - 1), (n, n), (n + 9, n), (None, n)]:
        assert draw(torch, ctx, "color", at, wd, clear, count) == [m, 0], count
        got, want = texture(ctx, "color", u8), S.draw(start, a, wd, u8, clear, m)  # (m == 0: a clear only)
        assert same(got, want), f"count {count}: {differing(got, want)}"
    ctx.upload("color", base_texture(W, H))
    for count, m in [(-(1 << 31), 0), (0, 0), (4, 4), ((1 << 31) - 1, n)]:  # without a clear: m == 0 leaves the texture
        before = texture(ctx, "color", u8)
        assert draw(torch, ctx, "color", at, wd, None, count) == [m, 0], count
        got, want = texture(ctx, "color", u8), S.draw(before, a, wd, u8, None, m)
        assert same(got, want), f"count {count}: {differing(got, want)}"
        if m == 0:
            assert same(got, before)
    # a count torch writes on the stream right before the call, and overwrites right after it has returned
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        t = torch.from_numpy(wd).to("cuda")
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        status = torch.full((2,), -77, dtype=torch.int32, device="cuda")
        cnt.fill_(4)
        ctx.sprites_xf_device("color", at, t, clear, cnt, status)
        cnt.fill_(-1)
        t.fill_(0x7FC00000)
    ctx.sync()
    assert status.cpu().numpy().tolist() == [4, 0]
    got, want = texture(ctx, "color", u8), S.draw(start, a, wd, u8, clear, 4)
    assert same(got, want), differing(got, want)
    ctx.set_stream(None)
    ctx.close()


def test_nothing_to_draw_without_a_clear_leaves_the_texture(R, torch):
    W, H = 64, 48
    at = to_dev(torch, atlas_np("uint8"))
    ctx = R.RC2DGI(W, H, cascade_count=2)
    start = np.broadcast_to(SENTINEL, (H, W, 4)).copy()
    ctx.upload("emissive", start)
    none = np.zeros((0, 12), np.int32)
    assert draw(torch, ctx, "emissive", at, none) == [0, 0]  # n == 0, a null list
    assert np.array_equal(ctx.download("emissive").view(u32), start.view(u32))
    off = S.words([placed(0, 0, 5, 5, -40.0, 10.0, 30.0, 1.0, 1.0, WHITE, 0), ident(0, 0, 5, 5, 70, 50)])
    assert draw(torch, ctx, "emissive", at, off) == [2, 0]  # an empty box draws nothing and is not refused
    assert np.array_equal(ctx.download("emissive").view(u32), start.view(u32))
    assert draw(torch, ctx, "emissive", at, none, (1, 2, 3, 4)) == [0, 0]  # n == 0: the clear
    assert np.array_equal(ctx.download("emissive"), np.broadcast_to(f32([1, 2, 3, 4]) / f32(255), (H, W, 4)))
    ctx.close()


# ------------------------------------------------------------------ 6. refused sprites and garbage
@pytest.mark.parametrize("storage", ["f32", "rgba8"])
def test_each_refusal_term_draws_nothing_and_is_counted(R, torch, storage):
    W, H = 64, 48
    a = atlas_np("uint8")
    at = to_dev(torch, a)
    good = nine(W, H)
    t, big, lim, e = (250, 10, 10, 255), 2**31 - 1, 2.0 ** 20, 2.0 ** -10
    up = float(np.nextafter(f32(lim), f32(np.inf)))
    bad = [ident(0, 0, 20, 20, 1, 1, t, 1),                     # RC2DGI_SPRITE_FLIP_X is not accepted in this record
           ident(0, 0, 20, 20, 1, 1, t, 2 | 8),                 # nor FLIP_Y
           ident(0, 0, 20, 20, 1, 1, t, 16),                    # a flag bit that is not defined
           ident(0, 0, 20, 20, 1, 1, t, -(1 << 31)),
           (0, 0, 0, 20, 1, 1, 20, 0, 0, 20, t, 0),             # w < 1
           (0, 0, 20, -3, 1, 1, 20, 0, 0, 20, t, 0),            # h < 1
           ident(-1, 0, 20, 20, 1, 1, t),                       # sx < 0
           ident(0, -(1 << 31), 20, 20, 1, 1, t),               # sy < 0
           ident(AW - 19, 0, 20, 20, 1, 1, t),                  # w > AW - sx by one
           ident(big, 0, 1, 1, 1, 1, t),                        # w > AW - sx, sx near INT_MAX
           ident(0, AH - 19, 20, 20, 1, 1, t),                  # h > AH - sy by one
           (0, big - 3, 20, big, 1, 1, 20, 0, 0, 20, t, 0),
           (0, 0, 20, 20, up, 1, 20, 0, 0, 20, t, 0),           # px the next float above 2^20
           (0, 0, 20, 20, 1, -up, 20, 0, 0, 20, t, 0),          # py
           (0, 0, 20, 20, 1, 1, np.nan, 0, 0, 20, t, 0),        # ax a NaN
           (0, 0, 20, 20, 1, 1, 20, np.inf, 0, 20, t, 0),       # ay an infinity
           (0, 0, 20, 20, 1, 1, 20, 0, -up, 20, t, 0),          # bx
           (0, 0, 20, 20, 1, 1, 20, 0, 0, -np.inf, t, 4),       # by
           (0, 0, 20, 20, 1, 1, 20, 10, 40, 20, t, 0),          # det = 0: A and B parallel
           (0, 0, 20, 20, 1, 1, e, 0, 0, float(np.nextafter(f32(e), f32(0))), t, 0),  # |det| just below 2^-20
           (0, 0, 20, 20, 1, 1, 0, 0, 0, 0, t, 8)]
    P = []
    for k, p in enumerate(bad):  # a refused form beside every valid sprite, and at both ends
        P.append(p)
        if k < len(good):
            P.append(good[k])
    # the limits themselves are accepted: components of exactly 2^20 (off the target: nothing drawn, nothing refused),
    # and a determinant of exactly 2^-20 (a sprite 2^-10 of a pixel wide and high, which covers no centre)
    edge = [(AW - 20, AH - 20, 20, 20, lim, -lim, 20, 0, 0, 20, t, 12), (0, 0, AW, AH, -lim, lim, lim, 0, 0, -lim, t, 0),
            (0, 0, 20, 20, 1.25, 1.25, e, 0, 0, e, t, 0)]
    P += edge
    wd = S.words(P)
    ok = S.accepted(wd, AW, AH)
    assert np.count_nonzero(~ok) == len(bad) and ok[-3:].all(), "the restated rule refuses exactly the forms above"
    u8 = storage == "rgba8"
    ctx = R.RC2DGI(W, H, cascade_count=2, storage=storage)
    assert draw(torch, ctx, "color", at, wd, (1, 2, 3, 255)) == [len(P), len(bad)]
    got = texture(ctx, "color", u8)
    # the restatement of the accepted ones alone: a refused sprite draws nothing and leaves the others as they are
    want = S.draw(np.zeros((H, W, 4), np.uint8 if u8 else f32), a, wd[ok], u8, (1, 2, 3, 255))
    assert same(got, want), differing(got, want)
    ctx.close()


def garbage(kinds):
    """4096 records of seeded random 32-bit words.  `raw`: as they come (the flags alone refuse all but one in 2^30).
    `narrowed`: the same words with the flags cut to 4 bits, the source fields to [-4, 28), and the six floats made of
    small integers -- P in [-32, 96) in halves, the components of A and B in [-8, 8) in quarters, so that a determinant
    of zero occurs -- but every eleventh record keeps one of its raw float words, which is out of bounds, an infinity
    or a NaN as often as not."""
    n = 4096
    rng = np.random.default_rng(2025)
    wd = rng.integers(0, 1 << 32, (n, 12), dtype=np.uint64).astype(u32).view(np.int32)
    if kinds == "narrowed":
        wd[:, 11] &= 15
        wd[:, 0:4] = (wd[:, 0:4] & 31) - 4
        fl = np.empty((n, 6), f32)
        fl[:, 0:2] = ((wd[:, 4:6] & 255) - 64).astype(f32) * f32(0.5)
        fl[:, 2:6] = ((wd[:, 6:10] & 63) - 32).astype(f32) * f32(0.25)
        raw = wd[:, 4:10].copy()
        new = fl.view(np.int32).copy()
        rows = np.arange(0, n, 11)
        new[rows, rows % 6] = raw[rows, rows % 6]
        wd[:, 4:10] = new
    return wd


ACCEPTED_OF_THE_NARROWED = 263  # of 4096, by the restatement's rule (asserted below, on the CPU)


@pytest.mark.parametrize("kinds", ["raw", "narrowed"])
def test_a_buffer_of_garbage_draws_what_the_rule_accepts(R, torch, kinds):
    W, H, n = 64, 48, 4096
    wd = garbage(kinds)
    a = atlas_np("float32")
    at = to_dev(torch, a)
    ok = S.accepted(wd, AW, AH)
    if kinds == "narrowed":
        terms = np.array(S.refusal_terms(wd, AW, AH))
        alone = [np.count_nonzero(terms[k] & ~np.delete(terms, k, axis=0).any(axis=0)) for k in range(4)]
        assert min(alone) > 0, f"every term of the rule decides alone on some record: {alone}"
        assert np.count_nonzero(ok) == ACCEPTED_OF_THE_NARROWED
    else:
        assert np.count_nonzero(ok) == 0
    ctx = R.RC2DGI(W, H, cascade_count=2)
    status = draw(torch, ctx, "emissive", at, wd, (0, 0, 0, 0))
    assert status == [n, n - np.count_nonzero(ok)], (status, np.count_nonzero(ok))
    want = S.draw(np.zeros((H, W, 4), f32), a, wd[ok], False, (0, 0, 0, 0))
    got = ctx.download("emissive")
    assert same(got, want), differing(got, want)
    if kinds == "narrowed":
        assert want.any()
    # and with a garbage count of its own
    assert draw(torch, ctx, "emissive", at, wd, (0, 0, 0, 0), count=-(1 << 31)) == [0, 0]
    assert not ctx.download("emissive").any()
    assert draw(torch, ctx, "emissive", at, wd, (0, 0, 0, 0), count=(1 << 31) - 1) == status
    assert same(ctx.download("emissive"), want)
    ctx.close()


# ------------------------------------------------------------------ 7. interplay
@pytest.mark.parametrize("storage", ["f32", "rgba8"])
def test_the_three_list_calls_share_the_working_memory(R, torch, storage):
    """paint, sprites, sprites_xf, paint, sprites_xf on one context, enqueued without a wait between them, equal the
    restatements composed in that order; then with sprites_xf first on a fresh context (it may be the call that
    allocates)."""
    W, H = 200, 150
    u8 = storage == "rgba8"
    a = atlas_np("uint8")
    at = to_dev(torch, a)
    P1, P2 = prims(W, H, 31), prims(W, H, 32)
    SP = [(int(k), int(k) % 9, 12, 9, 15 * k - 8, 11 * k, rand_tint(np.random.default_rng(k)), k % 8) for k in range(14)]
    X1, X2 = nine(W, H, 33) + nine(W, H, 34, 8), nine(W, H, 35)
    w1, w2 = (torch.from_numpy(prim_words(R, P)).to("cuda") for P in (P1, P2))
    ws = torch.from_numpy(S1.words(SP)).to("cuda")
    x1, x2 = (torch.from_numpy(S.words(X)).to("cuda") for X in (X1, X2))
    st = torch.full((5, 2), -77, dtype=torch.int32, device="cuda")
    ctx = R.RC2DGI(W, H, cascade_count=2, storage=storage)
    ctx.paint_device("color", w1, (10, 20, 30, 255), None, st[0])
    ctx.sprites_device("color", at, ws, None, None, st[1])
    ctx.sprites_xf_device("color", at, x1, None, None, st[2])
    ctx.paint_device("color", w2, None, None, st[3])
    ctx.sprites_xf_device("color", at, x2, None, None, st[4])
    ctx.sync()
    assert st.cpu().numpy().tolist() == [[9, 0], [14, 0], [18, 0], [9, 0], [9, 0]]
    want = paint_ref.paint(W, H, P1, (10, 20, 30, 255), rgba8=u8)
    want = S.draw(S1.draw(want, a, S1.words(SP), u8), a, S.words(X1), u8)
    want = S.draw(paint_ref.paint(W, H, P2, None, base=want, rgba8=u8), a, S.words(X2), u8)
    got = texture(ctx, "color", u8)
    assert same(got, want), differing(got, want)
    ctx.close()
    ctx = R.RC2DGI(W, H, cascade_count=2, storage=storage)
    ctx.sprites_xf_device("emissive", at, x1, (0, 0, 0, 255), None, st[0])
    ctx.paint_device("emissive", w1, None, None, st[1])
    ctx.sprites_xf_device("emissive", at, x2, None, None, st[2])
    ctx.sync()
    assert st[:3].cpu().numpy().tolist() == [[18, 0], [9, 0], [9, 0]]
    want = S.draw(np.zeros((H, W, 4), np.uint8 if u8 else f32), a, S.words(X1), u8, (0, 0, 0, 255))
    want = S.draw(paint_ref.paint(W, H, P1, None, base=want, rgba8=u8), a, S.words(X2), u8)
    got = texture(ctx, "emissive", u8)
    assert same(got, want), differing(got, want)
    ctx.close()


@pytest.mark.parametrize("storage", ["f32", "rgba8"])
def test_device_loop_equals_a_frame_of_the_restated_inputs(R, torch, storage):
    """torch makes the sprites on the device, sprites_xf_from_pro and pack_sprites_xf make the records, both inputs
    are drawn and a frame runs and is read, with no host synchronise between the steps; the merged COLOR equals that of
    a context given the restated inputs (the records are read back only after the run)."""
    W = H = 128
    u8 = storage == "rgba8"
    a = atlas_np("uint8")
    a[..., 3] = np.where(a[..., 3] > 100, 255, 0)  # walls and lights are opaque or absent
    stream = torch.cuda.Stream()
    ctx = R.RC2DGI(W, H, cascade_count=3, ray_range=2.0, storage=storage)
    ctx.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        at = to_dev(torch, a)
        g = torch.Generator(device="cuda")
        g.manual_seed(99)
        n = 24
        wh = torch.randint(3, 13, (n, 2), generator=g, device="cuda", dtype=torch.int32)
        sxy = torch.randint(0, AH - 12, (n, 2), generator=g, device="cuda", dtype=torch.int32)
        dest = torch.cat([torch.rand((n, 2), generator=g, device="cuda") * W,
                          wh.to(torch.float32) * (0.5 + 2.5 * torch.rand((n, 2), generator=g, device="cuda"))], 1)
        rot = torch.rand(n, generator=g, device="cuda") * 360.0
        p, av, bv = R.sprites_xf_from_pro(dest, dest[:, 2:4] * 0.5, rot)
        flags = torch.randint(0, 2, (n,), generator=g, device="cuda") * R.SPRITE_LINEAR
        walls = R.pack_sprites_xf(torch.cat([sxy, wh], 1), p, av, bv, None, flags)
        tint = torch.randint(0, 256, (n, 4), generator=g, device="cuda").to(torch.uint8)
        tint[::2] = 0  # every other sprite is a wall that emits nothing
        tint[:, 3] = 255
        lights = R.pack_sprites_xf(torch.cat([sxy, wh], 1), p, av, bv, tint, flags)
        status = torch.zeros((2, 2), dtype=torch.int32, device="cuda")
        ctx.sprites_xf_device("color", at, walls, (0, 0, 0, 0), None, status[0])
        ctx.sprites_xf_device("emissive", at, lights, (0, 0, 0, 255), None, status[1])
        ctx.do_rc2dgi()
        out = torch.empty((H, W, 4), device="cuda")
        ctx.read_into(out, "color")
    ctx.sync()
    got = out.cpu().numpy()
    assert status.cpu().numpy().tolist() == [[n, 0], [n, 0]]
    ww, lw = walls.cpu().numpy(), lights.cpu().numpy()
    ctx.set_stream(None)
    ctx.close()
    zero = np.zeros((H, W, 4), np.uint8 if u8 else f32)
    color, emissive = S.draw(zero, a, ww, u8, (0, 0, 0, 0)), S.draw(zero, a, lw, u8, (0, 0, 0, 255))
    assert color.any() and emissive[..., :3].any()
    b = R.RC2DGI(W, H, cascade_count=3, ray_range=2.0, storage=storage)
    b.frame(color, emissive)
    b.sync()
    want = b.download("color")
    b.close()
    assert np.array_equal(got.view(u32), want.view(u32)), differing(got, want)


def test_a_row_strip_shard_accepts_the_call(R, torch):
    W, H = 96, 64
    a = atlas_np("float32")
    at = to_dev(torch, a)
    wd = S.words(nine(W, H))
    ctx = R.RC2DGI(W, H, cascade_count=3)
    ctx.set_shard(0, 2)
    for which in ("color", "emissive"):
        assert draw(torch, ctx, which, at, wd, (4, 3, 2, 255)) == [9, 0]
        got, want = ctx.download(which), S.draw(np.zeros((H, W, 4), f32), a, wd, False, (4, 3, 2, 255))
        assert same(got, want), f"{which}: {differing(got, want)}"
    ctx.close()


# ------------------------------------------------------------------ 8. no wait
def test_two_calls_and_a_frame_enqueue_behind_a_busy_device(R, torch):
    """The method of test_gpu_sprites.py: on a torch stream given to rc2dgi_set_stream, behind a torch.cuda._sleep
    sized to three times what the synchronising twin's calls took on the host: sprites_xf into COLOR, sprites_xf into
    EMISSIVE (torch overwrites each list in place as soon as its call has returned), a frame, a read.  The event behind
    the sleep is unfinished after every call; the frame is the twin's.  One batch a call."""
    from test_gpu_pipeline import sleep_cycles_per_ms

    W = H = 256
    a = atlas_np("uint8")
    cc, ec = (0, 0, 0, 0), (0, 0, 0, 255)
    rng = np.random.default_rng(77)
    cw = S.words([placed(int(rng.integers(0, AW - 12)), int(rng.integers(0, AH - 12)), 12, 12, float(rng.uniform(0, W)),
                         float(rng.uniform(0, H)), float(rng.uniform(0, 360)), 1.5, 1.5, rand_tint(rng), (k % 4) * 4)
                  for k in range(400)])
    ew = cw.copy()
    ew[::2, 10] = np.int32(-(1 << 24))  # every other light is black and opaque
    assert len(cw) <= R.paint_device_limits(W, H)[0]

    def run(ctx, lib, at, lists):
        out = torch.full((H, W, 4), -7.0, device="cuda")
        gi = torch.full(tuple(reversed(ctx.cascade_resolution)) + (4,), -7.0, device="cuda")
        st = torch.full((2, 2), -77, dtype=torch.int32, device="cuda")
        lib("sprites_xf_device color", lambda: ctx.sprites_xf_device("color", at, lists[0], cc, None, st[0]))
        lists[0].fill_(0x7FC00000)
        lib("sprites_xf_device emissive", lambda: ctx.sprites_xf_device("emissive", at, lists[1], ec, None, st[1]))
        lists[1].fill_(-1)
        lib("do", ctx.do_rc2dgi)
        lib("read_into color", lambda: ctx.read_into(out, "color"))
        lib("read_into final_gi", lambda: ctx.read_into(gi, "final_gi"))
        return out, gi, st

    def fresh(stream):
        ctx = R.RC2DGI(W, H, cascade_count=4)
        ctx.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            at = to_dev(torch, a)
            warm = torch.from_numpy(cw).to("cuda")
            ctx.sprites_xf_device("color", at, warm)  # the first call allocates the working memory: the one wait
            ctx.do_rc2dgi()                           # (the tables)
        ctx.sync()
        return ctx, at

    stream = torch.cuda.Stream()
    twin, at = fresh(stream)
    with torch.cuda.stream(stream):
        lists = [torch.from_numpy(cw).to("cuda"), torch.from_numpy(ew).to("cuda")]
        stream.synchronize()

        def stepwise(name, fn):
            fn()
            twin.sync()

        t0 = time.perf_counter()
        want = run(twin, stepwise, at, lists)
        twin.sync()
        twin_seconds = time.perf_counter() - t0
        want = [t.cpu().numpy() for t in want]
    twin.set_stream(None)
    twin.close()

    ctx, at = fresh(stream)
    rate = sleep_cycles_per_ms(torch, stream)
    sleep_ms = 3.0 * twin_seconds * 1e3
    assert sleep_ms < 5000.0, f"the stepwise twin took {twin_seconds:.3f} s on the host"
    queried = []
    with torch.cuda.stream(stream):
        lists = [torch.from_numpy(cw).to("cuda"), torch.from_numpy(ew).to("cuda")]
        stream.synchronize()
        plug = torch.cuda.Event()
        torch.cuda._sleep(int(sleep_ms * rate))
        plug.record()

        def lib(name, fn):
            fn()
            queried.append((name, plug.query()))

        got = run(ctx, lib, at, lists)
        still_busy = not plug.query()
    ctx.sync()
    got = [t.cpu().numpy() for t in got]
    ctx.set_stream(None)
    ctx.close()
    print(f"\nstepwise twin {twin_seconds * 1e3:.2f} ms on the host, sleep {sleep_ms:.2f} ms")
    waited = [name for name, done in queried if done]
    assert not waited, f"the plug had run out after {waited[0]}"
    assert still_busy, "the device was idle before the last call returned"
    assert got[2].tolist() == [[len(cw), 0], [len(ew), 0]] and want[2].tolist() == got[2].tolist()
    for k, name in enumerate(("color", "final_gi")):
        assert np.array_equal(got[k].view(u32), want[k].view(u32)), f"{name} differs from the synchronising twin's"
    assert not np.array_equal(got[0], np.full_like(got[0], -7.0))


# ------------------------------------------------------------------ 9. argument errors
def test_argument_errors_in_the_documented_order_leave_the_texture(R, torch):
    W, H = 64, 48
    ctx = R.RC2DGI(W, H, cascade_count=2)
    start = np.broadcast_to(SENTINEL, (H, W, 4)).copy()
    for which in ("color", "emissive"):
        ctx.upload(which, start)
    L, h, vp = ctx._L, ctx._h, ctypes.c_void_p
    at = to_dev(torch, atlas_np("float32"))
    t = torch.from_numpy(S.words(nine(W, H))).to("cuda")
    cnt = torch.full((2,), 9, dtype=torch.int32, device="cuda")
    st = torch.full((4,), -77, dtype=torch.int32, device="cuda")
    clear = (ctypes.c_ubyte * 4)(255, 255, 255, 255)
    p, c, s, d = t.data_ptr(), cnt.data_ptr(), st.data_ptr(), at.data_ptr()
    F32, F16, U8 = R.FMT_RGBA32F, R.FMT_RGBA16F, R.FMT_RGBA8
    A = lambda dev=d, w=AW, hh=AH, pitch=0, fmt=F32: ctypes.byref(R.Atlas(dev, w, hh, pitch, fmt))  # noqa: E731
    good = A()
    bad = [("a bad which", (R.RT["dist"], clear, good, vp(p), 9, vp(c), vp(s))),
           ("a bad which before a bad n", (-1, clear, good, vp(p), -1, None, None)),
           ("n < 0", (0, clear, good, vp(p), -1, vp(c), vp(s))),
           ("n > 1 << 20", (0, clear, good, vp(p), (1 << 20) + 1, vp(c), vp(s))),
           ("n out of range before a null atlas", (0, clear, None, vp(p), -1, vp(c), vp(s))),
           ("a null atlas", (0, clear, None, vp(p), 9, vp(c), vp(s))),
           ("a null atlas before a null list", (0, clear, None, None, 9, vp(c), vp(s))),
           ("a null atlas image", (1, clear, A(dev=None), vp(p), 9, vp(c), vp(s))),
           ("an atlas 0 wide", (0, clear, A(w=0), vp(p), 9, vp(c), vp(s))),
           ("an atlas 32769 tall", (0, clear, A(hh=32769), vp(p), 9, vp(c), vp(s))),
           ("a bad atlas format", (0, clear, A(fmt=3), vp(p), 9, vp(c), vp(s))),
           ("a bad atlas format", (0, clear, A(fmt=-1), vp(p), 9, vp(c), vp(s))),
           ("a pitch smaller than a row", (0, clear, A(pitch=AW * 16 - 16), vp(p), 9, vp(c), vp(s))),
           ("a pitch that is no multiple of a pixel", (0, clear, A(pitch=AW * 16 + 8), vp(p), 9, vp(c), vp(s))),
           ("a negative pitch", (0, clear, A(pitch=-16), vp(p), 9, vp(c), vp(s))),
           ("a misaligned atlas", (0, clear, A(dev=d + 8), vp(p), 9, vp(c), vp(s))),
           ("a misaligned half atlas", (0, clear, A(dev=d + 4, fmt=F16), vp(p), 9, vp(c), vp(s))),
           ("a misaligned byte atlas", (0, clear, A(dev=d + 2, fmt=U8), vp(p), 9, vp(c), vp(s))),
           ("a null list with n > 0", (1, clear, good, None, 9, vp(c), vp(s))),
           ("a misaligned list", (0, clear, good, vp(p + 2), 8, vp(c), vp(s))),
           ("a misaligned count", (1, clear, good, vp(p), 9, vp(c + 1), vp(s))),
           ("a misaligned status", (0, clear, good, vp(p), 9, vp(c), vp(s + 3)))]
    for what, args in bad:
        assert L.rc2dgi_sprites_xf_device(h, *args) == -1, what
        assert L.rc2dgi_last_error(h), what
    # the order, told by the messages: which, n, the atlas, the list, the alignment
    for args, word in [((-1, clear, None, None, -1, vp(c + 1), None), b"COLOR"),
                       ((0, clear, None, None, -1, vp(c + 1), None), b"n is"),
                       ((0, clear, None, None, 9, vp(c + 1), None), b"atlas"),
                       ((0, clear, A(w=0), None, 9, vp(c + 1), None), b"32768"),
                       ((0, clear, A(fmt=7, pitch=-16), None, 9, vp(c + 1), None), b"format"),
                       ((0, clear, A(pitch=-16, dev=d + 8), None, 9, vp(c + 1), None), b"pitch"),
                       ((0, clear, A(dev=d + 8), None, 9, vp(c + 1), None), b"aligned to a pixel"),
                       ((0, clear, good, None, 9, vp(c + 1), None), b"null sprite"),
                       ((0, clear, good, vp(p), 9, vp(c + 1), None), b"aligned to 4")]:
        assert L.rc2dgi_sprites_xf_device(h, *args) == -1
        assert word in L.rc2dgi_last_error(h), (word, L.rc2dgi_last_error(h))
        assert b"sprites_xf_device" in L.rc2dgi_last_error(h) or word == b"COLOR"
    ctx.sync()
    assert st.cpu().numpy().tolist() == [-77] * 4, "a refused call writes no status"
    for which in ("color", "emissive"):
        assert np.array_equal(ctx.download(which).view(u32), start.view(u32)), which
    assert L.rc2dgi_sprites_xf_device(h, 0, None, good, None, 0, None, vp(s)) == 0  # n == 0 with a null list
    most = torch.zeros((1 << 20, 12), dtype=torch.int32, device="cuda")  # the largest n; the count says 9
    assert L.rc2dgi_sprites_xf_device(h, 0, None, good, vp(most.data_ptr()), 1 << 20, vp(c), vp(s + 8)) == 0
    ctx.sync()
    assert st.cpu().numpy().tolist() == [0, 0, 9, 9], "nine records of zeros: w < 1, refused"
    assert np.array_equal(ctx.download("color").view(u32), start.view(u32))
    with pytest.raises(TypeError):
        ctx.sprites_xf_device("color", at, t.cpu())
    with pytest.raises(TypeError):
        ctx.sprites_xf_device("color", at.cpu(), t)
    with pytest.raises(TypeError):
        ctx.sprites_xf_device("color", at.to(torch.float64), t)
    with pytest.raises(TypeError):
        ctx.sprites_xf_device("color", at, t.to(torch.float32))
    with pytest.raises(ValueError):
        ctx.sprites_xf_device("color", at[:, :, :3], t)
    with pytest.raises(ValueError):
        ctx.sprites_xf_device("color", at, t[:, :8].contiguous())
    with pytest.raises(ValueError):
        ctx.sprites_xf_device("color", at, t, status=st)
    ctx.close()
