"""GPU: rc2dgi_shapes_device -- rectangles, circles, triangles, thick lines and ellipses from a list in device memory,
set up, binned by their triangles' edges and rasterised on the device -- against the numpy restatement written from the
header (tests/shapes_ref.py), bit for bit: the three storage modes with and without a clear over a non-trivial texture,
RECT / CIRCLE lists against rc2dgi_paint_device on the same context, the header's five consequences, lists built to
cross every edge of the binning on three tile heights, the device count and the status words, three batches on two
plans, buffers of garbage, the stream order, a sharded frame, and the argument errors in their order."""
import ctypes
import itertools

import numpy as np
import pytest

import shapes_ref as S

pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32
SENTINEL = f32([0.375, -2.5, 7.0, 0.625])
SCREENS = [(64, 48), (200, 72)]  # one tile column; four, the last one partial
C = (200, 100, 50, 128)
EPS = 1.0 / 256.0


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def R(torch):
    from radiancecascade2dglobalillumination_amd import rc2dgi

    return rc2dgi


def code(t, b):
    return t | b << 8


def get(ctx, which, u8=False):
    return ctx.download(which, np.uint8) if u8 else ctx.download(which)


def shapes_dev(torch, ctx, which, words, clear=None, count=None, u8=False):
    """shapes_device of (n, 8) words; returns the texture and the status words"""
    t = torch.from_numpy(np.ascontiguousarray(words, np.int32).reshape(-1, 8)).to("cuda")
    status = torch.full((2,), -77, dtype=torch.int32, device="cuda")
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device="cuda")
    ctx.shapes_device(which, t, clear, cnt, status)
    ctx.sync()
    return get(ctx, which, u8), status.cpu().numpy().tolist()


def same(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


def differing(got, want):
    return f"{np.count_nonzero(np.any(got != want, axis=-1))} texels differ"


def col(rng, lo=40, hi=230):
    return tuple(int(v) for v in rng.integers(0, 256, 3)) + (int(rng.integers(lo, hi)),)


def base_texture(W, H, u8, seed=4):
    rng = np.random.default_rng(seed)
    if u8:
        return rng.integers(0, 256, (H, W, 4)).astype(np.uint8)
    return (rng.integers(0, 512, (H, W, 4)) / 256.0).astype(f32)  # (values every storage mode holds exactly)


# ------------------------------------------------------------------ lists
def mixed_list(W, H, seed, n=60):
    """n translucent shapes of all five kinds across a W x H target, some partly off it"""
    rng = np.random.default_rng(seed)
    u = lambda lo, hi: float(rng.uniform(lo, hi))  # noqa: E731
    L = []
    for k in range(n):
        kind = k % 5
        x, y = u(-10, W + 10), u(-10, H + 10)
        if kind == S.RECT:
            v = (x, y, u(-8, 40), u(-8, 30))
        elif kind == S.CIRCLE:
            v = (x, y, u(-1, 14))
        elif kind == S.TRIANGLE:
            v = (x, y, x + u(-40, 40), y + u(-30, 30), x + u(-40, 40), y + u(-30, 30))
        elif kind == S.LINE:
            v = (x, y, x + u(-80, 80), y + u(-40, 40), u(0.3, 6))
        else:
            v = (x, y, u(-3, 25), u(-3, 12))
        L.append((kind, v, col(rng)))
    return L


def edge_list(W, H, seed):
    """Shapes on every edge of the binning: TRIANGLE vertices on tile cuts (x = 64, 128; rows 4 and 8 from either end,
    tiles being cut in GL rows) and 1/256 either side, on pixel centres, slivers narrower than a pixel, thin LINEs along
    both diagonals, LINEs whose edge grazes a tile corner, a triangle with vertices a million pixels away, degenerate
    lines and ellipses, all translucent: a tile wrongly rejected or a texel blended twice changes the texture."""
    rng = np.random.default_rng(seed)
    u = lambda lo, hi: float(rng.uniform(lo, hi))  # noqa: E731
    L = []
    for x in (64.0, 128.0):
        for y in (4.0, 8.0, H - 4.0, H - 8.0):
            for d in (-EPS, 0.0, EPS):
                for sx, sy in ((1, 1), (-1, 1), (1, -1), (-1, -1)):  # the triangle lies in one quadrant about the cut
                    L.append((S.TRIANGLE, (x + d, y + d, x + d + sx * u(3, 20), y + d + sy * u(0, 2),
                                           x + d + sx * u(0, 2), y + d + sy * u(3, 12)), col(rng)))
                L.append((S.TRIANGLE, (x + d - 9, y + d, x + d + 9, y + d, x + d, y + d + u(-7, 7)), col(rng)))
    for x, y in ((10.5, 10.5), (63.5, 3.5), (64.5, 4.5), (0.5, 0.5), (W - 0.5, H - 0.5)):  # vertices on pixel centres
        L.append((S.TRIANGLE, (x, y, x + 10.0, y, x, y + 10.0), col(rng)))
        L.append((S.TRIANGLE, (x, y, x - 7.0, y - 3.0, x + 5.0, y - 6.0), col(rng)))
    L.append((S.TRIANGLE, (2.0, 3.3, W - 2.0, H - 3.1, W - 2.2, H - 3.6), col(rng)))  # slivers
    L.append((S.TRIANGLE, (5.0, 5.0, W - 4.0, H - 8.0, W - 4.0, H - 7.3), col(rng)))
    L.append((S.TRIANGLE, (1.0, H - 2.0, W - 1.0, 2.0, W - 1.0, 2.4), col(rng)))
    L.append((S.TRIANGLE, (3.0, 20.5, W - 3.0, 20.5 + EPS, 3.0, 20.5 + 2 * EPS), col(rng)))  # thinner than 1/256
    for thick in (0.5, 1.0, 4.0):  # thin lines along both diagonals
        L.append((S.LINE, (0.0, 0.0, float(W), float(H), thick), col(rng)))
        L.append((S.LINE, (0.0, float(H), float(W), 0.0, thick), col(rng)))
    for cy in (8.0, H - 8.0):  # the edge of a line of thick 1 across (64, cy), and a little either side of it
        for o in (-0.36, -0.3536, -0.35, 0.0, 0.35, 0.3536, 0.36):
            L.append((S.LINE, (64.0 + o - 20, cy + o + 20, 64.0 + o + 20, cy + o - 20, 1.0), col(rng)))
    L.append((S.TRIANGLE, (-1048575.0, 10.0, 1048575.0, 30.0, 0.0, 1048575.0), col(rng)))  # crossing the target
    L.append((S.TRIANGLE, (-1048575.0, 40.0, 1048575.0, 20.0, 100.0, -1048575.0), col(rng)))
    L.append((S.LINE, (-1048575.0, -1048000.0, 1048575.0, 1048100.0, 3.0), col(rng)))
    L.append((S.LINE, (5.0, 5.0, 5.0, 5.0, 3.0), col(rng)))                    # len == 0
    L.append((S.LINE, (5.0, 5.0, 40.0, 30.0, 0.0), col(rng)))                  # thick == 0
    L.append((S.LINE, (5.0, 5.0, 40.0, 30.0, -2.0), col(rng)))                 # thick < 0
    L.append((S.LINE, (5.0, 5.0, 5.0 + 1e-30, 5.0, 3.0), col(rng)))            # dx * dx underflows to zero
    L.append((S.LINE, (0.0, 20.0, 1e-20, 20.0, 8.0), col(rng)))                # dx * dx is a denormal
    L.append((S.LINE, (0.0, 30.0, 3e-23, 30.0 + 3e-23, 6.0), col(rng)))
    for v in ((30.0, 20.0, 0.0, 5.0), (30.0, 20.0, 5.0, 0.0), (40.5, 20.5, -0.0, 3.0)):  # a zero radius: nothing
        L.append((S.ELLIPSE, v, col(rng)))
    L.append((S.ELLIPSE, (30.0, 20.0, -9.0, 5.0), col(rng)))                   # negative radii mirror the fan
    L.append((S.ELLIPSE, (W - 20.0, H - 10.0, 25.0, -7.0), col(rng)))
    L.append((S.ELLIPSE, (64.0, 8.0, 70.0, 1.2), col(rng)))                    # a flat ellipse along a tile cut
    L.append((S.CIRCLE, (64.0, H - 8.0, 0.0), col(rng)))                       # radius 0 -> 0.1, on a tile corner
    order = rng.permutation(len(L))
    return [L[k] for k in order]


_refs = {}


def ref(key, make):
    """a restatement computed once and shared, read-only"""
    if key not in _refs:
        out = make()
        out[0].setflags(write=False)
        _refs[key] = out
    return _refs[key]


# ------------------------------------------------------------------ 1. storage and content
@pytest.mark.parametrize("clear", [None, (9, 8, 7, 200)], ids=["noclear", "clear"])
@pytest.mark.parametrize("storage", ["f32", "f16", "rgba8"])
def test_a_mixed_list_in_every_storage_mode(R, torch, storage, clear):
    W, H = 200, 72
    u8 = storage == "rgba8"
    L = mixed_list(W, H, 31)
    assert {s[0] for s in L} == {0, 1, 2, 3, 4} and all(s[2][3] < 255 for s in L)
    words = S.words(L)
    base = base_texture(W, H, u8)
    want, m, nref = ref(("mixed", u8, clear), lambda: S.paint(W, H, words, clear=clear, base=base, rgba8=u8))
    assert (m, nref) == (len(L), 0)
    ctx = R.RC2DGI(W, H, cascade_count=2, storage=storage)
    for which in ("emissive", "color"):
        ctx.upload(which, base)
        got, status = shapes_dev(torch, ctx, which, words, clear, u8=u8)
        assert status == [len(L), 0]
        assert same(got, want), f"{storage} {which}: {differing(got, want)}"
    if clear is None:
        assert not same(want, base)
    ctx.close()


# ------------------------------------------------------------------ 2. cross-checks
@pytest.mark.parametrize("storage", ["f32", "rgba8"])
@pytest.mark.parametrize("W,H", SCREENS)
def test_rect_and_circle_lists_equal_paint_device(R, torch, W, H, storage):
    from test_gpu_paint_device import edge_list as prim_edge_list, to_words

    u8 = storage == "rgba8"
    P = prim_edge_list(W, H, 21, 12)
    c = (250, 10, 10, 255)
    big = 4194303.0
    P[3:3] = [(7, 1.0, 1.0, 20.0, 20.0) + c, (1, float("nan"), 5.0, 20.0, 0.0) + c, (0, big, 1.0, big, 20.0) + c,
              (1, 5.0, -big, -big, 0.0) + c, (0, 2.0, float("inf"), 20.0, 20.0) + c]  # refused by rc2dgi_prim's test
    prims = torch.from_numpy(to_words(R, P)).to("cuda")
    shapes = R.shapes_from_prims(prims)
    shapes[::3, 5:7] = 0x7FC00000  # (words the two kinds do not name are not read)
    shapes[1::2, 5] = -1
    ctx = R.RC2DGI(W, H, cascade_count=2, storage=storage)
    st = torch.full((2, 2), -77, dtype=torch.int32, device="cuda")
    ctx.paint_device("color", prims, (9, 8, 7, 200), None, st[0])
    ctx.sync()
    want = get(ctx, "color", u8)
    ctx.shapes_device("color", shapes, (9, 8, 7, 200), None, st[1])
    ctx.sync()
    got = get(ctx, "color", u8)
    st = st.cpu().numpy().tolist()
    assert st[0] == st[1] == [len(P), 5]
    assert same(got, want), differing(got, want)
    wantr, m, nref = S.paint(W, H, shapes.cpu().numpy(), clear=(9, 8, 7, 200), rgba8=u8)
    assert nref == 5 and same(got, wantr), differing(got, wantr)
    ctx.close()


def test_the_five_consequences_on_the_device(R, torch):
    W, H = 64, 48
    ctx = R.RC2DGI(W, H, cascade_count=2)
    draw = lambda L: shapes_dev(torch, ctx, "color", S.words(L), (1, 2, 3, 255))  # noqa: E731
    verts = ((3.3, 4.4), (50.2, 10.1), (20.7, 40.9))
    ims = [draw([(S.TRIANGLE, sum(p, ()), C)])[0] for p in itertools.permutations(verts)]
    assert all(same(ims[0], i) for i in ims[1:]) and same(ims[0], S.paint(W, H, S.words([(S.TRIANGLE, sum(verts, ()), C)]),
                                                                             clear=(1, 2, 3, 255))[0])
    for x, y, w, h in ((5, 7, 20, 11), (0, 0, 64, 48), (-3, 40, 70, 20), (8, 8, 31, 31)):
        r, _ = draw([(S.RECT, (x, y, w, h), C)])
        t, st = draw([(S.TRIANGLE, (x, y, x, y + h, x + w, y + h), C), (S.TRIANGLE, (x, y, x + w, y + h, x + w, y), C)])
        assert st == [2, 0] and same(r, t), (x, y, w, h, differing(r, t))
    for x0, y, length, thick in ((4, 20, 32, 6), (4, 7, 32, 6), (1, 30, 64, 2), (10, 11, 16, 1)):
        ln, _ = draw([(S.LINE, (x0, y, x0 + length, y, thick), C)])
        r, _ = draw([(S.RECT, (x0, y - thick / 2, length, thick), C)])
        assert same(ln, r), (x0, y, length, thick, differing(ln, r))
    for cx, cy, r in ((30.3, 20.7, 9.5), (32, 24, 20), (0.5, 0.5, 3.25), (70, 50, 12)):
        e, _ = draw([(S.ELLIPSE, (cx, cy, r, r), C)])
        c, _ = draw([(S.CIRCLE, (cx, cy, r), C)])
        assert same(e, c), (cx, cy, r, differing(e, c))
    blank = np.broadcast_to(f32([1, 2, 3, 255]) / f32(255), (H, W, 4))
    for v in ((30, 20, 0, 5), (30, 20, 5, 0), (30, 20, 0, 0)):
        e, st = draw([(S.ELLIPSE, v, C)])
        assert st == [1, 0] and same(e, blank), v
    ctx.close()


# ------------------------------------------------------------------ 3. binning and coverage edge cases
@pytest.mark.parametrize("tile", [2, 3, 7], ids=["tile4", "tile8", "tile128"])
@pytest.mark.parametrize("W,H", SCREENS)
def test_lists_on_every_edge_of_the_binning(R, torch, W, H, tile):
    L = edge_list(W, H, 77)
    words = S.words(L)
    want, m, nref = ref(("edge", W, H), lambda: S.paint(W, H, words, clear=(9, 8, 7, 200)))
    assert (m, nref) == (len(L), 0)
    ctx = R.RC2DGI(W, H, cascade_count=2)
    ctx.set_tuning("paint_plan", code(tile, 1))
    assert ctx.get_tuning("paint_tile_h") == 1 << tile
    got, status = shapes_dev(torch, ctx, "color", words, (9, 8, 7, 200))
    assert status == [len(L), 0]
    assert same(got, want), f"{W}x{H} tile {1 << tile}: {differing(got, want)}"
    # the list reversed: another texture (the order is kept), and the masks were left clear by the first call
    wantr, _, _ = ref(("edge_rev", W, H), lambda: S.paint(W, H, words[::-1], clear=(9, 8, 7, 200)))
    got, status = shapes_dev(torch, ctx, "color", words[::-1], (9, 8, 7, 200))
    assert status == [len(L), 0] and same(got, wantr), differing(got, wantr)
    assert not same(want, wantr)
    ctx.close()


@pytest.mark.parametrize("W,H", SCREENS)
def test_every_edge_shape_alone(R, torch, W, H):
    """each shape of the edge list painted on its own over the sentinel: what one shape's binning drops cannot be
    hidden by another shape"""
    L = edge_list(W, H, 77)
    ctx = R.RC2DGI(W, H, cascade_count=2)
    start = np.broadcast_to(SENTINEL, (H, W, 4)).copy()
    bad = []
    for k, s in enumerate(L):
        ctx.upload("emissive", start)
        got, status = shapes_dev(torch, ctx, "emissive", S.words([s]))
        want, _, nref = S.paint(W, H, S.words([s]), base=start)
        if status != [1, nref] or not same(got, want):
            bad.append((k, s, status, differing(got, want)))
    assert not bad, bad[:5]
    ctx.close()


def test_boxes_of_more_than_64_blocks_of_tiles(R, torch):
    """2048 x 1024 in tiles of 64 x 4 is 32 x 256 tiles, 4 x 32 blocks of 8 x 8: shapes whose box is the whole target
    take the binning's block walk through more than one round of 64 blocks"""
    W, H = 2048, 1024
    L = [(S.LINE, (0.0, 0.0, float(W), float(H), 3.0), (250, 200, 40, 160)),
         (S.LINE, (0.0, float(H), float(W), 0.0, 1.0), (40, 200, 250, 200)),
         (S.TRIANGLE, (3.0, 5.0, W - 2.0, H * 0.4, W * 0.3, H - 1.0), (90, 250, 90, 90)),
         (S.TRIANGLE, (-1048575.0, 10.0, 1048575.0, 900.0, 0.0, 1048575.0), (250, 90, 90, 60)),
         (S.RECT, (-5.0, -5.0, W + 10.0, H + 10.0), (10, 20, 30, 40))]
    words = S.words(L)
    want, m, nref = S.paint(W, H, words, clear=(1, 2, 3, 255))
    ctx = R.RC2DGI(W, H, cascade_count=2)
    ctx.set_tuning("paint_plan", code(2, 1))
    got, status = shapes_dev(torch, ctx, "emissive", words, (1, 2, 3, 255))
    assert status == [len(L), 0] and nref == 0
    assert same(got, want), differing(got, want)
    ctx.close()


def test_shapes_off_the_target_draw_nothing_and_are_not_refused(R, torch):
    W, H = 64, 48
    L = []
    for dx, dy in ((-60, 0), (W + 30, 0), (0, -60), (0, H + 30), (-1e5, -1e5), (1e5, 1e5)):
        L += [(S.RECT, (dx, dy, 20, 20), C), (S.CIRCLE, (dx + 10, dy + 10, 9), C),
              (S.TRIANGLE, (dx, dy, dx + 20, dy + 3, dx + 5, dy + 20), C), (S.LINE, (dx, dy, dx + 20, dy + 20, 4), C),
              (S.ELLIPSE, (dx + 10, dy + 10, 10, 5), C)]
    L.append((S.LINE, (-40.0, 10.0, 10.0, -40.0, 2.0), C))  # its box meets the target, the line does not
    L.append((S.TRIANGLE, (-50.0, 20.0, 20.0, -50.0, -50.0, -50.0), C))
    ctx = R.RC2DGI(W, H, cascade_count=2)
    start = np.broadcast_to(SENTINEL, (H, W, 4)).copy()
    ctx.upload("emissive", start)
    got, status = shapes_dev(torch, ctx, "emissive", S.words(L))
    assert status == [len(L), 0] and same(got, start)
    assert S.paint(W, H, S.words(L), base=start)[2] == 0
    ctx.close()


# ------------------------------------------------------------------ 4. list handling
def nine(W, H):
    return mixed_list(W, H, 5, 9)


@pytest.mark.parametrize("storage", ["f32", "rgba8"])
def test_count_and_status_words(R, torch, storage):
    W, H, n = 64, 48, 9
    words = S.words(nine(W, H))
    u8 = storage == "rgba8"
    clear = (20, 30, 40, 255)
    ctx = R.RC2DGI(W, H, cascade_count=2, storage=storage)
    for count, m in [(-3, 0), (0, 0), (5, 5), (n + 100, n), (None, n), (-(1 << 31), 0), ((1 << 31) - 1, n)]:
        got, status = shapes_dev(torch, ctx, "color", words, clear, count, u8=u8)
        assert status == [m, 0], (count, status)
        want = S.paint(W, H, words, clear=clear, rgba8=u8, count=m)[0]  # (m == 0: a clear only)
        assert same(got, want), f"count {count}: {differing(got, want)}"
    ctx.close()


def test_nothing_to_paint_without_a_clear_leaves_the_texture(R, torch):
    W, H = 64, 48
    ctx = R.RC2DGI(W, H, cascade_count=2)
    start = np.broadcast_to(SENTINEL, (H, W, 4)).copy()
    ctx.upload("emissive", start)
    words = S.words(nine(W, H))
    for count in (0, -3):
        got, status = shapes_dev(torch, ctx, "emissive", words, None, count)
        assert status == [0, 0] and same(got, start)  # the status is written at m == 0
    got, status = shapes_dev(torch, ctx, "emissive", np.zeros((0, 8), np.int32))  # n == 0, a null list
    assert status == [0, 0] and same(got, start)
    got, status = shapes_dev(torch, ctx, "emissive", np.zeros((0, 8), np.int32), (1, 2, 3, 4))  # n == 0: the clear
    assert status == [0, 0] and same(got, np.broadcast_to(f32([1, 2, 3, 4]) / f32(255), (H, W, 4)))
    ctx.close()


def tiny_list(W, H, n):
    """n tiny translucent shapes (one or two triangles each) with a few larger ones across each batch boundary"""
    rng = np.random.default_rng(8)
    words = np.zeros((n, 8), np.int32)
    kind = rng.integers(0, 3, n)
    kind[kind == 1] = S.LINE
    x, y = rng.uniform(-2, W, n).astype(f32), rng.uniform(-2, H, n).astype(f32)
    v = np.zeros((n, 6), f32)
    v[:, 0], v[:, 1] = x, y
    a, b = rng.uniform(0.5, 3, n).astype(f32), rng.uniform(0.5, 3, n).astype(f32)
    r = kind == S.RECT
    v[r, 2], v[r, 3] = a[r], b[r]
    t = kind == S.TRIANGLE
    v[t, 2], v[t, 3], v[t, 4], v[t, 5] = x[t] + a[t], y[t], x[t], y[t] + b[t]
    ln = kind == S.LINE
    v[ln, 2], v[ln, 3], v[ln, 4] = x[ln] + a[ln], y[ln] + b[ln], 1.0
    rgba = rng.integers(0, 256, (n, 4)).astype(np.uint8)
    rgba[:, 3] = rng.integers(30, 220, n)
    for bnd in (2048, 4096):  # ellipses straddling each batch boundary, over the same pixels
        for k in range(bnd - 3, bnd + 3):
            kind[k] = S.ELLIPSE
            v[k] = [20.0 + (k - bnd), 24.0, 9.0, 6.0, 0.0, 0.0]
    words[:, 0] = kind
    words[:, 1:7] = v.view(np.int32)
    words[:, 7] = rgba.view(np.int32)[:, 0]
    return words


def test_three_batches_on_two_plans_of_a_live_context(R, torch):
    W, H, n = 64, 48, 2 * 2048 + 5
    words = tiny_list(W, H, n)
    clear = (5, 5, 5, 255)
    want, m, nref = ref(("tiny", n), lambda: S.paint(W, H, words, clear=clear))
    assert (m, nref) == (n, 0)
    cut, _, _ = ref(("tiny", 2048), lambda: S.paint(W, H, words, clear=clear, count=2048))
    drop = np.delete(words, 2048, axis=0)  # (a shape at a batch boundary matters to the result)
    assert not same(S.paint(W, H, drop[2040:2056], base=S.paint(W, H, words[:2040], clear=clear)[0])[0],
                    S.paint(W, H, words[2040:2057], base=S.paint(W, H, words[:2040], clear=clear)[0])[0])
    ctx = R.RC2DGI(W, H, cascade_count=2)
    for t in (2, 7):  # tile 4 / batch 2048, then tile 128 / batch 2048: a plan change on a live context
        ctx.set_tuning("paint_plan", code(t, 1))
        assert (ctx.get_tuning("paint_tile_h"), ctx.get_tuning("paint_batch")) == (1 << t, 2048)
        got, status = shapes_dev(torch, ctx, "color", words, clear)
        assert status == [n, 0]
        assert same(got, want), f"tile {1 << t}: {differing(got, want)}"
        got, status = shapes_dev(torch, ctx, "color", words, clear, count=2048)  # cut at a batch boundary
        assert status == [2048, 0] and same(got, cut), differing(got, cut)
    ctx.close()


@pytest.mark.parametrize("kinds", ["raw", "kind_0_7"])
def test_a_buffer_of_garbage_paints_what_the_rule_accepts(R, torch, kinds):
    """4096 records of seeded random 32-bit words on 64 x 48.  `raw`: as they come (nearly every kind is unknown).
    `kind_0_7`: the same words with the kind reduced to its three lowest bits, so that the coordinates decide."""
    W, H, n = 64, 48, 4096
    rng = np.random.default_rng(2025)
    words = rng.integers(0, 1 << 32, (n, 8), dtype=np.uint64).astype(u32).view(np.int32)
    if kinds == "kind_0_7":
        words[:, 0] &= 7
    want, m, nref = S.paint(W, H, words, clear=(0, 0, 0, 0))
    if kinds == "kind_0_7":
        assert 100 < n - nref < n - 100
        assert {int(w[0]) for w in words if not S.refused(w)} == {0, 1, 2, 3, 4}
    ctx = R.RC2DGI(W, H, cascade_count=2)
    got, status = shapes_dev(torch, ctx, "emissive", words, (0, 0, 0, 0))
    assert status == [n, nref], (status, nref)
    assert same(got, want), differing(got, want)
    got, status = shapes_dev(torch, ctx, "emissive", words, (0, 0, 0, 0), count=-(1 << 31))
    assert status == [0, 0] and not got.any()
    got, status = shapes_dev(torch, ctx, "emissive", words, (0, 0, 0, 0))  # a second call: the masks were left clear
    assert status == [n, nref] and same(got, want)
    ctx.close()


# ------------------------------------------------------------------ 5. order
def test_two_paintings_and_two_frames_with_one_sync(R, torch):
    """shapes_device, do, read_device, a second shapes_device, do, read, one sync at the end: each capture equals that
    of a twin context that syncs after every call"""
    W = H = 128
    la, lb = S.words(mixed_list(W, H, 41, 30)), S.words(mixed_list(W, H, 42, 30))
    la[:, 7] |= np.int32(-16777216)  # opaque walls
    stream = torch.cuda.Stream()

    def run(step):
        ctx = R.RC2DGI(W, H, cascade_count=3, ray_range=2.0)
        ctx.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            ta, tb = torch.from_numpy(la).to("cuda"), torch.from_numpy(lb).to("cuda")
            outs = [torch.full((H, W, 4), -7.0, device="cuda") for _ in range(2)]
            st = torch.full((3, 2), -77, dtype=torch.int32, device="cuda")
            stream.synchronize()
            step(ctx, lambda: ctx.shapes_device("color", ta, (0, 0, 0, 0), None, st[0]))
            step(ctx, lambda: ctx.shapes_device("emissive", tb, (0, 0, 0, 255), None, st[1]))
            ta.fill_(0x7FC00000)  # (the list may be overwritten on the stream once the call has returned)
            step(ctx, ctx.do_rc2dgi)
            step(ctx, lambda: ctx.read_into(outs[0], "color"))
            step(ctx, lambda: ctx.shapes_device("emissive", tb[:11], None, None, st[2]))
            step(ctx, ctx.do_rc2dgi)
            step(ctx, lambda: ctx.read_into(outs[1], "color"))
        ctx.sync()
        got = [o.cpu().numpy() for o in outs] + [st.cpu().numpy().tolist()]
        ctx.set_stream(None)
        ctx.close()
        return got

    def stepwise(ctx, fn):
        fn()
        ctx.sync()

    want = run(stepwise)
    got = run(lambda ctx, fn: fn())
    assert got[2] == want[2] == [[30, 0], [30, 0], [11, 0]]
    for k in range(2):
        assert same(got[k], want[k]), f"capture {k}: {differing(got[k], want[k])}"
    assert not same(got[0], got[1]) and not same(got[0], np.full_like(got[0], -7.0))


def test_a_sharded_frame_after_shapes_on_both_ranks(R, torch):
    from shard_compare import assert_shard_matches_whole, whole_frame

    W = H = 256
    N = 4
    rng = np.random.default_rng(6)
    walls = [(k, v, c[:3] + (255,)) for k, v, c in mixed_list(W, H, 43, 40)]
    lights = [(S.CIRCLE, (float(rng.uniform(0, W)), float(rng.uniform(0, H)), float(rng.uniform(3, 9))),
               (255, 220, 180, 255)) for _ in range(6)]
    lights.append((S.LINE, (20.0, 20.0, 230.0, 200.0, 3.0), (90, 200, 255, 255)))
    wc, we = S.words(walls), S.words(lights)
    color = S.paint(W, H, wc, clear=(0, 0, 0, 0))[0]
    emis = S.paint(W, H, we, clear=(0, 0, 0, 255))[0]
    want = whole_frame(R, W, H, N, 2.0, 1.0, 1.5, color, emis)
    ctxs = []
    for k in range(2):
        c = R.RC2DGI(W, H, cascade_count=N, ray_range=2.0)
        c.set_shader_value("_BlurRadius", 1.5)
        c.set_shard(k, 2)
        got, status = shapes_dev(torch, c, "color", wc, (0, 0, 0, 0))
        assert status == [len(walls), 0] and same(got, color), f"rank {k}: the input is whole on every rank"
        got, status = shapes_dev(torch, c, "emissive", we, (0, 0, 0, 255))
        assert status == [len(lights), 0] and same(got, emis)
        ctxs.append(c)
    R.do_group(ctxs)
    for c in ctxs:
        c.sync()
    for c in ctxs:
        assert_shard_matches_whole(c, want, W, H, 1.5, expect_strip_tables=False)
    for c in ctxs:
        c.close()


# ------------------------------------------------------------------ 6. argument errors
def test_argument_errors_in_their_order_leave_the_texture(R, torch):
    W, H = 64, 48
    ctx = R.RC2DGI(W, H, cascade_count=2)
    start = np.broadcast_to(SENTINEL, (H, W, 4)).copy()
    for which in ("color", "emissive"):
        ctx.upload(which, start)
    L, h, vp = ctx._L, ctx._h, ctypes.c_void_p
    t = torch.from_numpy(S.words(nine(W, H))).to("cuda")
    cnt = torch.full((2,), 9, dtype=torch.int32, device="cuda")
    st = torch.full((4,), -77, dtype=torch.int32, device="cuda")
    clear = (ctypes.c_ubyte * 4)(255, 255, 255, 255)
    p, c, s = t.data_ptr(), cnt.data_ptr(), st.data_ptr()
    # each call is wrong in the way named and in every way checked after it: the message names the first
    bad = [("only COLOR and EMISSIVE", (R.RT["dist"], clear, None, -1, vp(c + 1), vp(s))),
           ("only COLOR and EMISSIVE", (-1, clear, vp(p), 9, None, None)),
           ("n is 0 .. 1 << 20", (0, clear, None, -1, vp(c + 1), vp(s))),
           ("n is 0 .. 1 << 20", (0, clear, vp(p + 2), (1 << 20) + 1, vp(c), vp(s))),
           ("null primitive list", (1, clear, None, 9, vp(c + 1), vp(s))),
           ("aligned to 4 bytes", (0, clear, vp(p + 2), 8, vp(c), vp(s))),
           ("aligned to 4 bytes", (1, clear, vp(p), 9, vp(c + 1), vp(s))),
           ("aligned to 4 bytes", (0, clear, vp(p), 9, vp(c), vp(s + 3)))]
    for what, args in bad:
        assert L.rc2dgi_shapes_device(h, *args) == -1, what
        msg = L.rc2dgi_last_error(h)
        msg = msg.decode() if isinstance(msg, bytes) else str(msg)
        assert what in msg, (what, msg)
    assert "shapes_device" in msg
    ctx.sync()
    assert st.cpu().numpy().tolist() == [-77] * 4, "a refused call writes no status"
    for which in ("color", "emissive"):
        assert same(ctx.download(which), start), which
    assert L.rc2dgi_shapes_device(h, 0, None, None, 0, None, vp(s)) == 0  # n == 0 with a null list
    most = torch.zeros((1 << 20, 8), dtype=torch.int32, device="cuda")  # the largest n; the count says 9
    assert L.rc2dgi_shapes_device(h, 0, None, vp(most.data_ptr()), 1 << 20, vp(c), vp(s + 8)) == 0
    ctx.sync()
    assert st.cpu().numpy().tolist() == [0, 0, 9, 0]
    with pytest.raises(TypeError):
        ctx.shapes_device("color", t.cpu())
    with pytest.raises(TypeError):
        ctx.shapes_device("color", t.to(torch.float32))
    with pytest.raises(ValueError):
        ctx.shapes_device("color", t.reshape(-1, 6))
    with pytest.raises(ValueError):
        ctx.shapes_device("color", t, status=st)
    ctx.close()
