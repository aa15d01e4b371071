"""GPU: rc2dgi_gradients_device -- the five shapes with a colour a vertex and an HDR gain, from a list in device memory
-- against the numpy restatement written from the header (tests/gradients_ref.py), bit for bit (a NaN equal to any
NaN): the three storage modes with and without a clear over a non-trivial texture, equal-colour lists against
rc2dgi_shapes_device on the same context, lists built to cross every edge of the binning on three tile heights, a
circle whose fan closes inside the target, the device count and the status words, three batches on two plans, buffers
of garbage, shapes off the target, the painters' working memory, soft lights and gradient walls through a frame, the
stream order, a sharded frame, and the argument errors in their order."""
import ctypes

import numpy as np
import pytest

import gradients_ref as G
import shapes_ref as S
from test_gpu_shapes import SCREENS, SENTINEL, base_texture, code, edge_list, get, mixed_list, tiny_list

pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32
GAINS = (1.0, 0.5, 8.0)


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def R(torch):
    from radiancecascade2dglobalillumination_amd import rc2dgi

    return rc2dgi


def grads_dev(torch, ctx, which, words, clear=None, count=None, u8=False):
    """gradients_device of (n, 12) words; returns the texture and the status words"""
    t = torch.from_numpy(np.ascontiguousarray(words, np.int32).reshape(-1, 12)).to("cuda")
    status = torch.full((2,), -77, dtype=torch.int32, device="cuda")
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device="cuda")
    ctx.gradients_device(which, t, clear, cnt, status)
    ctx.sync()
    return get(ctx, which, u8), status.cpu().numpy().tolist()


def same(got, want):
    """equal in bits, a NaN equal to any NaN"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype.kind == "f":
        return got.shape == want.shape and bool(np.all((got.view(u32) == want.view(u32)) | (np.isnan(got) & np.isnan(want))))
    return np.array_equal(got, want)


def differing(got, want):
    return f"{np.count_nonzero(np.any(got != want, axis=-1))} texels differ"


def as_grads(L, seed):
    """the shapes (kind, v, colour) as gradients: four translucent colours a record and a gain of 1, 0.5 or 8"""
    rng = np.random.default_rng(seed)
    out = []
    for k, (kind, v, _) in enumerate(L):
        cols = rng.integers(0, 256, (4, 4))
        cols[:, 3] = rng.integers(30, 256, 4)
        out.append((kind, v, cols.astype(np.uint8), GAINS[k % 3]))
    return out


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
    L = as_grads(mixed_list(W, H, 31), 51)
    assert {g[0] for g in L} == {0, 1, 2, 3, 4} and {g[3] for g in L} == set(GAINS)
    words = G.words(L)
    base = base_texture(W, H, u8)
    want, m, nref = ref(("mixed", u8, clear), lambda: G.paint(W, H, words, clear=clear, base=base, rgba8=u8))
    assert (m, nref) == (len(L), 0)
    ctx = R.RC2DGI(W, H, cascade_count=2, storage=storage)
    for which in ("emissive", "color"):
        ctx.upload(which, base)
        got, status = grads_dev(torch, ctx, which, words, clear, u8=u8)
        assert status == [len(L), 0]
        assert same(got, want), f"{storage} {which}: {differing(got, want)}"
    if clear is None:
        assert not same(want, base)
    if not u8:
        assert want.max() > 1.5, "the gain reaches past 1.0 in float storage"
    ctx.close()


# ------------------------------------------------------------------ 2. the header's first consequence on the device
@pytest.mark.parametrize("storage", ["f32", "rgba8"])
@pytest.mark.parametrize("W,H", SCREENS)
def test_equal_colours_and_gain_one_leave_shapes_device_bits(R, torch, W, H, storage):
    u8 = storage == "rgba8"
    L = mixed_list(W, H, 33) + edge_list(W, H, 77)
    L[5] = (S.TRIANGLE, (float("nan"), 0, 1, 1, 2, 2), (1, 2, 3, 4))  # refused by both, counted by both
    L[9] = (11, (0, 0, 1, 1), (1, 2, 3, 4))
    shapes = torch.from_numpy(S.words(L)).to("cuda")
    grads = R.gradients_from_shapes(shapes)
    assert np.array_equal(grads.cpu().numpy(), G.from_shapes(S.words(L)))
    base = base_texture(W, H, u8, seed=9)
    ctx = R.RC2DGI(W, H, cascade_count=2, storage=storage)
    st = torch.full((2, 2), -77, dtype=torch.int32, device="cuda")
    ctx.upload("color", base)
    ctx.shapes_device("color", shapes, None, None, st[0])
    ctx.sync()
    want = get(ctx, "color", u8)
    ctx.upload("color", base)
    ctx.gradients_device("color", grads, None, None, st[1])
    ctx.sync()
    got = get(ctx, "color", u8)
    st = st.cpu().numpy().tolist()
    assert st[0] == st[1] == [len(L), 2]
    assert same(got, want), differing(got, want)
    assert not same(got, base)
    ctx.close()


# ------------------------------------------------------------------ 3. binning and coverage edge cases
@pytest.mark.parametrize("tile", [2, 3, 7], ids=["tile4", "tile8", "tile128"])
@pytest.mark.parametrize("W,H", SCREENS)
def test_lists_on_every_edge_of_the_binning(R, torch, W, H, tile):
    L = as_grads(edge_list(W, H, 77), 52)
    words = G.words(L)
    want, m, nref = ref(("edge", W, H), lambda: G.paint(W, H, words, clear=(9, 8, 7, 200)))
    assert (m, nref) == (len(L), 0)
    ctx = R.RC2DGI(W, H, cascade_count=2)
    ctx.set_tuning("paint_plan", code(tile, 1))
    assert ctx.get_tuning("paint_tile_h") == 1 << tile
    got, status = grads_dev(torch, ctx, "color", words, (9, 8, 7, 200))
    assert status == [len(L), 0]
    assert same(got, want), f"{W}x{H} tile {1 << tile}: {differing(got, want)}"
    # the list reversed: another texture (the order is kept), and the masks were left clear by the first call
    wantr, _, _ = ref(("edge_rev", W, H), lambda: G.paint(W, H, words[::-1], clear=(9, 8, 7, 200)))
    got, status = grads_dev(torch, ctx, "color", words[::-1], (9, 8, 7, 200))
    assert status == [len(L), 0] and same(got, wantr), differing(got, wantr)
    assert not same(want, wantr)
    ctx.close()


@pytest.mark.parametrize("W,H", SCREENS)
def test_every_edge_shape_alone(R, torch, W, H):
    """each gradient of the edge list painted on its own over the sentinel: what one shape's binning or colour
    association gets wrong cannot be hidden by another shape"""
    L = as_grads(edge_list(W, H, 77), 52)
    ctx = R.RC2DGI(W, H, cascade_count=2)
    start = np.broadcast_to(SENTINEL, (H, W, 4)).copy()
    bad = []
    for k, g in enumerate(L):
        ctx.upload("emissive", start)
        got, status = grads_dev(torch, ctx, "emissive", G.words([g]))
        want, _, nref = G.paint(W, H, G.words([g]), base=start)
        if status != [1, nref] or not same(got, want):
            bad.append((k, g[0], g[1], status, differing(got, want)))
    assert not bad, bad[:5]
    ctx.close()


def test_a_large_circle_whose_fan_closes_inside_the_target(R, torch):
    """radius 2^19 with T(0) = (40, 24.45) inside the 64 x 48 target: T(36) lies 0.09 pixel below T(0) (sinf of the
    float 2 pi times the radius), so the centres of screen row 24 left of x = 40 are covered by the first AND the last
    triangle of the fan; the first in listed order supplies the colour"""
    W, H = 64, 48
    r = 524288.0
    rec = (G.CIRCLE, (40.0 - r, 24.45, r), [(255, 40, 10, 250), (20, 90, 255, 60)], 2.0)
    words = G.words([rec])
    assert not G.refused(words[0])
    cover = np.zeros((H, W), int)
    for t in S.snapped(words[0][:8], W, H):
        ef = G.edge_functions(t, W, H)
        if ef is not None:
            cover += ef[3]
    assert (cover > 1).sum() >= 10, "the seam crosses the target and texel centres lie in both triangles"
    cov, _, tri = G.shade(words[0], W, H)
    assert set(np.unique(tri[cover > 1])) == {0}, "the first covering triangle"
    base = base_texture(W, H, False)
    want, m, nref = G.paint(W, H, words, base=base)
    ctx = R.RC2DGI(W, H, cascade_count=2)
    ctx.upload("emissive", base)
    got, status = grads_dev(torch, ctx, "emissive", words)
    assert status == [1, 0] and same(got, want), differing(got, want)
    ctx.close()


def test_shapes_off_the_target_draw_nothing_and_are_not_refused(R, torch):
    W, H = 64, 48
    L = []
    c = (200, 100, 50, 128)
    for dx, dy in ((-60, 0), (W + 30, 0), (0, -60), (0, H + 30), (-1e5, -1e5), (1e5, 1e5)):
        L += [(S.RECT, (dx, dy, 20, 20), c), (S.CIRCLE, (dx + 10, dy + 10, 9), c),
              (S.TRIANGLE, (dx, dy, dx + 20, dy + 3, dx + 5, dy + 20), c), (S.LINE, (dx, dy, dx + 20, dy + 20, 4), c),
              (S.ELLIPSE, (dx + 10, dy + 10, 10, 5), c)]
    L.append((S.LINE, (-40.0, 10.0, 10.0, -40.0, 2.0), c))  # its box meets the target, the line does not
    L.append((S.TRIANGLE, (-50.0, 20.0, 20.0, -50.0, -50.0, -50.0), c))
    words = G.words(as_grads(L, 53))
    ctx = R.RC2DGI(W, H, cascade_count=2)
    start = np.broadcast_to(SENTINEL, (H, W, 4)).copy()
    ctx.upload("emissive", start)
    got, status = grads_dev(torch, ctx, "emissive", words)
    assert status == [len(L), 0] and same(got, start)
    assert G.paint(W, H, words, base=start)[2] == 0
    ctx.close()


# ------------------------------------------------------------------ 4. list handling
def nine(W, H):
    return G.words(as_grads(mixed_list(W, H, 5, 9), 54))


@pytest.mark.parametrize("storage", ["f32", "rgba8"])
def test_count_and_status_words(R, torch, storage):
    W, H, n = 64, 48, 9
    words = nine(W, H)
    u8 = storage == "rgba8"
    clear = (20, 30, 40, 255)
    ctx = R.RC2DGI(W, H, cascade_count=2, storage=storage)
    for count, m in [(-3, 0), (0, 0), (5, 5), (n, n), (n + 100, n), (None, n), (-(1 << 31), 0), ((1 << 31) - 1, n)]:
        got, status = grads_dev(torch, ctx, "color", words, clear, count, u8=u8)
        assert status == [m, 0], (count, status)
        want = G.paint(W, H, words, clear=clear, rgba8=u8, count=m)[0]  # (m == 0: a clear only)
        assert same(got, want), f"count {count}: {differing(got, want)}"
    t = torch.from_numpy(words).to("cuda")
    ctx.gradients_device("color", t, clear)  # a null status
    ctx.sync()
    assert same(get(ctx, "color", u8), G.paint(W, H, words, clear=clear, rgba8=u8)[0])
    ctx.close()


def test_nothing_to_paint_without_a_clear_leaves_the_texture(R, torch):
    W, H = 64, 48
    ctx = R.RC2DGI(W, H, cascade_count=2)
    start = np.broadcast_to(SENTINEL, (H, W, 4)).copy()
    ctx.upload("emissive", start)
    words = nine(W, H)
    for count in (0, -3):
        got, status = grads_dev(torch, ctx, "emissive", words, None, count)
        assert status == [0, 0] and same(got, start)  # the status is written at m == 0
    got, status = grads_dev(torch, ctx, "emissive", np.zeros((0, 12), np.int32))  # n == 0, a null list
    assert status == [0, 0] and same(got, start)
    got, status = grads_dev(torch, ctx, "emissive", np.zeros((0, 12), np.int32), (1, 2, 3, 4))  # n == 0: the clear
    assert status == [0, 0] and same(got, np.broadcast_to(f32([1, 2, 3, 4]) / f32(255), (H, W, 4)))
    got, status = grads_dev(torch, ctx, "emissive", words, (1, 2, 3, 4), 0)  # m == 0 with a clear
    assert status == [0, 0] and same(got, np.broadcast_to(f32([1, 2, 3, 4]) / f32(255), (H, W, 4)))
    ctx.close()


def tiny_grads(W, H, n):
    """tiny_list's shapes with two colours and a gain each: the second colour differs, so LINEs and ELLIPSEs shade"""
    s = tiny_list(W, H, n)
    rng = np.random.default_rng(18)
    words = np.zeros((n, 12), np.int32)
    words[:, :8] = s
    cols = rng.integers(0, 256, (n, 3, 4)).astype(np.uint8)
    cols[:, :, 3] = rng.integers(30, 220, (n, 3))
    words[:, 8:11] = cols.reshape(n, 12).view(np.int32)
    words[:, 11] = np.asarray(GAINS, f32)[rng.integers(0, 3, n)].view(np.int32)
    return words


def test_three_batches_on_two_plans_of_a_live_context(R, torch):
    W, H, n = 64, 48, 2 * 2048 + 5
    words = tiny_grads(W, H, n)
    clear = (5, 5, 5, 255)
    want, m, nref = ref(("tiny", n), lambda: G.paint(W, H, words, clear=clear))
    assert (m, nref) == (n, 0)
    cut, _, _ = ref(("tiny", 2048), lambda: G.paint(W, H, words, clear=clear, count=2048))
    ctx = R.RC2DGI(W, H, cascade_count=2)
    for t in (2, 7):  # tile 4 / batch 2048, then tile 128 / batch 2048: a plan change on a live context
        ctx.set_tuning("paint_plan", code(t, 1))
        assert (ctx.get_tuning("paint_tile_h"), ctx.get_tuning("paint_batch")) == (1 << t, 2048)
        got, status = grads_dev(torch, ctx, "color", words, clear)
        assert status == [n, 0]
        assert same(got, want), f"tile {1 << t}: {differing(got, want)}"
        got, status = grads_dev(torch, ctx, "color", words, clear, count=2048)  # cut at a batch boundary
        assert status == [2048, 0] and same(got, cut), differing(got, cut)
    assert not same(want, cut)
    ctx.close()


GARBAGE_SEED = 2026


def garbage(kinds):
    """4096 records of seeded random 32-bit words.  `raw`: as they come.  `kind_0_7`: the kind reduced to its three
    lowest bits and the gain word replaced by a finite float, so that the coordinates decide."""
    n = 4096
    rng = np.random.default_rng(GARBAGE_SEED)
    words = rng.integers(0, 1 << 32, (n, 12), dtype=np.uint64).astype(u32).view(np.int32)
    if kinds == "kind_0_7":
        words[:, 0] &= 7
        words[:, 11] = rng.uniform(-4, 12, n).astype(f32).view(np.int32)
    return words


@pytest.mark.parametrize("kinds", ["raw", "kind_0_7"])
def test_a_buffer_of_garbage_paints_what_the_rule_accepts(R, torch, kinds):
    W, H, n = 64, 48, 4096
    words = garbage(kinds)
    want, m, nref = G.paint(W, H, words, clear=(0, 0, 0, 0))
    if kinds == "kind_0_7":
        assert 100 < n - nref < n - 100 and want.any(), "the seed leaves records drawn and records refused"
        assert {int(w[0]) for w in words if not G.refused(w)} == {0, 1, 2, 3, 4}
    ctx = R.RC2DGI(W, H, cascade_count=2)
    got, status = grads_dev(torch, ctx, "emissive", words, (0, 0, 0, 0))
    assert status == [n, nref], (status, nref)
    assert same(got, want), differing(got, want)
    got, status = grads_dev(torch, ctx, "emissive", words, (0, 0, 0, 0), count=-(1 << 31))
    assert status == [0, 0] and not got.any()
    got, status = grads_dev(torch, ctx, "emissive", words, (0, 0, 0, 0))  # a second call: the masks were left clear
    assert status == [n, nref] and same(got, want)
    ctx.close()


# ------------------------------------------------------------------ 5. the painters' working memory
@pytest.mark.parametrize("first", ["gradients", "paint"])
def test_the_call_shares_the_painters_working_memory_in_either_order(R, torch, first):
    """the call owns no memory: whichever of the two list painters runs first on a fresh context allocates the shared
    working memory, and each paints its bits before and after the other"""
    from oracle import paint_ref
    from test_gpu_tilemap import prim_words, prims

    W, H = 200, 72
    P = prims(W, H, 31)
    pw = torch.from_numpy(prim_words(R, P)).to("cuda")
    gw = nine(W, H)
    gt = torch.from_numpy(gw).to("cuda")
    st = torch.full((3, 2), -77, dtype=torch.int32, device="cuda")
    ctx = R.RC2DGI(W, H, cascade_count=2)
    clear = (10, 20, 30, 255)
    if first == "gradients":
        ctx.gradients_device("color", gt, clear, None, st[0])
        ctx.paint_device("color", pw, None, None, st[1])
        ctx.gradients_device("color", gt, None, None, st[2])
        want = G.paint(W, H, gw, clear=clear)[0]
        want = G.paint(W, H, gw, base=paint_ref.paint(W, H, P, None, base=want))[0]
    else:
        ctx.paint_device("color", pw, clear, None, st[0])
        ctx.gradients_device("color", gt, None, None, st[1])
        ctx.paint_device("color", pw, None, None, st[2])
        want = G.paint(W, H, gw, base=paint_ref.paint(W, H, P, clear))[0]
        want = paint_ref.paint(W, H, P, None, base=want)
    ctx.sync()
    assert st.cpu().numpy().tolist() == [[9, 0]] * 3
    got = ctx.download("color")
    assert same(got, want), differing(got, want)
    ctx.close()


# ------------------------------------------------------------------ 6. lights and walls through a frame
def scene(R, torch, W, H, seed):
    """soft lights for EMISSIVE and gradient walls for COLOR, as device lists and as the restatement's words"""
    rng = np.random.default_rng(seed)
    n = 7
    xy = rng.uniform(4, min(W, H) - 4, (n, 2)).astype(f32)
    rad = rng.uniform(3, 11, n).astype(f32)
    rgb = rng.integers(60, 256, (n, 3)).astype(np.uint8)
    gain = np.asarray([1.0, 4.0, 0.5, 8.0, 2.0, 1.0, 3.0], f32)
    t = lambda a: torch.from_numpy(a).to("cuda")  # noqa: E731
    lights = R.soft_lights(t(xy), t(rad), t(rgb), t(gain))
    walls = [(G.RECT, (W * 0.1, H * 0.7, W * 0.5, 5.0), [(200, 30, 30, 255), (30, 200, 30, 255), (30, 30, 200, 255), (200, 200, 30, 255)], 1.0),
             (G.LINE, (W * 0.8, H * 0.1, W * 0.6, H * 0.6, 3.0), [(255, 255, 255, 255), (40, 40, 40, 255)], 1.0),
             (G.TRIANGLE, (W * 0.2, H * 0.2, W * 0.35, H * 0.25, W * 0.25, H * 0.45), [(250, 120, 0, 255), (0, 120, 250, 255), (120, 250, 0, 255)], 1.0)]
    return lights, G.words(walls)


@pytest.mark.parametrize("storage", ["f32", "rgba8"])
def test_soft_lights_and_gradient_walls_then_a_frame_equal_the_oracle(R, torch, storage):
    import oracle

    W, H, N = 64, 48, 3
    u8 = storage == "rgba8"
    lights, walls = scene(R, torch, W, H, 61)
    lw = lights.cpu().numpy()
    ctx = R.RC2DGI(W, H, cascade_count=N, ray_range=2.0, storage=storage)
    st = torch.full((2, 2), -77, dtype=torch.int32, device="cuda")
    wt = torch.from_numpy(walls).to("cuda")
    ctx.gradients_device("color", wt, (0, 0, 0, 0), None, st[0])
    ctx.gradients_device("emissive", lights, (0, 0, 0, 255), None, st[1])
    ctx.do_rc2dgi()
    ctx.sync()
    got = ctx.download("color")
    color = G.paint(W, H, walls, clear=(0, 0, 0, 0), rgba8=u8)[0]
    emissive = G.paint(W, H, lw, clear=(0, 0, 0, 255), rgba8=u8)[0]
    assert st.cpu().numpy().tolist() == [[3, 0], [len(lw), 0]]
    assert color.any() and emissive[..., :3].any() and (u8 or emissive[..., :3].max() > 1.5)
    ctx.close()
    fr = oracle.frame(oracle.Params(W=W, H=H, N=N, ray_range=2.0, rgba8=u8), color, emissive)
    assert same(got, np.ascontiguousarray(fr.color_out, f32)), \
        f"{np.count_nonzero(np.any(got != fr.color_out, axis=-1))} texels differ from the oracle's frame"


def test_two_paintings_and_two_frames_with_one_sync(R, torch):
    """gradients_device twice, do, read, a third gradients_device, do, read, one sync at the end, behind a busy
    device: each capture equals that of a twin context that syncs after every call"""
    W = H = 128
    la = G.words(as_grads(mixed_list(W, H, 41, 30), 55))
    la[:, 7:11] |= np.int32(-16777216)  # opaque walls
    la[:, 11] = np.array([1.0], f32).view(np.int32)[0]
    lb = G.words(as_grads(mixed_list(W, H, 42, 30), 56))
    stream = torch.cuda.Stream()

    def run(step, busy):
        ctx = R.RC2DGI(W, H, cascade_count=3, ray_range=2.0)
        ctx.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            ta, tb = torch.from_numpy(la).to("cuda"), torch.from_numpy(lb).to("cuda")
            outs = [torch.full((H, W, 4), -7.0, device="cuda") for _ in range(2)]
            st = torch.full((3, 2), -77, dtype=torch.int32, device="cuda")
            big = torch.ones(1 << 26, device="cuda")
            stream.synchronize()
            if busy:  # work in flight on the stream when the calls are enqueued
                for _ in range(20):
                    big.mul_(1.0001).add_(0.5)
            step(ctx, lambda: ctx.gradients_device("color", ta, (0, 0, 0, 0), None, st[0]))
            step(ctx, lambda: ctx.gradients_device("emissive", tb, (0, 0, 0, 255), None, st[1]))
            ta.fill_(0x7FC00000)  # (the list may be overwritten on the stream once the call has returned)
            step(ctx, ctx.do_rc2dgi)
            step(ctx, lambda: ctx.read_into(outs[0], "color"))
            step(ctx, lambda: ctx.gradients_device("emissive", tb[:11], None, None, st[2]))
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

    want = run(stepwise, False)
    got = run(lambda ctx, fn: fn(), True)
    assert got[2] == want[2] == [[30, 0], [30, 0], [11, 0]]
    for k in range(2):
        assert same(got[k], want[k]), f"capture {k}: {differing(got[k], want[k])}"
    assert not same(got[0], got[1]) and not same(got[0], np.full_like(got[0], -7.0))


def test_a_sharded_frame_after_gradients_on_both_ranks(R, torch):
    from shard_compare import assert_shard_matches_whole, whole_frame

    W = H = 256
    N = 4
    lights, walls = scene(R, torch, W, H, 62)
    lw = lights.cpu().numpy()
    color = G.paint(W, H, walls, clear=(0, 0, 0, 0))[0]
    emis = G.paint(W, H, lw, clear=(0, 0, 0, 255))[0]
    want = whole_frame(R, W, H, N, 2.0, 1.0, 1.5, color, emis)
    ctxs = []
    for k in range(2):
        c = R.RC2DGI(W, H, cascade_count=N, ray_range=2.0)
        c.set_shader_value("_BlurRadius", 1.5)
        c.set_shard(k, 2)
        got, status = grads_dev(torch, c, "color", walls, (0, 0, 0, 0))
        assert status == [len(walls), 0] and same(got, color), f"rank {k}: the input is whole on every rank"
        got, status = grads_dev(torch, c, "emissive", lw, (0, 0, 0, 255))
        assert status == [len(lw), 0] and same(got, emis)
        ctxs.append(c)
    R.do_group(ctxs)
    for c in ctxs:
        c.sync()
    for c in ctxs:
        assert_shard_matches_whole(c, want, W, H, 1.5, expect_strip_tables=False)
    for c in ctxs:
        c.close()


# ------------------------------------------------------------------ 7. argument errors
def test_argument_errors_in_their_order_leave_the_texture(R, torch):
    W, H = 64, 48
    ctx = R.RC2DGI(W, H, cascade_count=2)
    start = np.broadcast_to(SENTINEL, (H, W, 4)).copy()
    for which in ("color", "emissive"):
        ctx.upload(which, start)
    L, h, vp = ctx._L, ctx._h, ctypes.c_void_p
    t = torch.from_numpy(nine(W, H)).to("cuda")
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
        assert L.rc2dgi_gradients_device(h, *args) == -1, what
        msg = L.rc2dgi_last_error(h)
        msg = msg.decode() if isinstance(msg, bytes) else str(msg)
        assert what in msg, (what, msg)
    assert "gradients_device" in msg
    ctx.sync()
    assert st.cpu().numpy().tolist() == [-77] * 4, "a refused call writes no status"
    for which in ("color", "emissive"):
        assert same(ctx.download(which), start), which
    assert L.rc2dgi_gradients_device(h, 0, None, None, 0, None, vp(s)) == 0  # n == 0 with a null list
    most = torch.zeros((1 << 20, 12), dtype=torch.int32, device="cuda")  # the largest n; the count says 9
    assert L.rc2dgi_gradients_device(h, 0, None, vp(most.data_ptr()), 1 << 20, vp(c), vp(s + 8)) == 0
    ctx.sync()
    assert st.cpu().numpy().tolist() == [0, 0, 9, 0]
    with pytest.raises(TypeError):
        ctx.gradients_device("color", t.cpu())
    with pytest.raises(TypeError):
        ctx.gradients_device("color", t.to(torch.float32))
    with pytest.raises(ValueError):
        ctx.gradients_device("color", t.reshape(-1, 6))
    with pytest.raises(ValueError):
        ctx.gradients_device("color", t, status=st)
    ctx.close()
