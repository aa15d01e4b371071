"""GPU: rc2dgi_paint_device -- the painter fed from a primitive list in device memory, set up, binned and rasterised on
the device and enqueued without a wait -- against the numpy restatement the llvmpipe fixtures pin
(oracle/paint_ref.py), bit for bit: the fixtures themselves, lists built to cross every edge of the binning (targets
that are no multiple of a tile, primitives off the target on each side, more than 64 over one pixel, the order
reversed), the device count and status words, refused primitives and a buffer of garbage, a list of more than two
batches against rc2dgi_paint, the stream order behind a busy device, a device-only loop through a frame, and the
argument errors."""
import ctypes
import time

import numpy as np
import pytest

from oracle import paint_ref
from test_paint_cpu import paint_cases

pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32
LIM = f32(4194304.0)  # 2^22 pixels
SENTINEL = f32([0.375, -2.5, 7.0, 0.625])


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def R(torch):
    from radiancecascade2dglobalillumination_amd import rc2dgi

    return rc2dgi


# ------------------------------------------------------------------ lists
def to_words(R, prims):
    """(n, 6) int32: the bytes of the rc2dgi_prim records of (kind, x, y, w, h, r, g, b, a) tuples"""
    arr = (R.Prim * max(len(prims), 1))()
    for k, p in enumerate(prims):
        arr[k] = R.Prim(int(p[0]), float(p[1]), float(p[2]), float(p[3]), float(p[4]), *(int(v) for v in p[5:9]))
    return np.frombuffer(bytes(arr), np.int32).reshape(-1, 6)[:len(prims)].copy()


def from_words(words):
    """the tuples paint_ref takes, of (n, 6) int32 words"""
    w = np.ascontiguousarray(words, np.int32)
    xy = w[:, 1:5].copy().view(f32)
    c = w[:, 5].copy().view(np.uint8).reshape(-1, 4)
    return [(int(w[k, 0]),) + tuple(xy[k]) + tuple(int(v) for v in c[k]) for k in range(len(w))]


def accepted(words):
    """rc2dgi_paint's test of a primitive (rc2dgi_capi.cpp), in float32 as it is written there: a bool a record"""
    w = np.ascontiguousarray(words, np.int32)
    kind = w[:, 0]
    x, y, ww, h = (w[:, k].copy().view(f32) for k in (1, 2, 3, 4))
    with np.errstate(all="ignore"):
        ok = lambda c: np.abs(c) < LIM  # noqa: E731  (false for a NaN and an infinity)
        rect = (kind == 0) & ok(x) & ok(y) & ok(ww) & ok(h) & ok((x + ww).astype(f32)) & ok((y + h).astype(f32))
        circ = (kind == 1) & ok(x) & ok(y) & ok(ww) & ((np.abs(x) + np.abs(ww)).astype(f32) < LIM) & \
            ((np.abs(y) + np.abs(ww)).astype(f32) < LIM)
    return rect | circ


def paint_dev(torch, ctx, which, words, clear=None, count=None):
    """paint_device of (n, 6) words; returns the texture (floats) and the status words"""
    t = torch.from_numpy(np.ascontiguousarray(words, np.int32).reshape(-1, 6)).to("cuda")
    status = torch.full((2,), -77, dtype=torch.int32, device="cuda")
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device="cuda")
    ctx.paint_device(which, t, clear, cnt, status)
    ctx.sync()
    return ctx.download(which), status.cpu().numpy().tolist()


def differing(got, want):
    return f"{np.count_nonzero(np.any(got != want, axis=-1))} texels differ"


# ------------------------------------------------------------------ 1. the llvmpipe fixtures
@pytest.mark.parametrize("storage", ["f32", "rgba8"])
@pytest.mark.parametrize("case", list(paint_cases()), ids=lambda c: c[0])
def test_fixtures_through_the_device_list(R, torch, case, storage):
    name, W, H, clear, prims, want, want_u8 = case
    ctx = R.RC2DGI(W, H, cascade_count=2, storage=storage)
    ctx.upload("emissive", np.zeros((H, W, 4), f32))  # a fresh (zero) render texture
    _, status = paint_dev(torch, ctx, "emissive", to_words(R, prims), clear)
    assert status == [len(prims), 0]
    if storage == "rgba8":  # an RGBA8 render texture: compare the texels
        got, want = ctx.download("emissive", np.uint8), want_u8
    else:
        got = ctx.download("emissive")
    assert np.array_equal(got, want), f"{name}: {differing(got, want)}"
    ctx.close()


# ------------------------------------------------------------------ 2. lists across every edge of the binning
def tile_rows(H, tile_hs):
    """The screen rows at the cuts of tiles of the heights `tile_hs`: texel rows k * tile_h - 1, k * tile_h and
    k * tile_h + 1 for the first cut and the last one on the target (the start of a last, perhaps partly covered, tile
    row), counted from both ends.  Tiles are cut in GL rows: screen row Y is texel row H - 1 - Y."""
    rows = set()
    for th in tile_hs:
        for k in {1, (H - 1) // th}:
            for g in (k * th - 1, k * th, k * th + 1):
                if k > 0 and 0 <= g < H:
                    rows |= {H - 1 - g, g}
    return sorted(rows)


def edge_list(W, H, seed, circles, tile_hs=()):
    """About 300 translucent primitives of both kinds on a W x H target: wholly off the target on each side, one over
    the whole target, negative w / h, radius 0 and below, centres on pixel centres and on tile corners (columns that
    are multiples of 64, rows that are multiples of 4 from either end), and 70 over one pixel.  With `tile_hs`, for
    every row of tile_rows a circle centred on it and a rectangle with an edge on it, on columns that are multiples of
    64 (tests/test_gpu_paint_plans.py)."""
    rng = np.random.default_rng(seed)
    col = lambda: tuple(int(v) for v in rng.integers(0, 256, 3)) + (int(rng.integers(1, 255)),)  # noqa: E731
    P = []
    for dx, dy in ((-40, 0), (W + 5, 0), (0, -40), (0, H + 5)):  # off the target: left, right, above, below
        P.append((0, float(dx), float(dy), 30.0, 30.0) + col())
        P.append((1, float(dx + (15 if dx <= 0 else 20)), float(dy + (15 if dy <= 0 else 20)), 12.0, 0.0) + col())
    P.append((0, -3.0, -2.0, float(W + 9), float(H + 7)) + col())  # the whole target
    P.append((0, W * 0.75, H * 0.75, -W * 0.5, -H * 0.5) + col())  # negative w and h
    P.append((0, W * 0.25, H * 0.75, W * 0.25, -H * 0.25) + col())
    P.append((1, W * 0.5, H * 0.5, 0.0, 0.0) + col())              # radius 0 -> 0.1
    P.append((1, W * 0.5 + 0.5, H * 0.5 + 0.5, -3.0, 0.0) + col())  # a negative radius -> 0.1, on a pixel centre
    px, py = min(W - 2, 37), min(H - 2, 5)
    for k in range(70):  # more than 64 over one pixel: the walk crosses the mask's word boundaries
        P.append((0, px - 0.25 * (k % 5), py - 0.25 * (k % 3), 1.5 + (k % 4), 1.5 + (k % 2)) + col())
    centres = [(x, y) for x in (0.0, 64.0, min(W, 128.0), float(W)) for y in (0.0, 4.0, 8.0, H - 4.0, float(H))]
    centres += [(x + 0.5, y + 0.5) for x in (10.0, 63.0, 64.0) for y in (1.0, 3.0, 4.0)]
    for k, (x, y) in enumerate(centres[:circles]):
        P.append((1, x, y, float(rng.uniform(0.4, 9.0)), 0.0) + col())
    cols = [float(x) for x in range(0, W + 1, 64)]
    for k, Y in enumerate(tile_rows(H, tile_hs)):
        x = cols[k % len(cols)]
        # a centre on the row's pixel centres or on its upper boundary; a rectangle whose top or bottom edge is that
        # boundary, across the tile column's cut
        P.append((1, x + 0.5 * (k % 2), Y + 0.5 * (k // 2 % 2), float(rng.uniform(0.4, 6.0)), 0.0) + col())
        P.append((0, x - 3.0, float(Y), float(rng.uniform(4, 12)), float(rng.uniform(1, 9)) * (1 - k % 3 % 2 * 2)) + col())
    while len(P) < 300:
        P.append((0, float(rng.uniform(-20, W)), float(rng.uniform(-20, H)), float(rng.uniform(-6, 40)),
                  float(rng.uniform(-6, 30))) + col())
    order = rng.permutation(len(P))
    return [P[k] for k in order]


_edge_refs = {}


def edge_ref(W, H, reverse, u8):
    """the restatement of the list (or of the list reversed), computed once and shared"""
    key = (W, H, reverse, u8)
    if key not in _edge_refs:
        P = edge_list(W, H, 21, 29 if W < 100 else 12)
        _edge_refs[key] = paint_ref.paint(W, H, P[::-1] if reverse else P, (9, 8, 7, 200), rgba8=u8)
        _edge_refs[key].setflags(write=False)
    return _edge_refs[key]


@pytest.mark.parametrize("W,H,storage", [(70, 9, "f32"), (70, 9, "rgba8"), (70, 9, "f16"),  # (F16 storage paints floats,
                                         (333, 250, "f32"), (333, 250, "rgba8")])          # as F32 storage does)
def test_lists_across_tile_and_word_boundaries_in_both_orders(R, torch, W, H, storage):
    P = edge_list(W, H, 21, 29 if W < 100 else 12)
    assert len(P) == 300 and {p[0] for p in P} == {0, 1}
    u8 = storage == "rgba8"
    ctx = R.RC2DGI(W, H, cascade_count=2, storage=storage)
    outs = []
    for reverse in (False, True):
        words = to_words(R, P[::-1] if reverse else P)
        _, status = paint_dev(torch, ctx, "color", words, (9, 8, 7, 200))
        assert status == [300, 0]
        got = ctx.download("color", np.uint8) if u8 else ctx.download("color")
        want = edge_ref(W, H, reverse, u8)
        assert np.array_equal(got, want), f"{W}x{H} {storage} reversed={reverse}: {differing(got, want)}"
        outs.append(got)
    assert not np.array_equal(outs[0], outs[1]), "the two orders give different textures: the order is kept"
    ctx.close()


# ------------------------------------------------------------------ 3. the device count and the status words
def nine(W, H):
    rng = np.random.default_rng(3)
    P = []
    for k in range(9):
        c = tuple(int(v) for v in rng.integers(0, 256, 3)) + (int(rng.integers(60, 255)),)
        if k % 2:
            P.append((1, float(rng.uniform(0, W)), float(rng.uniform(0, H)), float(rng.uniform(2, 14)), 0.0) + c)
        else:
            P.append((0, float(rng.uniform(-5, W - 10)), float(rng.uniform(-5, H - 10)), float(rng.uniform(4, 30)),
                      float(rng.uniform(4, 20))) + c)
    return P


@pytest.mark.parametrize("storage", ["f32", "rgba8"])
def test_count_and_status_words(R, torch, storage):
    W, H, n = 64, 48, 9
    P = nine(W, H)
    words = to_words(R, P)
    u8 = storage == "rgba8"
    clear = (20, 30, 40, 255)
    ctx = R.RC2DGI(W, H, cascade_count=2, storage=storage)
    get = lambda: ctx.download("color", np.uint8) if u8 else ctx.download("color")  # noqa: E731
    for count, m in [(-3, 0), (0, 0), (5, 5), (n + 100, n), (None, n)]:
        _, status = paint_dev(torch, ctx, "color", words, clear, count)
        assert status == [m, 0], (count, status)
        want = paint_ref.paint(W, H, P[:m], clear, rgba8=u8)  # (m == 0: a clear only)
        assert np.array_equal(get(), want), f"count {count}: {differing(get(), want)}"
    # a count torch writes on the stream right before the call, and overwrites right after it has returned
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        t = torch.from_numpy(words).to("cuda")
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        status = torch.full((2,), -77, dtype=torch.int32, device="cuda")
        cnt.fill_(4)
        ctx.paint_device("color", t, clear, cnt, status)
        cnt.fill_(-1)
        t.fill_(0x7FC00000)
    ctx.sync()
    assert status.cpu().numpy().tolist() == [4, 0]
    want = paint_ref.paint(W, H, P[:4], clear, rgba8=u8)
    assert np.array_equal(get(), want), differing(get(), want)
    ctx.set_stream(None)
    ctx.close()


def test_nothing_to_paint_without_a_clear_leaves_the_texture(R, torch):
    W, H = 64, 48
    ctx = R.RC2DGI(W, H, cascade_count=2)
    start = np.broadcast_to(SENTINEL, (H, W, 4)).copy()
    ctx.upload("emissive", start)
    words = to_words(R, nine(W, H))
    for count in (0, -3):
        got, status = paint_dev(torch, ctx, "emissive", words, None, count)
        assert status == [0, 0] and np.array_equal(got.view(u32), start.view(u32))
    got, status = paint_dev(torch, ctx, "emissive", np.zeros((0, 6), np.int32))  # n == 0, a null list
    assert status == [0, 0] and np.array_equal(got.view(u32), start.view(u32))
    got, status = paint_dev(torch, ctx, "emissive", np.zeros((0, 6), np.int32), (1, 2, 3, 4))  # n == 0: the clear
    assert status == [0, 0] and np.array_equal(got, np.broadcast_to(f32([1, 2, 3, 4]) / f32(255), (H, W, 4)))
    ctx.close()


# ------------------------------------------------------------------ 4. refused primitives and garbage
@pytest.mark.parametrize("storage", ["f32", "rgba8"])
def test_each_refused_form_draws_nothing_and_is_counted(R, torch, storage):
    W, H = 64, 48
    good = nine(W, H)
    c = (250, 10, 10, 255)
    big = 4194303.0
    bad = [(7, 1.0, 1.0, 20.0, 20.0) + c,            # an unknown kind
           (-1, 1.0, 1.0, 20.0, 20.0) + c,
           (1, float("nan"), 5.0, 20.0, 0.0) + c,    # NaN
           (0, 2.0, float("inf"), 20.0, 20.0) + c,   # +inf
           (0, 1e7, 1.0, 2.0, 2.0) + c,              # 1e7
           (0, 1.0, 1.0, 20.0, float("-inf")) + c,
           (0, big, 1.0, big, 20.0) + c,             # a rectangle whose x + w is out of range
           (0, 1.0, -big, 20.0, -big) + c,
           (1, big, 5.0, 10.0, 0.0) + c,             # a circle whose |x| + |w| is out of range
           (1, 5.0, -big, -big, 0.0) + c]
    P = []
    for k, p in enumerate(good):  # one refused form between every two valid primitives, and at both ends
        P += [bad[k], p]
    P.append(bad[9])
    words = to_words(R, P)
    ok = accepted(words)
    assert ok.tolist() == [k % 2 == 1 for k in range(len(P))], "the restated rule refuses exactly the forms above"
    u8 = storage == "rgba8"
    ctx = R.RC2DGI(W, H, cascade_count=2, storage=storage)
    _, status = paint_dev(torch, ctx, "color", words, (1, 2, 3, 255))
    assert status == [len(P), len(bad)]
    got = ctx.download("color", np.uint8) if u8 else ctx.download("color")
    want = paint_ref.paint(W, H, good, (1, 2, 3, 255), rgba8=u8)
    assert np.array_equal(got, want), differing(got, want)
    # a circle's h is not read: any bits there are accepted, as rc2dgi_paint accepts them
    P2 = [(1,) + p[1:4] + (float("nan"),) + p[5:] if p[0] == 1 else p for p in good]
    _, status = paint_dev(torch, ctx, "color", to_words(R, P2), (1, 2, 3, 255))
    assert status == [len(good), 0]
    got = ctx.download("color", np.uint8) if u8 else ctx.download("color")
    assert np.array_equal(got, want), differing(got, want)
    ctx.close()


@pytest.mark.parametrize("kinds", ["raw", "kind_0_1"])
def test_a_buffer_of_garbage_paints_what_the_host_rule_accepts(R, torch, kinds):
    """4096 records of seeded random 32-bit words on 64 x 48.  `raw`: as they come (nearly every kind is unknown).
    `kind_0_1`: the same words with the kind reduced to its lowest bit, so that the coordinates decide."""
    W, H, n = 64, 48, 4096
    rng = np.random.default_rng(2024)
    words = rng.integers(0, 1 << 32, (n, 6), dtype=np.uint64).astype(u32).view(np.int32)
    if kinds == "kind_0_1":
        words[:, 0] &= 1
    ok = accepted(words)
    keep = from_words(words[ok])
    if kinds == "kind_0_1":
        assert 100 < len(keep) < n - 100
    ctx = R.RC2DGI(W, H, cascade_count=2)
    got, status = paint_dev(torch, ctx, "emissive", words, (0, 0, 0, 0))
    assert status[0] == n and status[0] - status[1] == len(keep), (status, len(keep))
    want = paint_ref.paint(W, H, keep, (0, 0, 0, 0))
    assert np.array_equal(got, want), differing(got, want)
    # and with a garbage count of its own
    got, status = paint_dev(torch, ctx, "emissive", words, (0, 0, 0, 0), count=-(1 << 31))
    assert status == [0, 0] and not got.any()
    got, status = paint_dev(torch, ctx, "emissive", words, (0, 0, 0, 0), count=(1 << 31) - 1)
    assert status == [n, n - len(keep)] and np.array_equal(got, want)
    ctx.close()


# ------------------------------------------------------------------ 5. more than two batches
def test_more_than_two_batches_keep_the_draw_order(R, torch):
    W, H = 64, 48
    batch, work = R.paint_device_limits(W, H)
    if batch == 1 << 20:
        pytest.skip("this design paints without batches")
    n = 2 * batch + 3
    rng = np.random.default_rng(8)
    kind = np.zeros(n, np.int32)
    xywh = np.stack([rng.uniform(-2, W, n), rng.uniform(-2, H, n), rng.uniform(0.5, 3, n), rng.uniform(0.5, 3, n)], 1).astype(f32)
    rgba = rng.integers(0, 256, (n, 4)).astype(np.uint8)
    rgba[:, 3] = rng.integers(30, 220, n)
    for b in (batch, 2 * batch):  # circles straddling each batch boundary, over the same pixels
        for k in range(b - 3, b + 3):
            kind[k] = 1
            xywh[k] = [20.0 + (k - b), 24.0, 9.0, 0.0]
    words = np.concatenate([kind[:, None], xywh.view(np.int32), rgba.view(np.int32)], 1)
    P = from_words(words)
    twin = R.RC2DGI(W, H, cascade_count=2)
    twin.paint("color", P, (5, 5, 5, 255))
    want = twin.download("color")
    twin.paint("color", P[:batch] + P[batch + 1:], (5, 5, 5, 255))  # (a primitive at a boundary matters to the result)
    assert not np.array_equal(twin.download("color"), want)
    twin.close()
    ctx = R.RC2DGI(W, H, cascade_count=2)
    got, status = paint_dev(torch, ctx, "color", words, (5, 5, 5, 255))
    assert status == [n, 0]
    assert np.array_equal(got, want), differing(got, want)
    # the same list cut by the count inside the third batch and at a batch boundary
    for m in (2 * batch + 1, batch):
        got, status = paint_dev(torch, ctx, "color", words, (5, 5, 5, 255), count=m)
        twin = R.RC2DGI(W, H, cascade_count=2)
        twin.paint("color", P[:m], (5, 5, 5, 255))
        assert status == [m, 0] and np.array_equal(got, twin.download("color")), m
        twin.close()
    ctx.close()


# ------------------------------------------------------------------ 6. no wait
def demo_words(R, W, H):
    from radiancecascade2dglobalillumination_amd import scenes

    cc, cp, ec, ep = scenes.demo_prims(W, H)
    return cc, to_words(R, cp), ec, to_words(R, ep)


def test_two_paints_and_a_frame_enqueue_behind_a_busy_device(R, torch):
    """On a torch stream given to rc2dgi_set_stream, behind a torch.cuda._sleep sized to three times what the
    synchronising twin's calls took on the host: paint COLOR, paint EMISSIVE (torch overwrites each list in place as
    soon as its call has returned), a frame, a read.  The event behind the sleep is unfinished after every call; the
    frame is the twin's."""
    from test_gpu_pipeline import sleep_cycles_per_ms

    W = H = 256
    cc, cw, ec, ew = demo_words(R, W, H)

    def run(ctx, lib, lists):
        out = torch.full((H, W, 4), -7.0, device="cuda")
        gi = torch.full(tuple(reversed(ctx.cascade_resolution)) + (4,), -7.0, device="cuda")
        st = torch.full((2, 2), -77, dtype=torch.int32, device="cuda")
        lib("paint_device color", lambda: ctx.paint_device("color", lists[0], cc, None, st[0]))
        lists[0].fill_(0x7FC00000)
        lib("paint_device emissive", lambda: ctx.paint_device("emissive", lists[1], ec, None, st[1]))
        lists[1].fill_(-1)
        lib("do", ctx.do_rc2dgi)
        lib("read_into color", lambda: ctx.read_into(out, "color"))
        lib("read_into final_gi", lambda: ctx.read_into(gi, "final_gi"))
        return out, gi, st

    def fresh(stream):
        ctx = R.RC2DGI(W, H, cascade_count=4)
        ctx.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            warm = torch.from_numpy(cw).to("cuda")
            ctx.paint_device("color", warm)  # the first call allocates the working memory: the one wait by design
            ctx.do_rc2dgi()                  # (the tables)
        ctx.sync()
        return ctx

    stream = torch.cuda.Stream()
    twin = fresh(stream)
    with torch.cuda.stream(stream):
        lists = [torch.from_numpy(cw).to("cuda"), torch.from_numpy(ew).to("cuda")]
        stream.synchronize()

        def stepwise(name, fn):
            fn()
            twin.sync()

        t0 = time.perf_counter()
        want = run(twin, stepwise, lists)
        twin.sync()
        twin_seconds = time.perf_counter() - t0
        want = [t.cpu().numpy() for t in want]
    twin.set_stream(None)
    twin.close()

    ctx = fresh(stream)
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

        got = run(ctx, lib, lists)
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


# ------------------------------------------------------------------ 7. a loop that never leaves the device
@pytest.mark.parametrize("storage", ["f32", "rgba8"])
def test_device_loop_equals_a_frame_of_the_restated_paintings(R, torch, storage):
    """torch makes discs on the device, pack_prims packs them, both inputs are painted and a frame runs, with no host
    synchronise between the steps; the merged COLOR equals that of a context given paint_ref's two images."""
    W = H = 128
    u8 = storage == "rgba8"
    stream = torch.cuda.Stream()
    ctx = R.RC2DGI(W, H, cascade_count=3, ray_range=2.0, storage=storage)
    ctx.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        g = torch.Generator(device="cuda")
        g.manual_seed(99)
        n = 24
        pos = torch.rand((n, 2), generator=g, device="cuda") * W
        rad = torch.rand((n, 1), generator=g, device="cuda") * 9 + 1
        xywh = torch.cat([pos, rad, torch.zeros((n, 1), device="cuda")], 1)
        kind = torch.ones(n, dtype=torch.int64, device="cuda")
        walls = torch.randint(0, 256, (n, 4), generator=g, device="cuda").to(torch.uint8)
        walls[:, 3] = 255
        lights = walls.clone()
        lights[::2] = 0  # every other disc is a wall that emits nothing
        lights[:, 3] = 255
        pc, pe = R.pack_prims(kind, xywh, walls), R.pack_prims(kind, xywh, lights)
        status = torch.zeros((2, 2), dtype=torch.int32, device="cuda")
        ctx.paint_device("color", pc, (0, 0, 0, 0), None, status[0])
        ctx.paint_device("emissive", pe, (0, 0, 0, 255), None, status[1])
        ctx.do_rc2dgi()
        out = torch.empty((H, W, 4), device="cuda")
        ctx.read_into(out, "color")
    ctx.sync()
    got = out.cpu().numpy()
    assert status.cpu().numpy().tolist() == [[n, 0], [n, 0]]
    pcs, pes = from_words(pc.cpu().numpy()), from_words(pe.cpu().numpy())
    assert all(p[0] == 1 and p[8] == 255 for p in pcs)
    ctx.set_stream(None)
    ctx.close()
    b = R.RC2DGI(W, H, cascade_count=3, ray_range=2.0, storage=storage)
    b.frame(paint_ref.paint(W, H, pcs, (0, 0, 0, 0), rgba8=u8), paint_ref.paint(W, H, pes, (0, 0, 0, 255), rgba8=u8))
    b.sync()
    want = b.download("color")
    b.close()
    assert np.array_equal(got.view(u32), want.view(u32)), differing(got, want)


def test_a_row_strip_shard_accepts_the_call(R, torch):
    W, H = 96, 64
    P = nine(W, H)
    ctx = R.RC2DGI(W, H, cascade_count=3)
    ctx.set_shard(1, 2)
    for which in ("color", "emissive"):
        got, status = paint_dev(torch, ctx, which, to_words(R, P), (4, 3, 2, 255))
        assert status == [9, 0]
        want = paint_ref.paint(W, H, P, (4, 3, 2, 255))
        assert np.array_equal(got, want), f"{which}: {differing(got, want)}"
    ctx.close()


# ------------------------------------------------------------------ 8. argument errors
def test_argument_errors_leave_the_texture(R, torch):
    W, H = 64, 48
    ctx = R.RC2DGI(W, H, cascade_count=2)
    start = np.broadcast_to(SENTINEL, (H, W, 4)).copy()
    for which in ("color", "emissive"):
        ctx.upload(which, start)
    L, h, vp = ctx._L, ctx._h, ctypes.c_void_p
    t = torch.from_numpy(to_words(R, nine(W, H))).to("cuda")
    cnt = torch.full((2,), 9, dtype=torch.int32, device="cuda")
    st = torch.full((4,), -77, dtype=torch.int32, device="cuda")
    clear = (ctypes.c_ubyte * 4)(255, 255, 255, 255)
    p, c, s = t.data_ptr(), cnt.data_ptr(), st.data_ptr()
    bad = [("a bad which", (R.RT["dist"], clear, vp(p), 9, vp(c), vp(s))),
           ("a bad which", (-1, clear, vp(p), 9, None, None)),
           ("n < 0", (0, clear, vp(p), -1, vp(c), vp(s))),
           ("n > 1 << 20", (0, clear, vp(p), (1 << 20) + 1, vp(c), vp(s))),
           ("a null list with n > 0", (1, clear, None, 9, vp(c), vp(s))),
           ("a misaligned list", (0, clear, vp(p + 2), 8, vp(c), vp(s))),
           ("a misaligned count", (1, clear, vp(p), 9, vp(c + 1), vp(s))),
           ("a misaligned status", (0, clear, vp(p), 9, vp(c), vp(s + 3)))]
    for what, args in bad:
        assert L.rc2dgi_paint_device(h, *args) == -1, what
        assert L.rc2dgi_last_error(h), what
    ctx.sync()
    assert st.cpu().numpy().tolist() == [-77] * 4, "a refused call writes no status"
    for which in ("color", "emissive"):
        assert np.array_equal(ctx.download(which).view(u32), start.view(u32)), which
    assert L.rc2dgi_paint_device(h, 0, None, None, 0, None, vp(s)) == 0  # n == 0 with a null list
    most = torch.zeros((1 << 20, 6), dtype=torch.int32, device="cuda")  # the largest n; the count says 9
    assert L.rc2dgi_paint_device(h, 0, None, vp(most.data_ptr()), 1 << 20, vp(c), vp(s + 8)) == 0
    ctx.sync()
    assert st.cpu().numpy().tolist() == [0, 0, 9, 0]
    with pytest.raises(TypeError):
        ctx.paint_device("color", t.cpu())
    with pytest.raises(TypeError):
        ctx.paint_device("color", t.to(torch.float32))
    with pytest.raises(ValueError):
        ctx.paint_device("color", t.reshape(-1, 9))
    with pytest.raises(ValueError):
        ctx.paint_device("color", t, status=st)
    ctx.close()
