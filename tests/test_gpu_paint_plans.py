"""GPU: rc2dgi_paint_device and rc2dgi_sprites_device on every plan of paint_dev_plan -- tiles of 64 x 4 .. 128 texels,
batches of 2048, 4096 and 8192 primitives -- bit for bit against the numpy restatements (oracle/paint_ref.py,
tests/sprites_ref.py).  The plan follows the texel count, and the restatement of the painter evaluates every triangle
over the whole frame, so the plans of the large screens are put on small ones with the tuning key "paint_plan"
(section 3 of this file's tests: the edge lists on all eighteen plans, the mask words at the top of a short batch, three
batches, sprites, a plan changed on a live context); two screens of 32768 columns then run the plans their own size
gives them, without the key.  There the sprites are held to the restatement, which is cheap at any size, and
rc2dgi_paint_device to rc2dgi_paint on a twin context: a cross-check of two paths of the library, the reference check
being the forced plans.

The edge lists are those of test_gpu_paint_device.py and test_gpu_sprites.py with, for every tile height at once, a
circle centre, a rectangle edge and a sprite's first and last row on the texel rows beside each tile cut: one list a
screen serves every plan, so a restatement is computed once a screen, order and storage and shared by the eighteen.

Left out: the plan of 8192 x 8192 (tile_h 16 with batch 4096) at its own size.  It begins at 42 M texels, 0.67 GB a
texture and more than a few seconds a test; its tile height and its batch run here under the key."""
import numpy as np
import pytest

import sprites_ref as S
import test_gpu_sprites as TS
from oracle import paint_ref
from test_gpu_paint_device import differing, edge_list, from_words, paint_dev, tile_rows, to_words

pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32
TILE_HS = (4, 8, 16, 32, 64, 128)
PLANS = [(t, b) for b in (1, 2, 4) for t in range(2, 8)]  # log2(tile_h), batch / 2048
PLAN_IDS = [f"{1 << t}x{2048 * b}" for t, b in PLANS]
CLEAR = (9, 8, 7, 200)


def code(t, b):
    return t | b << 8


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def R(torch):
    from radiancecascade2dglobalillumination_amd import rc2dgi

    return rc2dgi


def planned(R, W, H, t, b, storage="f32"):
    """a context whose device painters run the plan (t, b); the read-only keys report it"""
    ctx = R.RC2DGI(W, H, cascade_count=2, storage=storage)
    ctx.set_tuning("paint_plan", code(t, b))
    assert ctx.get_tuning("paint_plan") == code(t, b)
    assert (ctx.get_tuning("paint_tile_h"), ctx.get_tuning("paint_batch")) == (1 << t, 2048 * b)
    return ctx


def one_nan(x):
    """the uint32 view with every NaN mapped to one pattern (a NaN's payload is not part of the contract)"""
    v = np.ascontiguousarray(x, f32).view(u32).copy()
    v[np.isnan(x)] = 0x7FC00000
    return v


def same_bits(got, want):
    if got.dtype == np.uint8:
        return np.array_equal(got, want)
    return np.array_equal(one_nan(got), one_nan(want))


# ------------------------------------------------------------------ a. every plan paints the edge list
def plan_edge_list(W, H):
    return edge_list(W, H, 21, 12, TILE_HS)


_edge_refs = {}


def edge_ref(W, H, reverse, u8):
    """the restatement of the list (or of the list reversed), computed once and shared by the plans"""
    key = (W, H, reverse, u8)
    if key not in _edge_refs:
        P = plan_edge_list(W, H)
        _edge_refs[key] = paint_ref.paint(W, H, P[::-1] if reverse else P, CLEAR, rgba8=u8)
        _edge_refs[key].setflags(write=False)
    return _edge_refs[key]


def test_the_edge_list_meets_every_tile_cut():
    """(no device work) the list keeps the whole-target primitive and the 70 over one pixel, and has a circle centre
    and a rectangle edge on each row beside a cut of every tile height, from both ends; 150 = 128 + 22 gives the
    128-row tiles a partly covered last row, and 250 is no multiple of 8"""
    for W, H in ((333, 250), (200, 150)):
        P = plan_edge_list(W, H)
        assert len(P) == 300 and {p[0] for p in P} == {0, 1}
        assert sum(1 for p in P if p[0] == 0 and p[3] >= W and p[4] >= H) == 1
        assert sum(1 for p in P if p[0] == 0 and abs(p[1] - 37) <= 1 and abs(p[2] - 5) <= 1 and p[3] < 5) == 70
        rows = tile_rows(H, TILE_HS)
        for th in TILE_HS:
            last = (H - 1) // th * th  # the first texel row of the last tile row
            for g in (th - 1, th, th + 1, last - 1, last, last + 1):
                if 0 <= g < H:
                    assert H - 1 - g in rows and g in rows, (th, g)
        centres = {int(np.floor(p[2])) for p in P if p[0] == 1}
        edges = {int(p[2]) for p in P if p[0] == 0 and p[2] == int(p[2])}
        assert set(rows) <= centres and set(rows) <= edges
        assert {p[1] - 0.5 * (p[1] % 1 != 0) for p in P if p[0] == 1} >= {float(x) for x in range(0, W + 1, 64)}


@pytest.mark.parametrize("reverse", [False, True], ids=["listorder", "reversed"])
@pytest.mark.parametrize("storage", ["f32", "rgba8"])
@pytest.mark.parametrize("W,H", [(333, 250), (200, 150)])
@pytest.mark.parametrize("t,b", PLANS, ids=PLAN_IDS)
def test_every_plan_paints_the_edge_list(R, torch, t, b, W, H, storage, reverse):
    """(the two orders are two cases, so that the case that computes a restatement computes one)"""
    P = plan_edge_list(W, H)
    u8 = storage == "rgba8"
    ctx = planned(R, W, H, t, b, storage)
    _, status = paint_dev(torch, ctx, "color", to_words(R, P[::-1] if reverse else P), CLEAR)
    assert status == [300, 0]
    got = ctx.download("color", np.uint8) if u8 else ctx.download("color")
    want = edge_ref(W, H, reverse, u8)
    assert np.array_equal(got, want), f"{W}x{H} {storage} reversed={reverse}: {differing(got, want)}"
    if reverse:  # the two orders give different textures: the order is kept
        assert not np.array_equal(want, edge_ref(W, H, False, u8))
    assert ctx.get_tuning("paint_tile_h") == 1 << t and ctx.get_tuning("paint_batch") == 2048 * b
    ctx.close()


# ------------------------------------------------------------------ b. mask words at the top of a short batch
BW, BH = 200, 150
# (column, screen row): texel row 72 of column 100 is inside a tile of 16 and of 128 rows (and inside its 64 columns);
# texel row 147 lies in the last tile row of both heights, which the target covers in part (150 = 9 * 16 + 6 = 128 + 22)
B_PIXELS = [(100, BH - 1 - 72), (130, BH - 1 - 147)]


def short_batch_positions(batch):
    """the first and last bits of the first words, of the word at 2048 and of the last words of a batch's mask"""
    return sorted({0, 31, 32, 2047, batch - 33, batch - 32, batch - 1} | ({2048} if batch > 2048 else set()))


def off_target(rng, n, W, H):
    """n (x, y) positions at least 40 pixels off a W x H target, on every side"""
    side = rng.integers(0, 4, n)
    x = np.where(side == 0, -60 - rng.integers(0, 500, n), np.where(side == 1, W + 40 + rng.integers(0, 500, n),
                                                                      rng.integers(-50, W + 50, n)))
    y = np.where(side == 2, -60 - rng.integers(0, 500, n), np.where(side == 3, H + 40 + rng.integers(0, 500, n),
                                                                      rng.integers(-50, H + 50, n)))
    return x, y


@pytest.mark.parametrize("storage", ["f32", "rgba8"])
@pytest.mark.parametrize("t", [4, 7], ids=["tile16", "tile128"])
@pytest.mark.parametrize("b", [1, 2], ids=["batch2048", "batch4096"])
def test_mask_words_at_the_top_of_a_short_batch(R, torch, b, t, storage):
    """A list of exactly one batch of 2048 or 4096, whose mask is 64 or 128 words: a lane's upper words stay zero and
    are not zeroed back into the next tile's mask.  Every primitive lies off the target but those at the positions of
    short_batch_positions, which cover one pixel: a first call puts them on the pixel inside a tile, a second (no clear:
    the masks were left clean) on the pixel in the last tile row."""
    batch = 2048 * b
    rng = np.random.default_rng(31 + b)
    x, y = off_target(rng, batch, BW, BH)
    rgba = rng.integers(0, 256, (batch, 4))
    rgba[:, 3] = rng.integers(60, 200, batch)
    pos = short_batch_positions(batch)
    u8 = storage == "rgba8"
    ctx = planned(R, BW, BH, t, b, storage)
    want = None
    for call, (px, py) in enumerate(B_PIXELS):
        P = [(k % 2, float(x[k]), float(y[k]), 9.0, 9.0) + tuple(int(v) for v in rgba[k]) for k in range(batch)]
        for k in pos:
            P[k] = (0, px + 0.25, py + 0.25, 0.5, 0.5) + P[k][5:]
        _, status = paint_dev(torch, ctx, "emissive", to_words(R, P), CLEAR if call == 0 else None)
        assert status == [batch, 0]
        want = paint_ref.paint(BW, BH, [P[k] for k in pos], CLEAR if call == 0 else None, base=want, rgba8=u8)
        got = ctx.download("emissive", np.uint8) if u8 else ctx.download("emissive")
        assert np.array_equal(got, want), f"call {call}: {differing(got, want)}"
        clear = np.array(CLEAR, np.uint8) if u8 else (np.array(CLEAR, f32) / f32(255))
        changed = np.argwhere(np.any(want != clear, axis=-1)).tolist()
        assert changed == sorted([BH - 1 - Y, X] for X, Y in B_PIXELS[:call + 1]), "one pixel a call"
    ctx.close()


# ------------------------------------------------------------------ c. batches
CW, CH = 64, 48
C_CLEAR = (5, 5, 5, 255)


def three_batches(batch):
    """test_gpu_paint_device's three-batch list at this batch size: n = 2 * batch + 3 small rectangles, and circles
    straddling both batch boundaries over the same pixels"""
    n = 2 * batch + 3
    rng = np.random.default_rng(8)
    kind = np.zeros(n, np.int32)
    xywh = np.stack([rng.uniform(-2, CW, n), rng.uniform(-2, CH, n), rng.uniform(0.5, 3, n), rng.uniform(0.5, 3, n)],
                    1).astype(f32)
    rgba = rng.integers(0, 256, (n, 4)).astype(np.uint8)
    rgba[:, 3] = rng.integers(30, 220, n)
    for bd in (batch, 2 * batch):
        for k in range(bd - 3, bd + 3):
            kind[k] = 1
            xywh[k] = [20.0 + (k - bd), 24.0, 9.0, 0.0]
    return np.concatenate([kind[:, None], xywh.view(np.int32), rgba.view(np.int32)], 1)


_batch_refs = {}


def batch_refs(batch):
    """the restatement of the first `batch`, 2 * batch + 1 and all primitives, each painted over the one before;
    computed once a batch size and shared by the tile heights"""
    if batch not in _batch_refs:
        P = from_words(three_batches(batch))
        cuts = [0, batch - 1, batch, 2 * batch + 1, len(P)]
        refs, img = {}, None
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            img = paint_ref.paint(CW, CH, P[lo:hi], C_CLEAR if lo == 0 else None, base=img)
            img.setflags(write=False)
            refs[hi] = img
        _batch_refs[batch] = refs
    return _batch_refs[batch]


@pytest.mark.parametrize("t", [2, 5], ids=["tile4", "tile32"])
@pytest.mark.parametrize("b", [1, 2], ids=["batch2048", "batch4096"])
def test_three_batches_keep_the_draw_order_and_leave_the_masks_clean(R, torch, b, t):
    batch = 2048 * b
    words = three_batches(batch)
    n = len(words)
    refs = batch_refs(batch)
    # (the last primitive of the first batch matters to the result)
    assert not np.array_equal(refs[batch - 1], refs[batch])
    ctx = planned(R, CW, CH, t, b)
    # the whole list, the count cutting inside the third batch, the count at a batch boundary
    for m, count in ((n, None), (2 * batch + 1, 2 * batch + 1), (batch, batch)):
        got, status = paint_dev(torch, ctx, "color", words, C_CLEAR, count)
        assert status == [m, 0]
        assert np.array_equal(got, refs[m]), f"count {count}: {differing(got, refs[m])}"
    # a following call whose list lies wholly off the target, without a clear, finds the masks clean: no bit is left
    # that would draw a primitive of the last batch over the texture again
    off = words.copy()
    off[:, 1] = (off[:, 1].view(f32) + f32(CW + 40)).view(np.int32)
    before = ctx.download("color")
    got, status = paint_dev(torch, ctx, "color", off, None)
    assert status == [n, 0]
    assert np.array_equal(got.view(u32), before.view(u32)), differing(got, before)
    ctx.close()


# ------------------------------------------------------------------ d. sprites on every plan
SW, SH = 200, 150
PAIRS = [("f32", "uint8"), ("rgba8", "float16")]


def plan_sprites(a):
    return TS.edge_list(SW, SH, a.shape[1], a.shape[0], 21, tile_rows(SH, TILE_HS))


_sprite_refs = {}


def sprite_case(R, storage, fmt, reverse):
    """(atlas, words, start texels, restated texels) of the sprite list in one order: in list order over the uploaded
    texture, reversed under a clear.  Computed once a storage / format pair and shared by the plans."""
    key = (storage, fmt, reverse)
    if key not in _sprite_refs:
        u8 = storage == "rgba8"
        a = TS.big_atlas_np(fmt, SW, SH)
        P = plan_sprites(a)
        wd = S.words(P[::-1] if reverse else P)
        start = TS.texture_of_upload(R, SW, SH, storage)
        want = S.draw(start, a, wd, u8, CLEAR if reverse else None)
        want.setflags(write=False)
        _sprite_refs[key] = (a, wd, want)
    return _sprite_refs[key]


def test_the_sprite_list_meets_every_tile_cut():
    a = TS.big_atlas_np("uint8", SW, SH)
    P = plan_sprites(a)
    assert len(P) == 300 and {p[7] for p in P} == set(range(8))
    assert sum(1 for p in P if p[2] >= SW and p[3] >= SH) == 1                       # one over the whole target
    assert sum(1 for p in P if p[4] + p[2] <= 0 or p[4] >= SW or p[5] + p[3] <= 0 or p[5] >= SH) >= 8  # off it
    rows = set(tile_rows(SH, TILE_HS))
    assert rows <= {p[5] for p in P} and rows <= {p[5] + p[3] - 1 for p in P}


@pytest.mark.parametrize("storage,fmt", PAIRS)
@pytest.mark.parametrize("t,b", PLANS, ids=PLAN_IDS)
def test_every_plan_draws_the_sprite_list_in_both_orders(R, torch, t, b, storage, fmt):
    u8 = storage == "rgba8"
    ctx = planned(R, SW, SH, t, b, storage)
    outs = []
    for reverse in (False, True):
        a, wd, want = sprite_case(R, storage, fmt, reverse)
        at = TS.to_dev(torch, a, 6)
        ctx.upload("color", TS.base_texture(SW, SH))
        assert TS.draw(torch, ctx, "color", at, wd, CLEAR if reverse else None) == [300, 0]
        got = TS.texture(ctx, "color", u8)
        assert same_bits(got, want), f"{storage} {fmt} reversed={reverse}: {differing(got, want)}"
        outs.append(got)
    assert not np.array_equal(outs[0], outs[1])
    ctx.close()


@pytest.mark.parametrize("storage,fmt", PAIRS)
@pytest.mark.parametrize("t", [4, 7], ids=["tile16", "tile128"])
@pytest.mark.parametrize("b", [1, 2], ids=["batch2048", "batch4096"])
def test_sprite_mask_words_at_the_top_of_a_short_batch(R, torch, b, t, storage, fmt):
    """test_mask_words_at_the_top_of_a_short_batch with 1 x 1 sprites: the records the binning reads are laid over
    PaintPrim, the masks are the same"""
    batch = 2048 * b
    rng = np.random.default_rng(41 + b)
    a = TS.atlas_np(fmt)
    at = TS.to_dev(torch, a)
    x, y = off_target(rng, batch, BW, BH)
    pos = short_batch_positions(batch)
    u8 = storage == "rgba8"
    ctx = planned(R, BW, BH, t, b, storage)
    ctx.upload("emissive", TS.base_texture(BW, BH))
    want = start = TS.texture(ctx, "emissive", u8)
    for call, (px, py) in enumerate(B_PIXELS):
        P = [(int(rng.integers(0, TS.AW - 3)), int(rng.integers(0, TS.AH - 3)), 1 + k % 3, 1 + k % 2, int(x[k]), int(y[k]),
              TS.rand_tint(rng), k % 4) for k in range(batch)]
        for k in pos:
            P[k] = P[k][:2] + (1, 1, px, py) + P[k][6:]
        wd = S.words(P)
        assert TS.draw(torch, ctx, "emissive", at, wd) == [batch, 0]
        want = S.draw(want, a, wd[pos], u8)
        got = TS.texture(ctx, "emissive", u8)
        assert same_bits(got, want), f"call {call}: {differing(got, want)}"
        changed = np.argwhere(np.any(one_nan(want) != one_nan(start), axis=-1) if not u8 else
                              np.any(want != start, axis=-1)).tolist()
        assert changed == sorted([BH - 1 - Y, X] for X, Y in B_PIXELS[:call + 1]), "one pixel a call"
    ctx.close()


# ------------------------------------------------------------------ e. changing the plan on a live context
def test_the_plan_changes_on_a_live_context(R, torch):
    """One context on a torch stream: paint under 8-row tiles and batches of 8192, set 64-row tiles and batches of 2048
    with the painting still in flight, draw sprites, paint again, go back to plan 0 and paint.  No step waits but the
    sets that change the plan (the working memory is laid out by it) and the allocation that follows each; every
    step's texture is copied on the stream and compared when all are enqueued."""
    W, H = SW, SH
    P = plan_edge_list(W, H)
    a = TS.big_atlas_np("uint8", W, H)
    wd = S.words(plan_sprites(a))
    tail = P[::-1][:60]
    stream = torch.cuda.Stream()
    ctx = R.RC2DGI(W, H, cascade_count=2)
    ctx.set_stream(stream.cuda_stream)
    snaps, plans, keep = [], [], []

    def step(fn):
        fn()
        snaps.append(torch.full((H, W, 4), -7.0, device="cuda"))
        ctx.read_into(snaps[-1], "emissive")
        plans.append((ctx.get_tuning("paint_tile_h"), ctx.get_tuning("paint_batch")))

    def paint(prims, clear):
        keep.append(torch.from_numpy(to_words(R, prims)).to("cuda"))
        keep.append(torch.full((2,), -77, dtype=torch.int32, device="cuda"))
        ctx.paint_device("emissive", keep[-2], clear, None, keep[-1])

    def sprites():
        keep.append(TS.to_dev(torch, a, 6))
        keep.append(torch.from_numpy(wd).to("cuda"))
        keep.append(torch.full((2,), -77, dtype=torch.int32, device="cuda"))
        ctx.sprites_device("emissive", keep[-3], keep[-2], None, None, keep[-1])

    with torch.cuda.stream(stream):
        ctx.set_tuning("paint_plan", code(3, 4))  # (no working memory yet: nothing to free)
        step(lambda: paint(P, CLEAR))
        ctx.set_tuning("paint_plan", code(6, 1))  # another tile height and another batch: the masks are laid out anew
        step(sprites)
        step(lambda: paint(tail, None))
        ctx.set_tuning("paint_plan", code(6, 1))  # (the plan in force: nothing changes, nothing waits)
        step(lambda: paint(tail, None))
        ctx.set_tuning("paint_plan", 0)
        step(lambda: paint(P, CLEAR))
    ctx.sync()
    assert plans == [(8, 8192), (64, 2048), (64, 2048), (64, 2048), (4, 8192)]
    assert [t.cpu().numpy().tolist() for t in keep if t.dtype == torch.int32 and t.numel() == 2] == \
        [[300, 0], [300, 0], [60, 0], [60, 0], [300, 0]]
    want = [edge_ref(W, H, False, False)]
    want.append(S.draw(want[0], a, wd, False))
    want.append(paint_ref.paint(W, H, tail, None, base=want[1]))
    want.append(paint_ref.paint(W, H, tail, None, base=want[2]))
    want.append(want[0])
    for k, (t, w) in enumerate(zip(snaps, want)):
        got = t.cpu().numpy()
        assert same_bits(got, w), f"step {k}: {differing(got, w)}"
    assert not same_bits(want[2], want[3])
    # the default plan's result: a context that never saw the key
    fresh = R.RC2DGI(W, H, cascade_count=2)
    got, _ = paint_dev(torch, fresh, "emissive", to_words(R, P), CLEAR)
    assert np.array_equal(got.view(u32), snaps[4].cpu().numpy().view(u32))
    fresh.close()
    ctx.set_stream(None)
    ctx.close()


def test_values_that_are_no_plan_are_refused_and_change_nothing(R, torch):
    ctx = planned(R, 64, 48, 5, 2)
    for v in (1, 7, -1, 1 | 1 << 8, 8 | 1 << 8, 2 | 3 << 8, 2 | 8 << 8, 2 << 8, 2 | 1 << 8 | 1 << 16, -(1 << 31)):
        with pytest.raises(R.RC2DGIError) as ei:
            ctx.set_tuning("paint_plan", v)
        assert ei.value.code == -1, v
        assert ctx.get_tuning("paint_plan") == code(5, 2)
        assert (ctx.get_tuning("paint_tile_h"), ctx.get_tuning("paint_batch")) == (32, 4096)
    for key in ("paint_tile_h", "paint_batch"):  # state, not knobs
        with pytest.raises(R.RC2DGIError):
            ctx.set_tuning(key, 8)
    ctx.close()


# ------------------------------------------------------------------ the plans two large screens take by themselves
NATURAL = [(32768, 324, 8, 8192),   # the smallest height of 32768 columns with 8-row tiles; its last tile row has 4 rows
           (32768, 644, 16, 8192)]  # the smallest with 16-row tiles; its last tile row has 4 rows
NATURAL_IDS = [f"{W}x{H}" for W, H, _, _ in NATURAL]


def natural_ctx(R, W, H, tile_h, batch):
    """cascades of 1 / 64 of the screen: the cascade textures stay small"""
    ctx = R.RC2DGI(W, H, cascade_count=2, render_scale=1.0 / 64.0)
    assert ctx.get_tuning("paint_plan") == 0
    assert (ctx.get_tuning("paint_tile_h"), ctx.get_tuning("paint_batch")) == (tile_h, batch)
    assert R.paint_device_limits(W, H)[0] == batch
    return ctx


def corner_spots(W, H, tile_h):
    """(column, screen row) of texels at tile corners: the first and last columns of tile columns near both ends and in
    the middle of the target, the far right columns, and the rows beside the cuts of the tile rows, the last one too"""
    xs = [0, 63, 64, 127, W // 2 - 1, W // 2, W - 129, W - 65, W - 64, W - 2, W - 1]
    last = (H - 1) // tile_h * tile_h
    gs = sorted({0, tile_h - 1, tile_h, tile_h + 1, 5 * tile_h - 1, 5 * tile_h, last - 1, last, last + 1, H - 1})
    return [(x, H - 1 - g) for x in xs for g in gs]


@pytest.mark.parametrize("W,H,tile_h,batch", NATURAL, ids=NATURAL_IDS)
def test_sprites_on_the_plan_a_large_screen_takes(R, torch, W, H, tile_h, batch):
    rng = np.random.default_rng(H)
    a = TS.atlas_np("uint8")
    at = TS.to_dev(torch, a)
    P = []
    for k, (x, Y) in enumerate(corner_spots(W, H, tile_h)):  # a corner of the sprite on the spot, by turns
        w, h = int(rng.integers(1, 30)), int(rng.integers(1, 24))
        dx, dy = (x, x - w + 1)[k % 2], (Y, Y - h + 1)[k // 2 % 2]
        P.append((int(rng.integers(0, TS.AW - w + 1)), int(rng.integers(0, TS.AH - h + 1)), w, h, dx, dy, TS.rand_tint(rng),
                  k % 8))
    while len(P) < 300:
        w, h = int(rng.integers(1, 38)), int(rng.integers(1, 30))
        P.append((int(rng.integers(0, TS.AW - w + 1)), int(rng.integers(0, TS.AH - h + 1)), w, h,
                  int(rng.integers(-20, W)), int(rng.integers(-20, H)), TS.rand_tint(rng), len(P) % 8))
    wd = S.words([P[k] for k in rng.permutation(len(P))])
    ctx = natural_ctx(R, W, H, tile_h, batch)
    assert TS.draw(torch, ctx, "emissive", at, wd, CLEAR) == [300, 0]
    got = ctx.download("emissive")
    want = S.draw(np.zeros((H, W, 4), f32), a, wd, False, CLEAR)
    assert same_bits(got, want), differing(got, want)
    # the plan with 4-row tiles would take more than 40 MiB of masks on this screen: refused, nothing changed
    with pytest.raises(R.RC2DGIError) as ei:
        ctx.set_tuning("paint_plan", code(2, 4))
    assert ei.value.code == -1
    assert ctx.get_tuning("paint_plan") == 0 and ctx.get_tuning("paint_tile_h") == tile_h
    ctx.close()


@pytest.mark.parametrize("W,H,tile_h,batch", NATURAL, ids=NATURAL_IDS)
def test_the_two_painters_agree_on_the_plan_a_large_screen_takes(R, torch, W, H, tile_h, batch):
    """rc2dgi_paint_device against rc2dgi_paint on a twin context, 300 primitives: a cross-check of two paths of the
    library (the restatement evaluates every triangle over the whole frame: too slow at 10 M texels and more).  The
    check against the restatement is the forced plans' above."""
    rng = np.random.default_rng(H + 1)
    col = lambda: tuple(int(v) for v in rng.integers(0, 256, 3)) + (int(rng.integers(1, 255)),)  # noqa: E731
    P = [(0, -3.0, -2.0, float(W + 9), float(H + 7)) + col()]  # the whole target
    for k, (x, Y) in enumerate(corner_spots(W, H, tile_h)):
        if k % 2:
            P.append((1, x + 0.5 * (k % 4 // 2), Y + 0.5 * (k % 8 // 4), float(rng.uniform(0.4, 9.0)), 0.0) + col())
        else:
            P.append((0, float(x) - 3.0 * (k % 4 // 2), float(Y), float(rng.uniform(2, 70)),
                      float(rng.uniform(1, 2 * tile_h)) * (1 - k % 8 // 4 * 2)) + col())
    while len(P) < 300:
        P.append((0, float(rng.uniform(-20, W)), float(rng.uniform(-20, H)), float(rng.uniform(-6, 300)),
                  float(rng.uniform(-6, 60))) + col())
    P = [P[k] for k in rng.permutation(len(P))]
    ctx = natural_ctx(R, W, H, tile_h, batch)
    got, status = paint_dev(torch, ctx, "emissive", to_words(R, P), CLEAR)
    ctx.close()
    assert status == [300, 0]
    twin = R.RC2DGI(W, H, cascade_count=2, render_scale=1.0 / 64.0)
    twin.paint("emissive", P, CLEAR)
    want = twin.download("emissive")
    twin.close()
    assert np.array_equal(got.view(u32), want.view(u32)), differing(got, want)
    assert np.count_nonzero(np.any(got != got[0, 0], axis=-1)) > 10000
