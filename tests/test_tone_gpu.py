"""GPU: toned views (rc2dgi_set_curve / rc2dgi_compose_tone) and histograms of rectangles (rc2dgi_histogram), include/
rc2dgi.h, against tests/tone_ref.c: the header's semantics restated in C over the `download` of the same textures, bin()
a linear scan.  Every comparison is exact equality: bytes of the window, 32-bit words of the records."""
import ctypes

import numpy as np
import pytest

from test_reduce_cpu import gpu_texture
from test_reduce_gpu import PLAN_FIFTH, PLAN_RECTS, build_rect_plan, demo_context, plan_context, planned, sprite_rects
from test_tone_cpu import INVALID, build_tone_ref, log_table, ref_compose, ref_hist, tone_curves

pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32
STORAGES = ["f32", "f16", "rgba8"]
ALL_RTS = ["color", "emissive", "jump1", "jump2", "dist", "gi1", "gi2", "temp", "blur", "final_gi"]
LINEAR_RTS = ("gi1", "gi2", "blur", "final_gi")
POINT, LINEAR = 1, 2
NONE = (0, 0, 0, 0)
RED = (230, 41, 55, 255)
E_ARG, E_UNSUPPORTED, E_STATE, E_DEVICE = -1, -5, -6, -7
SLOTS = {"q8": 1, "srgb": 2, "reinhard": 3, "odd": 4}   # the curve slots the contexts below set
EXPOSURES = [0.0, 0.125, 3.7, 255.0]
CHANNELS = ["r", "g", "b", "a", "luma"]


@pytest.fixture(scope="module")
def R():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from radiancecascade2dglobalillumination_amd import rc2dgi

    return rc2dgi


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return build_tone_ref(tmp_path_factory)


def set_curves(ctx):
    for name, slot in SLOTS.items():
        ctx.set_curve(slot, tone_curves()[name])


def slot_tables():
    return {slot: tone_curves()[name] for name, slot in SLOTS.items()}


class Downloads:
    """The textures of a context as rc2dgi_download returns them, fetched once each."""

    def __init__(self, ctx):
        self.ctx, self.f, self.b = ctx, {}, {}

    def floats(self, name):
        if name not in self.f:
            self.f[name] = np.ascontiguousarray(self.ctx.download(name, np.float32))
        return self.f[name]

    def bytes(self, name):
        if name not in self.b:
            self.b[name] = np.ascontiguousarray(self.ctx.download(name, np.uint8))
        return self.b[name]


def reference(ref_lib, dl, views, tones, size, clear=(0, 0, 0, 255)):
    """views: (name, x, y, w, h, filter, border) with filter 0 (the texture's own) / POINT / LINEAR; tones: (exposure,
    curve slot) a view, or None for the untoned frame."""
    names = sorted({v[0] for v in views})
    u8 = dl.ctx.storage == "rgba8"
    tex = [(dl.floats(n), dl.bytes(n) if u8 and n in LINEAR_RTS else None) for n in names]
    tones = tones or [(1.0, 0)] * len(views)
    rv = []
    for (name, x, y, w, h, filt, border), (e, c) in zip(views, tones):
        linear = filt == LINEAR or (filt == 0 and name in LINEAR_RTS)
        rv.append((names.index(name), x, y, w, h, (2 if u8 else 1) if linear else 0, border, e, c))
    return ref_compose(ref_lib, tex, rv, slot_tables(), size, clear)


def same_image(got, want, what):
    bad = np.any(got != want, axis=-1)
    where = np.argwhere(bad)[:4].tolist()
    assert np.array_equal(got, want), f"{what}: {np.count_nonzero(bad)} pixels differ, first at (row, col) {where}"


def same_records(got, want, what, rects=None):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(1))
    if len(bad):
        k = int(bad[0])
        cols = np.flatnonzero(got[k] != want[k])[:6]
        where = "" if rects is None else f" rectangle {np.asarray(rects).reshape(-1, 4)[k].tolist()}"
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} records differ, first {k}{where}: words {cols.tolist()} "
                             f"got {got[k, cols].tolist()} want {want[k, cols].tolist()}")


def layout_views(R, W, H):
    names = {v: k for k, v in R.RT.items()}
    return [(names[v.which], v.x, v.y, v.w, v.h, v.filter, (v.r, v.g, v.b, v.a)) for v in R.display_layout(W, H)]


# ------------------------------------------------------------------ 1: identity, and every texture toned
@pytest.fixture(scope="module", params=STORAGES)
def small(R, request):
    ctx, _, _ = demo_context(R, 96, 80, 2, 0.5, request.param)
    assert ctx.cascade_resolution == (48, 40)
    set_curves(ctx)
    yield ctx, Downloads(ctx)
    ctx.close()


def test_identity_tones_are_the_untoned_frame(R, ref_lib, small):
    ctx, dl = small
    views = layout_views(R, 96, 80) + [("final_gi", 3, 5, 70, 50, LINEAR, NONE), ("final_gi", 40, 33, 31, 17, LINEAR, RED)]
    assert len(views) == 10
    want = ctx.compose(views)
    same_image(want, reference(ref_lib, dl, views, None, (96, 80)), f"{ctx.storage} rc2dgi_compose against the reference")
    same_image(ctx.compose(views, tones=None), want, "tones = None")
    same_image(ctx.compose(views, tones=[(1.0, 0)] * 10), want, "every tone {1, 0}")
    same_image(ctx.compose(views, tones=[(1.0, SLOTS["q8"])] * 10), want, "every tone {1, the q8 table}")
    same_image(ctx.compose(views, tones=[(1.0, SLOTS["q8"] if k % 2 else 0) for k in range(10)]), want, "mixed")
    assert len(np.unique(want.reshape(-1, 4), axis=0)) > 50


def texture_views():
    """the ten textures as POINT thumbnails and the four filtered ones LINEAR too, over a 200 x 120 window, some
    overlapping, one bordered, two hanging over the edge"""
    views = []
    for k, name in enumerate(ALL_RTS):
        views.append((name, 3 + 38 * (k % 5), 2 + 56 * (k // 5), 45, 50, POINT, RED if k == 3 else NONE))
    for k, name in enumerate(LINEAR_RTS):
        views.append((name, -9 + 52 * k, 70 + 3 * k, 61, 47, LINEAR, NONE))
    return views


@pytest.mark.parametrize("exposure", EXPOSURES)
def test_every_texture_toned(R, ref_lib, small, exposure):
    ctx, dl = small
    views = texture_views()
    for name, slot in [("none", 0)] + list(SLOTS.items()):
        tones = [(exposure, slot)] * len(views)
        got = ctx.compose(views, size=(200, 120), clear=(40, 90, 200, 120), tones=tones)
        same_image(got, reference(ref_lib, dl, views, tones, (200, 120), (40, 90, 200, 120)),
                   f"{ctx.storage} exposure {exposure} curve {name}")
    # overlapping views, each with its own tone
    mixed = [(EXPOSURES[k % 4], (k * 3) % 5) for k in range(len(views))]
    got = ctx.compose(views, size=(200, 120), tones=mixed)
    same_image(got, reference(ref_lib, dl, views, mixed, (200, 120)), f"{ctx.storage} mixed tones")


def test_exposure_shows_on_the_final_gi(R, ref_lib, small):
    """The condition of the toned tests: at exposure 3.7 the reference's image of FINAL_GI differs from its untoned
    image in every view -- otherwise the scene would be too dark to tell a tone from none."""
    ctx, dl = small
    views = [("final_gi", 0, 0, 48, 40, POINT, NONE), ("final_gi", 50, 0, 48, 40, LINEAR, NONE),
             ("final_gi", 100, 0, 90, 70, LINEAR, NONE), ("final_gi", 0, 72, 33, 21, POINT, NONE)]
    plain = reference(ref_lib, dl, views, None, (200, 120))
    for name, slot in [("none", 0)] + list(SLOTS.items()):
        tones = [(3.7, slot)] * 4
        toned = reference(ref_lib, dl, views, tones, (200, 120))
        for (_, x, y, w, h, _, _) in views:
            assert (toned[y:y + h, x:x + w] != plain[y:y + h, x:x + w]).any(), (ctx.storage, name, x, y)
        same_image(ctx.compose(views, size=(200, 120), tones=tones), toned, f"{ctx.storage} final_gi at 3.7, curve {name}")


# ------------------------------------------------------------------ 2: the toned 1:1 blit
@pytest.fixture(scope="module", params=["f32", "rgba8"])
def display(R, request):
    ctx, _, _ = demo_context(R, 322, 203, 3, 0.5, request.param)
    set_curves(ctx)
    yield ctx, Downloads(ctx)
    ctx.close()


def test_toned_blit_crossed_by_a_thumbnail_and_cut_by_the_window(R, ref_lib, display):
    ctx, dl = display
    W, H = 322, 203
    views = layout_views(R, W, H)
    tones = [(3.7, SLOTS["srgb"])] + [(0.125 * (k + 1), k % 5) for k in range(7)]
    same_image(ctx.compose(views, tones=tones), reference(ref_lib, dl, views, tones, (W, H)), f"{ctx.storage} display")
    # the window's right edge cuts the 1:1 blit at every width where a wave's last lanes fall differently; a thumbnail
    # crosses the rows 10 .. 29 (the waves there walk the views per pixel), the others are the plain blit
    cross = [("color", 0, 0, W, H, 0, NONE), ("gi1", -5, 10, 300, 20, 0, RED)]
    ct = [(3.7, SLOTS["reinhard"]), (2.0, SLOTS["srgb"])]
    for w in list(range(1, 10)) + list(range(253, 261)):
        got = ctx.compose(cross, size=(w, 40), tones=ct)
        same_image(got, reference(ref_lib, dl, cross, ct, (w, 40)), f"{ctx.storage} out width {w}")
    # a 1:1 view hanging over the top left corner, toned, under a smaller window
    over = [("emissive", -37, -21, W, H, 0, NONE), ("color", 100, 50, W, H, 0, RED)]
    ot = [(255.0, SLOTS["odd"]), (0.125, SLOTS["q8"])]
    same_image(ctx.compose(over, size=(W - 101, H - 57), tones=ot),
               reference(ref_lib, dl, over, ot, (W - 101, H - 57)), f"{ctx.storage} overhang")


def test_set_curve_is_ordered_on_the_stream(R, ref_lib, display):
    import torch

    ctx, dl = display
    W, H = 322, 203
    views = layout_views(R, W, H)[:3]
    tones = [(3.7, 5), (1.0, 0), (2.0, 5)]
    a = torch.full((H, W, 4), 0xA5, dtype=torch.uint8, device="cuda")
    b = torch.full((H, W, 4), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.set_curve(5, tone_curves()["srgb"])
    ctx.compose_into(a, views, tones=tones)
    ctx.set_curve(5, tone_curves()["reinhard"])   # no sync between the four calls
    ctx.compose_into(b, views, tones=tones)
    ctx.sync()
    old = [(e, SLOTS["srgb"] if c else 0) for e, c in tones]
    new = [(e, SLOTS["reinhard"] if c else 0) for e, c in tones]
    want_a, want_b = reference(ref_lib, dl, views, old, (W, H)), reference(ref_lib, dl, views, new, (W, H))
    assert not np.array_equal(want_a, want_b)
    same_image(a.cpu().numpy(), want_a, "the compose enqueued before set_curve keeps the old curve")
    same_image(b.cpu().numpy(), want_b, "the compose enqueued after it uses the new one")
    ctx.set_curve(5, None)
    with pytest.raises(R.RC2DGIError) as ei:
        ctx.compose(views, tones=tones)
    assert ei.value.code == E_STATE


# ------------------------------------------------------------------ 3: wild values through every curve
def wild_context(R, W, H, specials=True):
    """f32, one cascade, no frame: COLOR is the uploaded values of tests/test_reduce_cpu.py's generator"""
    ctx = R.RC2DGI(W, H, cascade_count=1, storage="f32")
    v = gpu_texture(W, H, specials)
    ctx.upload("color", v)
    tex = ctx.download("color")
    bits = tex.view(u32)
    assert np.array_equal(bits, v.view(u32)), "an f32 upload is stored as it is"
    if specials:
        assert np.isnan(tex).any() and np.isinf(tex).any() and (bits == 0x80000000).any() and (bits == 0x7F7FFFFF).any()
        assert ((bits & 0x7F800000) == 0).any() and (bits == 1).any(), "subnormals reach the texture"
    return ctx, tex


@pytest.fixture(scope="module", params=[True, False], ids=["specials", "finite"])
def wide(R, request):
    ctx, tex = wild_context(R, 2051, 9, request.param)
    set_curves(ctx)
    yield ctx, tex, request.param
    ctx.close()


@pytest.fixture(scope="module", params=[True, False], ids=["specials", "finite"])
def tall(R, request):
    ctx, tex = wild_context(R, 9, 2051, request.param)
    yield ctx, tex, request.param
    ctx.close()


def test_wild_values_through_every_curve(R, ref_lib, wide):
    ctx, tex, specials = wide   # (with the specials NaN, +-inf, -0.0, FLT_MAX and subnormals reach T; without, none)
    dl = Downloads(ctx)
    views = [("color", 0, 0, 2051, 9, POINT, NONE)]
    for name, slot in [("none", 0)] + list(SLOTS.items()):
        for e in (1.0, 3.7, 0.0):
            got = ctx.compose(views, tones=[(e, slot)])
            same_image(got, reference(ref_lib, dl, views, [(e, slot)], (2051, 9)), f"wild values, curve {name}, exposure {e}")
    # scaled, so that the per-pixel walk tones them too
    thumb = [("color", 0, 0, 700, 7, POINT, NONE)]
    got = ctx.compose(thumb, size=(700, 7), tones=[(1.0, SLOTS["odd"])])
    same_image(got, reference(ref_lib, dl, thumb, [(1.0, SLOTS["odd"])], (700, 7)), "wild values, scaled")


# ------------------------------------------------------------------ 4: histograms -- the decode
@pytest.mark.parametrize("name", ALL_RTS)
def test_histogram_of_every_texture_and_channel(R, ref_lib, small, name):
    ctx, dl = small
    tex = dl.floats(name)
    ny, nx = tex.shape[:2]
    edges = tone_curves()["q8"]
    ys, xs = np.mgrid[ny - 16:ny, nx - 16:nx]
    ones = np.stack([xs.ravel(), ys.ravel(), np.ones(256, int), np.ones(256, int)], 1)
    for ci, ch in enumerate(CHANNELS):
        whole = ctx.histogram(name, edges, ch)   # rects = None: the whole texture
        same_records(whole, ref_hist(ref_lib, tex, ci, [[0, 0, nx, ny]], edges), f"{ctx.storage} {name} {ch} whole")
        assert whole[0, 0] == 0 and whole[0, 1] == nx * ny and whole[0, 2:].sum() == nx * ny
        got = ctx.histogram(name, edges, ch, ones)
        same_records(got, ref_hist(ref_lib, tex, ci, ones, edges), f"{ctx.storage} {name} {ch} 1 x 1", ones)
        assert (got[:, 1] == 1).all() and (got[:, 2:].sum(1) == 1).all() and (got[:, 2:].max(1) == 1).all()


# ------------------------------------------------------------------ 5: histograms -- shapes and edge tables
def own_table(tex, channel, seed):
    """1023 edges drawn from the texture's own finite values of a channel, so that e == v happens"""
    v = tex[..., channel].reshape(-1)
    v = v[np.isfinite(v)]
    e = np.sort(np.random.default_rng(seed).choice(v, 1023, replace=False)).astype(f32)
    return e


def tables_for(tex):
    return [("one", np.float32([0.5]), "luma"), ("q8", tone_curves()["q8"], "g"), ("log", log_table(), "r"),
            ("own", own_table(tex, 3, 31), "a")]


def check_hist(ctx, ref_lib, tex, rects, what, tables=None):
    for tname, edges, ch in tables or tables_for(tex):
        got = ctx.histogram("color", edges, ch, rects)
        same_records(got, ref_hist(ref_lib, tex, CHANNELS.index(ch), rects, edges), f"{what}, table {tname}, {ch}", rects)


def test_every_width_to_130_by_every_height_at_odd_origins(R, ref_lib, wide):
    ctx, tex, _ = wide
    rng = np.random.default_rng(41)
    rects = []
    for w in range(1, 131):
        for h in range(1, 10):
            x = int(rng.integers(0, (2051 - w) // 2)) * 2 + 1
            rects.append([x, int(rng.integers(0, 9 - h + 1)), w, h])
    check_hist(ctx, ref_lib, tex, rects, "widths 1 .. 130 x heights 1 .. 9")


def test_every_height_to_130_by_every_width_at_odd_origins(R, ref_lib, tall):
    ctx, tex, _ = tall
    rng = np.random.default_rng(42)
    rects = []
    for h in range(1, 131):
        for w in range(1, 10):
            y = int(rng.integers(0, (2051 - h) // 2)) * 2 + 1
            rects.append([int(rng.integers(0, 9 - w + 1)), y, w, h])
    check_hist(ctx, ref_lib, tex, rects, "heights 1 .. 130 x widths 1 .. 9")


EDGE_SIZES = [255, 256, 257, 258, 259, 260, 1023, 1024, 1025, 1026, 2047, 2048, 2049, 2050, 2051]


def test_widths_around_the_chunk_sizes(R, ref_lib, wide):
    """A workgroup walks a row in chunks of 1024 texels and packs rows of up to 1024 texels 256 / lanes-a-row to a pass:
    widths around 256 (64 lanes a row), 1024 (the last packed width) and 2048 (two chunks), at both ends of the texture"""
    ctx, tex, _ = wide
    rng = np.random.default_rng(43)
    rects = []
    for w in EDGE_SIZES:
        rects += [[0, 0, w, 9], [2051 - w, 0, w, 9], [int(rng.integers(0, 2051 - w + 1)), 2, w, 5]]
    check_hist(ctx, ref_lib, tex, rects, "wide rectangles")


def test_heights_around_the_chunk_sizes(R, ref_lib, tall):
    ctx, tex, _ = tall
    rng = np.random.default_rng(44)
    rects = []
    for h in EDGE_SIZES:
        rects += [[0, 0, 9, h], [0, 2051 - h, 9, h]]
        rects += [[int(rng.integers(0, 9 - w + 1)), int(rng.integers(0, 2051 - h + 1)), w, h] for w in (1, 3, 8)]
    check_hist(ctx, ref_lib, tex, rects, "tall rectangles")


def test_the_log_table_fills_its_bins(R, ref_lib, wide):
    """The condition of the shape tests: under the 1023-edge log table the reference alone fills at least 900 of the
    1024 bins in every channel of the 2051 x 9 texture, so a kernel that mislaid a range of bins would show."""
    ctx, tex, specials = wide
    edges = log_table()
    assert len(edges) == 1023 and np.signbit(edges[511]) and edges[511] == 0
    for ci, ch in enumerate(CHANNELS[:4]):
        want = ref_hist(ref_lib, tex, ci, [[0, 0, 2051, 9]], edges)
        filled = int((want[0, 3:] > 0).sum())
        assert filled >= 900, (ch, filled)
        assert (want[0, 2] > 0) == specials
        same_records(ctx.histogram("color", edges, ch), want, f"log table, {ch}")


@pytest.fixture(scope="module", params=[True, False], ids=["specials", "finite"])
def big(R, request):
    ctx, tex = wild_context(R, 2051, 1030, specials=request.param)
    yield ctx, tex
    ctx.close()


def big_rects():
    rng = np.random.default_rng(45)
    w, h = rng.integers(1, 301, 200), rng.integers(1, 61, 200)
    x, y = (rng.random(200) * (2051 - w + 1)).astype(int), (rng.random(200) * (1030 - h + 1)).astype(int)
    return np.concatenate([[[0, 0, 2051, 1030]], np.stack([x, y, w, h], 1)]).astype(np.int32)


@pytest.mark.parametrize("table", ["one", "q8", "log", "own"])
def test_many_workgroups_feed_one_record(R, ref_lib, big, table):
    """2051 x 1030: the whole texture is 515 blocks of two rows, whose workgroups all add into one record, beside 200
    random rectangles of one to eight blocks"""
    ctx, tex = big
    pick = [t for t in tables_for(tex) if t[0] == table]
    check_hist(ctx, ref_lib, tex, big_rects(), "2051 x 1030", pick)


def test_inline_and_uploaded_plans_give_the_same_records(R, ref_lib, tmp_path_factory):
    """tests/test_reduce_gpu.py's rectangles (section 2c there): a call of four takes the plan in the kernel's
    arguments, a call of five the uploaded one."""
    plan = build_rect_plan(tmp_path_factory)
    assert planned(plan.hist_block_rows, PLAN_RECTS[0]) == (8, 5), "narrow rows: five blocks"
    assert planned(plan.hist_block_rows, PLAN_RECTS[2]) == (2, 3), "rows of more than 1024 texels: three blocks"
    ctx, tex = plan_context(R)
    rects5 = PLAN_RECTS + PLAN_FIFTH
    for tname, edges, ch in tables_for(tex):
        want = ref_hist(ref_lib, tex, CHANNELS.index(ch), rects5, edges)
        assert want[:, 0].tolist() == [0, 0, 0, INVALID, 0]
        four = ctx.histogram("color", edges, ch, PLAN_RECTS)   # n = 4: the inline plan
        five = ctx.histogram("color", edges, ch, rects5)       # n = 5: the uploaded plan
        same_records(four, want[:4], f"the inline plan, table {tname}", PLAN_RECTS)
        same_records(five, want, f"the uploaded plan, table {tname}", rects5)
        assert four.tobytes() == five[:4].tobytes(), f"records 0 .. 3 of the two plans, table {tname}"
    ctx.close()


def test_sprites_across_a_batch_boundary(R, ref_lib, big):
    """70 000 rectangles of one block each, 5 % invalid: two batches of work items over the same plan buffer"""
    ctx, tex = big
    rects, bad = sprite_rects(70000, 2051, 1030, 46)
    edges = np.float32([-1.0, -0.0, 1e-3, 1.0, 1e3])
    got = ctx.histogram("color", edges, "b", rects)
    same_records(got, ref_hist(ref_lib, tex, 2, rects, edges), "sprites over two batches", rects)
    assert (got[bad, 0] == INVALID).all() and not got[bad, 1:].any()


# ------------------------------------------------------------------ 6: one bin
@pytest.mark.parametrize("others", [False, True], ids=["constant", "one-percent-others"])
def test_nearly_every_texel_in_one_bin(R, ref_lib, others):
    """A constant texture, and the same with 1 % other values: the lanes of a wave share a counter (the aggregation
    before the LDS atomic) -- all of them, or all but a few"""
    W, H = 259, 37
    ctx = R.RC2DGI(W, H, cascade_count=1, storage="f32")
    v = np.empty((H, W, 4), f32)
    v[...] = [0.25, 0.5, 0.125, 1.0]
    if others:
        rng = np.random.default_rng(47)
        hit = rng.random((H, W)) < 0.01
        v[hit] = gpu_texture(W, H, True)[hit]
        assert 50 < hit.sum() < 150
    ctx.upload("color", v)
    tex = ctx.download("color")
    rects = [[0, 0, W, H], [1, 1, 257, 35], [3, 0, 64, 37], [0, 5, 259, 1], [100, 7, 5, 5]]
    for tname, edges in (("q8", tone_curves()["q8"]), ("log", log_table()), ("one", np.float32([0.5]))):
        for ci, ch in enumerate(CHANNELS):
            got = ctx.histogram("color", edges, ch, rects)
            same_records(got, ref_hist(ref_lib, tex, ci, rects, edges), f"one bin, table {tname}, {ch}", rects)
            if not others:
                assert ((got[:, 3:] > 0).sum(1) == 1).all() and (got[:, 3:].max(1) == got[:, 1]).all()
    ctx.close()


# ------------------------------------------------------------------ 7: lists
@pytest.fixture(scope="module", params=STORAGES)
def sprites_ctx(R, request):
    ctx, _, _ = demo_context(R, 200, 160, 3, 1.0, request.param)
    yield ctx
    ctx.close()


def test_twenty_thousand_sprites(R, ref_lib, sprites_ctx):
    ctx = sprites_ctx
    tw, th = ctx.cascade_resolution
    assert tw >= 41 and th >= 41
    rects, bad = sprite_rects(20000, tw, th, 21)
    assert 800 < len(bad) < 1200
    edges = (2.0 ** np.linspace(-10, 2, 31)).astype(f32)
    tex = ctx.download("final_gi")
    got = ctx.histogram("final_gi", edges, "luma", rects)
    same_records(got, ref_hist(ref_lib, tex, 4, rects, edges), f"{ctx.storage} sprites", rects)
    assert (got[bad, 0] == INVALID).all() and not got[bad, 1:].any(), "an invalid record is its status and zeros"
    ok = np.setdiff1d(np.arange(20000), bad)
    assert (got[ok, 0] == 0).all() and np.array_equal(got[ok, 1], (rects[ok, 2] * rects[ok, 3]).astype(u32))
    assert np.array_equal(got[ok, 2:].sum(1), got[ok, 1]) and (got[ok, 3:] > 0).sum() > len(ok), "some sprites span bins"


# ------------------------------------------------------------------ 8: the device variant
@pytest.mark.parametrize("storage", STORAGES)
def test_device_variant_after_an_enqueued_frame(R, ref_lib, storage):
    import torch

    ctx, _, _ = demo_context(R, 200, 160, 3, 1.0, storage)
    tw, th = ctx.cascade_resolution
    rects, _ = sprite_rects(500, tw, th, 22)
    rects = np.concatenate([rects, np.int32([[0, 0, tw, th]])])
    n, edges = len(rects), (2.0 ** np.linspace(-12, 3, 256)).astype(f32)
    ctx.set_shader_value("_SunAngle", 1.25)  # the next frame differs from the one already there
    old = ctx.histogram("final_gi", edges, "luma", rects)
    raw = torch.full((1 + n * 260 + 3,), -1, dtype=torch.int32, device="cuda")   # 0xFF bytes; 4 bytes off 16
    dst = raw[1:1 + n * 260].view(n, 260)
    assert dst.data_ptr() % 16 == 4 and dst.is_contiguous()
    torch.cuda.synchronize()
    ctx.do_rc2dgi()
    ctx.histogram_into(dst, "final_gi", edges, "luma", rects)  # no sync between the two
    ctx.sync()
    words = raw.cpu().numpy()
    assert words[0] == -1 and (words[1 + n * 260:] == -1).all(), "words outside the records"
    got = dst.cpu().numpy().view(u32)
    want = ctx.histogram("final_gi", edges, "luma", rects)
    same_records(got, want, storage + " device variant against the host variant", rects)
    same_records(want, ref_hist(ref_lib, ctx.download("final_gi"), 4, rects, edges), storage + " host variant", rects)
    assert not np.array_equal(old, want), "the records are of the new frame"
    # a destination 2 bytes off alignment; n == 0 with null pointers
    L, h = ctx._L, ctx._h
    r = R._rect_array(rects)
    ep = edges.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert L.rc2dgi_histogram_device(h, 9, 4, r.ctypes.data, n, ep, 256, ctypes.c_void_p(raw.data_ptr() + 2)) == E_ARG
    assert b"4 bytes" in L.rc2dgi_last_error(h)
    assert L.rc2dgi_histogram_device(h, 9, 4, None, 0, ep, 256, None) == 0
    assert L.rc2dgi_histogram(h, 9, 4, None, 0, ep, 256, None) == 0
    ctx.sync()
    assert np.array_equal(raw.cpu().numpy(), words), "a refused call wrote"
    with pytest.raises((TypeError, ValueError)):
        ctx.histogram_into(dst[:, :100], "final_gi", edges, "luma", rects)
    ctx.close()


# ------------------------------------------------------------------ 9: errors
def test_errors_leave_a_valid_context(R, ref_lib):
    import torch

    ctx, _, _ = demo_context(R, 96, 80, 3, 0.5, "f32")
    set_curves(ctx)
    L, h = ctx._L, ctx._h
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))  # noqa: E731
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    views = [("color", 0, 0, 96, 80), ("final_gi", 5, 5, 40, 30)]
    tones = [(3.7, SLOTS["srgb"]), (2.0, 0)]
    want_img = ctx.compose(views, tones=tones)
    rects = R._rect_array([[0, 0, 48, 40], [3, 5, 17, 9], [47, 39, 1, 1], [40, 0, 9, 1]])
    n, edges = len(rects), tone_curves()["q8"]
    want = ctx.histogram("final_gi", edges, "luma", rects)
    assert want[:, 0].tolist() == [0, 0, 0, INVALID]
    out = np.zeros((n, 259), u32)
    d_out = torch.zeros((n + 1, 259), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dp = lambda off=0: ctypes.c_void_p(d_out.data_ptr() + off)  # noqa: E731

    def still_fine():
        same_image(ctx.compose(views, tones=tones), want_img, "after an error")
        same_records(ctx.histogram("final_gi", edges, "luma", rects), want, "after an error")

    def tone_code(tn, expect):
        with pytest.raises(R.RC2DGIError) as ei:
            ctx.compose(views, tones=tn)
        assert ei.value.code == expect and str(ei.value), (tn, ei.value.code)
        dev = torch.zeros((80, 96, 4), dtype=torch.uint8, device="cuda")
        with pytest.raises(R.RC2DGIError) as ei:
            ctx.compose_into(dev, views, tones=tn)
        assert ei.value.code == expect
        ctx.sync()
        assert not dev.cpu().numpy().any(), "a refused call wrote"

    for bad in (float("nan"), float("inf"), -float("inf"), -1.0, -1e-45):
        tone_code([(bad, 0), (1.0, 0)], E_ARG)
        tone_code([(1.0, 0), (bad, SLOTS["q8"])], E_ARG)
    for bad in (-1, 9, 1 << 20):
        tone_code([(1.0, bad), (1.0, 0)], E_ARG)
    tone_code([(1.0, 7), (1.0, 0)], E_STATE)   # a slot that was never set
    still_fine()
    q8 = tone_curves()["q8"]
    for slot in (0, -1, 9):
        assert L.rc2dgi_set_curve(h, slot, fp(q8)) == E_ARG and L.rc2dgi_last_error(h)
    for k, v in ((5, np.nan), (100, 0.0), (254, -np.inf)):
        broken = q8.copy()
        broken[k] = v
        assert L.rc2dgi_set_curve(h, 2, fp(broken)) == E_ARG   # refused: slot 2 keeps its sRGB table
    assert L.rc2dgi_set_curve(h, 0, None) == E_ARG
    still_fine()

    def hist_code(code):
        assert code == E_ARG and L.rc2dgi_last_error(h), code

    e = fp(edges)
    for m in (0, -1, 1024):
        hist_code(L.rc2dgi_histogram(h, 9, 4, p(rects), n, e, m, p(out)))
        hist_code(L.rc2dgi_histogram_device(h, 9, 4, p(rects), n, e, m, dp()))
    for k, v in ((0, np.nan), (7, 0.0)):
        broken = edges.copy()
        broken[k] = v
        hist_code(L.rc2dgi_histogram(h, 9, 4, p(rects), n, fp(broken), 255, p(out)))
        hist_code(L.rc2dgi_histogram_device(h, 9, 4, p(rects), n, fp(broken), 255, dp()))
    hist_code(L.rc2dgi_histogram(h, 9, 4, p(rects), n, None, 255, p(out)))
    for ch in (-1, 5):
        hist_code(L.rc2dgi_histogram(h, 9, ch, p(rects), n, e, 255, p(out)))
        hist_code(L.rc2dgi_histogram_device(h, 9, ch, p(rects), n, e, 255, dp()))
    for which in (-1, 10):
        hist_code(L.rc2dgi_histogram(h, which, 4, p(rects), n, e, 255, p(out)))
        hist_code(L.rc2dgi_histogram_device(h, which, 4, p(rects), n, e, 255, dp()))
    for bad_n in (-1, (1 << 20) + 1, (1 << 26) // 259 + 1):   # the last: n * (m + 4) > 1 << 26
        hist_code(L.rc2dgi_histogram(h, 9, 4, p(rects), bad_n, e, 255, p(out)))
        hist_code(L.rc2dgi_histogram_device(h, 9, 4, p(rects), bad_n, e, 255, dp()))
    hist_code(L.rc2dgi_histogram(h, 9, 4, None, n, e, 255, p(out)))
    hist_code(L.rc2dgi_histogram(h, 9, 4, p(rects), n, e, 255, None))
    hist_code(L.rc2dgi_histogram_device(h, 9, 4, p(rects), n, e, 255, None))
    for off in (1, 2, 3):
        hist_code(L.rc2dgi_histogram_device(h, 9, 4, p(rects), n, e, 255, dp(off)))
    ctx.sync()
    assert not out.any() and not d_out.cpu().numpy().any(), "a refused call wrote"
    assert L.rc2dgi_histogram_device(h, 9, 4, p(rects), n, e, 255, dp(4)) == 0   # 4 bytes in is aligned
    ctx.sync()
    same_records(d_out.cpu().numpy().view(u32).reshape(-1)[1:1 + n * 259].reshape(n, 259), want, "records 4 bytes in")
    still_fine()
    # a row-strip shard's textures hold windows and bands
    ctx.set_shard(0, 2)
    assert L.rc2dgi_histogram(h, 9, 4, p(rects), n, e, 255, p(out)) == E_UNSUPPORTED and b"shard" in L.rc2dgi_last_error(h)
    assert L.rc2dgi_histogram_device(h, 9, 4, p(rects), n, e, 255, dp()) == E_UNSUPPORTED
    with pytest.raises(R.RC2DGIError) as ei:
        ctx.compose(views, tones=tones)
    assert ei.value.code == E_UNSUPPORTED and "shard" in str(ei.value)
    ctx.set_shard(0, 1)
    ctx.do_rc2dgi()
    ctx.sync()
    still_fine()
    ctx.close()


def test_chain_timeout_is_reported_by_the_host_variants(R, ref_lib):
    """The existing diagnostic knob, as tests/test_query_gpu.py uses it: rc_chain_spin -1 makes every wait of the chained
    cascade launch time out at once (no fault, no hang), the frame's cascades are wrong, and the next synchronising call
    says so."""
    from radiancecascade2dglobalillumination_amd import scenes

    W, H, N = 1200, 900, 6
    color, emis = scenes.demo(W, H)
    ctx = R.RC2DGI(W, H, cascade_count=N, ray_range=2.0)
    set_curves(ctx)
    ctx.frame(color, emis)
    ctx.sync()
    cw, ch = ctx.cascade_resolution
    rects = np.int32([[0, 0, cw, ch], [100, 200, 64, 64]])
    edges = (2.0 ** np.linspace(-12, 3, 64)).astype(f32)
    views = [("color", 0, 0, W, H), ("final_gi", 10, 10, 100, 100)]
    tones = [(3.7, SLOTS["srgb"]), (1.0, SLOTS["reinhard"])]
    want_h, want_i = ctx.histogram("final_gi", edges, "luma", rects), ctx.compose(views, tones=tones)
    for call in (lambda: ctx.histogram("final_gi", edges, "luma", rects), lambda: ctx.compose(views, tones=tones)):
        ctx.set_tuning("rc_chain", 1)
        ctx.set_tuning("rc_chain_spin", -1)
        ctx.do_rc2dgi()
        with pytest.raises(R.RC2DGIError) as ei:
            call()
        assert ei.value.code == E_DEVICE and "cascade chain" in str(ei.value)
        assert ctx.get_tuning("rc_chain") == 0
        ctx.set_tuning("rc_chain_spin", 0)
        ctx.do_rc2dgi()
        same_records(ctx.histogram("final_gi", edges, "luma", rects), want_h, "records after the fallback", rects)
        same_image(ctx.compose(views, tones=tones), want_i, "the frame after the fallback")
    same_records(want_h, ref_hist(ref_lib, ctx.download("final_gi"), 4, rects, edges), "against the reference", rects)
    ctx.close()
