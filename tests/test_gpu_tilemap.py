"""GPU: rc2dgi_tilemap_device -- a grid of Tiled cell words drawn from a tile set as one layer -- bit for bit against
the numpy restatement of the header (tests/tilemap_ref.py) and against rc2dgi_sprites_device on the expanded list
(rc2dgi.tilemap_sprites) on the same context: every atlas format in every storage, blended and replacing; the edge maps
of tests/tilemap_cases.py with and without a clear and their status words; non-finite texels and atlas pixels; raw and
narrowed garbage; the painters' working memory, which this call must not allocate; two layers and a frame against the
CPU oracle; a shard; the stream order behind a busy device; the argument errors in the documented order."""
import ctypes
import time

import numpy as np
import pytest

import oracle
import sprites_ref as S
import tilemap_cases as C
import tilemap_ref as T
from oracle import paint_ref

pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32
CLEAR = (9, 8, 7, 200)


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def R(torch):
    from radiancecascade2dglobalillumination_amd import rc2dgi

    return rc2dgi


_ctx = {}


@pytest.fixture(scope="module")
def ctx_of(R):
    """one context a (W, H, storage), shared by the tests that only draw into its inputs"""

    def get(W, H, storage="f32"):
        key = (W, H, storage)
        if key not in _ctx:
            _ctx[key] = R.RC2DGI(W, H, cascade_count=2, storage=storage)
        return _ctx[key]

    yield get
    for c in _ctx.values():
        c.close()
    _ctx.clear()


# ------------------------------------------------------------------ atlases, textures, calls
def atlas_np(fmt, aw, ah, seed=1):
    """(ah, aw, 4) pixels, row 0 the top: bytes, or floats a little outside [0, 1] with alphas from 0 to above 1"""
    rng = np.random.default_rng(seed)
    if fmt == "uint8":
        a = rng.integers(0, 256, (ah, aw, 4)).astype(np.uint8)
        a[::3, ::2, 3] = 255
        a[1::5, 1::3, 3] = 0
        return a
    a = rng.uniform(-0.25, 1.25, (ah, aw, 4)).astype(f32)
    a[..., 3] = rng.uniform(-0.1, 1.1, (ah, aw))
    a[::3, ::2, 3] = 1.0
    a[1::5, 1::3, 3] = 0.0
    return a.astype(np.float16) if fmt == "float16" else a


def to_dev(torch, a, pad=0):
    t = torch.from_numpy(a).to("cuda")
    if not pad:
        return t
    wide = torch.zeros((a.shape[0], a.shape[1] + pad, 4), dtype=t.dtype, device="cuda")
    wide[:, :a.shape[1]] = t
    return wide[:, :a.shape[1]]


def cells_dev(torch, g, window=None):
    """the grid on the device; window (r0, c0, world_rows, world_cols): a view into a larger world of other words"""
    t = torch.from_numpy(np.ascontiguousarray(g).view(np.int32)).to("cuda")
    if window is None:
        return t
    r0, c0, wr, wc = window
    world = torch.full((wr, wc), 0x7FFFFFFF, dtype=torch.int32, device="cuda")  # (words the rule refuses)
    world[r0:r0 + g.shape[0], c0:c0 + g.shape[1]] = t
    return world[r0:r0 + g.shape[0], c0:c0 + g.shape[1]]


def base_texture(W, H, seed=5):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (H, W, 4)).astype(f32)


_bases = {}


def start_of(R, W, H, storage):
    """(what is uploaded, the texture that upload leaves): computed once a (W, H, storage)"""
    key = (W, H, storage)
    if key not in _bases:
        c = R.RC2DGI(W, H, cascade_count=2, storage=storage)
        c.upload("emissive", base_texture(W, H))
        _bases[key] = texture(c, "emissive", storage == "rgba8")
        _bases[key].setflags(write=False)
        c.close()
    return _bases[key]


def texture(ctx, which, u8):
    return ctx.download(which, np.uint8) if u8 else ctx.download(which)


def one_nan(x):
    """the uint32 view with every NaN mapped to one pattern (a NaN's payload is not part of the contract)"""
    if x.dtype == np.uint8:
        return x
    v = np.ascontiguousarray(x, f32).view(u32).copy()
    v[np.isnan(x)] = 0x7FC00000
    return v


def same(got, want, what=""):
    g, w = one_nan(got), one_nan(want)
    assert np.array_equal(g, w), f"{what}: {np.count_nonzero(np.any(g != w, axis=-1))} texels differ"


def tilemap(torch, ctx, which, at, cells_t, m, clear=None, status=True):
    st = torch.full((2,), -77, dtype=torch.int32, device="cuda") if status else None
    ctx.tilemap_device(which, at, cells_t, m["tile"], m["origin"], m["set_cols"], m["margin"], m["spacing"], m["tint"],
                       m["replace"], clear, st)
    ctx.sync()
    return st.cpu().numpy().tolist() if status else None


def expanded(torch, R, cells_t, m, a, W, H):
    return R.tilemap_sprites(cells_t, m["tile"], m["origin"], (a.shape[1], a.shape[0]), (W, H), m["set_cols"],
                             m["margin"], m["spacing"], m["tint"], m["replace"])


# ------------------------------------------------------------------ 1. formats, storages, blend and replace
@pytest.mark.parametrize("replace", [False, True], ids=["blend", "replace"])
@pytest.mark.parametrize("storage", ["f32", "f16", "rgba8"])
@pytest.mark.parametrize("fmt", ["uint8", "float16", "float32"])
def test_formats_and_storages_equal_the_restatement_and_the_sprite_list(R, torch, ctx_of, fmt, storage, replace):
    W, H = 64, 48
    u8 = storage == "rgba8"
    AW, AH = C.set_size((16, 16), 4, 3)
    a = atlas_np(fmt, AW, AH)
    at = to_dev(torch, a, 6)  # (a pitch wider than a row)
    g = C.grid(5, 6, 12, 41)
    g[1, 1], g[2, 3] = 1 | T.DIAGONAL, 13  # two refused cells among them
    m = T.layer((16, 16), (-9, -5), tint=C.TINT, replace=replace)
    ct = cells_dev(torch, g)
    start = start_of(R, W, H, storage)
    ctx = ctx_of(W, H, storage)
    ctx.upload("emissive", base_texture(W, H))
    status = tilemap(torch, ctx, "emissive", at, ct, m)
    got = texture(ctx, "emissive", u8)
    want, wstatus = T.draw(start, a, g, m, u8)
    assert status == wstatus and status[0] > 10 and status[1] == 2
    same(got, want, "against the restatement")
    assert not np.array_equal(want, start), "the layer changed the texture"
    # rc2dgi_sprites_device with the expanded list, on the same context
    ctx.upload("emissive", base_texture(W, H))
    sp = expanded(torch, R, ct, m, a, W, H)
    st2 = torch.full((2,), -77, dtype=torch.int32, device="cuda")
    ctx.sprites_device("emissive", at, sp, None, None, st2)
    ctx.sync()
    assert st2.cpu().numpy().tolist() == [status[0], 0]
    same(got, texture(ctx, "emissive", u8), "against rc2dgi_sprites_device")


# ------------------------------------------------------------------ 2. the edge maps and their status words
@pytest.mark.parametrize("clear", [None, CLEAR], ids=["noclear", "clear"])
@pytest.mark.parametrize("k", C.edge_cases(), ids=lambda k: k["name"])
def test_edge_maps_and_status_words(R, torch, ctx_of, k, clear):
    W, H, m = k["W"], k["H"], k["m"]
    a = atlas_np("uint8", k["AW"], k["AH"], seed=3)
    at = to_dev(torch, a)
    ct = cells_dev(torch, k["cells"], k["window"])
    if k["window"]:
        assert ct.stride(0) > ct.shape[1]
    for storage in ("f32", "rgba8"):
        u8 = storage == "rgba8"
        start = start_of(R, W, H, storage)
        ctx = ctx_of(W, H, storage)
        ctx.upload("color", base_texture(W, H))
        status = tilemap(torch, ctx, "color", at, ct, m, clear)
        got = texture(ctx, "color", u8)
        want, wstatus = T.draw(start, a, k["cells"], m, u8, clear)
        assert status == wstatus, (status, wstatus)
        same(got, want, f"{k['name']} {storage}")
        if k["name"].startswith("off"):
            assert status == [0, 0]
            if clear is None:
                same(got, start, "a map off the target leaves the texture")
        if k["name"] == "smaller than the target":  # the uncovered texels keep their bits, or become the clear
            inside = np.zeros((H, W), bool)
            inside[H - 10 - 32:H - 10, 20:20 + 48] = True
            keep = start if clear is None else S.draw(start, a, np.zeros((0, 8), np.int32), u8, clear)
            assert np.array_equal(one_nan(got)[~inside], one_nan(keep)[~inside])
    # a null status is accepted and draws the same bits
    ctx = ctx_of(W, H, "f32")
    ctx.upload("color", base_texture(W, H))
    assert tilemap(torch, ctx, "color", at, ct, m, clear, status=False) is None
    same(ctx.download("color"), T.draw(start_of(R, W, H, "f32"), a, k["cells"], m, False, clear)[0], "null status")


def test_an_empty_grid_draws_nothing_or_the_clear(R, torch, ctx_of):
    W, H = 64, 48
    a = atlas_np("uint8", 64, 48)
    at = to_dev(torch, a)
    ctx = ctx_of(W, H)
    start = start_of(R, W, H, "f32")
    m = T.layer((16, 16))
    for shape in ((0, 5), (5, 0), (0, 0)):
        ct = torch.zeros(shape, dtype=torch.int32, device="cuda")
        ctx.upload("emissive", base_texture(W, H))
        assert tilemap(torch, ctx, "emissive", at, ct, m) == [0, 0]
        same(ctx.download("emissive"), start, shape)
        assert tilemap(torch, ctx, "emissive", at, ct, m, CLEAR) == [0, 0]
        same(ctx.download("emissive"), S.draw(start, a, np.zeros((0, 8), np.int32), False, CLEAR), shape)


# ------------------------------------------------------------------ 3. non-finite texels and atlas pixels
def test_non_finite_texels_and_atlas_pixels_propagate(R, torch, ctx_of):
    W, H = 64, 48
    AW, AH = C.set_size((16, 16), 4, 3)
    a = atlas_np("float32", AW, AH)
    nan, inf = f32(np.nan), f32(np.inf)
    for ty in range(3):
        for tx in range(4):
            y, x = 16 * ty, 16 * tx
            a[y + 2, x + 3] = [nan, 0.5, 0.5, 0.5]
            a[y + 2, x + 4] = [0.5, 0.5, 0.5, nan]
            a[y + 3, x + 3] = [inf, -inf, 0.25, 0.5]
            a[y + 3, x + 4] = [0.25, 0.5, 0.75, inf]
            a[y + 4, x + 3] = [0.25, 0.5, 0.75, -inf]
            a[y + 4, x + 4] = [inf, inf, inf, 0.0]
            a[y + 5, x + 3] = [-inf, nan, inf, 1.0]
    at = to_dev(torch, a)
    g = C.grid(4, 5, 12, 43, empty=0.1)
    ct = cells_dev(torch, g)
    base = base_texture(W, H)
    base[5, 7] = [nan, 0.5, inf, 0.25]
    base[20, 33] = [-inf, 1.0, 0.0, nan]
    base[40:44, 10:14] = inf
    ctx = ctx_of(W, H)
    for tint, replace in ((C.TINT, False), ((255, 255, 255, 255), True), ((0, 0, 0, 0), False), ((0, 128, 255, 255), False)):
        m = T.layer((16, 16), (-5, -7), tint=tint, replace=replace)
        ctx.upload("emissive", base)
        status = tilemap(torch, ctx, "emissive", at, ct, m)
        want, wstatus = T.draw(base, a, g, m, False)
        assert status == wstatus
        assert np.isnan(want).any() and np.isinf(want).any()
        same(ctx.download("emissive"), want, f"tint {tint} replace {replace}")


# ------------------------------------------------------------------ 4. garbage
@pytest.mark.parametrize("kind", ["raw", "narrowed"])
def test_a_grid_of_garbage_draws_what_the_rule_accepts(R, torch, ctx_of, kind):
    q = C.GARBAGE
    W, H = q["W"], q["H"]
    AW, AH = C.set_size(q["tile"], *q["set_tiles"])
    ntiles = q["set_tiles"][0] * q["set_tiles"][1]
    g = C.narrowed_garbage(q["rows"], q["cols"], ntiles, 123) if kind == "narrowed" else C.raw_garbage(q["rows"], q["cols"], 123)
    m = T.layer(q["tile"], q["origin"], tint=C.TINT)
    a = atlas_np("float32", AW, AH)
    at = to_dev(torch, a)
    for storage in ("f32", "rgba8"):
        u8 = storage == "rgba8"
        ctx = ctx_of(W, H, storage)
        for clear in (None, (0, 0, 0, 0)):
            ctx.upload("color", base_texture(W, H))
            status = tilemap(torch, ctx, "color", at, cells_dev(torch, g), m, clear)
            want, wstatus = T.draw(start_of(R, W, H, storage), a, g, m, u8, clear)
            assert status == wstatus, (status, wstatus)
            same(texture(ctx, "color", u8), want, f"{kind} {storage}")
        if kind == "narrowed":
            assert status[0] >= 4 and status[1] >= 4
        else:
            assert status[1] > 50
    # a large grid of raw words far beyond the target on every side, and a set_cols of 1
    big = C.raw_garbage(300, 400, 7)
    m = T.layer((3, 5), (-600, -700), set_cols=1)
    a = atlas_np("uint8", 9, 23)
    ctx = ctx_of(W, H)
    ctx.upload("color", base_texture(W, H))
    status = tilemap(torch, ctx, "color", to_dev(torch, a), cells_dev(torch, big), m)
    want, wstatus = T.draw(start_of(R, W, H, "f32"), a, big, m, False)
    assert status == wstatus
    same(ctx.download("color"), want, "the large grid")


# ------------------------------------------------------------------ 5. the painters' working memory
def prims(W, H, seed):
    rng = np.random.default_rng(seed)
    P = []
    for k in range(9):
        c = tuple(int(v) for v in rng.integers(0, 256, 3)) + (int(rng.integers(60, 255)),)
        if k % 2:
            P.append((1, float(rng.uniform(0, W)), float(rng.uniform(0, H)), float(rng.uniform(2, 14)), 0.0) + c)
        else:
            P.append((0, float(rng.uniform(-5, W - 10)), float(rng.uniform(-5, H - 10)), float(rng.uniform(4, 30)),
                      float(rng.uniform(4, 20))) + c)
    return P


def prim_words(R, P):
    arr = (R.Prim * len(P))()
    for k, p in enumerate(P):
        arr[k] = R.Prim(int(p[0]), float(p[1]), float(p[2]), float(p[3]), float(p[4]), *(int(v) for v in p[5:9]))
    return np.frombuffer(bytes(arr), np.int32).reshape(-1, 6).copy()


@pytest.mark.parametrize("first", ["tilemap", "paint"])
def test_the_painters_working_memory_is_not_allocated_by_this_call(R, torch, first):
    """rc2dgi_paint_device allocates and zeroes the working memory at its first call; a tilemap call before it on a
    fresh context must leave that to it (the painter still paints its bits), and one after it must not disturb it"""
    W, H = 200, 72
    AW, AH = C.set_size((16, 16), 4, 3)
    a = atlas_np("uint8", AW, AH)
    at = to_dev(torch, a)
    g = C.grid(6, 14, 12, 44)
    ct = cells_dev(torch, g)
    m = T.layer((16, 16), (-3, -9), tint=C.TINT)
    P1, P2 = prims(W, H, 31), prims(W, H, 32)
    w1, w2 = (torch.from_numpy(prim_words(R, P)).to("cuda") for P in (P1, P2))
    st = torch.full((3, 2), -77, dtype=torch.int32, device="cuda")
    ctx = R.RC2DGI(W, H, cascade_count=2)
    zero = np.zeros((H, W, 4), f32)
    args = (m["tile"], m["origin"], m["set_cols"], m["margin"], m["spacing"], m["tint"], False)
    if first == "tilemap":
        ctx.tilemap_device("color", at, ct, *args, (10, 20, 30, 255), st[0])
        ctx.paint_device("color", w1, None, None, st[1])
        ctx.paint_device("color", w2, None, None, st[2])
        ctx.sync()
        want, ws = T.draw(zero, a, g, m, False, (10, 20, 30, 255))
        want = paint_ref.paint(W, H, P2, None, base=paint_ref.paint(W, H, P1, None, base=want))
        assert st.cpu().numpy().tolist() == [ws, [9, 0], [9, 0]]
    else:
        ctx.paint_device("color", w1, (10, 20, 30, 255), None, st[0])
        ctx.tilemap_device("color", at, ct, *args, None, st[1])
        ctx.paint_device("color", w2, None, None, st[2])
        ctx.sync()
        want, ws = T.draw(paint_ref.paint(W, H, P1, (10, 20, 30, 255)), a, g, m, False)
        want = paint_ref.paint(W, H, P2, None, base=want)
        assert st.cpu().numpy().tolist() == [[9, 0], ws, [9, 0]]
    same(ctx.download("color"), want, first)
    ctx.close()


# ------------------------------------------------------------------ 6. two layers and a frame
@pytest.mark.parametrize("storage", ["f32", "rgba8"])
def test_two_layers_then_a_frame_equal_the_oracle_on_the_restated_inputs(R, torch, storage):
    """a wall layer with REPLACE over a clear, a decal layer blended over it, lights into EMISSIVE, then rc2dgi_do: the
    frame is oracle.frame of the inputs the restatement gives"""
    W = H = 128
    N = 3
    u8 = storage == "rgba8"
    AW, AH = C.set_size((16, 16), 4, 3)
    a = atlas_np("uint8", AW, AH)
    a[..., 3] = np.where(a[..., 3] > 100, 255, 0)  # walls and lights are opaque or absent
    at = to_dev(torch, a)
    walls, decals, lights = C.grid(9, 9, 12, 51, empty=0.6), C.grid(5, 6, 12, 52, empty=0.5), C.grid(9, 9, 12, 53, empty=0.85)
    mw = T.layer((16, 16), (-7, -5), replace=True)
    md = T.layer((16, 16), (20, 30), tint=(255, 255, 255, 128))
    ml = T.layer((16, 16), (-7, -5), tint=(255, 200, 120, 255), replace=True)
    ctx = R.RC2DGI(W, H, cascade_count=N, ray_range=2.0, storage=storage)
    st = torch.full((3, 2), -77, dtype=torch.int32, device="cuda")
    tens = [cells_dev(torch, g) for g in (walls, decals, lights)]
    for t, m, which, clear, s in ((tens[0], mw, "color", (0, 0, 0, 0), st[0]), (tens[1], md, "color", None, st[1]),
                                  (tens[2], ml, "emissive", (0, 0, 0, 255), st[2])):
        ctx.tilemap_device(which, at, t, m["tile"], m["origin"], m["set_cols"], m["margin"], m["spacing"], m["tint"],
                           m["replace"], clear, s)
    ctx.do_rc2dgi()
    ctx.sync()
    got = ctx.download("color")
    zero = np.zeros((H, W, 4), np.uint8 if u8 else f32)
    color, s0 = T.draw(zero, a, walls, mw, u8, (0, 0, 0, 0))
    color, s1 = T.draw(color, a, decals, md, u8)
    emissive, s2 = T.draw(zero, a, lights, ml, u8, (0, 0, 0, 255))
    assert st.cpu().numpy().tolist() == [s0, s1, s2] and s0[0] > 5 and s1[0] > 5 and s2[0] > 2
    assert color.any() and emissive[..., :3].any()
    ctx.close()
    fr = oracle.frame(oracle.Params(W=W, H=H, N=N, ray_range=2.0, rgba8=u8), color, emissive)
    assert np.array_equal(got.view(u32), np.ascontiguousarray(fr.color_out, f32).view(u32)), \
        f"{np.count_nonzero(np.any(got != fr.color_out, axis=-1))} texels differ from the oracle's frame"


def test_a_row_strip_shard_accepts_the_call(R, torch):
    W, H = 96, 64
    AW, AH = C.set_size((16, 16), 4, 3)
    a = atlas_np("float32", AW, AH)
    at = to_dev(torch, a)
    g = C.grid(5, 7, 12, 61)
    m = T.layer((16, 16), (-5, -6), tint=C.TINT)
    ctx = R.RC2DGI(W, H, cascade_count=3)
    ctx.set_shard(0, 2)
    for which in ("color", "emissive"):
        status = tilemap(torch, ctx, which, at, cells_dev(torch, g), m, (4, 3, 2, 255))
        want, ws = T.draw(np.zeros((H, W, 4), f32), a, g, m, False, (4, 3, 2, 255))
        assert status == ws
        same(ctx.download(which), want, which)
    ctx.close()


# ------------------------------------------------------------------ 7. no wait
def test_two_tilemap_calls_and_a_frame_enqueue_behind_a_busy_device(R, torch):
    """On a torch stream given to rc2dgi_set_stream, behind a torch.cuda._sleep sized to three times what the
    synchronising twin's calls took on the host: a layer into COLOR, a layer into EMISSIVE (torch overwrites each grid
    in place as soon as its call has returned), a frame, two reads.  The event behind the sleep is unfinished after
    every call; the frame is the twin's."""
    from test_gpu_pipeline import sleep_cycles_per_ms

    W = H = 256
    AW, AH = C.set_size((16, 16), 4, 3)
    a = atlas_np("uint8", AW, AH)
    a[..., 3] = np.where(a[..., 3] > 100, 255, 0)
    gw, gl = C.grid(17, 17, 12, 71, empty=0.6), C.grid(17, 17, 12, 72, empty=0.9)
    cc, ec = (0, 0, 0, 0), (0, 0, 0, 255)

    def run(ctx, lib, at, grids):
        out = torch.full((H, W, 4), -7.0, device="cuda")
        gi = torch.full(tuple(reversed(ctx.cascade_resolution)) + (4,), -7.0, device="cuda")
        st = torch.full((2, 2), -77, dtype=torch.int32, device="cuda")
        lib("tilemap_device color", lambda: ctx.tilemap_device("color", at, grids[0], (16, 16), (-9, -3), clear=cc,
                                                               replace=True, status=st[0]))
        grids[0].fill_(0x7FC00000)
        lib("tilemap_device emissive", lambda: ctx.tilemap_device("emissive", at, grids[1], (16, 16), (-9, -3), clear=ec,
                                                                  tint=(255, 180, 90, 255), replace=True, status=st[1]))
        grids[1].fill_(-1)
        lib("do", ctx.do_rc2dgi)
        lib("read_into color", lambda: ctx.read_into(out, "color"))
        lib("read_into final_gi", lambda: ctx.read_into(gi, "final_gi"))
        return out, gi, st

    def fresh(stream):
        ctx = R.RC2DGI(W, H, cascade_count=4)
        ctx.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            at = to_dev(torch, a)
            warm = cells_dev(torch, gw)
            ctx.tilemap_device("color", at, warm, (16, 16), status=torch.zeros(2, dtype=torch.int32, device="cuda"))
            ctx.do_rc2dgi()  # (the counters and the tables: allocated)
        ctx.sync()
        return ctx, at

    stream = torch.cuda.Stream()
    twin, at = fresh(stream)
    with torch.cuda.stream(stream):
        grids = [cells_dev(torch, gw), cells_dev(torch, gl)]
        stream.synchronize()

        def stepwise(name, fn):
            fn()
            twin.sync()

        t0 = time.perf_counter()
        want = run(twin, stepwise, at, grids)
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
        grids = [cells_dev(torch, gw), cells_dev(torch, gl)]
        stream.synchronize()
        plug = torch.cuda.Event()
        torch.cuda._sleep(int(sleep_ms * rate))
        plug.record()

        def lib(name, fn):
            fn()
            queried.append((name, plug.query()))

        got = run(ctx, lib, at, grids)
        still_busy = not plug.query()
    ctx.sync()
    got = [t.cpu().numpy() for t in got]
    ctx.set_stream(None)
    ctx.close()
    print(f"\nstepwise twin {twin_seconds * 1e3:.2f} ms on the host, sleep {sleep_ms:.2f} ms")
    waited = [name for name, done in queried if done]
    assert not waited, f"the plug had run out after {waited[0]}"
    assert still_busy, "the device was idle before the last call returned"
    m = T.layer((16, 16), (-9, -3))
    ws = [T.expand(g, AW, AH, W, H, m)[1] for g in (gw, gl)]
    assert got[2].tolist() == ws and want[2].tolist() == ws
    for k, name in enumerate(("color", "final_gi")):
        assert np.array_equal(got[k].view(u32), want[k].view(u32)), f"{name} differs from the synchronising twin's"
    assert not np.array_equal(got[0], np.full_like(got[0], -7.0))


# ------------------------------------------------------------------ 8. argument errors
def test_argument_errors_in_the_documented_order_leave_the_texture(R, torch):
    W, H = 64, 48
    AW, AH = 64, 48
    ctx = R.RC2DGI(W, H, cascade_count=2)
    start = np.broadcast_to(f32([0.375, -2.5, 7.0, 0.625]), (H, W, 4)).copy()
    for which in ("color", "emissive"):
        ctx.upload(which, start)
    L, h, vp = ctx._L, ctx._h, ctypes.c_void_p
    at = to_dev(torch, atlas_np("float32", AW, AH))
    g = C.grid(4, 5, 12, 81, empty=0.0)
    ct = cells_dev(torch, g)
    st = torch.full((4,), -77, dtype=torch.int32, device="cuda")
    clear = (ctypes.c_ubyte * 4)(255, 255, 255, 255)
    p, s, d = ct.data_ptr(), st.data_ptr(), at.data_ptr()
    F32, F16, U8 = R.FMT_RGBA32F, R.FMT_RGBA16F, R.FMT_RGBA8
    A = lambda dev=d, w=AW, hh=AH, pitch=0, fmt=F32: ctypes.byref(R.Atlas(dev, w, hh, pitch, fmt))  # noqa: E731

    def M(cells=p, cols=5, rows=4, pitch=0, tw=16, th=16, ox=0, oy=0, set_cols=4, margin=0, spacing=0, flags=0):
        return ctypes.byref(R.Tilemap(cells, cols, rows, pitch, tw, th, ox, oy, set_cols, margin, spacing, 255, 255, 255,
                                      255, flags))

    good, gm = A(), M()
    lim = 1 << 22
    bad = [("a bad which", b"COLOR", (R.RT["dist"], clear, good, gm, vp(s))),
           ("a bad which before a null atlas", b"COLOR", (-1, clear, None, None, vp(s + 1))),
           ("a null atlas", b"null atlas", (0, clear, None, gm, vp(s))),
           ("a null atlas before a null map", b"null atlas", (0, clear, None, None, vp(s))),
           ("a null atlas image", b"null atlas", (1, clear, A(dev=None), gm, vp(s))),
           ("an atlas 0 wide", b"1 .. 32768 pixels", (0, clear, A(w=0), gm, vp(s))),
           ("an atlas 32769 tall", b"1 .. 32768 pixels", (0, clear, A(hh=32769), gm, vp(s))),
           ("a bad atlas format", b"bad atlas format", (0, clear, A(fmt=3), gm, vp(s))),
           ("a pitch smaller than a row", b"atlas pitch", (0, clear, A(pitch=AW * 16 - 16), gm, vp(s))),
           ("a pitch that is no multiple of a pixel", b"atlas pitch", (0, clear, A(pitch=AW * 16 + 8), gm, vp(s))),
           ("a misaligned atlas", b"aligned to a pixel", (0, clear, A(dev=d + 8), gm, vp(s))),
           ("a misaligned half atlas", b"aligned to a pixel", (0, clear, A(dev=d + 4, fmt=F16), gm, vp(s))),
           ("a misaligned byte atlas", b"aligned to a pixel", (0, clear, A(dev=d + 2, fmt=U8), gm, vp(s))),
           ("a bad atlas before a null map", b"bad atlas format", (0, clear, A(fmt=-1), None, vp(s))),
           ("a null map", b"null map", (0, clear, good, None, vp(s))),
           ("a null map before a misaligned status", b"null map", (0, clear, good, None, vp(s + 1))),
           ("a flip flag", b"flags", (0, clear, good, M(flags=1), vp(s))),
           ("flags 8", b"flags", (0, clear, good, M(flags=12), vp(s))),
           ("flags before cols", b"flags", (0, clear, good, M(flags=2, cols=-1), vp(s))),
           ("cols < 0", b"cols and rows", (0, clear, good, M(cols=-1), vp(s))),
           ("rows > 32768", b"cols and rows", (0, clear, good, M(rows=32769), vp(s))),
           ("cols before the pitch", b"cols and rows", (0, clear, good, M(cols=32769, pitch=3), vp(s))),
           ("a pitch below cols", b"pitch_cells", (0, clear, good, M(pitch=4), vp(s))),
           ("a negative pitch", b"pitch_cells", (0, clear, good, M(pitch=-5), vp(s))),
           ("a pitch above 1 << 20", b"pitch_cells", (0, clear, good, M(pitch=(1 << 20) + 1), vp(s))),
           ("the pitch before the tile", b"pitch_cells", (0, clear, good, M(pitch=4, tw=0), vp(s))),
           ("tile_w 0", b"tile_w and tile_h", (0, clear, good, M(tw=0), vp(s))),
           ("tile_h 32769", b"tile_w and tile_h", (0, clear, good, M(th=32769), vp(s))),
           ("the tile before the origin", b"tile_w and tile_h", (0, clear, good, M(th=-1, ox=lim + 1), vp(s))),
           ("ox above 2^22", b"ox and oy", (0, clear, good, M(ox=lim + 1), vp(s))),
           ("oy below -2^22", b"ox and oy", (0, clear, good, M(oy=-lim - 1), vp(s))),
           ("the origin before set_cols", b"ox and oy", (0, clear, good, M(ox=-lim - 1, set_cols=0), vp(s))),
           ("set_cols 0", b"set_cols is", (0, clear, good, M(set_cols=0), vp(s))),
           ("set_cols 32769", b"set_cols is", (0, clear, good, M(set_cols=32769), vp(s))),
           ("a negative margin", b"set_cols is", (0, clear, good, M(margin=-1), vp(s))),
           ("a spacing of 32769", b"set_cols is", (0, clear, good, M(spacing=32769), vp(s))),
           ("set_cols before the fit", b"set_cols is", (0, clear, good, M(spacing=-1, tw=65), vp(s))),
           ("a tile wider than the atlas", b"tile 0 does not fit", (0, clear, good, M(tw=65), vp(s))),
           ("a margin that pushes tile 0 out", b"tile 0 does not fit", (0, clear, good, M(margin=33, th=16), vp(s))),
           ("the fit before null cells", b"tile 0 does not fit", (0, clear, good, M(cells=None, th=49), vp(s))),
           ("null cells", b"null cells", (1, clear, good, M(cells=None), vp(s))),
           ("null cells before the alignment", b"null cells", (1, clear, good, M(cells=None), vp(s + 2))),
           ("misaligned cells", b"aligned to 4", (0, clear, good, M(cells=p + 2), vp(s))),
           ("a misaligned status", b"aligned to 4", (0, clear, good, gm, vp(s + 3)))]
    for what, word, args in bad:
        assert L.rc2dgi_tilemap_device(h, *args) == -1, what
        assert word in L.rc2dgi_last_error(h), (what, L.rc2dgi_last_error(h))
    assert L.rc2dgi_tilemap_device(None, 0, clear, good, gm, vp(s)) == -1  # a null context, before everything
    ctx.sync()
    assert st.cpu().numpy().tolist() == [-77] * 4, "a refused call writes no status"
    for which in ("color", "emissive"):
        assert np.array_equal(ctx.download(which).view(u32), start.view(u32)), which
    # on the bounds: accepted
    for what, m in (("null cells with an empty grid", M(cells=None, cols=0)), ("rows == 0", M(cells=None, rows=0)),
                    ("the origin on its bounds, off the target", M(ox=lim, oy=-lim)),
                    ("a tile as large as the atlas", M(tw=64, th=48, set_cols=1, ox=-lim)),
                    ("pitch == cols, the largest spacing", M(pitch=5, spacing=32768, set_cols=32768, ox=100))):
        assert L.rc2dgi_tilemap_device(h, 0, None, good, m, vp(s)) == 0, (what, L.rc2dgi_last_error(h))
    ctx.sync()
    assert st.cpu().numpy().tolist()[:2] == [0, 0]
    assert np.array_equal(ctx.download("color").view(u32), start.view(u32)), "nothing of those met the target"
    # the Python arguments
    with pytest.raises(TypeError):
        ctx.tilemap_device("color", at, ct.cpu(), (16, 16))
    with pytest.raises(TypeError):
        ctx.tilemap_device("color", at.cpu(), ct, (16, 16))
    with pytest.raises(TypeError):
        ctx.tilemap_device("color", at, ct.to(torch.int64), (16, 16))
    with pytest.raises(TypeError):
        ctx.tilemap_device("color", at.to(torch.float64), ct, (16, 16))
    with pytest.raises(ValueError):
        ctx.tilemap_device("color", at, ct.reshape(-1), (16, 16))
    with pytest.raises(ValueError):
        ctx.tilemap_device("color", at, ct[:, ::2], (16, 16))
    with pytest.raises(ValueError):
        ctx.tilemap_device("color", at[:, :, :3], ct, (16, 16))
    with pytest.raises(ValueError):
        ctx.tilemap_device("color", at, ct, (16, 16), status=st)
    with pytest.raises(R.RC2DGIError):
        ctx.tilemap_device("dist", at, ct, (16, 16))
    ctx.close()
