"""What a row-strip shard must hold after a frame, bit for bit against the unsharded frame: shared by the in-process
group frame (test_gpu_shard.py, test_gpu_shard_edges.py) and the ranks over the stand-in transport
(rccl_ranks_worker.py)."""
import numpy as np

WHOLE_FRAME_TEXTURES = ("color", "temp", "dist", "jump1", "jump2", "blur", "final_gi")


def whole_frame(R, W, H, N, rr, rs, blur, color, emis, storage=None, keep_levels=False, uniforms=None, **ctx_kw):
    """The unsharded frame on a plain context: every texture the shards are compared with; with keep_levels also
    "levels", the list of every level G_L as its pass stored it.  uniforms: {name: value} set before the frame;
    ctx_kw: further keywords of the context (linux_merge_fallback)."""
    kw = dict(ctx_kw) if storage is None else dict(ctx_kw, storage=storage)
    ctx = R.RC2DGI(W, H, cascade_count=N, render_scale=rs, ray_range=rr, **kw)
    ctx.set_shader_value("_BlurRadius", blur)
    for name, value in (uniforms or {}).items():
        ctx.set_shader_value(name, value)
    if keep_levels:
        ctx.set_keep_levels(True)
    ctx.frame(color, emis)
    ctx.sync()
    out = {k: ctx.download(k) for k in WHOLE_FRAME_TEXTURES}
    if keep_levels:
        out["levels"] = [ctx.download_level(L) for L in range(N)]
    out["rc_fill_levels"] = ctx.get_tuning("rc_fill_levels")  # (bits: the levels the frame wrote as block fills)
    ctx.close()
    return out


def bits(a):
    """The 32-bit patterns of a float32 array (-0.0 is not +0.0, a NaN equals itself)."""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def level_rows(R, W, H, N, blur, rank, world, rs, L, CH):
    """The rows of level L's CH-row texture that shard `rank` computes: the probe rows rc2dgi_plan_rows returns,
    in every one of the level's 2^L direction-block rows."""
    bh = CH >> L
    own = [np.arange(a, b) for a, b in R.plan_rows(W, H, N, blur, rank, world, R.PLAN_LEVEL + L, rs)]
    own = np.concatenate(own) if own else np.zeros(0, np.int64)
    return (np.arange(1 << L)[:, None] * bh + own[None, :]).reshape(-1)


def assert_shard_levels(c, want_levels, W, H, N, blur, rank, world, rs):
    """Context `c` (a synced shard of a W x H frame with kept levels) against the whole frame's levels: level L equals
    want_levels[L] in bits on exactly the probe rows of every direction block the plan gives this rank."""
    from radiancecascade2dglobalillumination_amd import rc2dgi as R

    for L in range(N):
        got = c.download_level(L)
        want = want_levels[L]
        assert got.shape == want.shape, (L, got.shape, want.shape)
        rows = level_rows(R, W, H, N, blur, rank, world, rs, L, got.shape[0])
        assert len(rows) > 0, f"shard {rank} of {world}: no planned row at level {L}"
        mism = np.count_nonzero(bits(got[rows]) != bits(want[rows]))
        assert mism == 0, f"shard {rank} of {world} level {L}: {mism} values differ on {len(rows)} planned rows"


def assert_shard_matches_whole(c, want, W, H, blur, expect_strip_tables, strip_sized=None):
    """Context `c` (a synced shard of a W x H frame) against `want` (whole_frame): raises AssertionError.
    strip_sized: what blur_strip_sized must read; None: the rule of a dyadic radius on the default blur path with
    raylib's merge shader."""
    y0, y1 = c.shard_rows()
    # the merged strip, the JumpFlood textures' own rows (computed on the strip windows with
    # the row exchange) and the whole distance field (all-gathered)
    for k in ("color", "temp", "jump1", "jump2"):
        got = c.download(k)[y0:y1]
        mism = np.count_nonzero(got != want[k][y0:y1])
        assert mism == 0, f"shard {c.shard_rows()} {k}: {mism} values differ"
        if k in ("color", "temp"):
            mism = np.count_nonzero(bits(got) != bits(want[k][y0:y1]))
            assert mism == 0, f"shard {c.shard_rows()} {k}: {mism} values differ in bits"
    # cascadeBlurRT and the blurred final GI (cascades the size of the screen): the own rows; on the fused blur + merge
    # (power-of-two sizes) the shard holds only those (strip-sized textures)
    if c.cascade_resolution == (W, H) and blur > 0:
        for k in ("blur", "final_gi"):
            got = c.download(k)[y0:y1]
            mism = np.count_nonzero(got != want[k][y0:y1])
            assert mism == 0, f"shard {c.shard_rows()} {k}: {mism} values differ"
            mism = np.count_nonzero(bits(got) != bits(want[k][y0:y1]))
            assert mism == 0, f"shard {c.shard_rows()} {k}: {mism} values differ in bits"
    # (the fused blur + merge takes power-of-two cascades of at least 64 x 32 texels: blur_rows_plan)
    pow2 = (W & (W - 1)) == 0 and (H & (H - 1)) == 0 and W >= 64 and H >= 32
    sized = c.get_tuning("blur_strip_sized")
    if strip_sized is None:
        strip_sized = pow2 and c.cascade_resolution == (W, H) and 0 < blur < 3
    assert sized == strip_sized, f"blur_strip_sized {sized}"
    st = c.get_tuning("strip_tables_active")
    assert st == expect_strip_tables, (W, H, st)
    # strip tables on the fused blur + merge: giRT1 / giRT2 hold the shard's band of every direction block
    assert c.get_tuning("cascade_banded") == (st and blur > 0), (W, H, blur)
    # the whole distance field (all-gathered) -- with strip tables the shards exchange the march field
    # instead, and distRT holds the own rows
    d = c.download("dist")
    if st:
        assert np.array_equal(d[y0:y1], want["dist"][y0:y1]), f"shard {c.shard_rows()}: distRT rows"
    else:
        assert np.array_equal(d, want["dist"]), f"shard {c.shard_rows()}: distRT"
