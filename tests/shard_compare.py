"""What a row-strip shard must hold after a frame, bit for bit against the unsharded frame: shared by the in-process
group frame (test_gpu_shard.py) and the ranks over the stand-in transport (rccl_ranks_worker.py)."""
import numpy as np

WHOLE_FRAME_TEXTURES = ("color", "temp", "dist", "jump1", "jump2", "blur", "final_gi")


def whole_frame(R, W, H, N, rr, rs, blur, color, emis, storage=None):
    """The unsharded frame on a plain context: every texture the shards are compared with."""
    kw = {} if storage is None else {"storage": storage}
    ctx = R.RC2DGI(W, H, cascade_count=N, render_scale=rs, ray_range=rr, **kw)
    ctx.set_shader_value("_BlurRadius", blur)
    ctx.frame(color, emis)
    ctx.sync()
    out = {k: ctx.download(k) for k in WHOLE_FRAME_TEXTURES}
    ctx.close()
    return out


def assert_shard_matches_whole(c, want, W, H, blur, expect_strip_tables):
    """Context `c` (a synced shard of a W x H frame) against `want` (whole_frame): raises AssertionError."""
    y0, y1 = c.shard_rows()
    # the merged strip, the JumpFlood textures' own rows (computed on the strip windows with
    # the row exchange) and the whole distance field (all-gathered)
    for k in ("color", "temp", "jump1", "jump2"):
        got = c.download(k)[y0:y1]
        mism = np.count_nonzero(got != want[k][y0:y1])
        assert mism == 0, f"shard {c.shard_rows()} {k}: {mism} values differ"
    # cascadeBlurRT and the blurred final GI (cascades the size of the screen): the own rows; on the fused blur + merge
    # (power-of-two sizes) the shard holds only those (strip-sized textures)
    if c.cascade_resolution == (W, H) and blur > 0:
        for k in ("blur", "final_gi"):
            got = c.download(k)[y0:y1]
            mism = np.count_nonzero(got != want[k][y0:y1])
            assert mism == 0, f"shard {c.shard_rows()} {k}: {mism} values differ"
    # (the fused blur + merge takes power-of-two cascades of at least 64 x 32 texels: blur_rows_plan)
    pow2 = (W & (W - 1)) == 0 and (H & (H - 1)) == 0 and W >= 64 and H >= 32
    sized = c.get_tuning("blur_strip_sized")
    assert sized == (pow2 and c.cascade_resolution == (W, H) and 0 < blur < 3), f"blur_strip_sized {sized}"
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
