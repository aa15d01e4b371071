"""CPU: the host-only half of rc2dgi_paint_device (include/rc2dgi.h) -- rc2dgi_paint_device_limits on the screens the
interface admits and on both sides of every step of the plan, the two exports in the header, the library, C# and ctypes, the null-context refusal, and pack_prims
against the byte layout of rc2dgi_prim."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_host_cpu import CS

HEADER = os.path.join(ROOT, "include", "rc2dgi.h")
CALLS = ["rc2dgi_paint_device", "rc2dgi_paint_device_limits"]
E_ARG = -1
SCREENS = [(64, 48), (1200, 900), (4096, 4096), (8192, 8192), (32768, 8), (32768, 32768)]


@pytest.fixture(scope="module")
def R():
    from radiancecascade2dglobalillumination_amd import _build, rc2dgi

    _build.build()
    rc2dgi.load_library()
    return rc2dgi


@pytest.mark.parametrize("W,H", SCREENS)
def test_limits_fit_the_promise(R, W, H):
    batch, work = R.paint_device_limits(W, H)
    assert 256 <= batch <= 1 << 20
    assert 0 < work <= 64 << 20
    assert (batch, work) == R.paint_device_limits(W, H)  # a function of the screen size alone
    assert work >= batch * 24  # (it holds at least a batch of set-up records, none smaller than rc2dgi_prim)


def plan(W, H):
    """paint_dev_plan restated from the comments of rc2dgi_paint.h and rc2dgi_paint_dev.hip: (tile_h, batch, bytes).
    A tile is 64 x tile_h texels with a mask of `batch` bits; from 64 x 4 and 8192 the tile grows to 16 rows, then the
    batch halves down to 2048, then the tile grows again, while the masks exceed 40 MiB.  The working memory is 256
    bytes of counters, `batch` set-up records of 48 bytes, 36 triangle slots of 64 bytes a record, and the masks."""
    tile_h, batch, tiles_x = 4, 8192, (W + 63) // 64
    masks = lambda: tiles_x * ((H + tile_h - 1) // tile_h) * (batch // 8)  # noqa: E731
    while masks() > 40 << 20:
        if tile_h < 16:
            tile_h *= 2
        elif batch > 2048:
            batch //= 2
        else:
            tile_h *= 2
    return tile_h, batch, 256 + batch * 48 + batch * 36 * 64 + masks()


# W = 32768 is 512 tile columns, so 40 MiB are 80 tile rows of 8192-bit masks: (H below the step, tile_h, batch there)
STEPS = [(320, 4, 8192), (640, 8, 8192), (1280, 16, 8192), (2560, 16, 4096), (5120, 16, 2048), (10240, 32, 2048),
         (20480, 64, 2048), (32768, 128, 2048)]


def test_the_restated_plan_steps_where_the_arithmetic_says():
    """the restatement against the steps worked out by hand: the last height of each plan, the first of the next (one
    row more starts another tile row) and the height four rows on"""
    assert plan(64, 48)[:2] == (4, 8192) and plan(1200, 900)[:2] == (4, 8192)
    for k, (H, th, b) in enumerate(STEPS):
        assert plan(32768, H)[:2] == (th, b), H
        if k + 1 < len(STEPS):
            assert plan(32768, H + 1)[:2] == plan(32768, H + 4)[:2] == STEPS[k + 1][1:], H
    assert plan(4096, 4096)[:2] == (8, 8192)
    assert plan(8192, 8192)[:2] == (16, 4096)
    assert plan(32768, 32768)[:2] == (128, 2048)
    assert plan(32768, 324)[:2] == (8, 8192) and plan(32768, 644)[:2] == (16, 8192)  # (the GPU tests' natural plans)


@pytest.mark.parametrize("W,H", [(32768, H + d) for H, _, _ in STEPS[:-1] for d in (0, 1, 4)] +
                         [(32768, 1), (4096, 4096), (8192, 8192), (32768, 32768), (4097, 4096), (333, 250), (200, 150)])
def test_limits_report_the_restated_plan(R, W, H):
    tile_h, batch, work = plan(W, H)
    assert R.paint_device_limits(W, H) == (batch, work), (tile_h, batch, work)
    assert work - (256 + batch * 48 + batch * 36 * 64) <= 40 << 20


def test_limits_depend_on_the_screen_size_alone(R):
    L = R.load_library()
    out = set()
    for N, storage, scale in [(2, 0, 1.0), (6, 1, 0.5), (12, 2, 2.0)]:
        cfg = R._Config(1200, 900, N, scale, 2.0, storage, 0, 0, (ctypes.c_int * 4)())
        b, w = ctypes.c_int(), ctypes.c_longlong()
        assert L.rc2dgi_paint_device_limits(ctypes.byref(cfg), ctypes.byref(b), ctypes.byref(w)) == 0
        out.add((b.value, w.value))
    assert out == {R.paint_device_limits(1200, 900)}


def test_limits_refuse_a_null_config_and_a_bad_screen(R):
    L = R.load_library()
    b, w = ctypes.c_int(-5), ctypes.c_longlong(-5)
    assert L.rc2dgi_paint_device_limits(None, ctypes.byref(b), ctypes.byref(w)) == E_ARG
    assert (b.value, w.value) == (-5, -5)
    for W, H in [(0, 8), (8, 0), (-1, 8), (32769, 8), (8, 32769)]:
        cfg = R._Config(screen_width=W, screen_height=H)
        assert L.rc2dgi_paint_device_limits(ctypes.byref(cfg), ctypes.byref(b), ctypes.byref(w)) == E_ARG, (W, H)
        with pytest.raises(R.RC2DGIError):
            R.paint_device_limits(W, H)
    cfg = R._Config(screen_width=64, screen_height=48)
    assert L.rc2dgi_paint_device_limits(ctypes.byref(cfg), None, None) == 0  # either pointer may be null


def test_header_declares_the_two_calls():
    src = open(HEADER).read()
    assert re.search(r"^int rc2dgi_paint_device\(rc2dgi_ctx \*ctx, int which, const unsigned char \*clear_rgba, "
                     r"const void \*prims_dev, int n,\s*const void \*count_dev, void \*status_dev\);", src, re.M)
    assert re.search(r"^int rc2dgi_paint_device_limits\(const rc2dgi_config \*cfg, int \*batch_prims, "
                     r"long long \*work_bytes\);", src, re.M)
    assert "#define RC2DGI_ABI_VERSION 5" in src
    # the refusal test is restated where a host reads it
    for phrase in ("fabsf(c) < lim", "fabsf(x) + fabsf(w) < lim", "x + w", "lim = 2^22"):
        assert phrase in src, phrase


def test_exports_are_in_the_library_csharp_and_ctypes(R):
    L = R.load_library()
    cs = open(CS).read()
    for name in CALLS:
        assert hasattr(L, name), f"librc2dgi.so does not export {name}"
        assert getattr(L, name).argtypes is not None, f"rc2dgi.py gives {name} no ctypes signature"
        assert re.search(r"public static extern int %s\(" % name, cs), f"RC2DGINative.cs does not declare {name}"
    assert len(L.rc2dgi_paint_device.argtypes) == 7 and len(L.rc2dgi_paint_device_limits.argtypes) == 3
    assert L.rc2dgi_abi_version() == 5
    assert hasattr(R.RC2DGI, "paint_device") and callable(R.pack_prims) and callable(R.paint_device_limits)


def test_null_context_is_an_argument_error(R):
    L = R.load_library()
    assert L.rc2dgi_paint_device(None, 0, None, None, 0, None, None) == E_ARG
    assert L.rc2dgi_paint_device(None, 1, None, ctypes.c_void_p(64), 3, ctypes.c_void_p(4), ctypes.c_void_p(8)) == E_ARG


def test_pack_prims_lays_out_rc2dgi_prim():
    import torch

    from radiancecascade2dglobalillumination_amd.rc2dgi import Prim, pack_prims

    rng = np.random.default_rng(5)
    n = 37
    kind = rng.integers(0, 2, n)
    xywh = rng.uniform(-100, 100, (n, 4)).astype(np.float32)
    xywh[3] = [np.nan, -0.0, np.inf, 1e-40]
    rgba = rng.integers(0, 256, (n, 4)).astype(np.uint8)
    rgba[0] = [1, 2, 3, 255]  # (word 5 = 0xFF030201: the top bit set)
    got = pack_prims(torch.from_numpy(kind), torch.from_numpy(xywh), torch.from_numpy(rgba))
    assert got.dtype == torch.int32 and tuple(got.shape) == (n, 6) and got.is_contiguous()
    arr = (Prim * n)()
    for k in range(n):
        arr[k] = Prim(int(kind[k]), *(float(v) for v in xywh[k]), *(int(v) for v in rgba[k]))
    assert got.numpy().tobytes() == bytes(arr)
    assert int(got[0, 5]) == np.int32(np.uint32(0xFF030201).view(np.int32))
    assert tuple(pack_prims(torch.zeros(0, dtype=torch.int64), torch.zeros((0, 4)), torch.zeros((0, 4), dtype=torch.uint8)).shape) == (0, 6)
    with pytest.raises(ValueError):
        pack_prims(torch.from_numpy(kind), torch.from_numpy(xywh.astype(np.float64)), torch.from_numpy(rgba))
    with pytest.raises(ValueError):
        pack_prims(torch.from_numpy(kind), torch.from_numpy(xywh), torch.from_numpy(rgba[:, :3].copy()))
