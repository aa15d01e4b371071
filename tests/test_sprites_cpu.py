"""CPU: the host-only half of rc2dgi_sprites_device (include/rc2dgi.h) -- the export in the header, the library, C# and
ctypes, the two structs' layout in C, C# and ctypes, the null-context refusal, pack_sprites against the byte layout of
rc2dgi_sprite, the working memory rc2dgi_paint_device_limits reported before the call existed, and the restatement's
own acceptance rule and 8-bit formulas on a few values worked by hand."""
import ctypes
import os
import re

import numpy as np
import pytest

import sprites_ref
from conftest import ROOT
from test_host_cpu import CS, c_layout
from test_paint_device_cpu import SCREENS

HEADER = os.path.join(ROOT, "include", "rc2dgi.h")
E_ARG = -1
# (batch, working bytes) of rc2dgi_paint_device_limits on SCREENS before rc2dgi_sprites_device shared the memory:
# 256 bytes of counters, batch x 48 bytes of records, batch x 36 x 64 bytes of triangles, batch / 8 bytes a tile
LIMITS = [(8192, 19280128), (8192, 23645440), (8192, 52822272), (4096, 43188480), (8192, 20316416), (2048, 38371584)]


@pytest.fixture(scope="module")
def R():
    from radiancecascade2dglobalillumination_amd import _build, rc2dgi

    _build.build()
    rc2dgi.load_library()
    return rc2dgi


def test_header_declares_the_call_and_both_structs():
    src = open(HEADER).read()
    assert re.search(r"^int rc2dgi_sprites_device\(rc2dgi_ctx \*ctx, int which, const unsigned char \*clear_rgba, "
                     r"const rc2dgi_atlas \*atlas,\s*const void \*sprites_dev, int n, const void \*count_dev, "
                     r"void \*status_dev\);", src, re.M)
    assert re.search(r"typedef struct rc2dgi_atlas \{.*?\} rc2dgi_atlas;", src, re.S)
    assert re.search(r"typedef struct rc2dgi_sprite \{.*?\} rc2dgi_sprite;", src, re.S)
    assert re.search(r"RC2DGI_SPRITE_FLIP_X = 1, RC2DGI_SPRITE_FLIP_Y = 2, RC2DGI_SPRITE_REPLACE = 4", src)
    assert "#define RC2DGI_ABI_VERSION 5" in src
    # the refusal test is restated where a host reads it
    for phrase in ("flags & ~7 != 0", "w > AW - sx or h > AH - sy", "[-2^22, 2^22]"):
        assert phrase in src, phrase


def test_export_is_in_the_library_csharp_and_ctypes(R):
    L = R.load_library()
    cs = open(CS).read()
    assert hasattr(L, "rc2dgi_sprites_device"), "librc2dgi.so does not export rc2dgi_sprites_device"
    assert L.rc2dgi_sprites_device.argtypes is not None and len(L.rc2dgi_sprites_device.argtypes) == 8
    assert re.search(r"public static extern int rc2dgi_sprites_device\(", cs)
    assert re.search(r"public struct Atlas\b", cs) and re.search(r"public struct Sprite\b", cs)
    assert L.rc2dgi_abi_version() == 5
    assert hasattr(R.RC2DGI, "sprites_device") and callable(R.pack_sprites)
    assert (R.SPRITE_FLIP_X, R.SPRITE_FLIP_Y, R.SPRITE_REPLACE) == (1, 2, 4)


def test_structs_are_laid_out_alike_in_c_ctypes_and_csharp(R):
    sizes, fields = c_layout()
    assert sizes["rc2dgi_sprite"] == 32 == ctypes.sizeof(R.Sprite)
    assert sizes["rc2dgi_atlas"] == ctypes.sizeof(R.Atlas)
    for cname, cls in (("rc2dgi_sprite", R.Sprite), ("rc2dgi_atlas", R.Atlas)):
        for name, _ in cls._fields_:
            f = getattr(cls, name)
            assert fields[(cname, name)] == (f.offset, f.size), (cname, name)
    # the C# mirrors: Sequential layout, the fields in the header's order and of its sizes
    cs = open(CS).read()
    body = re.search(r"public struct Sprite\s*\{(.*?)\}", cs, re.S).group(1)
    decl = [ln.split("//")[0].strip() for ln in body.splitlines() if ln.strip()]
    assert decl == ["public int Sx, Sy, W, H;", "public int Dx, Dy;", "public byte R, G, B, A;", "public uint Flags;"]
    body = re.search(r"public struct Atlas\s*\{(.*?)\}", cs, re.S).group(1)
    decl = [ln.split("//")[0].strip() for ln in body.splitlines() if ln.strip()]
    assert decl == ["public void* Dev;", "public int W, H;", "public int PitchBytes;", "public int Format;"]


def test_null_context_is_an_argument_error(R):
    L = R.load_library()
    assert L.rc2dgi_sprites_device(None, 0, None, None, None, 0, None, None) == E_ARG
    a = R.Atlas(64, 8, 8, 0, R.FMT_RGBA8)
    assert L.rc2dgi_sprites_device(None, 1, None, ctypes.byref(a), ctypes.c_void_p(64), 3, ctypes.c_void_p(4),
                                   ctypes.c_void_p(8)) == E_ARG


def test_pack_sprites_lays_out_rc2dgi_sprite():
    import torch

    from radiancecascade2dglobalillumination_amd.rc2dgi import Sprite, pack_sprites

    rng = np.random.default_rng(6)
    n = 41
    src = rng.integers(-5, 4000, (n, 4)).astype(np.int32)
    dst = rng.integers(-(1 << 23), 1 << 23, (n, 2)).astype(np.int32)
    src[1] = [2**31 - 1, -2**31, 1, 1]
    tint = rng.integers(0, 256, (n, 4)).astype(np.uint8)
    tint[0] = [1, 2, 3, 255]  # (word 6 = 0xFF030201: the top bit set)
    flags = rng.integers(0, 8, n)
    flags[2] = 0x80000007 - (1 << 32)  # (a flag word with the top bit set: an int32 the device will refuse)
    got = pack_sprites(torch.from_numpy(src), torch.from_numpy(dst), torch.from_numpy(tint), torch.from_numpy(flags))
    assert got.dtype == torch.int32 and tuple(got.shape) == (n, 8) and got.is_contiguous()
    arr = (Sprite * n)()
    for k in range(n):
        arr[k] = Sprite(*(int(v) for v in src[k]), *(int(v) for v in dst[k]), *(int(v) for v in tint[k]),
                        int(flags[k]) & 0xFFFFFFFF)
    assert got.numpy().tobytes() == bytes(arr)
    assert int(got[0, 6]) == np.int32(np.uint32(0xFF030201).view(np.int32))
    assert np.array_equal(sprites_ref.words([tuple(src[k]) + tuple(dst[k]) + (tuple(tint[k]), int(flags[k]))
                                             for k in range(n)]), got.numpy()), "the restatement's packing"
    # the defaults: a white tint and no flags
    plain = pack_sprites(torch.from_numpy(src), torch.from_numpy(dst))
    assert np.array_equal(plain[:, :6].numpy(), got[:, :6].numpy())
    assert plain[:, 6].tolist() == [-1] * n and plain[:, 7].tolist() == [0] * n
    empty = pack_sprites(torch.zeros((0, 4), dtype=torch.int32), torch.zeros((0, 2), dtype=torch.int32),
                         torch.zeros((0, 4), dtype=torch.uint8), torch.zeros(0, dtype=torch.int64))
    assert tuple(empty.shape) == (0, 8) and empty.dtype == torch.int32
    assert tuple(pack_sprites(torch.zeros((0, 4), dtype=torch.int32), torch.zeros((0, 2), dtype=torch.int32)).shape) == (0, 8)
    with pytest.raises(ValueError):
        pack_sprites(torch.from_numpy(src.astype(np.int64)), torch.from_numpy(dst))
    with pytest.raises(ValueError):
        pack_sprites(torch.from_numpy(src), torch.from_numpy(dst[:, :1].copy()))
    with pytest.raises(ValueError):
        pack_sprites(torch.from_numpy(src), torch.from_numpy(dst), torch.from_numpy(tint[:, :3].copy()))
    with pytest.raises(ValueError):
        pack_sprites(torch.from_numpy(src), torch.from_numpy(dst), torch.from_numpy(tint.astype(np.int32)))
    with pytest.raises(ValueError):
        pack_sprites(torch.from_numpy(src), torch.from_numpy(dst), None, torch.from_numpy(flags.astype(np.float32)))


@pytest.mark.parametrize("screen,want", list(zip(SCREENS, LIMITS)), ids=lambda v: str(v))
def test_paint_device_limits_are_what_they_were(R, screen, want):
    assert R.paint_device_limits(*screen) == want


def test_white_tint_is_one_in_both_storages():
    assert np.float32(255) * (np.float32(1) / np.float32(255)) == np.float32(1)
    assert np.float32(255) / np.float32(255) == np.float32(1)
    assert sprites_ref.tint_of(-1, True).tolist() == [1.0] * 4 and sprites_ref.tint_of(-1, False).tolist() == [1.0] * 4


def test_the_restatement_on_values_worked_by_hand():
    S = sprites_ref
    # the acceptance rule, one record a term (atlas 37 x 29)
    ok = (0, 0, 37, 29, 0, 0, (255,) * 4, 7)
    rows = [ok, (0, 0, 37, 29, 0, 0, (255,) * 4, 8), (0, 0, 0, 1, 0, 0, (255,) * 4, 0), (0, 0, 1, 0, 0, 0, (255,) * 4, 0),
            (-1, 0, 1, 1, 0, 0, (255,) * 4, 0), (0, -1, 1, 1, 0, 0, (255,) * 4, 0), (1, 0, 37, 1, 0, 0, (255,) * 4, 0),
            (0, 1, 1, 29, 0, 0, (255,) * 4, 0), (2**31 - 1, 0, 1, 1, 0, 0, (255,) * 4, 0),
            (0, 0, 1, 1, (1 << 22) + 1, 0, (255,) * 4, 0), (0, 0, 1, 1, 0, -(1 << 22) - 1, (255,) * 4, 0),
            (36, 28, 1, 1, 1 << 22, -(1 << 22), (255,) * 4, 0)]
    assert S.accepted(S.words(rows), 37, 29).tolist() == [True] + [False] * 10 + [True]
    # q8 and mul8 as the header writes them
    assert S.q8(np.float32([np.nan, -1.0, 0.0, 0.5, 1.0, 7.0, np.inf, -np.inf])).tolist() == [0, 0, 0, 128, 255, 255, 255, 0]
    assert [int(S.mul8(np.int64(x), np.int64(y))) for x, y in [(255, 255), (255, 0), (128, 128), (1, 127), (1, 128)]] == \
        [255, 0, 64, 0, 1]
    # one opaque red pixel of an RGBA8 atlas, tinted half grey, into the top-left pixel of a 3 x 2 target
    atlas = np.zeros((2, 2, 4), np.uint8)
    atlas[1, 0] = [255, 0, 0, 255]
    wd = S.words([(0, 1, 1, 1, 0, 0, (128, 128, 128, 255), 0)])
    out = S.draw(np.zeros((2, 3, 4), np.float32), atlas, wd)
    half = np.float32(128) / np.float32(255)
    assert out[1, 0].tolist() == [float(half), 0.0, 0.0, 1.0] and not out[0].any() and not out[1, 1:].any()
    out = S.draw(np.zeros((2, 3, 4), np.uint8), atlas, wd, rgba8=True)
    assert out[1, 0].tolist() == [128, 0, 0, 255] and not out[0].any() and not out[1, 1:].any()
    # FLIP_X | FLIP_Y shows the opposite corner; the count cuts the list; a clear comes first
    wd = S.words([(0, 0, 2, 2, 1, 0, (255,) * 4, S.FLIP_X | S.FLIP_Y | S.REPLACE), (0, 0, 2, 2, 0, 0, (255,) * 4, 4)])
    out = S.draw(np.zeros((2, 3, 4), np.uint8), atlas, wd, rgba8=True, clear=(9, 9, 9, 9), m=1)
    assert out[1, 2].tolist() == [255, 0, 0, 255] and out[1, 0].tolist() == [9, 9, 9, 9] and out[0, 1].tolist() == [0] * 4
