"""CPU: the host-only half of rc2dgi_sprites_xf_device (include/rc2dgi.h) -- the export in the header, the library, C#
and ctypes, the record's layout in C, C# and ctypes, the null-context refusal, pack_sprites_xf against the byte layout of
rc2dgi_sprite_xf, sprites_xf_from_pro on values worked by hand, the unchanged working memory, and the restatement
(tests/sprites_xf_ref.py) alone: each refusal term on one record apiece, values worked by hand, and the header's three
"consequences" -- identity lists equal the 1:1 restatement (tests/sprites_ref.py), whole upscales equal np.repeat,
quarter turns equal np.rot90 and mirrors equal the FLIP sprites.  The GPU tests use those consequences on the strength
of these assertions."""
import ctypes
import os
import re

import numpy as np
import pytest

import sprites_ref as S1
import sprites_xf_ref as S
from conftest import ROOT
from test_host_cpu import CS, c_layout
from test_paint_device_cpu import SCREENS
from test_sprites_cpu import LIMITS

HEADER = os.path.join(ROOT, "include", "rc2dgi.h")
E_ARG = -1
f32 = np.float32
WHITE = (255, 255, 255, 255)
AW, AH = 37, 29


@pytest.fixture(scope="module")
def R():
    from radiancecascade2dglobalillumination_amd import _build, rc2dgi

    _build.build()
    rc2dgi.load_library()
    return rc2dgi


# ------------------------------------------------------------------ the export and the record
def test_header_declares_the_call_the_struct_and_the_contract():
    src = open(HEADER).read()
    assert re.search(r"^int rc2dgi_sprites_xf_device\(rc2dgi_ctx \*ctx, int which, const unsigned char \*clear_rgba, "
                     r"const rc2dgi_atlas \*atlas,\s*const void \*sprites_dev, int n, const void \*count_dev, "
                     r"void \*status_dev\);", src, re.M)
    assert re.search(r"typedef struct rc2dgi_sprite_xf \{.*?\} rc2dgi_sprite_xf;", src, re.S)
    assert re.search(r"RC2DGI_SPRITE_LINEAR = 8", src)
    assert "#define RC2DGI_ABI_VERSION 5" in src
    # the contract is restated where a host reads it
    for phrase in ("flags & ~(4 | 8) != 0", "w > AW - sx or h > AH - sy", "fabsf(c) <= 0x1p20f", "fabsf(det) >= 0x1p-20f",
                   "det = ax * by - ay * bx", "i00 = by / det, i01 = (-bx) / det, i10 = (-ay) / det, i11 = ax / det",
                   "X0 = max((int)floorf(lo_x) - 1, 0), X1 = min((int)floorf(hi_x) + 1, W - 1)",
                   "a = dxp * i00 + dyp * i01, b = dxp * i10 + dyp * i11", "a >= 0 && a < 1 && b >= 0 && b < 1",
                   "sx + min((int)s, w - 1), sy + min((int)t, h - 1)", "lerp(p, q, f) = p + f * (q - p)",
                   "has not been probed against a GL implementation"):
        assert phrase in src, phrase


def test_export_is_in_the_library_csharp_and_ctypes(R):
    L = R.load_library()
    cs = open(CS).read()
    assert hasattr(L, "rc2dgi_sprites_xf_device"), "librc2dgi.so does not export rc2dgi_sprites_xf_device"
    assert L.rc2dgi_sprites_xf_device.argtypes is not None and len(L.rc2dgi_sprites_xf_device.argtypes) == 8
    assert re.search(r"public static extern int rc2dgi_sprites_xf_device\(", cs)
    assert re.search(r"public struct SpriteXf\b", cs) and re.search(r"public const uint SpriteLinear = 8;", cs)
    assert L.rc2dgi_abi_version() == 5
    assert hasattr(R.RC2DGI, "sprites_xf_device") and callable(R.pack_sprites_xf) and callable(R.sprites_xf_from_pro)
    assert R.SPRITE_LINEAR == 8 and R.SPRITE_REPLACE == 4


def test_struct_is_laid_out_alike_in_c_ctypes_and_csharp(R):
    sizes, fields = c_layout()
    assert sizes["rc2dgi_sprite_xf"] == 48 == ctypes.sizeof(R.SpriteXf)
    for name, _ in R.SpriteXf._fields_:
        f = getattr(R.SpriteXf, name)
        assert fields[("rc2dgi_sprite_xf", name)] == (f.offset, f.size), name
    assert [n for n, _ in R.SpriteXf._fields_] == ["sx", "sy", "w", "h", "px", "py", "ax", "ay", "bx", "by", "r", "g",
                                                   "b", "a", "flags"]
    assert [fields[("rc2dgi_sprite_xf", n)][0] for n in ("sx", "px", "ax", "bx", "r", "flags")] == [0, 16, 24, 32, 40, 44]
    cs = open(CS).read()
    assert re.search(r"\[StructLayout\(LayoutKind\.Sequential, Size = 48\)\]\s*public struct SpriteXf\b", cs)
    body = re.search(r"public struct SpriteXf\s*\{(.*?)\}", cs, re.S).group(1)
    decl = [ln.split("//")[0].strip() for ln in body.splitlines() if ln.strip()]
    assert decl == ["public int Sx, Sy, W, H;", "public float Px, Py;", "public float Ax, Ay;", "public float Bx, By;",
                    "public byte R, G, B, A;", "public uint Flags;"]


def test_null_context_is_an_argument_error(R):
    L = R.load_library()
    assert L.rc2dgi_sprites_xf_device(None, 0, None, None, None, 0, None, None) == E_ARG
    a = R.Atlas(64, 8, 8, 0, R.FMT_RGBA8)
    assert L.rc2dgi_sprites_xf_device(None, 1, None, ctypes.byref(a), ctypes.c_void_p(64), 3, ctypes.c_void_p(4),
                                      ctypes.c_void_p(8)) == E_ARG


@pytest.mark.parametrize("screen,want", list(zip(SCREENS, LIMITS)), ids=lambda v: str(v))
def test_paint_device_limits_are_what_they_were(R, screen, want):
    assert R.paint_device_limits(*screen) == want


# ------------------------------------------------------------------ the two Python helpers
def test_pack_sprites_xf_lays_out_rc2dgi_sprite_xf():
    import torch

    from radiancecascade2dglobalillumination_amd.rc2dgi import SpriteXf, pack_sprites_xf

    rng = np.random.default_rng(7)
    n = 41
    src = rng.integers(-5, 4000, (n, 4)).astype(np.int32)
    src[1] = [2**31 - 1, -2**31, 1, 1]
    pab = rng.uniform(-3000, 3000, (n, 6)).astype(f32)
    pab[0] = [np.nan, np.inf, -np.inf, -0.0, 1e-42, 2.0 ** 20]  # (every bit pattern goes through as it is)
    tint = rng.integers(0, 256, (n, 4)).astype(np.uint8)
    tint[0] = [1, 2, 3, 255]  # (word 10 = 0xFF030201: the top bit set)
    flags = rng.integers(0, 16, n)
    flags[2] = 0x8000000C - (1 << 32)
    t = torch.from_numpy
    got = pack_sprites_xf(t(src), t(pab[:, 0:2].copy()), t(pab[:, 2:4].copy()), t(pab[:, 4:6].copy()), t(tint), t(flags))
    assert got.dtype == torch.int32 and tuple(got.shape) == (n, 12) and got.is_contiguous()
    arr = (SpriteXf * n)()
    for k in range(n):
        arr[k] = SpriteXf(*(int(v) for v in src[k]), *(float(v) for v in pab[k]), *(int(v) for v in tint[k]),
                          int(flags[k]) & 0xFFFFFFFF)
    want = np.frombuffer(bytes(arr), np.int32).reshape(n, 12).copy()
    want[:, 4:10] = pab.view(np.int32)  # (ctypes quiets a signalling NaN on the way through a Python float; none here)
    assert np.array_equal(got.numpy(), want)
    assert got.numpy()[1:].tobytes() == bytes(arr)[48:]
    assert int(got[0, 10]) == np.int32(np.uint32(0xFF030201).view(np.int32))
    assert np.array_equal(S.words([tuple(src[k]) + tuple(pab[k]) + (tuple(tint[k]), int(flags[k])) for k in range(n)]),
                          got.numpy()), "the restatement's packing"
    # the defaults: a white tint and no flags
    plain = pack_sprites_xf(t(src), t(pab[:, 0:2].copy()), t(pab[:, 2:4].copy()), t(pab[:, 4:6].copy()))
    assert np.array_equal(plain[:, :10].numpy(), got[:, :10].numpy())
    assert plain[:, 10].tolist() == [-1] * n and plain[:, 11].tolist() == [0] * n
    z4, z2 = torch.zeros((0, 4), dtype=torch.int32), torch.zeros((0, 2), dtype=torch.float32)
    assert tuple(pack_sprites_xf(z4, z2, z2, z2).shape) == (0, 12)
    p, a, b = t(pab[:, 0:2].copy()), t(pab[:, 2:4].copy()), t(pab[:, 4:6].copy())
    with pytest.raises(ValueError):
        pack_sprites_xf(t(src.astype(np.int64)), p, a, b)
    with pytest.raises(ValueError):
        pack_sprites_xf(t(src), p[:, :1], a, b)
    with pytest.raises(ValueError):
        pack_sprites_xf(t(src), p, a.to(torch.float64), b)
    with pytest.raises(ValueError):
        pack_sprites_xf(t(src), p, a, b.to(torch.int32))
    with pytest.raises(ValueError):
        pack_sprites_xf(t(src), p, a, b, t(tint[:, :3].copy()))
    with pytest.raises(ValueError):
        pack_sprites_xf(t(src), p, a, b, None, t(flags.astype(np.float32)))


def test_sprites_xf_from_pro_on_values_worked_by_hand():
    """DrawTexturePro's geometry to float tolerance only: the trigonometry is torch's and outside the exact contract"""
    import torch

    from radiancecascade2dglobalillumination_amd.rc2dgi import sprites_xf_from_pro

    dest = torch.tensor([[10.0, 20.0, 30.0, 40.0]] * 4)
    origin = torch.tensor([[0.0, 0.0], [0.0, 0.0], [15.0, 20.0], [15.0, 20.0]])
    rot = torch.tensor([0.0, 90.0, 90.0, 180.0])
    p, a, b = sprites_xf_from_pro(dest, origin, rot)
    assert all(x.dtype == torch.float32 and tuple(x.shape) == (4, 2) for x in (p, a, b))
    # 0 deg: the destination rectangle itself.  90 deg (clockwise, y down): the top edge points down, the left edge to
    # the left.  With the origin at the centre the rectangle turns about (10, 20): its corner goes to (10 + 20, 20 - 15).
    # 180 deg about the centre: the corner goes to (10 + 15, 20 + 20), both edges reversed.
    np.testing.assert_allclose(p.numpy(), [[10, 20], [10, 20], [30, 5], [25, 40]], atol=1e-4)
    np.testing.assert_allclose(a.numpy(), [[30, 0], [0, 30], [0, 30], [-30, 0]], atol=1e-4)
    np.testing.assert_allclose(b.numpy(), [[0, 40], [-40, 0], [-40, 0], [0, -40]], atol=1e-4)
    assert p[0].tolist() == [10.0, 20.0] and a[0].tolist() == [30.0, 0.0] and b[0].tolist() == [0.0, 40.0]
    with pytest.raises(ValueError):
        sprites_xf_from_pro(dest, origin, rot.to(torch.float64))
    with pytest.raises(ValueError):
        sprites_xf_from_pro(dest[:, :3], origin, rot)
    with pytest.raises(ValueError):
        sprites_xf_from_pro(dest, origin[:2], rot)


# ------------------------------------------------------------------ the restatement alone
def ident(sx, sy, w, h, x, y, tint=WHITE, flags=0):
    return (sx, sy, w, h, x, y, w, 0, 0, h, tint, flags)


def test_each_refusal_term_decides_on_one_record_apiece():
    up = lambda v: float(np.nextafter(f32(v), f32(np.inf)))  # noqa: E731
    down = lambda v: float(np.nextafter(f32(v), f32(0)))  # noqa: E731
    big, e = 2.0 ** 20, 2.0 ** -10
    rows = [(ident(0, 0, 37, 29, 0, 0, WHITE, 12), True),
            (ident(0, 0, 37, 29, 0, 0, WHITE, 1), False),           # RC2DGI_SPRITE_FLIP_X is not accepted here
            (ident(0, 0, 37, 29, 0, 0, WHITE, 2), False),           # nor FLIP_Y
            (ident(0, 0, 37, 29, 0, 0, WHITE, 16), False),          # an undefined bit
            (ident(0, 0, 37, 29, 0, 0, WHITE, -(1 << 31)), False),
            ((0, 0, 0, 1, 0, 0, 1, 0, 0, 1, WHITE, 0), False),      # w < 1
            ((0, 0, 1, 0, 0, 0, 1, 0, 0, 1, WHITE, 0), False),      # h < 1
            (ident(-1, 0, 1, 1, 0, 0), False),                      # sx < 0
            (ident(0, -1, 1, 1, 0, 0), False),                      # sy < 0
            (ident(1, 0, 37, 1, 0, 0), False),                      # w > AW - sx
            (ident(0, 1, 1, 29, 0, 0), False),                      # h > AH - sy
            (ident(2**31 - 1, 0, 1, 1, 0, 0), False),               # (sx near INT_MAX: the form of the comparison)
            (ident(36, 28, 1, 1, 0, 0), True)]
    for k in range(6):  # each of px, py, ax, ay, bx, by: exactly 2^20 is accepted, the next float above it refused
        for v, want in ((big, True), (-big, True), (up(big), False), (-up(big), False), (np.nan, False), (np.inf, False),
                        (-np.inf, False)):
            c = [3.0, 4.0, 5.0, 1.0, -1.0, 6.0]  # (det = 31)
            c[k] = v
            rows.append(((0, 0, 2, 2) + tuple(c) + (WHITE, 0), want))
    rows += [((0, 0, 2, 2, 0, 0, e, 0, 0, e, WHITE, 0), True),            # det = 2^-20 exactly
             ((0, 0, 2, 2, 0, 0, e, 0, 0, down(e), WHITE, 0), False),     # just below it
             ((0, 0, 2, 2, 0, 0, e, 0, 0, -e, WHITE, 0), True),           # det = -2^-20: a mirrored sprite
             ((0, 0, 2, 2, 0, 0, e, 0, 0, -down(e), WHITE, 0), False),
             ((0, 0, 2, 2, 0, 0, 3, 5, 6, 10, WHITE, 0), False),          # det = 0: A and B parallel
             ((0, 0, 2, 2, 0, 0, 0, 0, 0, 0, WHITE, 0), False),
             ((0, 0, 2, 2, 0, 0, 0, e, -e, 0, WHITE, 0), True)]           # det = 0 * 0 - e * -e = 2^-20
    got = S.accepted(S.words([r for r, _ in rows]), AW, AH).tolist()
    assert got == [w for _, w in rows], [k for k, (g, (_, w)) in enumerate(zip(got, rows)) if g != w]


def test_the_restatement_on_values_worked_by_hand():
    # a 2 x 1 source, black then white, over four pixels at (1, 0) of a 6 x 2 target, replacing
    atlas = np.zeros((1, 2, 4), f32)
    atlas[0, 1] = 1.0
    start = np.full((2, 6, 4), 0.5, f32)
    point = S.draw(start, atlas, S.words([(0, 0, 2, 1, 1, 0, 4, 0, 0, 1, WHITE, S.REPLACE)]))
    assert point[1, :, 0].tolist() == [0.5, 0.0, 0.0, 1.0, 1.0, 0.5] and (point[0] == 0.5).all()  # (GL rows: row 1 is the top)
    # LINEAR: s = 0.25, 0.75, 1.25, 1.75; xs = s - 0.5; i0 = -1, 0, 0, 1; fx = 0.75, 0.25, 0.75, 0.25; the taps are
    # clamped into the rectangle, so the ends are the end pixels themselves
    lin = S.draw(start, atlas, S.words([(0, 0, 2, 1, 1, 0, 4, 0, 0, 1, WHITE, S.REPLACE | S.LINEAR)]))
    assert lin[1, :, 0].tolist() == [0.5, 0.0, 0.25, 0.75, 1.0, 0.5] and (lin[0] == 0.5).all()
    # the box: P = (1.5, 0.25), A = (1, 0), B = (0, 1) covers the one centre with 1.5 <= X + 0.5 < 2.5 and
    # 0.25 <= Y + 0.5 < 1.25, pixel (1, 0)
    wd = S.words([(1, 0, 1, 1, 1.5, 0.25, 1, 0, 0, 1, WHITE, S.REPLACE)])
    assert S.box(wd, 6, 2) == (0, 3, 0, 1)
    one = S.draw(start, atlas, wd)
    assert one[1, 1, 0] == 1.0 and np.count_nonzero(one != 0.5) == 4
    # a centre exactly on the left edge is covered (a == 0), one exactly on the right edge is not (a == 1)
    wd = S.words([(1, 0, 1, 1, 1.5, 0.0, 2, 0, 0, 1, WHITE, S.REPLACE)])
    assert (S.draw(start, atlas, wd)[1, :, 0] != 0.5).tolist() == [False, True, True, False, False, False]
    # 8-bit storage, a half-grey tint, blended over black; the count cuts the list; a clear comes first
    a8 = np.zeros((2, 2, 4), np.uint8)
    a8[1, 0] = [255, 0, 0, 255]
    wd = S.words([(0, 1, 1, 1, 0, 0, 2, 0, 0, 2, (128, 128, 128, 255), 0), ident(0, 0, 2, 2, 0, 0, WHITE, 4)])
    out = S.draw(np.zeros((2, 3, 4), np.uint8), a8, wd, rgba8=True, clear=(9, 9, 9, 9), m=1)
    assert out[:, :2].reshape(-1, 4).tolist() == [[128, 0, 0, 255]] * 4 and out[:, 2].tolist() == [[9, 9, 9, 9]] * 2
    assert S.draw(np.zeros((2, 3, 4), np.uint8), a8, wd, rgba8=True, m=-3).any() == False  # noqa: E712


IDENTITY_WIDTHS = list(range(1, 300)) + [1000, 4095, 4096, 4097, 32767, 32768]


def test_consequence_identity_equals_the_one_to_one_sprite():
    """A = (w, 0), B = (0, h), integer P, POINT: the bits of rc2dgi_sprites_device's restatement, for every width up to
    299 and the widths around 2^12 and 2^15 (1 / w is not a float there), hanging over the target's edges too."""
    rng = np.random.default_rng(12)
    for w in IDENTITY_WIDTHS:
        h = 1 + w % 3 if w < 300 else 1
        aw, ah = w + 2, h + 1
        atlas = rng.integers(0, 256, (ah, aw, 4)).astype(np.uint8)
        W, H = w + 7, h + 4
        start = rng.uniform(0, 1, (H, W, 4)).astype(f32)
        for x, y in ((3, 2), (-(w // 2), -1), (W - 1 - w // 3, 3)):
            for flags in (0, S.REPLACE):
                tint = tuple(int(v) for v in rng.integers(0, 256, 4))
                got = S.draw(start, atlas, S.words([ident(1, 1, w, h, x, y, tint, flags)]))
                want = S1.draw(start, atlas, S1.words([(1, 1, w, h, x, y, tint, flags)]))
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (w, h, x, y, flags)
    # tall ones, 8-bit storage
    atlas = rng.integers(0, 256, (300, 5, 4)).astype(np.uint8)
    start = rng.integers(0, 256, (310, 9, 4)).astype(np.uint8)
    for h in (1, 2, 3, 7, 100, 255, 256, 257, 299):
        got = S.draw(start, atlas, S.words([ident(1, 1, 3, h, 2, 4, (200, 100, 50, 180))]), rgba8=True)
        want = S1.draw(start, atlas, S1.words([(1, 1, 3, h, 2, 4, (200, 100, 50, 180), 0)]), rgba8=True)
        assert np.array_equal(got, want), h


def test_consequence_whole_upscales_repeat_every_pixel():
    rng = np.random.default_rng(13)
    atlas = rng.uniform(0, 1, (AH, AW, 4)).astype(f32)
    for k in range(1, 8):
        for m in range(1, 8):
            sx, sy, w, h = 3, 2, 5 + k, 4 + m % 3
            W, H = k * w + 5, m * h + 4
            start = np.zeros((H, W, 4), f32)
            got = S.draw(start, atlas, S.words([(sx, sy, w, h, 2, 1, k * w, 0, 0, m * h, WHITE, S.REPLACE)]))
            want = start.copy()
            want[1:1 + m * h, 2:2 + k * w] = np.repeat(np.repeat(atlas[sy:sy + h, sx:sx + w], m, axis=0), k, axis=1)
            assert np.array_equal(got, want[::-1]), (k, m)  # (the texture is in GL rows)


def test_consequence_quarter_turns_and_mirrors():
    rng = np.random.default_rng(14)
    atlas = rng.integers(0, 256, (AH, AW, 4)).astype(np.uint8)
    W, H = 64, 48
    start = rng.uniform(0, 1, (H, W, 4)).astype(f32)
    for sx, sy, w, h, x, y in ((0, 0, 37, 29, 5, 9), (4, 3, 1, 1, 0, 0), (4, 3, 9, 1, 60, 40), (4, 3, 1, 9, -3, 30),
                               (7, 5, 20, 13, 50, -5)):
        tint = tuple(int(v) for v in rng.integers(0, 256, 4))
        for flags in (0, S.REPLACE):
            # P = (x + w, y), A = (-w, 0), B = (0, h): the FLIP_X sprite; with B = (0, -h) from y + h: FLIP_X | FLIP_Y
            got = S.draw(start, atlas, S.words([(sx, sy, w, h, x + w, y, -w, 0, 0, h, tint, flags)]))
            want = S1.draw(start, atlas, S1.words([(sx, sy, w, h, x, y, tint, flags | S1.FLIP_X)]))
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), ("flip x", w, h)
            got = S.draw(start, atlas, S.words([(sx, sy, w, h, x + w, y + h, -w, 0, 0, -h, tint, flags)]))
            want = S1.draw(start, atlas, S1.words([(sx, sy, w, h, x, y, tint, flags | S1.FLIP_X | S1.FLIP_Y)]))
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), ("flip xy", w, h)
            # P = (x + h, y), A = (0, w), B = (-h, 0): the sub-image turned a quarter clockwise, h wide and w tall,
            # which is the 1:1 sprite of an atlas that holds the turned image
            turned = np.ascontiguousarray(np.rot90(atlas[sy:sy + h, sx:sx + w], -1))
            got = S.draw(start, atlas, S.words([(sx, sy, w, h, x + h, y, 0, w, -h, 0, tint, flags)]))
            want = S1.draw(start, turned, S1.words([(0, 0, h, w, x, y, tint, flags)]))
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), ("turn", w, h)
