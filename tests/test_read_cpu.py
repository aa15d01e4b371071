"""CPU: the host-only half of rc2dgi_read / rc2dgi_read_device (include/rc2dgi.h) -- the two exports, the two constants
in C, C# and Python, the null-context refusal, and tests/read_ref.c, the C restatement the GPU tests compare against:
its float32 -> binary16 conversion (round to nearest even, in integer arithmetic) against numpy on every half, every
midpoint between adjacent halves and the floats beside it, and its crop / flip / pitch on a case worked out by hand."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_host_cpu import CS

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(ROOT, "include", "rc2dgi.h")
CALLS = ["rc2dgi_read", "rc2dgi_read_device"]
E_ARG = -1
FMT_RGBA8, FMT_RGBA32F, FMT_RGBA16F = 0, 1, 2
f32, f16, u16, u32 = np.float32, np.float16, np.uint16, np.uint32


@pytest.fixture(scope="module")
def R():
    from radiancecascade2dglobalillumination_amd import _build, rc2dgi

    _build.build()
    rc2dgi.load_library()
    return rc2dgi


# ------------------------------------------------------------------ tests/read_ref.c (shared with test_read_gpu.py)
def build_read_ref(tmp_path_factory):
    """tests/read_ref.c as a ctypes library, compiled as tests/tone_ref.c is"""
    so = str(tmp_path_factory.mktemp("read_ref") / "libread_ref.so")
    subprocess.run(["gcc", "-O1", "-ffp-contract=off", "-std=c11", "-Wall", "-shared", "-fPIC", "-o", so,
                    os.path.join(HERE, "read_ref.c"), "-lm"], check=True)
    L = ctypes.CDLL(so)
    vp, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    L.read_half.argtypes, L.read_half.restype = [ctypes.c_float], ctypes.c_uint16
    L.read_half_array.argtypes, L.read_half_array.restype = [vp, vp, ll], None
    L.read_q8.argtypes, L.read_q8.restype = [ctypes.c_float], ctypes.c_uint
    L.read_q8_array.argtypes, L.read_q8_array.restype = [vp, vp, ll], None
    L.read_image_ref.argtypes, L.read_image_ref.restype = [vp, i, i, i, i, i, i, i, i, vp, ll], i
    return L


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return build_read_ref(tmp_path_factory)


def ref_half(ref_lib, values):
    """read_ref.c's binary16 bits of float32 values, same shape, uint16"""
    v = np.ascontiguousarray(values, f32)
    out = np.empty(v.shape, u16)
    ref_lib.read_half_array(v.ctypes.data, out.ctypes.data, v.size)
    return out


def ref_q8(ref_lib, values):
    v = np.ascontiguousarray(values, f32)
    out = np.empty(v.shape, np.uint8)
    ref_lib.read_q8_array(v.ctypes.data, out.ctypes.data, v.size)
    return out


DTYPE_FORMAT = {"float32": FMT_RGBA32F, "float16": FMT_RGBA16F, "uint8": FMT_RGBA8}


def ref_image(ref_lib, tex, rect, dtype, flip=False, pitch=None, fill=0xA5):
    """read_ref.c's image of rect (x, y, w, h; None: the whole texture) of tex, float32 (th, tw, 4) as rc2dgi_download
    returns it.  pitch None: the (h, w, 4) array of dtype; else the uint8 (h, pitch) rows, padding bytes = fill."""
    tex = np.ascontiguousarray(tex, f32)
    assert tex.ndim == 3 and tex.shape[2] == 4
    th, tw = tex.shape[:2]
    x, y, w, h = (0, 0, tw, th) if rect is None else (int(v) for v in rect)
    dt = np.dtype(dtype)
    row = w * 4 * dt.itemsize
    out = np.full((h, row if pitch is None else pitch), fill, np.uint8)
    assert ref_lib.read_image_ref(tex.ctypes.data, tw, th, x, y, w, h, DTYPE_FORMAT[dt.name], int(bool(flip)),
                                  out.ctypes.data, out.shape[1]) == 0
    return out.view(dt).reshape(h, w, 4) if pitch is None else out


def same_halves(got, want):
    """two uint16 arrays of binary16 bits are equal, a NaN in one place equal to any NaN in the other"""
    got, want = np.asarray(got, u16), np.asarray(want, u16)
    nan_g, nan_w = (got & 0x7FFF) > 0x7C00, (want & 0x7FFF) > 0x7C00
    return got.shape == want.shape and bool(np.array_equal(nan_g, nan_w) and np.array_equal(got[~nan_g], want[~nan_w]))


# ------------------------------------------------------------------ the conversion sweep (the GPU test uploads it)
SPECIALS = [65520.0, -65520.0, 2.0 ** -25, -(2.0 ** -25), 0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-39,
            -1e-39, 1.1754942e-38, 65519.996, -65519.996, 65536.0, 1e5, -1e5, 3.4028235e38, -3.4028235e38,
            2.0 ** -24, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 2.0 ** -14, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11]


@functools.lru_cache(maxsize=None)
def half_sweep():
    """(65536, 4) float32, read-only.  Row b, for the binary16 bit pattern b: the half as a float; the midpoint between
    it and the next half away from zero (65520 after 65504); that midpoint's float predecessor and successor.  The
    rows of the infinities and NaNs have no midpoint: their three slots hold SPECIALS, the upper neighbour of +-2^-25
    and random bit patterns."""
    b32 = np.arange(65536, dtype=u32)
    b = b32.astype(u16)
    with np.errstate(invalid="ignore"):  # (the NaN halves pass through the casts)
        val = b.view(f16).astype(f32)
        finite = (b & 0x7FFF) < 0x7C00
        last = (b & 0x7FFF) == 0x7BFF  # +-65504: the next binade would start at 2^16
        nb = np.where(finite & ~last, b32 + 1, b32).astype(u16)
        nxt = np.where(last, np.copysign(65536.0, val.astype(np.float64)), nb.view(f16).astype(np.float64))
        mid64 = (val.astype(np.float64) + nxt) / 2
        mid = mid64.astype(f32)
        assert np.array_equal(mid[finite].astype(np.float64), mid64[finite]), "a midpoint of two halves is a float"
        away = np.where(np.signbit(val), f32(-np.inf), f32(np.inf))
        out = np.stack([val, mid, np.nextafter(mid, -away), np.nextafter(mid, away)], 1).astype(f32)
    free = np.argwhere(~finite).reshape(-1)
    rng = np.random.default_rng(7)
    extra = np.concatenate([np.asarray(SPECIALS, f32), np.nextafter(f32(2.0 ** -25), f32(1)).reshape(1),
                            np.nextafter(f32(-(2.0 ** -25)), f32(-1)).reshape(1)])
    fill = rng.integers(0, 1 << 32, 3 * len(free), dtype=np.uint64).astype(u32).view(f32)
    fill[:len(extra)] = extra
    out[free, 1:] = fill.reshape(len(free), 3)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------ the ABI
def test_header_declares_the_two_calls():
    src = open(HEADER).read()
    for name in CALLS:
        assert re.search(r"^int %s\(rc2dgi_ctx \*ctx, int which, const rc2dgi_rect \*rect, int format, int flags,\s*"
                         r"void \*\w+,\s*int pitch_bytes\);" % name, src, re.M), name
    assert "#define RC2DGI_ABI_VERSION 5" in src


def test_library_exports_the_two_calls(R):
    L = R.load_library()
    for name in CALLS:
        assert hasattr(L, name), f"librc2dgi.so does not export {name}"
    assert L.rc2dgi_abi_version() == 5


def test_constants_agree_in_c_csharp_and_python(R, tmp_path):
    c = tmp_path / "consts.c"
    c.write_text('#include <stdio.h>\n#include "rc2dgi.h"\n'
                 'int main(void) { printf("%d %d %d %d\\n", (int)RC2DGI_FMT_RGBA8, (int)RC2DGI_FMT_RGBA32F, '
                 "(int)RC2DGI_FMT_RGBA16F, (int)RC2DGI_READ_FLIP); return 0; }\n")
    exe = str(tmp_path / "consts")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, str(c)], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [0, 1, 2, 1]
    assert (R.FMT_RGBA8, R.FMT_RGBA32F, R.FMT_RGBA16F, R.READ_FLIP) == (0, 1, 2, 1)
    src = open(CS).read()
    assert re.search(r"enum Format \{[^}]*\bRGBA16F = 2\b[^}]*\}", src)
    assert re.search(r"public const int ReadFlip = 1;", src)
    for name in CALLS:
        assert re.search(r"public static extern int %s\(IntPtr ctx, int which, TexRect\* rect, int format, int flags, "
                         r"void\* \w+, int pitchBytes\);" % name, src), f"RC2DGINative.cs does not declare {name}"


def test_null_context_is_an_argument_error(R):
    L = R.load_library()
    buf = np.zeros(64, np.uint8)
    rect = R._rect_array([[0, 0, 1, 1]])
    for name in CALLS:
        fn = getattr(L, name)
        assert fn(None, 0, None, FMT_RGBA32F, 0, buf.ctypes.data_as(ctypes.c_void_p), 0) == E_ARG
        assert fn(None, 9, rect.ctypes.data_as(ctypes.c_void_p), FMT_RGBA16F, 1, buf.ctypes.data_as(ctypes.c_void_p), 16) == E_ARG
    assert not buf.any()
    # the calls that know two formats refuse every format without a context as well (with one: tests/test_read_gpu.py)
    assert L.rc2dgi_download(None, 0, buf.ctypes.data_as(ctypes.c_void_p), 0, FMT_RGBA16F) == E_ARG
    assert L.rc2dgi_upload(None, 0, buf.ctypes.data_as(ctypes.c_void_p), 0, FMT_RGBA16F) == E_ARG


# ------------------------------------------------------------------ the reference's conversions
def test_reference_half_is_numpys_on_every_half_midpoint_and_neighbour(ref_lib):
    v = half_sweep()
    assert v.shape == (65536, 4) and v.size == 256 * 256 * 4
    finite = (np.arange(65536) & 0x7FFF) < 0x7C00
    with np.errstate(over="ignore"):
        want = v.astype(f16).view(u16)
    got = ref_half(ref_lib, v)
    assert same_halves(got, want), np.argwhere(got != want)[:8]
    # a half converts to itself; a midpoint is a tie and goes to the even neighbour, the floats beside it do not tie
    b = np.arange(65536, dtype=u32)
    assert np.array_equal(got[finite, 0], b[finite])
    up = np.where((b & 0x7FFF) == 0x7BFF, (b & 0x8000) | 0x7C00, b + 1)
    assert np.array_equal(got[finite, 1], np.where(b & 1, up, b)[finite])
    assert np.array_equal(got[finite, 2], b[finite]) and np.array_equal(got[finite, 3], up[finite])
    # every special is in the sweep, bit for bit
    bits = set(v.view(u32).reshape(-1).tolist())
    for s in SPECIALS:
        if not np.isnan(s):
            assert int(f32(s).view(u32)) in bits, s
    assert np.isnan(v).any() and ((v != 0) & (np.abs(v) < f32(1.1754944e-38))).any()


def test_reference_half_on_the_cases_worked_out_by_hand(ref_lib):
    cases = [(65519.996, 0x7BFF), (65520.0, 0x7C00), (2.0 ** -25, 0x0000), (float(np.nextafter(f32(2.0 ** -25), f32(1))), 0x0001),
             (1.0 + 2.0 ** -11, 0x3C00), (1.0 + 3 * 2.0 ** -11, 0x3C02), (-0.0, 0x8000), (0.0, 0x0000),
             (-(2.0 ** -25), 0x8000), (-65520.0, 0xFC00), (np.inf, 0x7C00), (-np.inf, 0xFC00), (1e-45, 0x0000),
             (2.0 ** -24, 0x0001), (1.5 * 2.0 ** -24, 0x0002), (2.5 * 2.0 ** -24, 0x0002), (2.0 ** -14, 0x0400),
             (2.0 ** -14 - 2.0 ** -25, 0x0400), (1.0, 0x3C00), (-2.0, 0xC000), (65504.0, 0x7BFF), (3.4028235e38, 0x7C00)]
    for x, want in cases:
        assert ref_lib.read_half(float(f32(x))) == want, (x, hex(ref_lib.read_half(float(f32(x)))), hex(want))
        with np.errstate(over="ignore"):
            assert int(f32(x).astype(f16).view(u16)) == want, x
    assert (ref_lib.read_half(float("nan")) & 0x7FFF) > 0x7C00


def test_reference_q8_is_the_q8_table(R, ref_lib):
    e = R.curve_q8()
    v = np.stack([np.nextafter(e, f32(-np.inf)), e, np.nextafter(e, f32(np.inf))], 1)
    k = np.arange(1, 256)
    assert np.array_equal(ref_q8(ref_lib, v), np.stack([k - 1, k, k], 1).astype(np.uint8))
    assert ref_q8(ref_lib, [np.nan, -np.inf, np.inf, -0.0, 2.0, -1.0, 0.5]).tolist() == [0, 0, 255, 0, 255, 0, 128]
    nans = np.array([0x7F800001, 0x7FA00000, 0xFF800001, 0x7FC00000, 0xFFFFFFFF], u32).view(f32)  # signalling ones too
    assert not ref_q8(ref_lib, nans).any()


def test_reference_image_crops_flips_and_keeps_the_padding(ref_lib):
    tw, th = 7, 5
    tex = (np.arange(th * tw * 4, dtype=f32).reshape(th, tw, 4) - 30) / 64
    tex[2, 3] = [np.nan, -0.0, 70000.0, 2.0 ** -25]
    whole = ref_image(ref_lib, tex, None, f32)
    assert np.array_equal(whole.view(u32), tex.view(u32))
    crop = ref_image(ref_lib, tex, (2, 1, 4, 3), f32)
    assert np.array_equal(crop.view(u32), tex[1:4, 2:6].view(u32))
    flipped = ref_image(ref_lib, tex, (2, 1, 4, 3), f32, flip=True)
    assert np.array_equal(flipped.view(u32), tex[1:4, 2:6][::-1].view(u32))
    with np.errstate(over="ignore", invalid="ignore"):
        assert same_halves(ref_image(ref_lib, tex, (2, 1, 4, 3), f16, flip=True).view(u16),
                           tex[1:4, 2:6][::-1].astype(f16).view(u16))
        want8 = np.rint(np.nan_to_num(np.clip(tex, 0, 1), nan=0.0) * 255).astype(np.uint8)
    assert np.array_equal(ref_image(ref_lib, tex, (0, 4, 7, 1), np.uint8), want8[4:5])
    rows = ref_image(ref_lib, tex, (2, 1, 4, 3), np.uint8, pitch=19)
    assert rows.shape == (3, 19) and (rows[:, 16:] == 0xA5).all()
    assert np.array_equal(rows[:, :16].reshape(3, 4, 4), want8[1:4, 2:6])
    # rectangles that do not lie inside the texture, a bad format, a short pitch: refused, nothing written
    out = np.full(4096, 0xA5, np.uint8)
    big = 2 ** 31 - 1
    for rect in [(0, 0, 0, 1), (0, 0, 1, 0), (-1, 0, 1, 1), (0, -1, 1, 1), (4, 0, 4, 1), (0, 3, 1, 3), (big, 0, 1, 1),
                 (0, 0, big, 1), (1, 1, big, big), (0, 0, -big - 1, 1)]:
        assert ref_lib.read_image_ref(tex.ctypes.data, tw, th, *rect, FMT_RGBA8, 0, out.ctypes.data, 1 << 20) == -1, rect
    assert ref_lib.read_image_ref(tex.ctypes.data, tw, th, 0, 0, 7, 5, 3, 0, out.ctypes.data, 1 << 20) == -1
    assert ref_lib.read_image_ref(tex.ctypes.data, tw, th, 0, 0, 7, 5, FMT_RGBA8, 0, out.ctypes.data, 27) == -1
    assert (out == 0xA5).all()
