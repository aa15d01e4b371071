"""CPU: the host-only half of rc2dgi_shapes_device (include/rc2dgi.h) -- the export in the header, the library, C# and
ctypes, the record's layout in C, C# and ctypes, the null-context refusal (the first of the argument errors; the rest
need a context and are in tests/test_gpu_shapes.py), pack_shapes and shapes_from_prims against the byte layout of
rc2dgi_shape, the unchanged working memory, and the restatement (tests/shapes_ref.py) alone: each refusal term on both
sides of its bound, the header's five "consequences", and RECT / CIRCLE lists against oracle.paint_ref.paint and the
llvmpipe images of tests/golden/paint_fixtures.npz.  The tile rejection of k_shapes_bin is checked by a stand-alone
program, tests/shapes_tile_check.cpp, built here with the host compiler and -fsanitize=address,undefined."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import shapes_ref as S
from conftest import ROOT
from oracle import paint_ref as P
from test_host_cpu import CS, c_layout
from test_paint_device_cpu import SCREENS
from test_sprites_cpu import LIMITS

HEADER = os.path.join(ROOT, "include", "rc2dgi.h")
HERE = os.path.dirname(os.path.abspath(__file__))
E_ARG = -1
f32 = np.float32
W, H = 64, 48
C = (200, 100, 50, 128)  # a translucent colour: a texel blended twice differs from one blended once


@pytest.fixture(scope="module")
def R():
    from radiancecascade2dglobalillumination_amd import _build, rc2dgi

    _build.build()
    rc2dgi.load_library()
    return rc2dgi


def img(shapes, **kw):
    return S.paint(W, H, S.words(shapes), **kw)[0]


# ------------------------------------------------------------------ the export and the record
def test_header_declares_the_call_the_struct_and_the_contract():
    src = open(HEADER).read()
    assert re.search(r"^int rc2dgi_shapes_device\(rc2dgi_ctx \*ctx, int which, const unsigned char \*clear_rgba, "
                     r"const void \*shapes_dev, int n,\s*const void \*count_dev, void \*status_dev\);", src, re.M)
    assert re.search(r"typedef struct rc2dgi_shape \{.*?\} rc2dgi_shape;", src, re.S)
    assert re.search(r"RC2DGI_SHAPE_RECT = 0, RC2DGI_SHAPE_CIRCLE = 1, RC2DGI_SHAPE_TRIANGLE = 2,\s*RC2DGI_SHAPE_LINE = 3,"
                     r"\s*RC2DGI_SHAPE_ELLIPSE = 4", src)
    assert "#define RC2DGI_ABI_VERSION 5" in src
    for phrase in ("fabsf(c) < 0x1p20f", "len = sqrtf(dx * dx + dy * dy)", "len > 0 && thick > 0",
                   "scale = thick / (2.0f * len), rx = (-scale) * dy, ry = scale * dx",
                   "s0 = (x0 - rx, y0 - ry), s1 = (x0 + rx, y0 + ry), s2 = (x1 - rx, y1 - ry), s3 = (x1 + rx, y1 + ry)",
                   "{s0, s1, s2} and {s1, s2, s3}", "T(k) = (cx + c37[k] * rh, cy + s37[k] * rv)",
                   "(c, T(k + 1), T(k)), k = 0 .. 35", "No radius substitution", "blends over that texel ONCE",
                   "Any other `kind` is refused", "have not been probed against a GL implementation"):
        assert phrase in src, phrase


def test_export_is_in_the_library_csharp_and_ctypes(R):
    L = R.load_library()
    cs = open(CS).read()
    assert hasattr(L, "rc2dgi_shapes_device"), "librc2dgi.so does not export rc2dgi_shapes_device"
    assert L.rc2dgi_shapes_device.argtypes is not None and len(L.rc2dgi_shapes_device.argtypes) == 7
    assert re.search(r"public static extern int rc2dgi_shapes_device\(", cs)
    assert re.search(r"public const int ShapeRect = 0, ShapeCircle = 1, ShapeTriangle = 2, ShapeLine = 3, "
                     r"ShapeEllipse = 4;", cs)
    assert L.rc2dgi_abi_version() == 5
    assert hasattr(R.RC2DGI, "shapes_device") and callable(R.pack_shapes) and callable(R.shapes_from_prims)
    assert (R.SHAPE_RECT, R.SHAPE_CIRCLE, R.SHAPE_TRIANGLE, R.SHAPE_LINE, R.SHAPE_ELLIPSE) == (0, 1, 2, 3, 4)
    assert (S.RECT, S.CIRCLE, S.TRIANGLE, S.LINE, S.ELLIPSE) == (0, 1, 2, 3, 4)


def test_struct_is_laid_out_alike_in_c_ctypes_and_csharp(R):
    sizes, fields = c_layout()
    assert sizes["rc2dgi_shape"] == 32 == ctypes.sizeof(R.Shape)
    for name, _ in R.Shape._fields_:
        f = getattr(R.Shape, name)
        assert fields[("rc2dgi_shape", name)] == (f.offset, f.size), name
    assert [fields[("rc2dgi_shape", n)] for n in ("kind", "v", "r", "g", "b", "a")] == \
        [(0, 4), (4, 24), (28, 1), (29, 1), (30, 1), (31, 1)]
    cs = open(CS).read()
    assert re.search(r"\[StructLayout\(LayoutKind\.Sequential, Size = 32\)\]\s*public struct Shape\b", cs)
    body = re.search(r"public struct Shape\s*\{(.*?)\}", cs, re.S).group(1)
    decl = [ln.split("//")[0].strip() for ln in body.splitlines() if ln.strip()]
    assert decl == ["public int Kind;", "public float V0, V1, V2, V3, V4, V5;", "public byte R, G, B, A;"]


def test_null_context_is_an_argument_error(R):
    L = R.load_library()
    assert L.rc2dgi_shapes_device(None, 0, None, None, 0, None, None) == E_ARG
    assert L.rc2dgi_shapes_device(None, 1, None, ctypes.c_void_p(64), 3, ctypes.c_void_p(4), ctypes.c_void_p(8)) == E_ARG


@pytest.mark.parametrize("screen,want", list(zip(SCREENS, LIMITS)), ids=lambda v: str(v))
def test_paint_device_limits_are_what_they_were(R, screen, want):
    assert R.paint_device_limits(*screen) == want


# ------------------------------------------------------------------ the two Python helpers
def test_pack_shapes_lays_out_rc2dgi_shape():
    import torch

    from radiancecascade2dglobalillumination_amd.rc2dgi import Shape, pack_shapes

    rng = np.random.default_rng(11)
    n = 29
    kind = rng.integers(-2, 7, n)
    kind[1] = -2**31
    v6 = rng.uniform(-3000, 3000, (n, 6)).astype(f32)
    v6[0] = [np.nan, np.inf, -np.inf, -0.0, 1e-42, 2.0 ** 20]  # (every bit pattern goes through as it is)
    rgba = rng.integers(0, 256, (n, 4)).astype(np.uint8)
    rgba[0] = [1, 2, 3, 255]  # (word 7 = 0xFF030201: the top bit set)
    t = torch.from_numpy
    got = pack_shapes(t(kind), t(v6), t(rgba))
    assert got.dtype == torch.int32 and tuple(got.shape) == (n, 8) and got.is_contiguous()
    arr = (Shape * n)()
    for k in range(1, n):
        arr[k] = Shape(int(kind[k]), (ctypes.c_float * 6)(*(float(v) for v in v6[k])), *(int(v) for v in rgba[k]))
    assert got.numpy()[1:].tobytes() == bytes(arr)[32:]
    assert np.array_equal(got.numpy()[0, 1:7], v6[0].view(np.int32))
    assert int(got[0, 7]) == np.int32(np.uint32(0xFF030201).view(np.int32))
    assert np.array_equal(S.words([(int(kind[k]), v6[k], tuple(rgba[k])) for k in range(n)]), got.numpy()), \
        "the restatement's packing"
    z = torch.zeros
    assert tuple(pack_shapes(z(0, dtype=torch.int64), z((0, 6)), z((0, 4), dtype=torch.uint8)).shape) == (0, 8)
    with pytest.raises(ValueError):
        pack_shapes(t(kind), t(v6.astype(np.float64)), t(rgba))
    with pytest.raises(ValueError):
        pack_shapes(t(kind), t(v6[:, :4].copy()), t(rgba))
    with pytest.raises(ValueError):
        pack_shapes(t(kind), t(v6), t(rgba[:, :3].copy()))
    with pytest.raises(ValueError):
        pack_shapes(t(kind.astype(np.float32)), t(v6), t(rgba))


def test_shapes_from_prims_moves_the_colour_to_word_7():
    import torch

    from radiancecascade2dglobalillumination_amd.rc2dgi import pack_prims, shapes_from_prims

    rng = np.random.default_rng(12)
    n = 17
    kind = rng.integers(0, 2, n)
    xywh = rng.uniform(-50, 50, (n, 4)).astype(f32)
    rgba = rng.integers(0, 256, (n, 4)).astype(np.uint8)
    prims = pack_prims(torch.from_numpy(kind), torch.from_numpy(xywh), torch.from_numpy(rgba))
    got = shapes_from_prims(prims)
    assert got.dtype == torch.int32 and tuple(got.shape) == (n, 8) and got.is_contiguous()
    g = got.numpy()
    assert np.array_equal(g[:, :5], prims.numpy()[:, :5]) and not g[:, 5:7].any()
    assert np.array_equal(g[:, 7], prims.numpy()[:, 5])
    assert np.array_equal(g, S.words([(int(kind[k]), xywh[k], tuple(rgba[k])) for k in range(n)]))
    assert tuple(shapes_from_prims(prims[:0]).shape) == (0, 8)
    with pytest.raises(ValueError):
        shapes_from_prims(got)
    with pytest.raises(ValueError):
        shapes_from_prims(prims.to(torch.int64))


# ------------------------------------------------------------------ the restatement: refusal
BELOW, AT = np.nextafter(f32(2.0 ** 20), f32(0)), f32(2.0 ** 20)
GOOD = {S.TRIANGLE: (3.0, 4.0, 30.0, 9.0, 12.0, 40.0), S.LINE: (3.0, 4.0, 30.0, 9.0, 2.0), S.ELLIPSE: (30.0, 20.0, 9.0, 5.0)}


@pytest.mark.parametrize("kind,term", [(k, i) for k in (S.TRIANGLE, S.LINE, S.ELLIPSE) for i in range(S.NV[k])])
def test_each_refusal_term_on_both_sides_of_its_bound(kind, term):
    def rec(c):
        v = list(GOOD[kind])
        v[term] = c
        return S.words([(kind, v, C)])[0]

    assert not S.refused(rec(GOOD[kind][term]))
    for sign in (1, -1):
        assert not S.refused(rec(sign * BELOW)), "just inside 2^20"
        assert S.refused(rec(sign * AT)), "2^20 itself"
        assert S.refused(rec(sign * np.inf))
    assert S.refused(rec(np.nan))
    # a refused record draws nothing, is counted, and leaves its neighbours alone
    both = np.stack([rec(np.nan), rec(GOOD[kind][term])])
    got, m, nref = S.paint(W, H, both)
    assert (m, nref) == (2, 1) and np.array_equal(got, S.paint(W, H, both[1:])[0]) and got.any()


def test_words_a_kind_does_not_name_are_not_read():
    for kind in (S.RECT, S.CIRCLE, S.TRIANGLE, S.LINE, S.ELLIPSE):
        v = list(GOOD.get(kind, (10.0, 12.0, 9.0, 7.0)))[:S.NV[kind]]
        clean = S.words([(kind, v, C)])
        dirty = clean.copy()
        dirty[0, 1 + S.NV[kind]:7] = np.array([np.nan], f32).view(np.int32)[0]
        assert not S.refused(dirty[0])
        assert np.array_equal(S.paint(W, H, dirty)[0], S.paint(W, H, clean)[0])


def test_unknown_kinds_and_the_prim_bound():
    for kind in (-1, 5, 6, 7, 2 ** 31 - 1, -2 ** 31):
        assert S.refused(S.words([(kind, (1, 2, 3, 4, 5, 6), C)])[0]), kind
    big = np.nextafter(f32(2.0 ** 22), f32(0))
    assert not S.refused(S.words([(S.RECT, (big, 0, 0, 0), C)])[0])  # RECT and CIRCLE keep rc2dgi_prim's 2^22
    assert S.refused(S.words([(S.RECT, (2.0 ** 22, 0, 0, 0), C)])[0])
    assert S.refused(S.words([(S.RECT, (2.0 ** 21, 0, 2.0 ** 21, 0), C)])[0])  # x + w
    assert not S.refused(S.words([(S.CIRCLE, (2.0 ** 21, 0, 2.0 ** 20), C)])[0])
    assert S.refused(S.words([(S.CIRCLE, (2.0 ** 21, 0, 2.0 ** 21), C)])[0])  # fabsf(x) + fabsf(w)


# ------------------------------------------------------------------ the restatement: the header's consequences
VERTS = [((3.3, 4.4), (50.2, 10.1), (20.7, 40.9)), ((10.5, 10.5), (20.5, 10.5), (10.5, 20.5)),
         ((-30.0, 5.0), (90.0, 20.0), (31.0, 22.0)), ((5.0, 5.0), (60.0, 40.0), (60.0, 40.7))]


@pytest.mark.parametrize("verts", VERTS)
def test_a_triangle_is_the_same_for_all_six_vertex_orders(verts):
    ims = [img([(S.TRIANGLE, sum(p, ()), C)]) for p in itertools.permutations(verts)]
    assert ims[0].any() and all(np.array_equal(ims[0], i) for i in ims[1:])


@pytest.mark.parametrize("x,y,w,h", [(5, 7, 20, 11), (0, 0, 64, 48), (-3, 40, 70, 20), (10, 10, 1, 1), (8, 8, 31, 31)])
def test_two_triangles_are_the_rectangle_once(x, y, w, h):
    r = img([(S.RECT, (x, y, w, h), C)])
    t = img([(S.TRIANGLE, (x, y, x, y + h, x + w, y + h), C), (S.TRIANGLE, (x, y, x + w, y + h, x + w, y), C)])
    assert r.any() and np.array_equal(r, t)  # (a diagonal centre blended twice would differ: C is translucent)


@pytest.mark.parametrize("x0,y,length,thick", [(4, 20, 32, 6), (4, 7, 32, 6), (1, 30, 64, 2), (10, 11, 16, 1), (3, 5, 8, 4)])
def test_a_horizontal_line_of_power_of_two_length_is_a_rectangle(x0, y, length, thick):
    ln = img([(S.LINE, (x0, y, x0 + length, y, thick), C)])
    r = img([(S.RECT, (x0, y - thick / 2, length, thick), C)])
    assert r.any() and np.array_equal(ln, r)
    down = img([(S.LINE, (y, x0, y, x0 + length, thick), C)])  # and a vertical one
    assert np.array_equal(down, img([(S.RECT, (y - thick / 2, x0, thick, length), C)]))


@pytest.mark.parametrize("cx,cy,r", [(30.3, 20.7, 9.5), (32, 24, 20), (0.5, 0.5, 3.25), (70, 50, 12), (20, 20, 0.4)])
def test_an_ellipse_of_equal_radii_is_the_circle(cx, cy, r):
    e, c = img([(S.ELLIPSE, (cx, cy, r, r), C)]), img([(S.CIRCLE, (cx, cy, r), C)])
    assert np.array_equal(e, c) and (c.any() or r < 0.5)


def test_an_ellipse_with_a_zero_radius_draws_nothing_and_a_circle_does():
    for v in ((30, 20, 0, 5), (30, 20, 5, 0), (30, 20, 0, 0), (30.5, 20.5, -0.0, 3)):
        got, m, nref = S.paint(W, H, S.words([(S.ELLIPSE, v, C)]))
        assert not got.any() and (m, nref) == (1, 0)  # nothing drawn, not refused
    assert img([(S.CIRCLE, (30.5, 20.5, 0), (255, 255, 255, 255))]).any()  # the circle's radius substitution, 0.1
    assert img([(S.ELLIPSE, (30, 20, -9, 5), C)]).any()  # a negative radius mirrors the fan: drawn whatever the winding


def test_a_line_without_length_or_thickness_draws_nothing():
    for v in ((5, 5, 5, 5, 3), (5, 5, 40, 30, 0), (5, 5, 40, 30, -2), (5, 5, 5 + 1e-30, 5, 3)):
        got, m, nref = S.paint(W, H, S.words([(S.LINE, v, C)]))
        assert not got.any() and (m, nref) == (1, 0), v
    # dx * dx a denormal: len is sqrtf of it, positive, and the quad is the header's
    rec = S.words([(S.LINE, (0.0, 20.0, 1e-20, 20.0, 8.0), C)])[0]
    tris = S.vertices(rec)
    assert len(tris) == 2 and all(np.isfinite(c) for t in tris for p in t for c in p)


# ------------------------------------------------------------------ the restatement against the llvmpipe images
def fixture(name):
    d = np.load(os.path.join(HERE, "golden", "paint_fixtures.npz"), allow_pickle=False)
    w, h = (int(v) for v in d[name + "__size"])
    clear = d[name + "__clear"]
    prims = [(int(p[0]), float(p[1]), float(p[2]), float(p[3]), float(p[4])) + tuple(int(v) for v in p[5:9])
             for p in d[name + "__prims"]]
    return w, h, (None if clear[0] < 0 else tuple(int(v) for v in clear)), prims, d[name + "__image"], d[name + "__image_u8"]


@pytest.mark.parametrize("name", ["edges64x48", "redraw200_walls"])
def test_rect_and_circle_lists_equal_paint_ref_and_the_gl_images(name):
    w, h, clear, prims, image, image_u8 = fixture(name)
    recs = S.words([(p[0], p[1:5] if p[0] == P.RECT else p[1:4], p[5:9]) for p in prims])
    for rgba8, gl in ((False, image), (True, image_u8)):
        got, m, nref = S.paint(w, h, recs, clear=clear, rgba8=rgba8)
        assert (m, nref) == (len(prims), 0)
        assert np.array_equal(got, P.paint(w, h, prims, clear=clear, rgba8=rgba8))
        assert np.array_equal(got, gl), "the llvmpipe image"  # (a fresh render texture: zeros, as the restatement's)


# ------------------------------------------------------------------ the tile rejection, on the host
@pytest.fixture(scope="module")
def tile_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("shapes_tile") / "shapes_tile_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "radiancecascade2dglobalillumination_amd", "csrc"),
                    "-o", exe, os.path.join(HERE, "shapes_tile_check.cpp")], check=True)
    return exe


def test_tile_rejection_never_drops_a_covered_centre(tile_check):
    r = subprocess.run([tile_check], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"triangles drawn (\d+), tiles in their boxes (\d+), kept (\d+) \(of them empty (\d+)\), wrongly "
                  r"rejected 0", r.stdout)
    assert m, r.stdout
    drawn, tiles, kept, empty = (int(v) for v in m.groups())
    assert drawn > 15000 and kept < tiles  # the test rejects something: it is not vacuous


def test_the_check_sees_the_opposite_corner(tile_check):
    r = subprocess.run([tile_check, "--flip"], capture_output=True, text=True)
    assert r.returncode == 1 and "WRONG" in r.stdout and "runtime error" not in r.stderr
