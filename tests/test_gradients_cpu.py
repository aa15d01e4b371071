"""CPU: the host-only half of rc2dgi_gradients_device (include/rc2dgi.h) -- the export in the header, the library, C#
and ctypes, the record's layout in C, C# and ctypes, the null-context refusal (the rest of the argument errors need a
context and are in tests/test_gpu_gradients.py), pack_gradients, gradients_from_shapes and soft_lights against the byte
layout of rc2dgi_gradient, the unchanged working memory, and the restatement (tests/gradients_ref.py) alone: each
refusal term on both sides of its bound, the gain included; the header's consequences; and the restatement against a
float64 barycentric interpolation of the snapped triangles.  The kernel's own interpolation text
(csrc/rc2dgi_gradient_interp.h) is checked by a stand-alone program, tests/gradients_interp_check.cpp, built here with
the host compiler and -fsanitize=address,undefined."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import gradients_ref as G
import shapes_ref as S
from conftest import ROOT
from test_host_cpu import CS, c_layout
from test_paint_device_cpu import SCREENS
from test_sprites_cpu import LIMITS

HEADER = os.path.join(ROOT, "include", "rc2dgi.h")
HERE = os.path.dirname(os.path.abspath(__file__))
E_ARG = -1
f32 = np.float32
W, H = 64, 48
C4 = [(200, 100, 50, 128), (10, 250, 90, 255), (255, 0, 160, 40), (0, 30, 255, 200)]


@pytest.fixture(scope="module")
def R():
    from radiancecascade2dglobalillumination_amd import _build, rc2dgi

    _build.build()
    rc2dgi.load_library()
    return rc2dgi


# ------------------------------------------------------------------ the export and the record
def test_header_declares_the_call_the_struct_and_the_contract():
    src = open(HEADER).read()
    assert re.search(r"^int rc2dgi_gradients_device\(rc2dgi_ctx \*ctx, int which, const unsigned char \*clear_rgba, "
                     r"const void \*grads_dev, int n,\s*const void \*count_dev, void \*status_dev\);", src, re.M)
    assert re.search(r"typedef struct rc2dgi_gradient \{.*?\} rc2dgi_gradient;", src, re.S)
    assert re.search(r"RC2DGI_GRAD_RECT = 0, RC2DGI_GRAD_CIRCLE = 1, RC2DGI_GRAD_TRIANGLE = 2, RC2DGI_GRAD_LINE = 3,"
                     r"\s*RC2DGI_GRAD_ELLIPSE = 4", src)
    assert "#define RC2DGI_ABI_VERSION 5" in src
    for phrase in ("w1 = (float)E_1 / (float)A,  w2 = (float)E_2 / (float)A", "col = (q0 + w1 * (q1 - q0)) + w2 * (q2 - q0)",
                   "fabsf(gain) <= 0x1p20f", "(TL, BL, BR), then (TL, BR, TR)", "{s0, s1, s2}, then {s1, s2, s3}",
                   "FIRST covering triangle in the listed order", "smaller than 2^61 + 2^55", "c[0..3] = TL, BL, BR, TR",
                   "(float)k * (1.0f / 255.0f)", "has not been probed against a GL implementation",
                   "Any other `kind` is refused", "weight exactly 0 for the opposite vertex"):
        assert phrase in src, phrase


def test_export_is_in_the_library_csharp_ctypes_and_the_documents(R):
    L = R.load_library()
    cs = open(CS).read()
    assert hasattr(L, "rc2dgi_gradients_device"), "librc2dgi.so does not export rc2dgi_gradients_device"
    assert L.rc2dgi_gradients_device.argtypes is not None and len(L.rc2dgi_gradients_device.argtypes) == 7
    assert re.search(r"public static extern int rc2dgi_gradients_device\(", cs)
    assert re.search(r"public const int GradRect = 0, GradCircle = 1, GradTriangle = 2, GradLine = 3, GradEllipse = 4;", cs)
    assert L.rc2dgi_abi_version() == 5
    assert hasattr(R.RC2DGI, "gradients_device")
    assert callable(R.pack_gradients) and callable(R.gradients_from_shapes) and callable(R.soft_lights)
    assert (R.GRAD_RECT, R.GRAD_CIRCLE, R.GRAD_TRIANGLE, R.GRAD_LINE, R.GRAD_ELLIPSE) == (0, 1, 2, 3, 4)
    assert (G.RECT, G.CIRCLE, G.TRIANGLE, G.LINE, G.ELLIPSE) == (0, 1, 2, 3, 4)
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "rc2dgi_gradients_device" in open(os.path.join(ROOT, doc)).read(), doc


def test_struct_is_laid_out_alike_in_c_ctypes_and_csharp(R):
    sizes, fields = c_layout()
    assert sizes["rc2dgi_gradient"] == 48 == ctypes.sizeof(R.Gradient)
    for name, _ in R.Gradient._fields_:
        f = getattr(R.Gradient, name)
        assert fields[("rc2dgi_gradient", name)] == (f.offset, f.size), name
    assert [fields[("rc2dgi_gradient", n)] for n in ("kind", "v", "c", "gain")] == [(0, 4), (4, 24), (28, 16), (44, 4)]
    cs = open(CS).read()
    assert re.search(r"\[StructLayout\(LayoutKind\.Sequential, Size = 48\)\]\s*public struct Gradient\b", cs)
    body = re.search(r"public struct Gradient\s*\{(.*?)\}", cs, re.S).group(1)
    decl = [ln.split("//")[0].strip() for ln in body.splitlines() if ln.strip()]
    assert decl == ["public int Kind;", "public float V0, V1, V2, V3, V4, V5;", "public uint C0, C1, C2, C3;",
                    "public float Gain;"]  # 4 + 24 + 16 + 4 bytes, every field 4-aligned: no padding


def test_null_context_is_an_argument_error(R):
    L = R.load_library()
    assert L.rc2dgi_gradients_device(None, 0, None, None, 0, None, None) == E_ARG
    assert L.rc2dgi_gradients_device(None, 1, None, ctypes.c_void_p(64), 3, ctypes.c_void_p(4), ctypes.c_void_p(8)) == E_ARG


@pytest.mark.parametrize("screen,want", list(zip(SCREENS, LIMITS)), ids=lambda v: str(v))
def test_paint_device_limits_are_what_they_were(R, screen, want):
    assert R.paint_device_limits(*screen) == want


# ------------------------------------------------------------------ the three Python helpers
def test_pack_gradients_lays_out_rc2dgi_gradient(R):
    import torch

    rng = np.random.default_rng(21)
    n = 23
    kind = rng.integers(-2, 7, n)
    v6 = rng.uniform(-3000, 3000, (n, 6)).astype(f32)
    v6[0] = [np.nan, np.inf, -np.inf, -0.0, 1e-42, 2.0 ** 20]  # (every bit pattern goes through as it is)
    cols = rng.integers(0, 256, (n, 4, 4)).astype(np.uint8)
    cols[0, 3] = [1, 2, 3, 255]  # (word 10 = 0xFF030201: the top bit set)
    gain = rng.uniform(-4, 9, n).astype(f32)
    gain[0] = np.nan
    t = torch.from_numpy
    got = R.pack_gradients(t(kind), t(v6), t(cols), t(gain))
    assert got.dtype == torch.int32 and tuple(got.shape) == (n, 12) and got.is_contiguous()
    arr = (R.Gradient * n)()
    for k in range(1, n):
        c = ((ctypes.c_ubyte * 4) * 4)(*[(ctypes.c_ubyte * 4)(*(int(b) for b in cols[k, j])) for j in range(4)])
        arr[k] = R.Gradient(int(kind[k]), (ctypes.c_float * 6)(*(float(v) for v in v6[k])), c, float(gain[k]))
    assert got.numpy()[1:].tobytes() == bytes(arr)[48:]
    assert np.array_equal(got.numpy()[0, 1:7], v6[0].view(np.int32))
    assert int(got[0, 10]) == np.int32(np.uint32(0xFF030201).view(np.int32))
    assert np.array_equal(got.numpy()[:, 11], gain.view(np.int32))
    assert np.array_equal(G.words([(int(kind[k]), v6[k], cols[k], gain[k]) for k in range(n)]), got.numpy()), \
        "the restatement's packing"
    ones = R.pack_gradients(t(kind), t(v6), t(cols))
    assert np.array_equal(ones.numpy()[:, :11], got.numpy()[:, :11])
    assert np.array_equal(ones.numpy()[:, 11].view(f32), np.ones(n, f32))
    z = torch.zeros
    assert tuple(R.pack_gradients(z(0, dtype=torch.int64), z((0, 6)), z((0, 4, 4), dtype=torch.uint8)).shape) == (0, 12)
    for bad in ((t(kind), t(v6.astype(np.float64)), t(cols), None), (t(kind), t(v6[:, :4].copy()), t(cols), None),
                (t(kind), t(v6), t(cols[:, :3].copy()), None), (t(kind.astype(f32)), t(v6), t(cols), None),
                (t(kind), t(v6), t(cols), t(gain.astype(np.float64))), (t(kind), t(v6), t(cols), t(gain[:5].copy()))):
        with pytest.raises(ValueError):
            R.pack_gradients(*bad)


def test_gradients_from_shapes_repeats_the_colour_with_gain_one(R):
    import torch

    rng = np.random.default_rng(22)
    n = 19
    shapes = S.words([(int(rng.integers(0, 5)), rng.uniform(-50, 50, 6), tuple(rng.integers(0, 256, 4))) for _ in range(n)])
    got = R.gradients_from_shapes(torch.from_numpy(shapes))
    assert got.dtype == torch.int32 and tuple(got.shape) == (n, 12) and got.is_contiguous()
    g = got.numpy()
    assert np.array_equal(g[:, :7], shapes[:, :7])
    assert all(np.array_equal(g[:, 7 + k], shapes[:, 7]) for k in range(4))
    assert np.array_equal(g[:, 11].view(f32), np.ones(n, f32))
    assert np.array_equal(g, G.from_shapes(shapes)), "the restatement's helper"
    assert tuple(R.gradients_from_shapes(torch.from_numpy(shapes[:0])).shape) == (0, 12)
    with pytest.raises(ValueError):
        R.gradients_from_shapes(got)
    with pytest.raises(ValueError):
        R.gradients_from_shapes(torch.from_numpy(shapes).to(torch.int64))


def test_soft_lights_are_circles_that_fade_to_nothing(R):
    import torch

    rng = np.random.default_rng(23)
    n = 11
    xy = rng.uniform(0, 64, (n, 2)).astype(f32)
    rad = rng.uniform(1, 20, n).astype(f32)
    rgb = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    gain = rng.uniform(0.5, 16, n).astype(f32)
    t = torch.from_numpy
    got = R.soft_lights(t(xy), t(rad), t(rgb), t(gain))
    assert got.dtype == torch.int32 and tuple(got.shape) == (n, 12) and got.is_contiguous()
    want = G.words([(G.CIRCLE, (xy[k, 0], xy[k, 1], rad[k]), [tuple(rgb[k]) + (255,), tuple(rgb[k]) + (0,)] +
                     [tuple(rgb[k]) + (0,)] * 2, gain[k]) for k in range(n)])
    assert np.array_equal(got.numpy(), want)
    assert np.array_equal(R.soft_lights(t(xy), t(rad), t(rgb)).numpy()[:, 11].view(f32), np.ones(n, f32))
    assert tuple(R.soft_lights(t(xy[:0]), t(rad[:0]), t(rgb[:0])).shape) == (0, 12)
    for bad in ((t(xy.astype(np.float64)), t(rad), t(rgb)), (t(xy), t(rad[:3].copy()), t(rgb)),
                (t(xy), t(rad), t(rgb.astype(np.int32)))):
        with pytest.raises(ValueError):
            R.soft_lights(*bad)
    # the light itself, in the restatement: full alpha at the centre texel's triangle apex, nothing past the rim
    img = G.paint(W, H, G.words([(G.CIRCLE, (32.5, 24.5, 10), [(255, 128, 0, 255), (255, 128, 0, 0)], 4.0)]))[0]
    assert img[23, 32, 0] > 3.5 and img[23, 32, 3] > 0.9 and not img[:, :20].any() and not img[:, 45:].any()
    assert img[23, 38, 0] < img[23, 35, 0] < img[23, 32, 0]


# ------------------------------------------------------------------ the restatement: refusal
BELOW, AT, ABOVE = np.nextafter(f32(2.0 ** 20), f32(0)), f32(2.0 ** 20), np.nextafter(f32(2.0 ** 20), f32(np.inf))
GOOD = {G.RECT: (5.0, 6.0, 20.0, 11.0), G.CIRCLE: (30.0, 20.0, 9.0), G.TRIANGLE: (3.0, 4.0, 30.0, 9.0, 12.0, 40.0),
        G.LINE: (3.0, 4.0, 30.0, 9.0, 2.0), G.ELLIPSE: (30.0, 20.0, 9.0, 5.0)}
KINDS = (G.RECT, G.CIRCLE, G.TRIANGLE, G.LINE, G.ELLIPSE)


@pytest.mark.parametrize("kind,term", [(k, i) for k in (G.TRIANGLE, G.LINE, G.ELLIPSE) for i in range(S.NV[k])])
def test_each_geometry_term_on_both_sides_of_its_bound(kind, term):
    def rec(c):
        v = list(GOOD[kind])
        v[term] = c
        return G.words([(kind, v, C4, 1.0)])[0]

    assert not G.refused(rec(GOOD[kind][term]))
    for sign in (1, -1):
        assert not G.refused(rec(sign * BELOW)), "just inside 2^20"
        assert G.refused(rec(sign * AT)), "2^20 itself"
        assert G.refused(rec(sign * np.inf))
    assert G.refused(rec(np.nan))


def test_rect_and_circle_keep_the_prim_bound_and_other_kinds_are_refused():
    big = np.nextafter(f32(2.0 ** 22), f32(0))
    assert not G.refused(G.words([(G.RECT, (big, 0, 0, 0), C4, 1.0)])[0])
    assert G.refused(G.words([(G.RECT, (2.0 ** 22, 0, 0, 0), C4, 1.0)])[0])
    assert G.refused(G.words([(G.RECT, (2.0 ** 21, 0, 2.0 ** 21, 0), C4, 1.0)])[0])  # x + w
    assert not G.refused(G.words([(G.CIRCLE, (2.0 ** 21, 0, 2.0 ** 20), C4, 1.0)])[0])
    assert G.refused(G.words([(G.CIRCLE, (2.0 ** 21, 0, 2.0 ** 21), C4, 1.0)])[0])  # fabsf(x) + fabsf(w)
    for kind in (-1, 5, 6, 7, 2 ** 31 - 1, -2 ** 31):
        assert G.refused(G.words([(kind, (1, 2, 3, 4, 5, 6), C4, 1.0)])[0]), kind


@pytest.mark.parametrize("kind", KINDS)
def test_the_gain_on_both_sides_of_its_bound(kind):
    rec = lambda g: G.words([(kind, GOOD[kind], C4, g)])[0]  # noqa: E731
    for g in (1.0, 0.0, -0.0, -3.5, 1e-42, BELOW, -BELOW, AT, -AT):  # 2^20 itself is accepted: <=
        assert not G.refused(rec(g)), g
    for g in (ABOVE, -ABOVE, np.inf, -np.inf, np.nan, 3e38):
        assert G.refused(rec(g)), g
    # a refused record draws nothing, is counted, and leaves its neighbours alone
    both = np.stack([rec(np.nan), rec(2.0)])
    got, m, nref = G.paint(W, H, both)
    assert (m, nref) == (2, 1) and np.array_equal(got, G.paint(W, H, both[1:])[0]) and got.any()


def test_colour_bytes_a_kind_does_not_name_are_not_read():
    named = {G.RECT: 4, G.TRIANGLE: 3, G.CIRCLE: 2, G.ELLIPSE: 2, G.LINE: 2}
    for kind in KINDS:
        clean = G.words([(kind, GOOD[kind], C4[:named[kind]], 1.5)])
        dirty = G.words([(kind, GOOD[kind], C4[:named[kind]] + [(9, 8, 7, 6)] * (4 - named[kind]), 1.5)])
        a, b = G.paint(W, H, clean), G.paint(W, H, dirty)
        assert a[0].any() and np.array_equal(a[0], b[0]) and a[1:] == b[1:], kind


# ------------------------------------------------------------------ the restatement: the header's consequences
def mixed_shapes(seed, n=40):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        kind = k % 5
        cx, cy = rng.uniform(0, W), rng.uniform(0, H)
        v = {G.RECT: (cx - 8, cy - 5, rng.uniform(1, 30), rng.uniform(1, 20)), G.CIRCLE: (cx, cy, rng.uniform(0.3, 14)),
             G.TRIANGLE: tuple(rng.uniform(-10, 70, 6)), G.LINE: (cx, cy, rng.uniform(0, W), rng.uniform(0, H), rng.uniform(0.5, 6)),
             G.ELLIPSE: (cx, cy, rng.uniform(1, 20), rng.uniform(1, 9))}[kind]
        out.append((kind, v, tuple(int(c) for c in rng.integers(0, 256, 4))))
    out[7] = (G.TRIANGLE, (np.nan, 0, 1, 1, 2, 2), (1, 2, 3, 4))  # a refused one: the counts agree too
    out[11] = (9, (0, 0, 1, 1), (1, 2, 3, 4))
    return out


@pytest.mark.parametrize("rgba8", [False, True], ids=["float", "rgba8"])
def test_equal_colours_and_gain_one_leave_the_flat_shapes_bits(rgba8):
    shapes = S.words(mixed_shapes(31))
    rng = np.random.default_rng(32)
    base = rng.integers(0, 256, (H, W, 4)).astype(np.uint8) if rgba8 else rng.uniform(-1, 2, (H, W, 4)).astype(f32)
    want = S.paint(W, H, shapes, base=base, rgba8=rgba8)
    got = G.paint(W, H, G.from_shapes(shapes), base=base, rgba8=rgba8)
    assert want[2] == 2 and got[1:] == want[1:] and np.array_equal(got[0], want[0])
    assert not np.array_equal(got[0], base)


def test_q8_of_a_colour_byte_is_the_byte():
    k = np.arange(256, dtype=np.uint8)
    assert np.array_equal(G.q8(G.unorm(k)), k)  # q8(k * (1/255)) == k for all 256 values


def test_a_centre_on_an_included_edge_weighs_the_opposite_vertex_zero():
    # screen (10.5, 30.5), (30.5, 30.5), (10.5, 10.5) is window (10.5, 17.5), (30.5, 17.5), (10.5, 37.5), counter-clockwise:
    # R0 R1 runs along +x with dy == 0 (included) through the centres of GL row 17, R2 R0 runs down (dy < 0, included)
    # through the centres of column 10
    rec = G.words([(G.TRIANGLE, (10.5, 30.5, 30.5, 30.5, 10.5, 10.5), [(255, 0, 0, 255), (0, 255, 0, 255), (0, 0, 255, 255)], 1.0)])[0]
    cov, src, _ = G.shade(rec, W, H)
    assert cov[17, 10:30].all() and cov[17:37, 10].all() and not cov[16].any() and not cov[:, 9].any()
    assert not src[17, 10:30, 2].any(), "on R0 R1: none of R2's blue, exactly"
    assert not src[17:37, 10, 1].any(), "on R2 R0: none of R1's green, exactly"
    assert src[18, 11, 1] > 0 and src[18, 11, 2] > 0  # (one texel inside, both are there)
    assert src[17, 10].tolist() == [1.0, 0.0, 0.0, 1.0]  # the vertex itself


def test_a_rim_of_zero_alpha_contributes_nothing_on_the_rim_edge():
    rng = np.random.default_rng(33)
    E1 = rng.integers(1, 2 ** 60, 4000)
    E2 = rng.integers(1, 2 ** 60, 4000)
    E0 = np.zeros_like(E1)  # a centre on the edge opposite the fan's centre vertex: the rim edge
    q_rim = G.unorm((90, 200, 30, 0))
    src = G.interpolate(E0, E1, E2, G.unorm((90, 200, 30, 255)), q_rim, q_rim, 8.0)
    assert np.abs(src[:, 3]).max() < 2.0 ** -21
    assert not G.q8(src[:, 3]).any()  # RGBA8 storage: alpha 0, and the 8-bit blend with alpha 0 keeps the texel
    d = rng.integers(0, 256, (4000, 4)).astype(np.uint8)
    from oracle.paint_ref import _blend8
    assert np.array_equal(_blend8(G.q8(src), d), d)
    clear = G.interpolate(E0, E1, E2, G.unorm((90, 200, 30, 0)), q_rim, q_rim, 8.0)
    assert not clear[:, 3].any()


# ------------------------------------------------------------------ the restatement against float64 barycentrics
ANALYTIC = [
    (G.TRIANGLE, (3.3, 4.4, 50.2, 10.1, 20.7, 40.9)), (G.TRIANGLE, (3.3, 4.4, 20.7, 40.9, 50.2, 10.1)),  # both windings
    (G.TRIANGLE, (-30.0, 5.0, 90.0, 20.0, 31.0, 60.0)),
    (G.RECT, (5.25, 7.5, 40.0, 21.0)), (G.RECT, (-3.0, 30.0, 70.0, 30.0)),
    (G.CIRCLE, (30.3, 20.7, 15.5)), (G.CIRCLE, (60.0, 44.0, 12.0)), (G.ELLIPSE, (32.0, 24.0, 25.0, 9.0)),
    (G.ELLIPSE, (20.0, 20.0, -9.0, 12.0)),  # a negative radius mirrors the fan: every triangle is swapped the other way
    (G.LINE, (10.0, 10.0, 50.0, 30.0, 6.0)), (G.LINE, (50.0, 10.0, 10.0, 30.0, 6.0)),  # a LINE a quadrant of direction
    (G.LINE, (50.0, 30.0, 10.0, 10.0, 6.0)), (G.LINE, (10.0, 30.0, 50.0, 10.0, 6.0)),
    (G.LINE, (5.0, 24.0, 60.0, 24.0, 9.0)), (G.LINE, (32.0, 45.0, 32.0, 3.0, 9.0)),
]


@pytest.mark.parametrize("kind,v", ANALYTIC, ids=lambda p: str(p))
def test_restatement_against_float64_barycentrics(kind, v):
    """|restatement - float64| < 2^-20 for colours in [0, 1] and gain 1: a weight carries two conversions and one
    division, a channel two differences, two products and two sums, all of magnitude at most about 1 -- under sixteen
    half-ulps of 1.0 = 16 * 2^-24.  A wrong association of vertex and colour misses by orders of magnitude."""
    rec = G.words([(kind, v, C4, 1.0)])[0]
    assert not G.refused(rec)
    cov, src, tri = G.shade(rec, W, H)
    assert cov.sum() > 40
    cols = np.array(C4, np.float64) / 255.0
    want = np.zeros((H, W, 4))
    seen = np.zeros((H, W), bool)
    X = (np.arange(W) * 256 + 128).astype(np.float64)[None, :]
    Y = (np.arange(H) * 256 + 128).astype(np.float64)[:, None]
    swapped = 0
    for idx, t in enumerate(S.snapped(rec[:8], W, H)):
        P = np.array(t, np.float64)
        cross = lambda a, b, px, py: (b[0] - a[0]) * (py - a[1]) - (b[1] - a[1]) * (px - a[0])  # noqa: E731
        area = cross(P[0], P[1], P[2][0], P[2][1])
        if area == 0:
            continue
        swapped += area < 0
        b = [cross(P[1], P[2], X, Y) / area, cross(P[2], P[0], X, Y) / area, cross(P[0], P[1], X, Y) / area]
        m = (tri == idx)
        c = sum(b[k][..., None] * cols[G.COLOURS[kind][idx][k]] for k in range(3))
        want[m] = c[m]
        seen |= m
    assert np.array_equal(seen, cov)
    err = np.abs(src.astype(np.float64) - want)[cov].max()
    print(f"kind {kind}: covered {cov.sum()}, swapped triangles {swapped}, max error {err:.3g} (bound {2.0 ** -20:.3g})")
    assert err < 2.0 ** -20
    # the two ends differ, so a swapped association would be seen: the colours span most of [0, 1]
    assert np.ptp(src[cov][:, :3], axis=0).max() > 0.2


def test_the_analytic_cases_exercise_the_swap():
    swaps = set()
    for kind, v in ANALYTIC:
        for t in S.snapped(G.words([(kind, v, C4, 1.0)])[0][:8], W, H):
            (x0, y0), (x1, y1), (x2, y2) = t
            area = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
            if area:
                swaps.add((kind, area < 0))
    for kind in (G.TRIANGLE, G.LINE, G.ELLIPSE):
        assert (kind, True) in swaps and (kind, False) in swaps, kind


# ------------------------------------------------------------------ the kernel's interpolation text, on the host
@pytest.fixture(scope="module")
def interp_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gradients_interp") / "gradients_interp_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "radiancecascade2dglobalillumination_amd", "csrc"), "-o", exe,
                    os.path.join(HERE, "gradients_interp_check.cpp")], check=True)
    return exe


def test_interpolation_text_on_the_host_is_clean_and_exact(interp_check):
    r = subprocess.run([interp_check], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"centres walked (\d+), covered (\d+) \(in a swapped triangle (\d+), by the second triangle (\d+)\), "
                  r"worst error (\S+), wrong 0", r.stdout)
    assert m, r.stdout
    assert int(m.group(2)) > 100000 and int(m.group(3)) > 10000 and int(m.group(4)) > 0
    assert float(m.group(5)) < 2.0 ** -20 and "runtime error" not in r.stderr


def test_the_check_sees_colours_tagged_after_the_swap(interp_check):
    r = subprocess.run([interp_check, "--wrong"], capture_output=True, text=True)
    assert r.returncode == 1 and "WRONG" in r.stdout and "runtime error" not in r.stderr
