"""CPU: the host-only half of the edge tables (include/rc2dgi.h: rc2dgi_check_edges / rc2dgi_curve_q8, rc2dgi_set_curve /
rc2dgi_compose_tone, rc2dgi_histogram) -- the seven exports, the checks made before any device work, the byte layout of
rc2dgi_tone in C, C# and Python, the q8 table against q8 itself, and tests/tone_ref.c, the C restatement the GPU tests
compare against, on cases worked out by hand."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_host_cpu import CS, c_layout
from test_reduce_cpu import INT_MAX, cs_layout_d

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(ROOT, "include", "rc2dgi.h")
HOST_CALLS = ["rc2dgi_check_edges", "rc2dgi_curve_q8"]
CTX_CALLS = ["rc2dgi_set_curve", "rc2dgi_compose_tone", "rc2dgi_compose_tone_device", "rc2dgi_histogram",
             "rc2dgi_histogram_device"]
E_ARG = -1
f32, u32 = np.float32, np.uint32
INVALID = 0xFFFFFFFF  # RC2DGI_STATS_INVALID as a 32-bit word


@pytest.fixture(scope="module")
def R():
    from radiancecascade2dglobalillumination_amd import _build, rc2dgi

    _build.build()
    rc2dgi.load_library()
    return rc2dgi


# ------------------------------------------------------------------ tests/tone_ref.c (shared with test_tone_gpu.py)
class RefTex(ctypes.Structure):
    _fields_ = [("f", ctypes.c_void_p), ("b", ctypes.c_void_p), ("w", ctypes.c_int), ("h", ctypes.c_int)]


class RefView(ctypes.Structure):
    _fields_ = [("tex", ctypes.c_int), ("x", ctypes.c_int), ("y", ctypes.c_int), ("w", ctypes.c_int),
                ("h", ctypes.c_int), ("filter", ctypes.c_int), ("r", ctypes.c_ubyte), ("g", ctypes.c_ubyte),
                ("b", ctypes.c_ubyte), ("a", ctypes.c_ubyte), ("exposure", ctypes.c_float), ("curve", ctypes.c_int)]


def build_tone_ref(tmp_path_factory):
    """tests/tone_ref.c as a ctypes library, compiled as tests/present_ref.c is"""
    so = str(tmp_path_factory.mktemp("tone_ref") / "libtone_ref.so")
    subprocess.run(["gcc", "-O1", "-ffp-contract=off", "-std=c11", "-Wall", "-shared", "-fPIC", "-o", so,
                    os.path.join(HERE, "tone_ref.c"), "-lm"], check=True)
    L = ctypes.CDLL(so)
    vp, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    L.tone_bin.argtypes, L.tone_bin.restype = [vp, i, ctypes.c_float], i
    L.tone_q8.argtypes, L.tone_q8.restype = [ctypes.c_float], ctypes.c_uint
    L.tone_luma.argtypes, L.tone_luma.restype = [ctypes.c_float] * 3, ctypes.c_float
    L.tone_sweep.argtypes, L.tone_sweep.restype = [vp, ctypes.c_uint32, ctypes.c_uint32, ll], ll
    L.tone_sweep_list.argtypes, L.tone_sweep_list.restype = [vp, vp, ll], ll
    L.tone_compose_ref.argtypes = [ctypes.POINTER(RefTex), ctypes.POINTER(RefView), i, vp, i, i,
                                   ctypes.POINTER(ctypes.c_ubyte), vp]
    L.tone_compose_ref.restype = i
    L.tone_hist_ref.argtypes, L.tone_hist_ref.restype = [vp, i, i, i, vp, i, vp, i, vp], i
    return L


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return build_tone_ref(tmp_path_factory)


def ref_bin(ref_lib, edges, v):
    e = np.ascontiguousarray(edges, f32)
    return ref_lib.tone_bin(e.ctypes.data, len(e), float(f32(v)))


def ref_hist(ref_lib, tex, channel, rects, edges):
    """tone_ref.c's histogram over tex, float32 (th, tw, 4) as rc2dgi_download returns it: (n, m + 4) uint32"""
    tex = np.ascontiguousarray(tex, f32)
    assert tex.ndim == 3 and tex.shape[2] == 4
    rects = np.ascontiguousarray(rects, np.int32).reshape(-1, 4)
    e = np.ascontiguousarray(edges, f32).reshape(-1)
    out = np.full((len(rects), len(e) + 4), 0x5A5A5A5A, u32)
    assert ref_lib.tone_hist_ref(tex.ctypes.data, tex.shape[1], tex.shape[0], int(channel), rects.ctypes.data, len(rects),
                                 e.ctypes.data, len(e), out.ctypes.data) == 0
    return out


def ref_compose(ref_lib, textures, views, curves, size, clear=(0, 0, 0, 255)):
    """tone_ref.c's compositor.  textures: [(float array (h, w, 4), uint8 array or None)]; views: (tex index, x, y, w,
    h, filter 0 POINT / 1 LINEAR on floats / 2 LINEAR on bytes, border, exposure, curve); curves: {slot: 255 edges}."""
    tex = (RefTex * max(len(textures), 1))()
    keep = []
    for k, (f, b) in enumerate(textures):
        f = np.ascontiguousarray(f, f32)
        b = None if b is None else np.ascontiguousarray(b, np.uint8)
        keep += [f, b]
        tex[k] = RefTex(f.ctypes.data, None if b is None else b.ctypes.data, f.shape[1], f.shape[0])
    rv = (RefView * len(views))()
    for k, (t, x, y, w, h, filt, border, exposure, curve) in enumerate(views):
        rv[k] = RefView(t, x, y, w, h, filt, *border, exposure, curve)
    table = np.full((8, 255), np.nan, f32)  # (a slot no view names is never read)
    for slot, e in curves.items():
        table[slot - 1] = e
    out = np.empty((size[1], size[0], 4), np.uint8)
    cl = (ctypes.c_ubyte * 4)(*clear)
    assert ref_lib.tone_compose_ref(tex, rv, len(views), table.ctypes.data, size[0], size[1], cl, out.ctypes.data) == 0
    return out


# ------------------------------------------------------------------ the curves and edge tables of the GPU tests
def srgb(x):
    return np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(np.maximum(x, 0.0031308), 1 / 2.4) - 0.055)


def reinhard(x):
    return x / (1.0 + x)


@functools.lru_cache(maxsize=None)
def tone_curves():
    """{name: 255 float32 edges}: q8, sRGB and Reinhard by curve_from, and a table with repeated and infinite edges"""
    from radiancecascade2dglobalillumination_amd import rc2dgi as R

    odd = np.sort(np.concatenate([[-np.inf] * 3, [-1.0, -0.0, 0.0, 0.0], np.repeat(np.linspace(0.01, 2.0, 60), 4)[:238],
                                  [3.0e38] * 2, [np.inf] * 8]).astype(f32))
    assert len(odd) == 255
    out = {"q8": R.curve_q8(), "srgb": R.curve_from(srgb), "reinhard": R.curve_from(reinhard), "odd": odd}
    for e in out.values():
        e.setflags(write=False)
    return out


def log_table():
    """the 1023-edge table sort(-2^linspace(31, -31, 511), -0.0, 2^linspace(-31, 31, 511))"""
    p = 2.0 ** np.linspace(-31, 31, 511)
    return np.concatenate([-p[::-1], [-0.0], p]).astype(f32)


# ------------------------------------------------------------------ the ABI
def test_header_declares_the_seven_calls():
    src = open(HEADER).read()
    names = set(re.findall(r"^\s*int\s*(rc2dgi_\w+)\s*\(", src, re.M))
    for q in HOST_CALLS + CTX_CALLS:
        assert q in names, f"include/rc2dgi.h does not declare {q}"
    assert re.search(r"#define RC2DGI_ABI_VERSION 5\b", src)  # exports only: found by symbol lookup
    for macro, value in (("RC2DGI_CURVE_EDGES", 255), ("RC2DGI_MAX_CURVES", 8), ("RC2DGI_HIST_MAX_EDGES", 1023)):
        assert re.search(r"#define %s %d\b" % (macro, value), src), macro
    assert re.search(r"reported by the next rc2dgi_sync[^)]*_compose_tone[^)]*_histogram", src, re.S)


def test_library_exports_the_seven_calls(R):
    L = R.load_library()
    for q in HOST_CALLS + CTX_CALLS:
        assert hasattr(L, q), f"librc2dgi.so does not export {q}"
    assert L.rc2dgi_abi_version() == 5


def test_null_context_is_an_argument_error(R):
    L = R.load_library()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))  # noqa: E731
    edges = R.curve_q8()
    views = (R.View * 1)(R.View.make("color", 0, 0, 4, 4))
    tones = (R.Tone * 1)(R.Tone(1.0, 0))
    img = np.zeros((4, 4, 4), np.uint8)
    rects = np.zeros(1, R.RECT_DTYPE)
    rects["w"] = rects["h"] = 1
    counts = np.zeros(259, u32)
    assert L.rc2dgi_set_curve(None, 1, fp(edges)) == E_ARG
    assert L.rc2dgi_compose_tone(None, views, tones, 1, 4, 4, None, p(img), 0) == E_ARG
    assert L.rc2dgi_compose_tone_device(None, views, tones, 1, 4, 4, None, p(img), 0) == E_ARG
    assert L.rc2dgi_histogram(None, 0, 4, p(rects), 1, fp(edges), 255, p(counts)) == E_ARG
    assert L.rc2dgi_histogram_device(None, 0, 4, p(rects), 1, fp(edges), 255, p(counts)) == E_ARG
    assert L.rc2dgi_histogram(None, 0, 4, None, 0, fp(edges), 255, None) == E_ARG  # n == 0 is a no-op of a context
    assert not img.any() and not counts.any()


def test_tone_is_8_bytes_in_c_csharp_and_python(R):
    sizes, fields = c_layout()
    assert sizes["rc2dgi_tone"] == 8
    assert fields[("rc2dgi_tone", "exposure")] == (0, 4) and fields[("rc2dgi_tone", "curve")] == (4, 4)
    assert ctypes.sizeof(R.Tone) == 8 and [f[0] for f in R.Tone._fields_] == ["exposure", "curve"]
    assert (R.Tone.exposure.offset, R.Tone.exposure.size) == (0, 4) and (R.Tone.curve.offset, R.Tone.curve.size) == (4, 4)
    assert R.Tone._fields_[0][1] is ctypes.c_float and R.Tone._fields_[1][1] is ctypes.c_int
    cs, cs_size = cs_layout_d("Tone")
    assert cs_size == 8 and [(n.lower(), o, z) for n, o, z in cs] == [("exposure", 0, 4), ("curve", 4, 4)]
    src = open(CS).read()
    assert re.search(r"StructLayout\(LayoutKind\.Sequential, Size = 8\)\]\s*public struct Tone\b", src)
    assert re.search(r"public float Exposure;", src) and re.search(r"public int Curve;", src)
    for decl in HOST_CALLS + CTX_CALLS:
        assert re.search(r"public static extern int %s\(" % decl, src), f"RC2DGINative.cs does not declare {decl}"
    assert re.search(r"public static Tone AutoExposure\(TexRect rect, float key", src)
    for name in ("Tone", "CURVE_EDGES", "MAX_CURVES", "HIST_MAX_EDGES", "CHANNELS", "curve_q8", "curve_from",
                 "percentile", "check_edges"):
        assert name in R.__all__, name
    assert (R.CURVE_EDGES, R.MAX_CURVES, R.HIST_MAX_EDGES) == (255, 8, 1023)
    assert R.CHANNELS == {"r": 0, "g": 1, "b": 2, "a": 3, "luma": 4}


# ------------------------------------------------------------------ rc2dgi_check_edges
def test_check_edges_refuses_and_admits(R):
    L = R.load_library()

    def code(values, m=None):
        e = np.ascontiguousarray(values, f32)
        return L.rc2dgi_check_edges(e.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(e) if m is None else m)

    assert L.rc2dgi_check_edges(None, 3) == E_ARG                # null
    assert code([1.0, 2.0], 0) == E_ARG and code([1.0, 2.0], -1) == E_ARG   # m < 1
    assert code([np.nan]) == E_ARG and code([0.0, np.nan, 1.0]) == E_ARG and code([0.0, 1.0, np.nan]) == E_ARG
    assert code([1.0, 0.5]) == E_ARG and code([0.0, 1.0, 2.0, 1.9999999]) == E_ARG   # e[i] > e[i+1]
    assert code([np.inf, -np.inf]) == E_ARG and code([1e-45, 0.0]) == E_ARG
    assert code([7.0]) == 0 and code([1.0, 2.0, 3.0]) == 0
    assert code([1.0, 1.0, 1.0, 2.0, 2.0]) == 0                   # repeats
    assert code([-np.inf, -np.inf, 0.0, np.inf, np.inf]) == 0     # infinite edges
    assert code([-1.0, -0.0, 0.0, 1.0]) == 0 and code([-1.0, 0.0, -0.0, 1.0]) == 0   # -0.0 and +0.0 compare equal
    assert code([0.0, 1e-45, 1.1754942e-38]) == 0                 # subnormals are values
    assert R.check_edges([1, 2, 3]) and not R.check_edges([3, 2]) and not R.check_edges([])
    for e in tone_curves().values():
        assert R.check_edges(e)
    assert R.check_edges(log_table()) and len(log_table()) == 1023


# ------------------------------------------------------------------ rc2dgi_curve_q8
def test_curve_q8_is_strictly_ascending_around_one_half(R):
    L = R.load_library()
    assert L.rc2dgi_curve_q8(None) == E_ARG
    e = R.curve_q8()
    assert e.dtype == f32 and e.shape == (255,)
    assert (np.diff(e) > 0).all() and e[0] > 0 and e[-1] < 1
    assert e[127] == f32(0.5)  # k = 128: 0.5f * 255 = 127.5 ties to the even 128, and the float below 0.5f gives 127
    assert e.view(u32)[127] == 0x3F000000


def special_bits(e):
    """every bit pattern within 2 of an edge (and of its negative), +-0, +-inf, NaNs, and subnormals"""
    b = e.view(u32).astype(np.int64)
    near = (b[:, None] + np.arange(-2, 3)[None, :]).reshape(-1)
    sub = np.concatenate([np.arange(0, 64), np.arange(0x7FFFC0, 0x800040), 1 << np.arange(0, 23)])
    extra = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F7FFFFF, 0xFF7FFFFF,
                      0x3F800000, 0x3F7FFFFF, 0x3F800001, 0xBF800000])
    pos = np.concatenate([near, sub, extra])
    return np.unique(np.concatenate([pos, pos | 0x80000000]) & 0xFFFFFFFF).astype(u32)


def test_bin_over_the_q8_table_is_q8(R, ref_lib):
    """bin(v) over rc2dgi_curve_q8's table equals q8(v), both evaluated in C (tests/tone_ref.c: a linear scan, and q8 as
    the header states it), on every bit pattern within 2 of an edge, on +-0, +-inf and subnormals, and on every 251st
    bit pattern of all 2^32.  For the NaNs among them, where bin is undefined, a view's T gives 0."""
    e = R.curve_q8()
    bits = special_bits(e)
    assert len(bits) > 2 * 255 * 5 and (bits == 0x80000000).any() and (bits == 1).any() and (bits == 0x7F800000).any()
    assert ref_lib.tone_sweep_list(e.ctypes.data, bits.ctypes.data, len(bits)) == 0
    count = (2 ** 32 + 250) // 251   # 0, 251, 502, .. below 2^32: negatives, NaNs and infinities among them
    assert ref_lib.tone_sweep(e.ctypes.data, 0, 251, count) == 0
    # the sweep can fail: one edge moved by one bit pattern is found near that edge
    moved = e.copy()
    moved.view(u32)[200] += 1
    assert ref_lib.tone_sweep_list(moved.ctypes.data, bits.ctypes.data, len(bits)) == 1
    # and edge k - 1 is the SMALLEST float with q8 >= k
    below = (e.view(u32) - 1).view(f32)
    for k in (1, 2, 127, 128, 129, 254, 255):
        assert ref_lib.tone_q8(float(e[k - 1])) == k and ref_lib.tone_q8(float(below[k - 1])) == k - 1


def test_curve_from_the_identity_is_the_q8_table(R):
    assert np.array_equal(R.curve_from(lambda x: x).view(u32), R.curve_q8().view(u32))
    # other curves: ascending, and a byte below and at each edge as the curve's own arithmetic gives it
    for fn in (srgb, reinhard):
        e = R.curve_from(fn)
        assert R.check_edges(e) and (np.diff(e) >= 0).all()
        fin = np.isfinite(e)
        byte = lambda x: np.rint(np.clip(fn(x.astype(np.float64)), 0, 1).astype(f32) * f32(255))  # noqa: E731
        k = np.arange(1, 256)
        assert (byte(e[fin]) >= k[fin]).all()
        prev = (e.view(u32)[fin] - 1).view(f32)
        assert (byte(prev) < k[fin]).all()


def test_level_order_descent_equals_the_linear_scan(tmp_path):
    """The search both kernels run -- k = 2k + (T[k] <= v) down the level-order tree csrc/rc2dgi_tone.h lays out --
    counts what the linear scan counts: tests/tone_tree_check.cpp, host code over the header the kernels include."""
    from radiancecascade2dglobalillumination_amd import _build

    exe = str(tmp_path / "tone_tree_check")
    subprocess.run([_build.hipcc(), "-O1", "-std=c++17", "-fno-fast-math", "-I", _build.CSRC, "-I",
                    os.path.join(ROOT, "include"), os.path.join(HERE, "tone_tree_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    m = re.match(r"checked (\d+) bad (\d+)", p.stdout)
    assert p.returncode == 0 and m and int(m.group(1)) > 1_500_000 and int(m.group(2)) == 0, p.stdout + p.stderr


def test_percentile_reads_a_record(R):
    edges = np.arange(7, dtype=f32)
    rec = np.zeros(11, u32)
    rec[1], rec[2] = 12, 2
    rec[3:] = [1, 1, 1, 1, 1, 1, 2, 2]
    assert R.percentile(rec, edges, 0.5) == 4.0 and R.percentile(rec, edges, 1.0) == 6.0
    assert R.percentile(rec, edges, 0.0) == 0.0 and R.percentile(rec, edges, 0.1) == 0.0
    bad = rec.copy()
    bad[0] = INVALID
    assert np.isnan(R.percentile(bad, edges, 0.5))
    with pytest.raises(ValueError):
        R.percentile(rec[:-1], edges, 0.5)


# ------------------------------------------------------------------ the C restatement on hand-worked cases
def test_reference_bin_counts_the_edges_at_or_below(ref_lib):
    e = [1.0, 2.0, 2.0, 4.0]
    assert [ref_bin(ref_lib, e, v) for v in (0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 5.0)] == [0, 1, 1, 3, 3, 4, 4]
    # a value equal to an edge lands above it; the float just below lands below
    assert ref_bin(ref_lib, e, np.nextafter(f32(2.0), f32(0.0))) == 1
    # -0.0 against a +0.0 edge, and +0.0 against a -0.0 edge: IEEE <= treats them alike
    assert ref_bin(ref_lib, [0.0], -0.0) == 1 and ref_bin(ref_lib, [-0.0], 0.0) == 1
    assert ref_bin(ref_lib, [-0.0, 0.0], -0.0) == 2 and ref_bin(ref_lib, [0.0], -1e-45) == 0
    # infinite edges and values
    assert ref_bin(ref_lib, [-np.inf, 0.0, np.inf], -np.inf) == 1 and ref_bin(ref_lib, [-np.inf, 0.0, np.inf], np.inf) == 3
    assert ref_bin(ref_lib, [-np.inf, 0.0, np.inf], 3.4e38) == 2


def one_texel(rgba):
    return np.asarray(rgba, f32).reshape(1, 1, 4)


def test_reference_view_tones_colour_and_not_alpha(ref_lib):
    e = ((np.arange(255) + 1) / 8).astype(f32)  # edge i is (i + 1) / 8, exactly
    nan = np.nan

    def pixel(rgba, exposure, curve, clear=(0, 0, 0, 255)):
        views = [(0, 0, 0, 1, 1, 0, (0, 0, 0, 0), exposure, curve)]
        return ref_compose(ref_lib, [(one_texel(rgba), None)], views, {3: e}, (1, 1), clear)[0, 0].tolist()

    assert pixel([0.25, 0.5, 1.0, 1.0], 1.0, 0) == [64, 128, 255, 255]           # q8, untoned
    assert pixel([0.25, 0.5, 1.0, 1.0], 2.0, 0) == [128, 255, 255, 255]          # the exposure multiplies the colour
    assert pixel([0.25, 0.5, 1.0, 0.5], 2.0, 0, (0, 0, 0, 0))[3] == 64           # and not alpha (128 over 0 at 128/255)
    assert pixel([1.0, 2.0, 30.0, 1.0], 1.0, 3) == [8, 16, 240, 255]             # bin over the slot's edges
    assert pixel([float(e[41]), float(np.nextafter(e[41], f32(0))), -5.0, 1.0], 1.0, 3) == [42, 41, 0, 255]  # on an edge: above
    assert pixel([nan, nan, 1.0, 1.0], 1.0, 3) == [0, 0, 8, 255]                 # a NaN is byte 0 under a curve
    assert pixel([nan, 0.5, 0.5, 1.0], 1.0, 0) == [0, 128, 128, 255]             # and under q8
    assert pixel([np.inf, 0.5, 0.5, 1.0], 0.0, 3) == [0, 0, 0, 255]              # inf * 0 is a NaN; 0.5 * 0 = 0 < e[0]
    assert pixel([np.inf, -np.inf, 0.5, 1.0], 1.0, 3) == [255, 0, 4, 255]
    # an all-identity tone is the untoned frame whatever the value
    zero_edge = np.concatenate([[0.0], e[1:]]).astype(f32)
    views = [(0, 0, 0, 1, 1, 0, (0, 0, 0, 0), 1.0, 1)]
    got = ref_compose(ref_lib, [(one_texel([-0.0, 0.0, -1e-45, 1.0]), None)], views, {1: zero_edge}, (1, 1))
    assert got[0, 0].tolist() == [1, 1, 0, 255]                                  # -0.0 >= a +0.0 edge


def test_reference_luma_is_five_unfused_operations_in_order(ref_lib):
    r, g, b = f32(1.0000001), f32(3.0000002), f32(5.0000005)
    want = (f32(0.2126) * r + f32(0.7152) * g) + f32(0.0722) * b   # numpy float32: every operation rounds
    got = f32(ref_lib.tone_luma(float(r), float(g), float(b)))
    assert got == want
    # triples on which a fused (wider) sum, and a re-associated one, differ: found among a few hundred random ones
    rng = np.random.default_rng(5)
    t = rng.uniform(0, 4, (400, 3)).astype(f32)
    mine = (f32(0.2126) * t[:, 0] + f32(0.7152) * t[:, 1]) + f32(0.0722) * t[:, 2]
    wide = (0.2126 * t[:, 0].astype(np.float64) + 0.7152 * t[:, 1] + 0.0722 * t[:, 2]).astype(f32)
    assoc = f32(0.2126) * t[:, 0] + (f32(0.7152) * t[:, 1] + f32(0.0722) * t[:, 2])
    k1, k2 = int(np.flatnonzero(mine != wide)[0]), int(np.flatnonzero(mine != assoc)[0])
    for k in (k1, k2):
        assert f32(ref_lib.tone_luma(*[float(x) for x in t[k]])) == mine[k]
    # and in a histogram: the luma of that texel lands in the bin of the ordered sum, an edge placed between the two
    lo, hi = sorted([float(mine[k2]), float(assoc[k2])])
    edge = f32(hi)
    tex = one_texel([t[k2, 0], t[k2, 1], t[k2, 2], 1.0])
    rec = ref_hist(ref_lib, tex, 4, [[0, 0, 1, 1]], [edge])[0]
    assert rec.tolist() == [0, 1, 0] + ([0, 1] if float(mine[k2]) == hi else [1, 0])


def test_reference_histogram_counts_and_rejects(ref_lib):
    nan = np.nan
    tex = np.zeros((4, 5, 4), f32)   # 5 wide, 4 tall
    tex[..., 0] = np.arange(20).reshape(4, 5)
    tex[..., 1] = [[nan, 1, 2, 3, 4]] * 4
    tex[..., 3] = -0.0
    edges = [5.0, 10.0, 10.0, 15.0]
    rects = [[0, 0, 5, 4],                       # the whole texture
             [0, 0, 0, 1], [0, 0, 1, 0], [0, 0, -1, 1], [0, 0, 1, -3],   # no size
             [-1, 0, 1, 1], [0, -1, 1, 1],       # a negative origin
             [1, 0, 5, 1], [0, 1, 1, 4],         # one texel over the edge
             [5, 0, 1, 1], [0, 4, 1, 1],         # an origin on the edge
             [INT_MAX, 0, 1, 1], [0, INT_MAX, 1, 1], [1, 0, INT_MAX, 1], [0, 1, 1, INT_MAX],  # x + w past INT_MAX
             [INT_MAX, INT_MAX, INT_MAX, INT_MAX], [-INT_MAX - 1, 0, 1, 1],
             [4, 3, 1, 1]]                       # the last texel
    h = ref_hist(ref_lib, tex, 0, rects, edges)
    assert h.shape == (18, 8)
    assert h[0].tolist() == [0, 20, 0, 5, 5, 0, 5, 5]   # the repeated edge's bin is empty; 10 lands above both
    assert h[17].tolist() == [0, 1, 0, 0, 0, 0, 0, 1]
    for k in range(1, 17):
        assert h[k].tolist() == [INVALID, 0, 0, 0, 0, 0, 0, 0], rects[k]
    g = ref_hist(ref_lib, tex, 1, [[0, 0, 5, 4], [0, 2, 1, 1]], [2.0])
    assert g[0].tolist() == [0, 20, 4, 4, 12] and g[1].tolist() == [0, 1, 1, 0, 0]   # a NaN counts in `nan`
    assert (g[:, 2] + g[:, 3:].sum(1) == g[:, 1]).all()
    a = ref_hist(ref_lib, tex, 3, [[0, 0, 5, 4]], [0.0])
    assert a[0].tolist() == [0, 20, 0, 0, 20]           # -0.0 against a +0.0 edge
    inf = one_texel([np.inf, -np.inf, 0, 0])
    assert ref_hist(ref_lib, inf, 0, [[0, 0, 1, 1]], [0.0, np.inf])[0].tolist() == [0, 1, 0, 0, 0, 1]
    assert ref_hist(ref_lib, inf, 1, [[0, 0, 1, 1]], [-np.inf, 0.0])[0].tolist() == [0, 1, 0, 0, 1, 0]
