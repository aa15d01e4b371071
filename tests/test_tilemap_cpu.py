"""CPU: the host-only half of rc2dgi_tilemap_device (include/rc2dgi.h) -- the export in the header, the library, C# and
ctypes, the struct's layout in C, C# and ctypes, the null-context refusal (the first of the argument errors; the rest
need a context and are in tests/test_gpu_tilemap.py), the set_cols default against Tiled's formula, the Python argument
errors that need no context, tilemap_sprites on CPU tensors against the restatement's expansion (tests/tilemap_ref.py)
on the edge maps of tests/tilemap_cases.py, each refusal term on both sides of its bound, the garbage condition of the
GPU test's narrowed grid, and the kernel's cell logic (csrc/rc2dgi_tilemap_cell.h) checked by a stand-alone program,
tests/tilemap_cell_check.cpp, built here with the host compiler and -fsanitize=address,undefined."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import sprites_ref as S
import tilemap_cases as C
import tilemap_ref as T
from conftest import ROOT
from test_host_cpu import CS

HEADER = os.path.join(ROOT, "include", "rc2dgi.h")
HERE = os.path.dirname(os.path.abspath(__file__))
E_ARG = -1


@pytest.fixture(scope="module")
def R():
    from radiancecascade2dglobalillumination_amd import _build, rc2dgi

    _build.build()
    rc2dgi.load_library()
    return rc2dgi


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


# ------------------------------------------------------------------ the export and the struct
def test_header_declares_the_call_the_struct_and_the_contract():
    src = open(HEADER).read()
    assert re.search(r"^int rc2dgi_tilemap_device\(rc2dgi_ctx \*ctx, int which, const unsigned char \*clear_rgba, "
                     r"const rc2dgi_atlas \*atlas,\s*const rc2dgi_tilemap \*map, void \*status_dev\);", src, re.M)
    assert re.search(r"typedef struct rc2dgi_tilemap \{.*?\} rc2dgi_tilemap;", src, re.S)
    assert "#define RC2DGI_ABI_VERSION 5" in src
    for phrase in ("g == 0 is an", "id = g & 0x0FFFFFFF, t = id - 1", "tx = t % set_cols, ty = t / set_cols",
                   "bit 31 flips the tile horizontally and bit 30 vertically", "bits 29 (diagonal) and 28 (hexagonal)",
                   "max_tx = (AW - margin - tile_w) / (tile_w + spacing)", "max_ty = (AH - margin - tile_h) / (tile_h + spacing)",
                   "tx > max_tx or ty > max_ty", "sx = margin + tx * (tile_w + spacing)", "dx = ox + c * tile_w",
                   "in any order, with the same clear", "{drawn, refused}", "VISIBLE cells only",
                   "faults nothing", "tile 0 does not fit"):
        assert phrase in src, phrase


def test_export_is_in_the_library_csharp_and_ctypes(R):
    L = R.load_library()
    cs = open(CS).read()
    assert hasattr(L, "rc2dgi_tilemap_device"), "librc2dgi.so does not export rc2dgi_tilemap_device"
    assert L.rc2dgi_tilemap_device.argtypes is not None and len(L.rc2dgi_tilemap_device.argtypes) == 6
    assert re.search(r"public static extern int rc2dgi_tilemap_device\(", cs)
    assert re.search(r"public struct Tilemap\b", cs)
    assert L.rc2dgi_abi_version() == 5
    assert hasattr(R.RC2DGI, "tilemap_device") and callable(R.tilemap_sprites) and callable(R.tilemap_set_cols)
    assert (R.TILE_FLIP_X, R.TILE_FLIP_Y, R.TILE_UNSUPPORTED, R.TILE_ID_MASK) == (T.FLIP_X, T.FLIP_Y,
                                                                                  T.DIAGONAL | T.HEXAGONAL, T.ID_MASK)
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "rc2dgi_tilemap_device" in open(os.path.join(ROOT, doc)).read(), doc


FIELDS = ["cells_dev", "cols", "rows", "pitch_cells", "tile_w", "tile_h", "ox", "oy", "set_cols", "margin", "spacing",
          "r", "g", "b", "a", "flags"]


def test_struct_layout_in_c_ctypes_and_csharp(R, tmp_path):
    assert ctypes.sizeof(R.Tilemap) == 56
    assert [f[0] for f in R.Tilemap._fields_] == FIELDS
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rc2dgi.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(rc2dgi_tilemap));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(rc2dgi_tilemap, {f}));\n' for f in FIELDS) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)],
                   check=True)
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == 56
    assert out[1:] == [getattr(R.Tilemap, f).offset for f in FIELDS]
    assert out[1:] == [0, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 49, 50, 51, 52]
    cs = open(CS).read()
    body = re.search(r"\[StructLayout\(LayoutKind\.Sequential, Size = 56\)\]\s*public struct Tilemap\s*\{(.*?)\}", cs, re.S)
    assert body, "the C# struct is declared with Size = 56"
    names = []
    for line in body.group(1).splitlines():
        m = re.match(r"public (void\*|int|byte|uint) (.+);", line.split("//")[0].strip())
        if m:
            names += [(m.group(1), n.strip()) for n in m.group(2).split(",")]
    assert [t for t, _ in names] == ["void*"] + ["int"] * 10 + ["byte"] * 4 + ["uint"]
    assert [n.lower() for _, n in names] == [f.replace("_", "") for f in FIELDS]


def test_a_null_context_is_refused_first(R):
    L = R.load_library()
    assert L.rc2dgi_tilemap_device(None, -1, None, None, None, None) == E_ARG


# ------------------------------------------------------------------ set_cols and the Python arguments
@pytest.mark.parametrize("AW,tw,margin,spacing,want", [(64, 16, 0, 0, 4), (54, 16, 1, 2, 3), (55, 16, 1, 2, 3),
                                                        (71, 16, 1, 2, 3), (72, 16, 1, 2, 4), (267, 32, 2, 1, 8), (266, 32, 2, 1, 7),
                                                        (16, 16, 0, 0, 1), (100, 3, 0, 7, 10)])
def test_set_cols_default_is_tileds_formula(R, AW, tw, margin, spacing, want):
    assert R.tilemap_set_cols(AW, tw, margin, spacing) == want == T.tiled_set_cols(AW, tw, margin, spacing)
    # as many columns as tiles that fit between the two margins, a spacing between neighbours
    n = 0
    while 2 * margin + (n + 1) * tw + n * spacing <= AW:
        n += 1
    assert n == want


def test_tilemap_sprites_refuses_bad_arguments(R, torch):
    g = torch.zeros((2, 2), dtype=torch.int32)
    with pytest.raises(ValueError):
        R.tilemap_sprites(g.to(torch.int64), (16, 16), (0, 0), (64, 48), (64, 48))
    with pytest.raises(ValueError):
        R.tilemap_sprites(g.reshape(4), (16, 16), (0, 0), (64, 48), (64, 48))
    with pytest.raises(ValueError):
        R.tilemap_sprites(g, (65, 16), (0, 0), (64, 48), (64, 48))  # tile 0 does not fit
    with pytest.raises(ValueError):
        R.tilemap_sprites(g, (16, 16), (0, 0), (64, 48), (64, 48), margin=40)
    with pytest.raises(ValueError):
        R.tilemap_sprites(g, (16, 16), (0, 0), (64, 48), (64, 48), set_cols=0)
    assert tuple(R.tilemap_sprites(g, (16, 16), (0, 0), (64, 48), (64, 48)).shape) == (0, 8)


# ------------------------------------------------------------------ tilemap_sprites against the restatement
def expansion(R, torch, k, replace=False):
    m = dict(k["m"], replace=replace)
    got = R.tilemap_sprites(torch.from_numpy(k["cells"].view(np.int32)), m["tile"], m["origin"], (k["AW"], k["AH"]),
                            (k["W"], k["H"]), m["set_cols"], m["margin"], m["spacing"], m["tint"], replace)
    want, status = T.expand(k["cells"], k["AW"], k["AH"], k["W"], k["H"], m)
    return got.numpy(), want, status


@pytest.mark.parametrize("k", C.edge_cases(), ids=lambda k: k["name"])
def test_tilemap_sprites_equals_the_restated_expansion(R, torch, k):
    for replace in (False, True):
        got, want, status = expansion(R, torch, k, replace)
        assert got.dtype == np.int32 and got.shape == want.shape, (got.shape, want.shape)
        assert np.array_equal(got, want)
        assert status[0] == len(want)
        assert S.accepted(got, k["AW"], k["AH"]).all()
        # every sprite of the list meets the target
        assert ((got[:, 4] + got[:, 2] > 0) & (got[:, 4] < k["W"]) & (got[:, 5] + got[:, 3] > 0) & (got[:, 5] < k["H"])).all()
    if k["name"].startswith("off"):
        assert status == [0, 0] and len(want) == 0
    else:
        assert status[0] > 0
        assert status[1] >= 1 or k["cells"].size < 2, "a spoiled cell is visible and refused"


def test_the_edge_maps_hold_what_they_are_named_for():
    ks = {k["name"]: k for k in C.edge_cases()}
    for name, col in (("16x16 boundary on 63", 63), ("16x16 boundary on 64 and 128", 64),
                      ("16x16 boundary on 64 and 128", 128), ("16x16 boundary on 65", 65)):
        k = ks[name]
        assert (col - k["m"]["origin"][0]) % 16 == 0 and col < k["W"], name  # a cell's first column is `col`
    big = ks["300x100 tile"]
    assert big["m"]["tile"][0] > big["W"] and big["m"]["tile"][1] > big["H"]
    g = ks["16x16 boundary on 64 and 128"]["cells"]
    assert (g == 0).any() and (g & T.FLIP_X).any() and (g & T.FLIP_Y).any() and (g & T.DIAGONAL).any() \
        and (g & T.HEXAGONAL).any()


# ------------------------------------------------------------------ each refusal term on both sides of its bound
def kinds(words, AW, AH, m):
    return T.decode(np.array(words, np.int64), AW, AH, m)[0].tolist()


def test_each_refusal_term_on_both_sides_of_its_bound(R, torch):
    AW, AH = 64 + 5, 48 + 15  # 4 x 3 whole tiles of 16 x 16 and a part of one more on either axis
    m = T.layer((16, 16), set_cols=6)
    E, D, X = T.EMPTY, T.DRAWN, T.REFUSED
    assert kinds([0], AW, AH, m) == [E]
    assert kinds([1, 1 | T.FLIP_X, 1 | T.FLIP_Y, 1 | T.FLIP_X | T.FLIP_Y], AW, AH, m) == [D] * 4
    assert kinds([1 | T.DIAGONAL, 1 | T.HEXAGONAL, 1 | T.DIAGONAL | T.FLIP_X], AW, AH, m) == [X] * 3
    assert kinds([T.FLIP_X, T.FLIP_Y, T.FLIP_X | T.FLIP_Y], AW, AH, m) == [X] * 3  # flag bits alone: id == 0
    assert kinds([4, 5, 6, 7], AW, AH, m) == [D, X, X, D]          # tx = 3 (max_tx), 4, 5, then tx = 0 of row 1
    assert kinds([12 + 4, 18 + 1, T.ID_MASK], AW, AH, m) == [D, X, X]  # ty = 2 (max_ty), then 3, then far beyond
    # the quotient on both sides of a whole tile: 63 pixels hold three tiles, 64 hold four
    assert kinds([4], 63, 48, m) == [X] and kinds([4], 64, 48, m) == [D]
    assert kinds([13], 64, 47, m) == [X] and kinds([13], 64, 48, m) == [D]
    mm = T.layer((16, 16), set_cols=6, margin=1, spacing=2)  # tile tx begins at 1 + 18 tx
    assert kinds([3], 1 + 36 + 16, 48, mm) == [D] and kinds([3], 1 + 36 + 15, 48, mm) == [X]
    # tilemap_sprites agrees on every word above
    words = [0, 1, 1 | T.FLIP_X, 1 | T.DIAGONAL, 1 | T.HEXAGONAL, T.FLIP_X, 4, 5, 6, 7, 16, 19, T.ID_MASK]
    g = np.array(words, np.uint32).reshape(1, -1)
    got = R.tilemap_sprites(torch.from_numpy(g.view(np.int32)), (16, 16), (0, 0), (AW, AH), (16 * len(words), 16), 6)
    want, status = T.expand(g, AW, AH, 16 * len(words), 16, m)
    assert np.array_equal(got.numpy(), want) and status == [5, 7]
    # visibility on both sides of its bound: a cell whose last column is 0, and one a pixel further left
    one = np.array([[1]], np.uint32)
    for ox, n in ((-15, 1), (-16, 0), (63, 1), (64, 0)):
        assert T.expand(one, AW, AH, 64, 48, T.layer((16, 16), (ox, 0), 6))[1] == [n, 0], ox
        assert T.expand(one, AW, AH, 64, 48, T.layer((16, 16), (0, ox if ox < 0 else ox - 16), 6))[1] == [n, 0], ox


# ------------------------------------------------------------------ the garbage condition of the GPU test
def garbage_case(narrowed, seed=123):
    q = C.GARBAGE
    AW, AH = C.set_size(q["tile"], *q["set_tiles"])
    ntiles = q["set_tiles"][0] * q["set_tiles"][1]
    g = C.narrowed_garbage(q["rows"], q["cols"], ntiles, seed) if narrowed else C.raw_garbage(q["rows"], q["cols"], seed)
    return g, AW, AH, T.layer(q["tile"], q["origin"], None, 0, 0, C.TINT)


def test_the_narrowed_garbage_grid_is_neither_all_drawn_nor_all_refused():
    q = C.GARBAGE
    g, AW, AH, m = garbage_case(True)
    wd, (drawn, refused) = T.expand(g, AW, AH, q["W"], q["H"], m)
    c0, c1, r0, r1 = T.visible(m, q["rows"], q["cols"], q["W"], q["H"])
    nvis = (c1 - c0 + 1) * (r1 - r0 + 1)
    print(f"visible {nvis}, drawn {drawn}, refused {refused}")
    assert nvis >= 60
    assert drawn * 20 >= nvis, "at least one visible cell in twenty is accepted"
    assert refused * 20 >= nvis, "at least one visible cell in twenty is refused"
    assert drawn + refused <= nvis
    raw = garbage_case(False)
    assert T.expand(raw[0], raw[1], raw[2], q["W"], q["H"], raw[3])[1][1] >= nvis - 2, "raw words are refused"


# ------------------------------------------------------------------ the cell logic, on the host
@pytest.fixture(scope="module")
def cell_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tilemap_cell") / "tilemap_cell_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "radiancecascade2dglobalillumination_amd", "csrc"),
                    "-o", exe, os.path.join(HERE, "tilemap_cell_check.cpp")], check=True)
    return exe


def test_cell_logic_equals_a_64_bit_walk_under_the_sanitizers(cell_check):
    r = subprocess.run([cell_check], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"axis pixels checked (\d+), words and source pixels checked (\d+), wrong 0", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) > 5_000_000 and int(m.group(2)) > 100_000  # it is not vacuous
    assert "runtime error" not in r.stderr


def test_the_check_sees_a_tile_refused_too_late(cell_check):
    r = subprocess.run([cell_check, "--late"], capture_output=True, text=True)
    assert r.returncode == 1 and "WRONG decode" in r.stdout and "runtime error" not in r.stderr
