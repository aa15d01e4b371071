"""CPU: the host-only half of the display frame (include/rc2dgi.h, rc2dgi_display_layout / rc2dgi_view) -- the
reference's display layout (RC2DGI.cs:139-163, 435-448) and the byte layout of rc2dgi_view in C, C# and Python."""
import ctypes

import pytest

from test_host_cpu import c_layout, cs_layout

RED = (230, 41, 55, 255)
THUMBS = [0, 1, 3, 4, 5, 6, 7]  # COLOR, EMISSIVE, JUMP2, DIST, GI1, GI2, TEMP
VIEW_FIELDS = ["which", "x", "y", "w", "h", "filter", "r", "g", "b", "a"]


@pytest.fixture(scope="module")
def R():
    from radiancecascade2dglobalillumination_amd import _build, rc2dgi

    _build.build()
    rc2dgi.load_library()
    return rc2dgi


def as_tuple(v):
    return (v.which, v.x, v.y, v.w, v.h, v.filter, (v.r, v.g, v.b, v.a))


def expected_layout(W, H):
    want = [(0, 0, 0, W, H, 0, (0, 0, 0, 0))]
    for k, which in enumerate(THUMBS):
        want.append((which, W - 110, 10 * (k + 1) + 100 * k, 100, 100, 0, RED))
    return want


def test_display_layout_1200x900(R):
    views = R.display_layout(1200, 900)
    assert len(views) == 8
    assert [as_tuple(v) for v in views] == expected_layout(1200, 900)
    assert [v.y for v in views[1:]] == [10, 120, 230, 340, 450, 560, 670]
    assert all(v.x == 1090 for v in views[1:])


def test_display_layout_320x200(R):
    views = R.display_layout(320, 200)
    assert [as_tuple(v) for v in views] == expected_layout(320, 200)
    assert all(v.x == 210 for v in views[1:])


def test_display_layout_writes_at_most_max_views(R):
    L = R.load_library()
    cfg = R._Config(1200, 900, 6, 1.0, 2.0, 0, 0, 0, (ctypes.c_int * 4)())
    arr = (R.View * 5)()
    for v in arr:
        v.which = -77
    assert L.rc2dgi_display_layout(ctypes.byref(cfg), arr, 3) == 8
    assert [as_tuple(v) for v in arr[:3]] == expected_layout(1200, 900)[:3]
    assert arr[3].which == -77 and arr[4].which == -77
    assert L.rc2dgi_display_layout(ctypes.byref(cfg), None, 0) == 8


def test_display_layout_null_config(R):
    L = R.load_library()
    arr = (R.View * 8)()
    assert L.rc2dgi_display_layout(None, arr, 8) == -1  # RC2DGI_E_ARG


def test_view_is_28_bytes_in_c_csharp_and_python(R):
    sizes, fields = c_layout()
    assert sizes["rc2dgi_view"] == 28
    cs, cs_size = cs_layout("View")
    assert cs_size == 28 and ctypes.sizeof(R.View) == 28
    assert len(cs) == len(VIEW_FIELDS) == len(R.View._fields_)
    for (cs_name, cs_off, cs_sz), name in zip(cs, VIEW_FIELDS):
        off, size = fields[("rc2dgi_view", name)]
        assert (cs_off, cs_sz) == (off, size), f"C# View.{cs_name} at {cs_off} ({cs_sz} B), C {name} at {off} ({size} B)"
        py = getattr(R.View, name)
        assert (py.offset, py.size) == (off, size), f"Python View.{name} at {py.offset}, C at {off}"
    assert [f[0] for f in R.View._fields_] == VIEW_FIELDS
