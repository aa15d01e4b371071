"""Host-side mirror of the reference's GI path over the librc2dgi C ABI.

The reference drives its per-frame GI from C# (RC2DGI.cs):

* knobs/globals ``cascadeCount``, ``renderScale``, ``rayRange`` (RC2DGI.cs:28-31, 66-68)
  and the GUI-driven uniforms ``sunAngle``, ``sunColor``, ``skyColor``, ``skyRadiance``,
  ``reflectivity``, ``cascadeBlurRadius`` (RC2DGI.cs:33-41);
* ``DoRC2DGI()`` (RC2DGI.cs:267-406) -> :meth:`RC2DGI.do_rc2dgi`;
* ``SetGIShaderValues()`` (RC2DGI.cs:408-433) -> :meth:`RC2DGI.set_shader_value` with the
  reference uniform names (``_RayRange``, ``_SkyColor`` ...);
* the painted ``colorRT``/``emissiveRT`` inputs and the debug views of ``jumpRT2``,
  ``distRT``, ``giRT1``, ``giRT2``, ``tempRT`` (RC2DGI.cs:156-163) ->
  :meth:`RC2DGI.upload` / :meth:`RC2DGI.download`.

Every call goes through ``librc2dgi.so`` (HIP kernels for gfx950).  There is no CPU
fallback: if the library is missing or the GPU call fails, this module raises.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "librc2dgi.so")

# rc2dgi_rt (include/rc2dgi.h)
RT = {"color": 0, "emissive": 1, "jump1": 2, "jump2": 3, "dist": 4, "gi1": 5, "gi2": 6, "temp": 7, "blur": 8,
      "final_gi": 9}
SCREEN_RTS = ("color", "emissive", "jump1", "jump2", "dist", "temp")
FMT_RGBA8, FMT_RGBA32F = 0, 1
FMT_RGBA16F = 2  # IEEE binary16, round to nearest even: read / read_into only (upload and download refuse it)
READ_FLIP = 1    # rc2dgi_read: image row 0 is the rectangle's top row
WRITE_FLIP = 1   # rc2dgi_write: image row 0 is the rectangle's top row
WRITE_BLEND = 2  # rc2dgi_write: the image is blended over the texels (SRC_ALPHA, ONE_MINUS_SRC_ALPHA)
_READ_FORMATS = {"float32": FMT_RGBA32F, "float16": FMT_RGBA16F, "uint8": FMT_RGBA8}  # by numpy / torch dtype name
STATUS = {0: "OK", -1: "E_ARG", -2: "E_UNIFORM", -3: "E_HIP", -4: "E_OOM", -5: "E_UNSUPPORTED", -6: "E_STATE", -7: "E_DEVICE"}
PASS_NAMES = ("screenuv", "jfa", "rc", "blur", "merge", "total")


class RC2DGIError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"rc2dgi {STATUS.get(code, code)}: {msg}")
        self.code = code


class Prim(ctypes.Structure):
    """rc2dgi_prim: raylib DrawRectangleRec (kind 0) / DrawCircleV (kind 1, w = radius)."""
    _fields_ = [("kind", ctypes.c_int), ("x", ctypes.c_float), ("y", ctypes.c_float), ("w", ctypes.c_float),
                ("h", ctypes.c_float), ("r", ctypes.c_ubyte), ("g", ctypes.c_ubyte), ("b", ctypes.c_ubyte),
                ("a", ctypes.c_ubyte)]


class Atlas(ctypes.Structure):
    """rc2dgi_atlas: a device image of w x h pixels (row 0 = the top row) that rc2dgi_sprites_device draws from;
    pitch_bytes 0 is a tight row; format FMT_RGBA8 / FMT_RGBA16F / FMT_RGBA32F."""
    _fields_ = [("dev", ctypes.c_void_p), ("w", ctypes.c_int), ("h", ctypes.c_int), ("pitch_bytes", ctypes.c_int),
                ("format", ctypes.c_int)]


class Sprite(ctypes.Structure):
    """rc2dgi_sprite (32 bytes): the source rectangle (sx, sy, w, h) of the atlas, drawn 1:1 with its top-left pixel
    at (dx, dy) in raylib screen coordinates, a tint and SPRITE_* flags."""
    _fields_ = [("sx", ctypes.c_int), ("sy", ctypes.c_int), ("w", ctypes.c_int), ("h", ctypes.c_int),
                ("dx", ctypes.c_int), ("dy", ctypes.c_int), ("r", ctypes.c_ubyte), ("g", ctypes.c_ubyte),
                ("b", ctypes.c_ubyte), ("a", ctypes.c_ubyte), ("flags", ctypes.c_uint)]


SPRITE_FLIP_X, SPRITE_FLIP_Y, SPRITE_REPLACE = 1, 2, 4


class SpriteXf(ctypes.Structure):
    """rc2dgi_sprite_xf (48 bytes): the source rectangle (sx, sy, w, h) of the atlas mapped onto the parallelogram
    P, P + A, P + A + B, P + B of the screen (its top-left corner on P = (px, py), its top edge on A = (ax, ay), its
    left edge on B = (bx, by)), a tint and SPRITE_REPLACE | SPRITE_LINEAR."""
    _fields_ = [("sx", ctypes.c_int), ("sy", ctypes.c_int), ("w", ctypes.c_int), ("h", ctypes.c_int),
                ("px", ctypes.c_float), ("py", ctypes.c_float), ("ax", ctypes.c_float), ("ay", ctypes.c_float),
                ("bx", ctypes.c_float), ("by", ctypes.c_float), ("r", ctypes.c_ubyte), ("g", ctypes.c_ubyte),
                ("b", ctypes.c_ubyte), ("a", ctypes.c_ubyte), ("flags", ctypes.c_uint)]


SPRITE_LINEAR = 8


class Shape(ctypes.Structure):
    """rc2dgi_shape (32 bytes): kind SHAPE_*, six floats by kind (RECT x, y, w, h; CIRCLE x, y, radius; TRIANGLE
    x0, y0, x1, y1, x2, y2; LINE x0, y0, x1, y1, thick; ELLIPSE cx, cy, rh, rv) and a raylib Color."""
    _fields_ = [("kind", ctypes.c_int), ("v", ctypes.c_float * 6), ("r", ctypes.c_ubyte), ("g", ctypes.c_ubyte),
                ("b", ctypes.c_ubyte), ("a", ctypes.c_ubyte)]


SHAPE_RECT, SHAPE_CIRCLE, SHAPE_TRIANGLE, SHAPE_LINE, SHAPE_ELLIPSE = 0, 1, 2, 3, 4


class Gradient(ctypes.Structure):
    """rc2dgi_gradient (48 bytes): kind GRAD_*, Shape's six floats by kind, four raylib Colors (TRIANGLE c[0..2] a
    vertex; RECT c[0..3] = TL, BL, BR, TR; CIRCLE and ELLIPSE c[0] the centre, c[1] the rim; LINE c[0] the (x0, y0) end,
    c[1] the other) and the gain that multiplies r, g, b after the interpolation."""
    _fields_ = [("kind", ctypes.c_int), ("v", ctypes.c_float * 6), ("c", (ctypes.c_ubyte * 4) * 4),
                ("gain", ctypes.c_float)]


GRAD_RECT, GRAD_CIRCLE, GRAD_TRIANGLE, GRAD_LINE, GRAD_ELLIPSE = 0, 1, 2, 3, 4


class Tilemap(ctypes.Structure):
    """rc2dgi_tilemap (56 bytes): a rows x cols grid of 32-bit cell words on the device (Tiled's global tile ids, 0 an
    empty cell, bit 31 / 30 the horizontal / vertical flip), cells of tile_w x tile_h pixels with cell (0, 0) at (ox, oy)
    of the screen, the tile set's layout (set_cols, margin, spacing), the layer's tint and SPRITE_REPLACE or 0."""
    _fields_ = [("cells_dev", ctypes.c_void_p), ("cols", ctypes.c_int), ("rows", ctypes.c_int),
                ("pitch_cells", ctypes.c_int), ("tile_w", ctypes.c_int), ("tile_h", ctypes.c_int), ("ox", ctypes.c_int),
                ("oy", ctypes.c_int), ("set_cols", ctypes.c_int), ("margin", ctypes.c_int), ("spacing", ctypes.c_int),
                ("r", ctypes.c_ubyte), ("g", ctypes.c_ubyte), ("b", ctypes.c_ubyte), ("a", ctypes.c_ubyte),
                ("flags", ctypes.c_uint)]


TILE_FLIP_X, TILE_FLIP_Y, TILE_UNSUPPORTED, TILE_ID_MASK = 0x80000000, 0x40000000, 0x30000000, 0x0FFFFFFF

FILTER_RT, FILTER_POINT, FILTER_LINEAR = 0, 1, 2
MAX_VIEWS = 16
RED = (230, 41, 55, 255)  # raylib Color.Red, the thumbnails' border (RC2DGI.cs:435-448)


class View(ctypes.Structure):
    """rc2dgi_view: one draw of the display frame -- render texture `which` into the window rectangle
    (x, y, w, h) (y down, clipped to the window), then a one-pixel border (a == 0: none)."""
    _fields_ = [("which", ctypes.c_int), ("x", ctypes.c_int), ("y", ctypes.c_int), ("w", ctypes.c_int),
                ("h", ctypes.c_int), ("filter", ctypes.c_int), ("r", ctypes.c_ubyte), ("g", ctypes.c_ubyte),
                ("b", ctypes.c_ubyte), ("a", ctypes.c_ubyte)]

    @classmethod
    def make(cls, which, x, y, w, h, filter=FILTER_RT, border=(0, 0, 0, 0)):
        """which: a name of RT or an rc2dgi_rt id."""
        return cls(RT[which] if isinstance(which, str) else int(which), int(x), int(y), int(w), int(h), int(filter),
                   *(int(v) for v in border))


class Ray(ctypes.Structure):
    """rc2dgi_ray: origin and direction in GL texture coordinates (the direction is used as given) and the
    interval [t0, t1] marched."""
    _fields_ = [("ox", ctypes.c_float), ("oy", ctypes.c_float), ("dx", ctypes.c_float), ("dy", ctypes.c_float),
                ("t0", ctypes.c_float), ("t1", ctypes.c_float)]


class RayHit(ctypes.Structure):
    """rc2dgi_rayhit: how a ray ended (RAY_*), the distRT texels it read, the hit texel (GL order) or (-1, -1), where
    the loop ended (t, u, v) and the shader's hit record (r, g, b, a)."""
    _fields_ = [("status", ctypes.c_int), ("steps", ctypes.c_int), ("ix", ctypes.c_int), ("iy", ctypes.c_int),
                ("t", ctypes.c_float), ("u", ctypes.c_float), ("v", ctypes.c_float), ("r", ctypes.c_float),
                ("g", ctypes.c_float), ("b", ctypes.c_float), ("a", ctypes.c_float)]


RAY_INVALID, RAY_RANGE, RAY_EDGE, RAY_EMISSIVE, RAY_SURFACE, RAY_STEPS = -1, 0, 1, 2, 3, 4
RAY_DTYPE = np.dtype([(n, np.float32) for n, _ in Ray._fields_])
HIT_DTYPE = np.dtype([(n, np.int32 if t is ctypes.c_int else np.float32) for n, t in RayHit._fields_])
HIT_INT_FIELDS = 4  # status, steps, ix, iy; the seven float fields follow
QUERY_MAX = 1 << 24


def hit_floats(hits):
    """The float fields (t, u, v, r, g, b, a) of the int32 (n, 11) tensor RC2DGI.raycast returns for device rays: a
    float32 (n, 7) view of the same memory."""
    import torch

    return hits[:, HIT_INT_FIELDS:].view(torch.float32)


class Rect(ctypes.Structure):
    """rc2dgi_rect: w x h texels of a render texture from (x, y), GL order (row 0 = the bottom)."""
    _fields_ = [("x", ctypes.c_int), ("y", ctypes.c_int), ("w", ctypes.c_int), ("h", ctypes.c_int)]


class Stats(ctypes.Structure):
    """rc2dgi_stats: what rc2dgi_reduce reports for one rectangle -- status (STATS_*), texels = w * h and per channel
    r, g, b, a the count of NaN / infinite values, min and max of the finite ones and their float64 sum in the header's
    fixed order.  sum[c] / (texels - nonfinite[c]) is the mean."""
    _fields_ = [("status", ctypes.c_int), ("texels", ctypes.c_int), ("nonfinite", ctypes.c_int * 4),
                ("min", ctypes.c_float * 4), ("max", ctypes.c_float * 4), ("sum", ctypes.c_double * 4)]


STATS_OK, STATS_INVALID = 0, -1
RECT_DTYPE = np.dtype([(n, np.int32) for n, _ in Rect._fields_])
STATS_DTYPE = np.dtype([("status", np.int32), ("texels", np.int32), ("nonfinite", np.int32, (4,)),
                        ("min", np.float32, (4,)), ("max", np.float32, (4,)), ("sum", np.float64, (4,))])
STATS_WORDS = 22  # an rc2dgi_stats record as int32 words: 6 ints, 8 floats from word 6, 4 doubles from word 14
REDUCE_MAX = 1 << 20


def stats_view(words):
    """The float and double fields of the int32 (n, 22) tensor RC2DGI.reduce_into fills, from its numpy copy
    (`words`: that tensor, or an int32 (n, 22) array): a structured STATS_DTYPE array of n records over a copy of
    the same bytes."""
    if hasattr(words, "data_ptr"):
        words = words.cpu().numpy()
    a = np.ascontiguousarray(words, np.int32)
    if a.ndim != 2 or a.shape[1] != STATS_WORDS:
        raise ValueError(f"stats_view: expected (n, {STATS_WORDS}) int32 words, got {a.shape}")
    return a.reshape(-1).view(STATS_DTYPE)


def _rect_array(rects):
    """rects as a contiguous RECT_DTYPE array: an (n, 4) int array (x, y, w, h) or a RECT_DTYPE array."""
    a = np.asarray(rects)
    if a.dtype == RECT_DTYPE:
        return np.ascontiguousarray(a).reshape(-1)
    if a.size == 0:  # an empty list: n == 0, a successful no-op of the ABI
        return np.zeros(0, RECT_DTYPE)
    a = np.ascontiguousarray(a, np.int32)
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError(f"reduce: expected (n, 4) rectangles, got {a.shape}")
    return a.reshape(-1).view(RECT_DTYPE)


class Tone(ctypes.Structure):
    """rc2dgi_tone: how a view's colour channels become bytes -- T(c * exposure), T = q8 for curve 0, else bin() over
    the 255 edges of that curve slot (RC2DGI.set_curve).  Alpha and the border are not toned."""
    _fields_ = [("exposure", ctypes.c_float), ("curve", ctypes.c_int)]


CURVE_EDGES, MAX_CURVES, HIST_MAX_EDGES = 255, 8, 1023
CHANNELS = {"r": 0, "g": 1, "b": 2, "a": 3, "luma": 4}
HIST_HEAD = 3  # words of a histogram record before bin[0]: status, texels, nan


def _tone_array(tones, n):
    """tones as a ctypes array of n Tone: Tone records, (exposure, curve) pairs or bare exposures; None stays None."""
    if tones is None:
        return None
    if len(tones) != n:
        raise ValueError(f"compose: {n} views and {len(tones)} tones")
    arr = (Tone * max(n, 1))()
    for k, t in enumerate(tones):
        if isinstance(t, Tone):
            arr[k] = t
        elif isinstance(t, (tuple, list)):
            arr[k] = Tone(float(t[0]), int(t[1]))
        else:
            arr[k] = Tone(float(t), 0)
    return arr


def _edge_array(edges):
    e = np.ascontiguousarray(edges, np.float32).reshape(-1)
    return e, e.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _view_array(views):
    arr = (View * max(len(views), 1))()
    for k, v in enumerate(views):
        arr[k] = v if isinstance(v, View) else View.make(*v)
    return arr


class _Config(ctypes.Structure):
    _fields_ = [("screen_width", ctypes.c_int), ("screen_height", ctypes.c_int), ("cascade_count", ctypes.c_int),
                ("render_scale", ctypes.c_float), ("ray_range", ctypes.c_float), ("storage", ctypes.c_int),
                ("device", ctypes.c_int), ("flags", ctypes.c_int), ("reserved", ctypes.c_int * 4)]


_lib = None


def load_library(path: Optional[str] = None):
    """Load librc2dgi.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("RC2DGI_LIB") or LIB_PATH  # (an empty RC2DGI_LIB: the in-tree build)
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)")
    # One HIP runtime per process: PyTorch ships its own libamdhip64.so.7.  Loading torch first
    # makes this library bind to that copy instead of pulling a second runtime in later.
    try:
        import torch  # noqa: F401
    except Exception:  # torch is optional for the library itself
        pass
    L = ctypes.CDLL(path)
    vp, ip, fp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float)
    sig = {
        "rc2dgi_create": ([ctypes.POINTER(_Config), ctypes.POINTER(vp)], ctypes.c_int),
        "rc2dgi_destroy": ([vp], ctypes.c_int),
        "rc2dgi_set_uniform": ([vp, ctypes.c_char_p, fp, ctypes.c_int], ctypes.c_int),
        "rc2dgi_get_uniform": ([vp, ctypes.c_char_p, fp, ctypes.c_int], ctypes.c_int),
        "rc2dgi_set_uniform_i": ([vp, ctypes.c_char_p, ctypes.c_int], ctypes.c_int),
        "rc2dgi_upload": ([vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int], ctypes.c_int),
        "rc2dgi_upload_device": ([vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int], ctypes.c_int),
        "rc2dgi_do": ([vp], ctypes.c_int),
        "rc2dgi_sync": ([vp], ctypes.c_int),
        "rc2dgi_download": ([vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int], ctypes.c_int),
        "rc2dgi_query": ([vp, ip, ip, ip, ip], ctypes.c_int),
        "rc2dgi_last_error": ([vp], ctypes.c_char_p),
        "rc2dgi_abi_version": ([], ctypes.c_int),
        "rc2dgi_set_stream": ([vp, vp], ctypes.c_int),
        "rc2dgi_set_timing": ([vp, ctypes.c_int], ctypes.c_int),
        "rc2dgi_pass_times": ([vp, fp, ctypes.c_int, fp, ctypes.c_int], ctypes.c_int),
        "rc2dgi_set_direction_table": ([vp, ctypes.c_int, fp, ctypes.c_int], ctypes.c_int),
        "rc2dgi_set_sky_table": ([vp, fp, ctypes.c_int], ctypes.c_int),
        "rc2dgi_set_keep_levels": ([vp, ctypes.c_int], ctypes.c_int),
        "rc2dgi_set_tuning": ([vp, ctypes.c_char_p, ctypes.c_int], ctypes.c_int),
        "rc2dgi_get_tuning": ([vp, ctypes.c_char_p, ip], ctypes.c_int),
        "rc2dgi_download_level": ([vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int], ctypes.c_int),
        "rc2dgi_autotune": ([vp, ctypes.c_int], ctypes.c_int),
        "rc2dgi_paint": ([vp, ctypes.c_int, ctypes.POINTER(ctypes.c_ubyte), vp, ctypes.c_int], ctypes.c_int),
        "rc2dgi_set_shard": ([vp, ctypes.c_int, ctypes.c_int], ctypes.c_int),
        "rc2dgi_shard_rows": ([vp, ip, ip], ctypes.c_int),
        "rc2dgi_shard_unique_id": ([vp, ctypes.c_int], ctypes.c_int),
        "rc2dgi_shard_connect": ([vp, vp, ctypes.c_int], ctypes.c_int),
        "rc2dgi_do_phase": ([vp, ctypes.c_int], ctypes.c_int),
        "rc2dgi_do_group": ([ctypes.POINTER(vp), ctypes.c_int], ctypes.c_int),
        "rc2dgi_device_buffer": ([vp, ctypes.c_int, ctypes.POINTER(vp), ip], ctypes.c_int),
        "rc2dgi_plan_rows": ([ctypes.POINTER(_Config), ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_int, ip,
                              ctypes.c_int], ctypes.c_int),
        "rc2dgi_plan_jfa_exchange": ([ctypes.POINTER(_Config), ctypes.c_int, ctypes.c_int, ip, ip, ctypes.c_int],
                                     ctypes.c_int),
        "rc2dgi_plan_jfa_window": ([ctypes.POINTER(_Config), ctypes.c_int, ctypes.c_int, ctypes.c_int, ip, ip],
                                   ctypes.c_int),
        "rc2dgi_download_table": ([vp, ctypes.c_int, vp, ctypes.c_int], ctypes.c_int),
        "rc2dgi_plan_group_waits": ([ctypes.POINTER(_Config), ctypes.c_int, ctypes.c_int, ctypes.c_int, ip,
                                     ctypes.c_int], ctypes.c_int),
        "rc2dgi_display_layout": ([ctypes.POINTER(_Config), ctypes.POINTER(View), ctypes.c_int], ctypes.c_int),
        "rc2dgi_compose": ([vp, ctypes.POINTER(View), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                            ctypes.POINTER(ctypes.c_ubyte), vp, ctypes.c_int], ctypes.c_int),
        "rc2dgi_compose_device": ([vp, ctypes.POINTER(View), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                   ctypes.POINTER(ctypes.c_ubyte), vp, ctypes.c_int], ctypes.c_int),
        "rc2dgi_sample": ([vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp], ctypes.c_int),
        "rc2dgi_sample_device": ([vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp], ctypes.c_int),
        "rc2dgi_raycast": ([vp, vp, ctypes.c_int, vp], ctypes.c_int),
        "rc2dgi_raycast_device": ([vp, vp, ctypes.c_int, vp], ctypes.c_int),
        "rc2dgi_reduce": ([vp, ctypes.c_int, vp, ctypes.c_int, vp], ctypes.c_int),
        "rc2dgi_reduce_device": ([vp, ctypes.c_int, vp, ctypes.c_int, vp], ctypes.c_int),
        "rc2dgi_check_edges": ([fp, ctypes.c_int], ctypes.c_int),
        "rc2dgi_curve_q8": ([fp], ctypes.c_int),
        "rc2dgi_set_curve": ([vp, ctypes.c_int, fp], ctypes.c_int),
        "rc2dgi_compose_tone": ([vp, ctypes.POINTER(View), ctypes.POINTER(Tone), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                 ctypes.POINTER(ctypes.c_ubyte), vp, ctypes.c_int], ctypes.c_int),
        "rc2dgi_compose_tone_device": ([vp, ctypes.POINTER(View), ctypes.POINTER(Tone), ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, ctypes.POINTER(ctypes.c_ubyte), vp, ctypes.c_int], ctypes.c_int),
        "rc2dgi_histogram": ([vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, fp, ctypes.c_int, vp], ctypes.c_int),
        "rc2dgi_histogram_device": ([vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, fp, ctypes.c_int, vp],
                                    ctypes.c_int),
        "rc2dgi_read": ([vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int], ctypes.c_int),
        "rc2dgi_read_device": ([vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int], ctypes.c_int),
        "rc2dgi_write": ([vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int], ctypes.c_int),
        "rc2dgi_write_device": ([vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int], ctypes.c_int),
        "rc2dgi_paint_device": ([vp, ctypes.c_int, ctypes.POINTER(ctypes.c_ubyte), vp, ctypes.c_int, vp, vp],
                                ctypes.c_int),
        "rc2dgi_shapes_device": ([vp, ctypes.c_int, ctypes.POINTER(ctypes.c_ubyte), vp, ctypes.c_int, vp, vp],
                                 ctypes.c_int),
        "rc2dgi_paint_device_limits": ([ctypes.POINTER(_Config), ip, ctypes.POINTER(ctypes.c_longlong)], ctypes.c_int),
        "rc2dgi_sprites_device": ([vp, ctypes.c_int, ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(Atlas), vp,
                                   ctypes.c_int, vp, vp], ctypes.c_int),
        "rc2dgi_sprites_xf_device": ([vp, ctypes.c_int, ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(Atlas), vp,
                                      ctypes.c_int, vp, vp], ctypes.c_int),
        "rc2dgi_gradients_device": ([vp, ctypes.c_int, ctypes.POINTER(ctypes.c_ubyte), vp, ctypes.c_int, vp, vp],
                                    ctypes.c_int),
        "rc2dgi_tilemap_device": ([vp, ctypes.c_int, ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(Atlas),
                                   ctypes.POINTER(Tilemap), vp], ctypes.c_int),
    }
    for name, (args, res) in sig.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    _lib = L
    return L


def _fp(a: Optional[np.ndarray]):
    if a is None:
        return None
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


class RC2DGI:
    """One GI context = the reference's render-texture set + DoRC2DGI() on one GPU."""

    def __init__(self, screen_width: int = 1200, screen_height: int = 900, cascade_count: int = 6,
                 render_scale: float = 1.0, ray_range: float = 2.0, device: int = 0, storage: str = "f32",
                 linux_merge_fallback: bool = False):
        """storage: "f32" (RGBA32F render textures), "f16" (giRT1/2 as RGBA16F, RC2DGI.cs:105-106) or
        "rgba8" (every render texture RGBA8 with GL unorm8 arithmetic -- the literal app).
        linux_merge_fallback: the app on a case-sensitive filesystem, where "shaders/Merge.fs" is not
        found (RC2DGI.cs:62) and the merge pass adds no GI to colorRT."""
        self._L = load_library()
        st = {"f32": 0, "rgba8": 1, "f16": 2}[storage]
        cfg = _Config(screen_width, screen_height, cascade_count, render_scale, ray_range, st, device,
                      1 if linux_merge_fallback else 0, (ctypes.c_int * 4)())
        h = ctypes.c_void_p()
        rc = self._L.rc2dgi_create(ctypes.byref(cfg), ctypes.byref(h))
        if rc != 0:
            raise RC2DGIError(rc, f"rc2dgi_create({screen_width}x{screen_height}, N={cascade_count}) failed")
        self._h = h
        self.screen_width, self.screen_height = screen_width, screen_height
        self.render_scale = render_scale
        self.device = device
        self.storage = storage
        self._N = cascade_count

    # ---------------------------------------------------------------- lifetime
    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.rc2dgi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int, what: str) -> None:
        if rc != 0:
            msg = self._L.rc2dgi_last_error(self._h)
            raise RC2DGIError(rc, f"{what}: {msg.decode() if msg else ''}")

    # ---------------------------------------------------------------- sizes
    def query(self):
        cw, ch, s, f = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self._check(self._L.rc2dgi_query(self._h, ctypes.byref(cw), ctypes.byref(ch), ctypes.byref(s),
                                         ctypes.byref(f)), "query")
        return cw.value, ch.value, s.value, f.value

    @property
    def cascade_resolution(self):
        """(CW, CH), RC2DGI.cs:70-77"""
        return self.query()[:2]

    @property
    def jfa_steps(self) -> int:
        return self.query()[2]

    @property
    def final_gi(self) -> int:
        """1 or 2: which giRT holds the final GI (RC2DGI.cs:365)."""
        return self.query()[3]

    # ---------------------------------------------------------------- uniforms
    def set_shader_value(self, name: str, value) -> None:
        """SetShaderValue(GI/blur shader, GetShaderLocation(name), value) for the host-set uniforms."""
        v = np.atleast_1d(np.asarray(value, dtype=np.float32)).ravel().copy()
        self._check(self._L.rc2dgi_set_uniform(self._h, name.encode(), _fp(v), v.size), f"set {name}")

    def get_shader_value(self, name: str):
        n = 3 if name in ("_SkyColor", "_SunColor") else 1
        v = np.zeros(n, np.float32)
        self._check(self._L.rc2dgi_get_uniform(self._h, name.encode(), _fp(v), n), f"get {name}")
        return tuple(float(x) for x in v) if n == 3 else float(v[0])

    @property
    def cascade_count(self) -> int:
        """cascadeCount (RC2DGI.cs:66); setting it reallocates the cascade textures."""
        return self._N

    @cascade_count.setter
    def cascade_count(self, n: int) -> None:
        self._check(self._L.rc2dgi_set_uniform_i(self._h, b"_CascadeCount", int(n)), "set _CascadeCount")
        self._N = int(n)

    ray_range = property(lambda s: s.get_shader_value("_RayRange"),
                         lambda s, v: s.set_shader_value("_RayRange", v))
    sky_radiance = property(lambda s: s.get_shader_value("_SkyRadiance"),
                            lambda s, v: s.set_shader_value("_SkyRadiance", v))
    sky_color = property(lambda s: s.get_shader_value("_SkyColor"),
                         lambda s, v: s.set_shader_value("_SkyColor", v))
    sun_color = property(lambda s: s.get_shader_value("_SunColor"),
                         lambda s, v: s.set_shader_value("_SunColor", v))
    sun_angle = property(lambda s: s.get_shader_value("_SunAngle"),
                         lambda s, v: s.set_shader_value("_SunAngle", v))
    reflectivity = property(lambda s: s.get_shader_value("_Reflectivity"),
                            lambda s, v: s.set_shader_value("_Reflectivity", v))
    cascade_blur_radius = property(lambda s: s.get_shader_value("_BlurRadius"),
                                   lambda s, v: s.set_shader_value("_BlurRadius", v))

    # ---------------------------------------------------------------- tables (parity pinning)
    def set_direction_table(self, level: int, cos_sin: Optional[np.ndarray]) -> None:
        a = None if cos_sin is None else np.ascontiguousarray(cos_sin, np.float32).reshape(-1, 2)
        n = 0 if a is None else a.shape[0]
        self._check(self._L.rc2dgi_set_direction_table(self._h, level, _fp(a), n), "set direction table")

    def set_sky_table(self, rgb: Optional[np.ndarray]) -> None:
        a = None if rgb is None else np.ascontiguousarray(rgb, np.float32).reshape(-1, 3)
        n = 0 if a is None else a.shape[0]
        self._check(self._L.rc2dgi_set_sky_table(self._h, _fp(a), n), "set sky table")

    # ---------------------------------------------------------------- I/O
    def upload(self, which: str, img) -> None:
        """Painted colorRT / emissiveRT (H, W, 4) in GL row order: numpy float32/uint8 (host) or a
        torch tensor on this context's GPU (device-resident, enqueued on the context stream)."""
        w = RT[which]
        if hasattr(img, "data_ptr") and getattr(img, "is_cuda", False):
            t = img
            if tuple(t.shape) != (self.screen_height, self.screen_width, 4):
                raise ValueError(f"expected ({self.screen_height}, {self.screen_width}, 4), got {tuple(t.shape)}")
            if not t.is_contiguous():
                raise ValueError("device tensor must be contiguous")
            fmt = FMT_RGBA32F if str(t.dtype) == "torch.float32" else FMT_RGBA8
            if fmt == FMT_RGBA8 and str(t.dtype) != "torch.uint8":
                raise TypeError("device tensor must be float32 or uint8")
            pitch = self.screen_width * (16 if fmt == FMT_RGBA32F else 4)
            self._check(self._L.rc2dgi_upload_device(self._h, w, ctypes.c_void_p(t.data_ptr()), pitch, fmt),
                        f"upload_device {which}")
            return
        a = np.asarray(img)
        if a.shape != (self.screen_height, self.screen_width, 4):
            raise ValueError(f"expected ({self.screen_height}, {self.screen_width}, 4), got {a.shape}")
        if a.dtype == np.uint8:
            a = np.ascontiguousarray(a)
            fmt, pitch = FMT_RGBA8, self.screen_width * 4
        else:
            a = np.ascontiguousarray(a, np.float32)
            fmt, pitch = FMT_RGBA32F, self.screen_width * 16
        self._check(self._L.rc2dgi_upload(self._h, w, a.ctypes.data_as(ctypes.c_void_p), pitch, fmt),
                    f"upload {which}")

    def paint(self, which: str, prims, clear=None) -> None:
        """BeginTextureMode(colorRT | emissiveRT); ClearBackground(clear); raylib rectangles /
        circles (RenderScene / RedrawSceneToRTs, RC2DGI.cs:224-264, 528-545) -- on the GPU.
        prims: (kind, x, y, w_or_radius, h, r, g, b, a) in raylib screen coordinates."""
        arr = (Prim * max(len(prims), 1))()
        for k, p in enumerate(prims):
            arr[k] = Prim(int(p[0]), float(p[1]), float(p[2]), float(p[3]), float(p[4]),
                          *(int(v) for v in p[5:9]))
        cl = None if clear is None else (ctypes.c_ubyte * 4)(*[int(v) for v in clear])
        self._check(self._L.rc2dgi_paint(self._h, RT[which], cl, arr, len(prims)), f"paint {which}")

    def _dev_i32(self, call, t, what, numel=None):
        """the address of a contiguous int32 tensor on this context's GPU (a list, a count or a status of `call`)"""
        if not getattr(t, "is_cuda", False) or t.device.index != self.device:
            raise TypeError(f"{call}: {what}: expected a tensor on this context's GPU")
        if str(t.dtype) != "torch.int32" or not t.is_contiguous():
            raise TypeError(f"{call}: {what}: expected a contiguous int32 tensor")
        if numel is not None and t.numel() != numel:
            raise ValueError(f"{call}: {what}: expected {numel} element(s), got {t.numel()}")
        return ctypes.c_void_p(t.data_ptr())

    def paint_device(self, which, prims, clear=None, count=None, status=None) -> None:
        """The same painting from a primitive list in device memory, enqueued on the context stream
        (rc2dgi_paint_device): nothing waits.  prims: a contiguous torch.int32 (n, 6) tensor on this context's GPU, a row
        the six words of rc2dgi_prim (pack_prims makes one); count: None or an int32 tensor of one element, read on
        the stream when the work runs -- min(max(count, 0), n) primitives are painted; status: None or an int32 tensor
        of two elements that receives {painted, refused}.  A primitive paint() would raise on draws nothing and is
        counted in `refused`.  Keep the tensors alive until sync(); they may be overwritten on the same stream as soon
        as the call has returned."""
        self._paint_list("paint_device", self._L.rc2dgi_paint_device, 6, "prims", which, prims, clear, count, status)

    def shapes_device(self, which, shapes, clear=None, count=None, status=None) -> None:
        """Rectangles, circles, triangles, thick lines and ellipses from a list in device memory, mixed and painted
        in list order (rc2dgi_shapes_device): nothing waits.  shapes: a contiguous torch.int32 (n, 8) tensor on this
        context's GPU, a row the eight words of rc2dgi_shape (pack_shapes makes one, shapes_from_prims turns a
        paint_device list into one); clear, count and status as for paint_device.  A shape the header's rule refuses
        draws nothing and is counted in status[1].  Keep the tensors alive until sync()."""
        self._paint_list("shapes_device", self._L.rc2dgi_shapes_device, 8, "shapes", which, shapes, clear, count, status)

    def gradients_device(self, which, grads, clear=None, count=None, status=None) -> None:
        """The five shapes with a colour a vertex and an HDR gain, from a list in device memory, painted in list order
        (rc2dgi_gradients_device): nothing waits.  grads: a contiguous torch.int32 (n, 12) tensor on this context's
        GPU, a row the twelve words of rc2dgi_gradient (pack_gradients makes one, soft_lights makes round lights that
        fade to nothing at the rim, gradients_from_shapes turns a shapes_device list into one); clear, count and status
        as for paint_device.  A record the header's rule refuses draws nothing and is counted in status[1].  Keep the
        tensors alive until sync()."""
        self._paint_list("gradients_device", self._L.rc2dgi_gradients_device, 12, "grads", which, grads, clear, count,
                         status)

    def _paint_list(self, call, fn, words, what, which, recs, clear, count, status) -> None:
        w = RT[which] if isinstance(which, str) else int(which)
        dev_i32 = lambda t, what, numel=None: self._dev_i32(call, t, what, numel)  # noqa: E731
        p = dev_i32(recs, what)
        if recs.dim() != 2 or recs.shape[1] != words:
            raise ValueError(f"{call}: expected (n, {words}) words, got {tuple(recs.shape)}")
        n = int(recs.shape[0])
        cl = None if clear is None else (ctypes.c_ubyte * 4)(*[int(v) for v in clear])
        self._check(fn(self._h, w, cl, p if n else None, n, None if count is None else dev_i32(count, "count", 1),
                       None if status is None else dev_i32(status, "status", 2)), f"{call} {which}")

    def sprites_device(self, which, atlas, sprites, clear=None, count=None, status=None) -> None:
        """A sprite list in device memory drawn from one atlas image, enqueued on the context stream
        (rc2dgi_sprites_device): nothing waits.  atlas: a (AH, AW, 4) uint8, float16 or float32 tensor on this
        context's GPU with contiguous pixels, row 0 the top row (its row stride is the pitch, so a view of a larger
        tensor is accepted); sprites: a contiguous torch.int32 (n, 8) tensor, a row the eight words of rc2dgi_sprite
        (pack_sprites makes one); clear, count and status as for paint_device.  Each sprite is drawn 1:1 at its integer
        position, tinted, and blended over the texels (SPRITE_REPLACE: replaces them) with write()'s values; a sprite
        the header's rule refuses draws nothing and is counted in status[1].  Keep the tensors alive until sync()."""
        self._sprite_list("sprites_device", self._L.rc2dgi_sprites_device, 8, which, atlas, sprites, clear, count, status)

    def sprites_xf_device(self, which, atlas, sprites, clear=None, count=None, status=None) -> None:
        """The same list with every sprite scaled, rotated, sheared or mirrored (rc2dgi_sprites_xf_device): nothing
        waits.  atlas, clear, count and status as for sprites_device; sprites: a contiguous torch.int32 (n, 12) tensor,
        a row the twelve words of rc2dgi_sprite_xf (pack_sprites_xf makes one; sprites_xf_from_pro gives its P, A, B
        from DrawTexturePro's arguments).  Each source rectangle is mapped onto its parallelogram with POINT or, with
        SPRITE_LINEAR, four-tap sampling inside the rectangle, tinted, and blended over the texels (SPRITE_REPLACE:
        replaces them); a sprite the header's rule refuses draws nothing and is counted in status[1]."""
        self._sprite_list("sprites_xf_device", self._L.rc2dgi_sprites_xf_device, 12, which, atlas, sprites, clear, count,
                          status)

    def _atlas(self, call, atlas):
        """the rc2dgi_atlas of an (AH, AW, 4) tensor on this context's GPU (the sprite calls and tilemap_device)"""
        if not getattr(atlas, "is_cuda", False) or atlas.device.index != self.device:
            raise TypeError(f"{call}: atlas: expected a tensor on this context's GPU")
        fmt = _READ_FORMATS.get(str(atlas.dtype).replace("torch.", ""))
        if fmt is None:
            raise TypeError(f"{call}: atlas: expected a float32, float16 or uint8 tensor")
        if atlas.dim() != 3 or atlas.shape[2] != 4 or atlas.stride(2) != 1 or atlas.stride(1) != 4:
            raise ValueError(f"{call}: atlas: expected (AH, AW, 4) with contiguous pixels, got {tuple(atlas.shape)}")
        ah, aw = int(atlas.shape[0]), int(atlas.shape[1])
        return Atlas(atlas.data_ptr(), aw, ah, int(atlas.stride(0)) * atlas.element_size() if ah > 1 else 0, fmt)

    def _sprite_list(self, call, fn, words, which, atlas, sprites, clear, count, status) -> None:
        w = RT[which] if isinstance(which, str) else int(which)
        dev_i32 = lambda t, what, numel=None: self._dev_i32(call, t, what, numel)  # noqa: E731
        a = self._atlas(call, atlas)
        p = dev_i32(sprites, "sprites")
        if sprites.dim() != 2 or sprites.shape[1] != words:
            raise ValueError(f"{call}: expected (n, {words}) words, got {tuple(sprites.shape)}")
        n = int(sprites.shape[0])
        cl = None if clear is None else (ctypes.c_ubyte * 4)(*[int(v) for v in clear])
        self._check(fn(self._h, w, cl, ctypes.byref(a), p if n else None, n,
                       None if count is None else dev_i32(count, "count", 1),
                       None if status is None else dev_i32(status, "status", 2)), f"{call} {which}")

    def tilemap_device(self, which, atlas, cells, tile, origin=(0, 0), set_cols=None, margin=0, spacing=0, tint=None,
                       replace=False, clear=None, status=None) -> None:
        """A tile map drawn as one layer, enqueued on the context stream (rc2dgi_tilemap_device): nothing waits.
        atlas: the tile set, as for sprites_device; cells: a (rows, cols) torch.int32 tensor on this context's GPU with
        stride(1) == 1, row 0 the top row (its row stride is the pitch, so a window of a larger world tensor is
        accepted), a word Tiled's global tile id: 0 an empty cell, bit 31 / 30 (TILE_FLIP_X / TILE_FLIP_Y) the flips;
        tile: (tile_w, tile_h); origin: where the top-left pixel of cell (0, 0) goes (the scroll); set_cols: tiles per
        row of the set, None: Tiled's (AW - 2 * margin + spacing) // (tile_w + spacing); tint: (r, g, b, a) of the
        whole layer, None: white; replace: SPRITE_REPLACE; clear as for paint_device; status: None or an int32 tensor of
        two elements that receives {drawn, refused} over the visible cells.  A cell the header's rule refuses draws
        nothing.  Layers that need a tint a cell go through tilemap_sprites and sprites_device.  Keep the tensors alive
        until sync()."""
        call = "tilemap_device"
        w = RT[which] if isinstance(which, str) else int(which)
        a = self._atlas(call, atlas)
        if not getattr(cells, "is_cuda", False) or cells.device.index != self.device:
            raise TypeError(f"{call}: cells: expected a tensor on this context's GPU")
        if str(cells.dtype) != "torch.int32":
            raise TypeError(f"{call}: cells: expected an int32 tensor")
        if cells.dim() != 2 or (cells.shape[1] > 1 and cells.stride(1) != 1):
            raise ValueError(f"{call}: cells: expected (rows, cols) with contiguous rows, got {tuple(cells.shape)}")
        rows, cols = int(cells.shape[0]), int(cells.shape[1])
        if rows > 1 and cells.stride(0) < cols:
            raise ValueError(f"{call}: cells: the row stride {cells.stride(0)} is smaller than a row of {cols} cells")
        tw, th = (int(v) for v in tile)
        if set_cols is None:
            set_cols = tilemap_set_cols(a.w, tw, margin, spacing)
        r, g, b, al = (255, 255, 255, 255) if tint is None else (int(v) for v in tint)
        m = Tilemap(cells.data_ptr() if rows * cols else None, cols, rows, int(cells.stride(0)) if rows > 1 else 0, tw,
                    th, int(origin[0]), int(origin[1]), int(set_cols), int(margin), int(spacing), r, g, b, al,
                    SPRITE_REPLACE if replace else 0)
        cl = None if clear is None else (ctypes.c_ubyte * 4)(*[int(v) for v in clear])
        self._check(self._L.rc2dgi_tilemap_device(self._h, w, cl, ctypes.byref(a), ctypes.byref(m),
                                                  None if status is None else self._dev_i32(call, status, "status", 2)),
                    f"{call} {which}")

    def download(self, which: str, dtype=np.float32) -> np.ndarray:
        w = RT[which]
        cw, ch, _, fin = self.query()
        if which in SCREEN_RTS:
            shape = (self.screen_height, self.screen_width, 4)
        else:
            shape = (ch, cw, 4)
        fmt = FMT_RGBA8 if dtype == np.uint8 else FMT_RGBA32F
        out = np.empty(shape, np.uint8 if fmt == FMT_RGBA8 else np.float32)
        self._check(self._L.rc2dgi_download(self._h, w, out.ctypes.data_as(ctypes.c_void_p),
                                            shape[1] * (4 if fmt == FMT_RGBA8 else 16), fmt), f"download {which}")
        return out

    # ---------------------------------------------------------------- the display frame, composed on the GPU
    def _compose_args(self, views, size, clear):
        w, h = (self.screen_width, self.screen_height) if size is None else (int(size[0]), int(size[1]))
        cl = None if clear is None else (ctypes.c_ubyte * 4)(*[int(v) for v in clear])
        return _view_array(views), len(views), w, h, cl

    def set_curve(self, slot: int, edges) -> None:
        """The tone curve of slot 1 .. MAX_CURVES (rc2dgi_set_curve): 255 ascending float32 edges, a view toned with it
        shows byte bin(c * exposure) = the number of edges <= the value (curve_q8 / curve_from make such tables).
        Ordered on the context stream: a compose enqueued before keeps the old curve.  None clears the slot."""
        if edges is None:
            self._check(self._L.rc2dgi_set_curve(self._h, int(slot), None), "set_curve")
            return
        e, p = _edge_array(edges)
        if e.size != CURVE_EDGES:
            raise ValueError(f"set_curve: expected {CURVE_EDGES} edges, got {e.size}")
        self._check(self._L.rc2dgi_set_curve(self._h, int(slot), p), "set_curve")

    def compose(self, views, size=None, clear=None, tones=None) -> np.ndarray:
        """The window (RC2DGI.cs:135-165) as one RGBA8 image uint8[h, w, 4], row 0 = top: `clear` (default
        opaque black), then the views in order (View, or tuples for View.make), blended in 8 bits
        (rc2dgi_compose).  size: (w, h), default the screen.  Synchronous.
        tones: one Tone, (exposure, curve) pair or exposure a view (rc2dgi_compose_tone); None: untoned."""
        arr, n, w, h, cl = self._compose_args(views, size, clear)
        out = np.empty((max(h, 0), max(w, 0), 4), np.uint8)
        dst = out.ctypes.data_as(ctypes.c_void_p)
        if tones is None:
            self._check(self._L.rc2dgi_compose(self._h, arr, n, w, h, cl, dst, w * 4), "compose")
        else:
            self._check(self._L.rc2dgi_compose_tone(self._h, arr, _tone_array(tones, n), n, w, h, cl, dst, w * 4),
                        "compose")
        return out

    def compose_into(self, dst, views, size=None, clear=None, pitch=None, tones=None) -> None:
        """The same image into device memory, enqueued on the context stream (rc2dgi_compose_device; sync()
        or order the stream before reading).  dst: a torch uint8 tensor [h, w, 4] on this context's GPU --
        its rows may be padded, the pitch is the tensor's row stride -- or a device pointer (int) with
        size = (w, h) and pitch in bytes (default w * 4).  Bytes of a row past w * 4 are not written."""
        if hasattr(dst, "data_ptr"):
            t = dst
            if not getattr(t, "is_cuda", False) or str(t.dtype) != "torch.uint8":
                raise TypeError("compose_into: expected a uint8 tensor on the GPU")
            if t.dim() != 3 or t.shape[2] != 4 or t.stride(2) != 1 or t.stride(1) != 4:
                raise ValueError("compose_into: expected shape [h, w, 4] with contiguous pixels")
            if size is None:
                size = (int(t.shape[1]), int(t.shape[0]))
            elif (int(size[0]), int(size[1])) != (int(t.shape[1]), int(t.shape[0])):
                raise ValueError(f"compose_into: size {tuple(size)} does not match the tensor {tuple(t.shape)}")
            ptr, pitch = t.data_ptr(), int(t.stride(0))
        else:
            ptr = int(dst)
        arr, n, w, h, cl = self._compose_args(views, size, clear)
        if tones is None:
            self._check(self._L.rc2dgi_compose_device(self._h, arr, n, w, h, cl, ctypes.c_void_p(ptr),
                                                      int(pitch) if pitch else 0), "compose_into")
        else:  # (as compose: one tone a view)
            self._check(self._L.rc2dgi_compose_tone_device(self._h, arr, _tone_array(tones, n), n, w, h, cl,
                                                           ctypes.c_void_p(ptr), int(pitch) if pitch else 0),
                        "compose_into")

    def display_frame(self, thumbnails: bool = True) -> np.ndarray:
        """The reference's display: colorRT over the window and, with `thumbnails`, its seven debug views."""
        views = display_layout(self.screen_width, self.screen_height)
        return self.compose(views if thumbnails else views[:1])

    # ---------------------------------------------------------------- queries: a few values, no texture download
    def _on_device(self, t, what):
        if not getattr(t, "is_cuda", False) or t.device.index != self.device:
            raise TypeError(f"{what}: expected a tensor on this context's GPU")
        if str(t.dtype) != "torch.float32" or not t.is_contiguous():
            raise TypeError(f"{what}: expected a contiguous float32 tensor")

    def sample(self, which, uv, filter=FILTER_RT):
        """texture(T, (u, v)) for n points (rc2dgi_sample): which -- a name of RT or an rc2dgi_rt id; uv (n, 2)
        float32 in GL texture coordinates (v up; the centre of y-down pixel (x, y) is ((x + .5) / W,
        1 - (y + .5) / H)).  A numpy array returns numpy (n, 4) float32, synchronously.  A contiguous torch tensor on
        this context's GPU enqueues the kernel on the context stream (rc2dgi_sample_device) and returns a new (n, 4)
        tensor there: order the stream or sync() before reading, as with compose_into."""
        w = RT[which] if isinstance(which, str) else int(which)
        if hasattr(uv, "data_ptr"):
            import torch

            self._on_device(uv, "sample")
            if uv.dim() != 2 or uv.shape[1] != 2:
                raise ValueError(f"sample: expected (n, 2) points, got {tuple(uv.shape)}")
            out = torch.empty((uv.shape[0], 4), dtype=torch.float32, device=uv.device)
            self._check(self._L.rc2dgi_sample_device(self._h, w, int(filter), ctypes.c_void_p(uv.data_ptr()),
                                                     int(uv.shape[0]), ctypes.c_void_p(out.data_ptr())), "sample")
            return out
        a = np.ascontiguousarray(uv, np.float32)
        if a.ndim != 2 or a.shape[1] != 2:
            raise ValueError(f"sample: expected (n, 2) points, got {a.shape}")
        out = np.empty((a.shape[0], 4), np.float32)
        self._check(self._L.rc2dgi_sample(self._h, w, int(filter), a.ctypes.data_as(ctypes.c_void_p), a.shape[0],
                                          out.ctypes.data_as(ctypes.c_void_p)), "sample")
        return out

    def raycast(self, rays):
        """SampleRadianceSDF (RadianceCascades.fs:60-92) for n rays over the last frame (rc2dgi_raycast): rays
        (n, 6) float32 (ox, oy, dx, dy, t0, t1) or a structured array of RAY_DTYPE.  numpy in: a structured array of
        HIT_DTYPE out (status, steps, ix, iy, t, u, v, r, g, b, a), synchronously.  A contiguous (n, 6) torch tensor
        on this context's GPU enqueues the kernel on the context stream (rc2dgi_raycast_device) and returns a new
        int32 (n, 11) tensor there, the records' words; hit_floats(hits) views its float fields."""
        if hasattr(rays, "data_ptr"):
            import torch

            self._on_device(rays, "raycast")
            if rays.dim() != 2 or rays.shape[1] != 6:
                raise ValueError(f"raycast: expected (n, 6) rays, got {tuple(rays.shape)}")
            out = torch.empty((rays.shape[0], 11), dtype=torch.int32, device=rays.device)
            self._check(self._L.rc2dgi_raycast_device(self._h, ctypes.c_void_p(rays.data_ptr()), int(rays.shape[0]),
                                                      ctypes.c_void_p(out.data_ptr())), "raycast")
            return out
        a = np.asarray(rays)
        if a.dtype == RAY_DTYPE:
            a = np.ascontiguousarray(a).reshape(-1)
        else:
            a = np.ascontiguousarray(a, np.float32)
            if a.ndim != 2 or a.shape[1] != 6:
                raise ValueError(f"raycast: expected (n, 6) rays, got {a.shape}")
        out = np.empty(a.shape[0], HIT_DTYPE)
        self._check(self._L.rc2dgi_raycast(self._h, a.ctypes.data_as(ctypes.c_void_p), a.shape[0],
                                           out.ctypes.data_as(ctypes.c_void_p)), "raycast")
        return out

    # ---------------------------------------------------------------- region statistics
    def texture_size(self, which):
        """(width, height) of a render texture: the screen, or the cascade resolution for GI1 / GI2 / BLUR / FINAL_GI."""
        w = RT[which] if isinstance(which, str) else int(which)
        if w in (RT["gi1"], RT["gi2"], RT["blur"], RT["final_gi"]):
            return self.query()[:2]
        return self.screen_width, self.screen_height

    def reduce(self, which, rects=None):
        """Per rectangle and channel the count of non-finite values, min and max of the finite ones and their float64
        sum in the header's fixed order (rc2dgi_reduce): which -- a name of RT or an rc2dgi_rt id; rects -- an (n, 4)
        int array (x, y, w, h) in texels of that texture, GL order (row 0 = the bottom), or a RECT_DTYPE array; None:
        the whole texture.  Returns a structured STATS_DTYPE array of n records, synchronously; a rectangle that does
        not lie inside the texture has status STATS_INVALID and zeros."""
        w = RT[which] if isinstance(which, str) else int(which)
        if rects is None:
            tw, th = self.texture_size(w)
            rects = [[0, 0, tw, th]]
        a = _rect_array(rects)
        out = np.zeros(a.shape[0], STATS_DTYPE)
        self._check(self._L.rc2dgi_reduce(self._h, w, a.ctypes.data_as(ctypes.c_void_p), a.shape[0],
                                          out.ctypes.data_as(ctypes.c_void_p)), "reduce")
        return out

    def reduce_into(self, dst, which, rects) -> None:
        """The same records into device memory, enqueued on the context stream after whatever frame is in flight
        (rc2dgi_reduce_device; sync() or order the stream before reading, as with compose_into).  dst: a contiguous
        int32 (n, 22) torch tensor on this context's GPU, one rc2dgi_stats record of 88 bytes a row (stats_view reads
        its numpy copy); rects: host memory, as for reduce."""
        if not getattr(dst, "is_cuda", False) or dst.device.index != self.device:
            raise TypeError("reduce_into: expected a tensor on this context's GPU")
        if str(dst.dtype) != "torch.int32" or not dst.is_contiguous():
            raise TypeError("reduce_into: expected a contiguous int32 tensor")
        a = _rect_array(rects)
        if dst.dim() != 2 or dst.shape[1] != STATS_WORDS or dst.shape[0] != a.shape[0]:
            raise ValueError(f"reduce_into: expected shape ({a.shape[0]}, {STATS_WORDS}), got {tuple(dst.shape)}")
        w = RT[which] if isinstance(which, str) else int(which)
        self._check(self._L.rc2dgi_reduce_device(self._h, w, a.ctypes.data_as(ctypes.c_void_p), a.shape[0],
                                                 ctypes.c_void_p(dst.data_ptr())), "reduce_into")

    # ---------------------------------------------------------------- histograms of rectangles
    def _hist_args(self, which, edges, channel, rects):
        w = RT[which] if isinstance(which, str) else int(which)
        if rects is None:
            tw, th = self.texture_size(w)
            rects = [[0, 0, tw, th]]
        ch = CHANNELS[channel] if isinstance(channel, str) else int(channel)
        e, ep = _edge_array(edges)
        return w, ch, _rect_array(rects), e, ep

    def histogram(self, which, edges, channel="luma", rects=None):
        """Per rectangle the counts of its texels by bin of the ascending `edges` (rc2dgi_histogram): bin(s) = the number
        of edges <= s, s the texel's channel "r" / "g" / "b" / "a" or its "luma".  rects as for reduce; None: the whole
        texture.  Returns an (n, m + 4) uint32 array, a row {status, texels, nan, bin[0] .. bin[m]}, synchronously; an
        invalid rectangle has status 0xFFFFFFFF (STATS_INVALID) and zeros."""
        w, ch, a, e, ep = self._hist_args(which, edges, channel, rects)
        out = np.zeros((a.shape[0], e.size + 4), np.uint32)
        self._check(self._L.rc2dgi_histogram(self._h, w, ch, a.ctypes.data_as(ctypes.c_void_p), a.shape[0], ep, e.size,
                                             out.ctypes.data_as(ctypes.c_void_p)), "histogram")
        return out

    def histogram_into(self, dst, which, edges, channel="luma", rects=None) -> None:
        """The same records into device memory, enqueued on the context stream after whatever frame is in flight
        (rc2dgi_histogram_device; sync() or order the stream before reading).  dst: a contiguous int32 (n, m + 4) torch
        tensor on this context's GPU; every word of it is written.  rects and edges: host memory, as for histogram."""
        if not getattr(dst, "is_cuda", False) or dst.device.index != self.device:
            raise TypeError("histogram_into: expected a tensor on this context's GPU")
        if str(dst.dtype) != "torch.int32" or not dst.is_contiguous():
            raise TypeError("histogram_into: expected a contiguous int32 tensor")
        w, ch, a, e, ep = self._hist_args(which, edges, channel, rects)
        if dst.dim() != 2 or dst.shape[1] != e.size + 4 or dst.shape[0] != a.shape[0]:
            raise ValueError(f"histogram_into: expected shape ({a.shape[0]}, {e.size + 4}), got {tuple(dst.shape)}")
        self._check(self._L.rc2dgi_histogram_device(self._h, w, ch, a.ctypes.data_as(ctypes.c_void_p), a.shape[0], ep,
                                                    e.size, ctypes.c_void_p(dst.data_ptr())), "histogram_into")

    # ---------------------------------------------------------------- a rectangle as an image
    def _read_rect(self, which, rect):
        w = RT[which] if isinstance(which, str) else int(which)
        if rect is None:
            return w, None, self.texture_size(w)
        r = _rect_array([rect])
        return w, r, (int(r[0]["w"]), int(r[0]["h"]))

    def read(self, which, rect=None, dtype=np.float32, flip=False) -> np.ndarray:
        """A rectangle of a render texture as an (h, w, 4) image converted on the GPU (rc2dgi_read): which -- a name of
        RT or an rc2dgi_rt id; rect -- (x, y, w, h) in texels of that texture, GL order (row 0 = the bottom), None: the
        whole texture; dtype -- np.float32 (the values download returns), np.float16 (round to nearest even, as
        astype(np.float16)) or np.uint8 (q8, the bytes download returns); flip -- image row 0 is the rectangle's top
        row, the order compose writes.  Synchronous."""
        fmt = _READ_FORMATS.get(np.dtype(dtype).name)
        if fmt is None:
            raise TypeError("read: dtype is float32, float16 or uint8")
        w, r, (rw, rh) = self._read_rect(which, rect)
        tw, th = self.texture_size(w)
        if not (0 < rw <= tw and 0 < rh <= th):
            rw = rh = 1  # (the library refuses the rectangle: no image of its size is made first)
        out = np.empty((rh, rw, 4), dtype)
        self._check(self._L.rc2dgi_read(self._h, w, None if r is None else r.ctypes.data_as(ctypes.c_void_p), fmt,
                                        READ_FLIP if flip else 0, out.ctypes.data_as(ctypes.c_void_p), 0), "read")
        return out

    def read_into(self, dst, which, rect=None, flip=False) -> None:
        """The same image into device memory, enqueued on the context stream after whatever frame is in flight
        (rc2dgi_read_device; sync() or order the stream before reading, as with compose_into).  dst: a torch tensor
        (h, w, 4) on this context's GPU with contiguous pixels; its dtype float32 / float16 / uint8 selects the format,
        its row stride the pitch (rows may be padded; the padding is not written)."""
        if not getattr(dst, "is_cuda", False) or dst.device.index != self.device:
            raise TypeError("read_into: expected a tensor on this context's GPU")
        fmt = _READ_FORMATS.get(str(dst.dtype).replace("torch.", ""))
        if fmt is None:
            raise TypeError("read_into: expected a float32, float16 or uint8 tensor")
        w, r, (rw, rh) = self._read_rect(which, rect)
        if dst.dim() != 3 or tuple(dst.shape) != (rh, rw, 4) or dst.stride(2) != 1 or dst.stride(1) != 4:
            raise ValueError(f"read_into: expected shape ({rh}, {rw}, 4) with contiguous pixels, got {tuple(dst.shape)}")
        pitch = int(dst.stride(0)) * dst.element_size() if rh > 1 else 0
        self._check(self._L.rc2dgi_read_device(self._h, w, None if r is None else r.ctypes.data_as(ctypes.c_void_p), fmt,
                                               READ_FLIP if flip else 0, ctypes.c_void_p(dst.data_ptr()), pitch),
                    "read_into")

    # ---------------------------------------------------------------- an image into a rectangle of an input
    def write(self, which, img, rect=None, flip=False, blend=False) -> None:
        """An (h, w, 4) image into a rectangle of an input texture, converted on the GPU (rc2dgi_write /
        rc2dgi_write_device): which -- "color" or "emissive" (or the rc2dgi_rt id); rect -- (x, y, w, h) in texels, GL
        order (row 0 = the bottom), None: the whole texture; flip -- image row 0 is the rectangle's top row; blend --
        the image is blended over the texels (SRC_ALPHA, ONE_MINUS_SRC_ALPHA on all four channels) instead of replacing
        them.  The dtype float32 / float16 / uint8 selects the format; the texels become what upload would store.
        img: a numpy array (synchronous; its row stride is the pitch, any whole number of bytes) or a torch tensor on
        this context's GPU with contiguous pixels (enqueued on the context stream; its row stride is the pitch, so a
        view of a larger tensor is accepted as read_into accepts one; keep it alive until sync())."""
        w, r, (rw, rh) = self._read_rect(which, rect)
        flags = (WRITE_FLIP if flip else 0) | (WRITE_BLEND if blend else 0)
        rp = None if r is None else r.ctypes.data_as(ctypes.c_void_p)
        if hasattr(img, "data_ptr"):
            if not getattr(img, "is_cuda", False) or img.device.index != self.device:
                raise TypeError("write: expected a numpy array or a tensor on this context's GPU")
            fmt = _READ_FORMATS.get(str(img.dtype).replace("torch.", ""))
            if fmt is None:
                raise TypeError("write: expected a float32, float16 or uint8 tensor")
            if img.dim() != 3 or tuple(img.shape) != (rh, rw, 4) or img.stride(2) != 1 or img.stride(1) != 4:
                raise ValueError(f"write: expected shape ({rh}, {rw}, 4) with contiguous pixels, got {tuple(img.shape)}")
            pitch = int(img.stride(0)) * img.element_size() if rh > 1 else 0
            self._check(self._L.rc2dgi_write_device(self._h, w, rp, fmt, flags, ctypes.c_void_p(img.data_ptr()), pitch),
                        "write (device)")
            return
        a = np.asarray(img)
        fmt = _READ_FORMATS.get(a.dtype.name)
        if fmt is None:
            raise TypeError("write: dtype is float32, float16 or uint8")
        if a.shape != (rh, rw, 4):
            raise ValueError(f"write: expected shape ({rh}, {rw}, 4), got {a.shape}")
        px = 4 * a.itemsize
        if a.strides[2] != a.itemsize or a.strides[1] != px or (rh > 1 and a.strides[0] < rw * px):
            a = np.ascontiguousarray(a)  # (pixels apart, or rows that overlap or run backwards: a tight copy)
        pitch = int(a.strides[0]) if rh > 1 else 0
        self._check(self._L.rc2dgi_write(self._h, w, rp, fmt, flags, ctypes.c_void_p(a.ctypes.data), pitch), "write")

    def set_tuning(self, key: str, value: int) -> None:
        """Performance knobs (results are identical for every value), e.g. rc_variant."""
        self._check(self._L.rc2dgi_set_tuning(self._h, key.encode(), int(value)), f"set_tuning {key}")

    def get_tuning(self, key: str) -> int:
        v = ctypes.c_int()
        self._check(self._L.rc2dgi_get_tuning(self._h, key.encode(), ctypes.byref(v)), f"get_tuning {key}")
        return v.value

    def autotune(self, frames: int = 2) -> list:
        """Pick the fastest RC workgroup order per level on the uploaded scene (results are
        identical for every order); returns the chosen per-level codes."""
        self._check(self._L.rc2dgi_autotune(self._h, int(frames)), "autotune")
        return [self.get_tuning(f"rc_order_L{L}") for L in range(self._N)]

    def set_keep_levels(self, enable: bool = True) -> None:
        """Debug: keep every cascade level G_L as stored by its pass."""
        self._check(self._L.rc2dgi_set_keep_levels(self._h, int(bool(enable))), "set_keep_levels")

    def download_level(self, level: int) -> np.ndarray:
        cw, ch, _, _ = self.query()
        out = np.empty((ch, cw, 4), np.float32)
        self._check(self._L.rc2dgi_download_level(self._h, level, out.ctypes.data_as(ctypes.c_void_p), cw * 16,
                                                  FMT_RGBA32F), f"download_level {level}")
        return out

    TABLES = {"hitc": (0, np.uint8), "cmin": (1, np.uint8), "dclr": (2, np.uint8), "dboxes": (3, np.int32),
              "cellpal": (4, np.float32), "mfield": (5, np.uint16)}

    def download_table(self, name: str) -> np.ndarray:
        """The march's side tables of the last frame (rc2dgi_download_table): hitc / cmin (64, 64), dclr
        (64 bins, 64, 64), dboxes (64 bins, 64 steps, 4), cellpal (64, 64, 16, 4), mfield (H, pitch)."""
        which, dt = self.TABLES[name]
        n = self._L.rc2dgi_download_table(self._h, which, None, 0)
        self._check(n if n < 0 else 0, f"download_table {name}")
        out = np.empty(n // np.dtype(dt).itemsize, dt)
        self._check(min(0, self._L.rc2dgi_download_table(self._h, which, out.ctypes.data_as(ctypes.c_void_p), n)),
                    f"download_table {name}")
        shapes = {"hitc": (64, 64), "cmin": (64, 64), "dclr": (64, 64, 64), "dboxes": (64, 64, 4),
                  "cellpal": (64, 64, 16, 4), "mfield": (self.screen_height, -1)}
        return out.reshape(shapes[name])

    # ---------------------------------------------------------------- the pass chain
    def do_rc2dgi(self) -> None:
        """DoRC2DGI() (RC2DGI.cs:267-406): enqueue the whole pass chain on the context stream."""
        self._check(self._L.rc2dgi_do(self._h), "DoRC2DGI")

    do = do_rc2dgi

    def sync(self) -> None:
        self._check(self._L.rc2dgi_sync(self._h), "sync")

    def set_stream(self, hip_stream: Optional[int]) -> None:
        self._check(self._L.rc2dgi_set_stream(self._h, ctypes.c_void_p(hip_stream or 0)), "set_stream")

    def set_timing(self, enable=True) -> None:
        """True / 1: events around every pass and RC level; 2: around every pass only (no idle gaps
        between the levels); False / 0: off."""
        if isinstance(enable, bool):
            mode = int(enable)
        elif isinstance(enable, (int, np.integer)) and int(enable) in (0, 1, 2):
            mode = int(enable)
        else:
            raise ValueError(f"set_timing: expected a bool or 0, 1, 2, got {enable!r}")
        self._check(self._L.rc2dgi_set_timing(self._h, mode), "set_timing")

    def pass_times(self, levels: int = 0):
        """HIP-event milliseconds of the last frame: dict(screenuv, jfa, rc, blur, merge, total[, levels])."""
        p = np.zeros(len(PASS_NAMES), np.float32)
        lv = np.zeros(max(levels, 1), np.float32)
        self._check(self._L.rc2dgi_pass_times(self._h, _fp(p), p.size, _fp(lv) if levels else None, levels),
                    "pass_times")
        d = {k: float(v) for k, v in zip(PASS_NAMES, p)}
        if levels:
            d["levels"] = [float(x) for x in lv[:levels]]
        return d

    # ---------------------------------------------------------------- row-strip sharding
    def set_shard(self, rank: int, world: int) -> None:
        """Compute screen rows [rank*H/world, (rank+1)*H/world) of the merged colorRT (and what
        they depend on).  world = 1: the whole frame."""
        self._check(self._L.rc2dgi_set_shard(self._h, int(rank), int(world)), "set_shard")

    def shard_rows(self):
        y0, y1 = ctypes.c_int(), ctypes.c_int()
        self._check(self._L.rc2dgi_shard_rows(self._h, ctypes.byref(y0), ctypes.byref(y1)), "shard_rows")
        return y0.value, y1.value

    def connect(self, unique_id: bytes) -> None:
        """RCCL communicator over the shards (one process per GPU); then do_rc2dgi() runs the
        distRT exchange itself."""
        buf = ctypes.create_string_buffer(bytes(unique_id), UNIQUE_ID_BYTES)
        self._check(self._L.rc2dgi_shard_connect(self._h, buf, UNIQUE_ID_BYTES), "shard_connect")

    def do_phase(self, phase: int) -> None:
        """1: ScreenUV + JumpFlood + DistanceField; 2: cascades, blur, merge (exchange distRT between)."""
        self._check(self._L.rc2dgi_do_phase(self._h, int(phase)), f"do_phase {phase}")

    def device_buffer(self, which: str):
        """(device pointer, pitch in bytes) of a render texture's raw storage."""
        p, pitch = ctypes.c_void_p(), ctypes.c_int()
        self._check(self._L.rc2dgi_device_buffer(self._h, RT[which], ctypes.byref(p), ctypes.byref(pitch)),
                    f"device_buffer {which}")
        return p.value, pitch.value

    def frame(self, color, emissive) -> None:
        """Upload the painted scene and run one DoRC2DGI() (the reference's per-frame order,
        RC2DGI.cs:122-132)."""
        self.upload("color", color)
        self.upload("emissive", emissive)
        self.do_rc2dgi()


def abi_version() -> int:
    return load_library().rc2dgi_abi_version()


UNIQUE_ID_BYTES = 128
PLAN_JFA, PLAN_LEVEL, PLAN_BLUR, PLAN_MERGE = 0, 1000, 2000, 2001


def shard_unique_id() -> bytes:
    """RCCL unique id for rc2dgi_shard_connect (create on rank 0, send to the other ranks)."""
    L = load_library()
    buf = ctypes.create_string_buffer(UNIQUE_ID_BYTES)
    rc = L.rc2dgi_shard_unique_id(buf, UNIQUE_ID_BYTES)
    if rc != 0:
        raise RC2DGIError(rc, "rc2dgi_shard_unique_id")
    return buf.raw


def do_group(ctxs: Sequence["RC2DGI"]) -> None:
    """One sharded frame over in-process contexts (context k = shard k of len(ctxs))."""
    L = load_library()
    arr = (ctypes.c_void_p * len(ctxs))(*[c._h.value for c in ctxs])
    rc = L.rc2dgi_do_group(arr, len(ctxs))
    if rc != 0:
        msgs = [c._L.rc2dgi_last_error(c._h) for c in ctxs]
        raise RC2DGIError(rc, "rc2dgi_do_group: " + "; ".join(m.decode() for m in msgs if m))


def display_layout(W: int, H: int, max_views: int = 8):
    """Host-only: the reference's display for a W x H window (rc2dgi_display_layout) as a list of View --
    colorRT over the window, then the thumbnails color, emissive, jump2, dist, gi1, gi2, temp.  The layout
    depends on the window size alone."""
    L = load_library()
    cfg = _Config(screen_width=W, screen_height=H)  # (the only fields rc2dgi_display_layout reads)
    arr = (View * max(max_views, 1))()
    n = L.rc2dgi_display_layout(ctypes.byref(cfg), arr, max_views)
    if n < 0:
        raise RC2DGIError(n, "rc2dgi_display_layout")
    return [View.from_buffer_copy(arr[k]) for k in range(min(n, max_views))]


def pack_prims(kind, xywh, rgba):
    """The (n, 6) int32 tensor RC2DGI.paint_device takes, from device tensors with torch ops alone (nothing leaves the
    device, nothing waits): kind (n,) of any integer dtype (0 rectangle, 1 circle), xywh (n, 4) float32 (circle: x, y
    the centre, w the radius), rgba (n, 4) uint8.  The float bits are reinterpreted; the four colour bytes go little-
    endian into word 5, as rc2dgi_prim lays them out."""
    import torch

    n = int(kind.shape[0])
    if tuple(xywh.shape) != (n, 4) or xywh.dtype != torch.float32:
        raise ValueError(f"pack_prims: xywh is ({n}, 4) float32, got {tuple(xywh.shape)} {xywh.dtype}")
    if tuple(rgba.shape) != (n, 4) or rgba.dtype != torch.uint8:
        raise ValueError(f"pack_prims: rgba is ({n}, 4) uint8, got {tuple(rgba.shape)} {rgba.dtype}")
    return torch.cat([kind.reshape(n, 1).to(torch.int32), xywh.contiguous().view(torch.int32),
                      rgba.contiguous().view(torch.int32)], dim=1)


def pack_shapes(kind, v6, rgba):
    """The (n, 8) int32 tensor RC2DGI.shapes_device takes, with torch ops alone on the inputs' device (nothing waits):
    kind (n,) of any integer dtype (SHAPE_*), v6 (n, 6) float32 (the values the kind names; the rest are not read),
    rgba (n, 4) uint8.  The float bits are reinterpreted; the four colour bytes go little-endian into word 7, as
    rc2dgi_shape lays them out."""
    import torch

    n = int(kind.shape[0])
    if tuple(kind.shape) != (n,) or kind.dtype.is_floating_point or kind.dtype == torch.bool:
        raise ValueError(f"pack_shapes: kind is (n,) of an integer dtype, got {tuple(kind.shape)} {kind.dtype}")
    if tuple(v6.shape) != (n, 6) or v6.dtype != torch.float32:
        raise ValueError(f"pack_shapes: v6 is ({n}, 6) float32, got {tuple(v6.shape)} {v6.dtype}")
    if tuple(rgba.shape) != (n, 4) or rgba.dtype != torch.uint8:
        raise ValueError(f"pack_shapes: rgba is ({n}, 4) uint8, got {tuple(rgba.shape)} {rgba.dtype}")
    return torch.cat([kind.reshape(n, 1).to(torch.int32), v6.contiguous().view(torch.int32),
                      rgba.contiguous().view(torch.int32)], dim=1)


def shapes_from_prims(prims):
    """The (n, 8) shapes_device list that paints what the (n, 6) paint_device list `prims` paints: kind, x, y, w, h
    in words 0 .. 4, two zero words, the colour in word 7 (SHAPE_RECT == 0 and SHAPE_CIRCLE == 1 are rc2dgi_prim's
    kinds).  Torch ops alone on the input's device."""
    import torch

    if prims.dim() != 2 or prims.shape[1] != 6 or prims.dtype != torch.int32:
        raise ValueError(f"shapes_from_prims: prims is (n, 6) int32, got {tuple(prims.shape)} {prims.dtype}")
    return torch.cat([prims[:, :5], torch.zeros_like(prims[:, :2]), prims[:, 5:6]], dim=1).contiguous()


def pack_gradients(kind, v6, colors, gain=None):
    """The (n, 12) int32 tensor RC2DGI.gradients_device takes, with torch ops alone on the inputs' device (nothing
    waits): kind (n,) of any integer dtype (GRAD_*), v6 (n, 6) float32 (pack_shapes' v6), colors (n, 4, 4) uint8 (four
    r, g, b, a colours a record; those the kind does not name are not read), gain (n,) float32, None: 1.  The float
    bits are reinterpreted; colour k goes little-endian into word 7 + k, as rc2dgi_gradient lays them out."""
    import torch

    n = int(kind.shape[0])
    if tuple(kind.shape) != (n,) or kind.dtype.is_floating_point or kind.dtype == torch.bool:
        raise ValueError(f"pack_gradients: kind is (n,) of an integer dtype, got {tuple(kind.shape)} {kind.dtype}")
    if tuple(v6.shape) != (n, 6) or v6.dtype != torch.float32:
        raise ValueError(f"pack_gradients: v6 is ({n}, 6) float32, got {tuple(v6.shape)} {v6.dtype}")
    if tuple(colors.shape) != (n, 4, 4) or colors.dtype != torch.uint8:
        raise ValueError(f"pack_gradients: colors is ({n}, 4, 4) uint8, got {tuple(colors.shape)} {colors.dtype}")
    if gain is None:
        gain = torch.ones(n, dtype=torch.float32, device=v6.device)
    if tuple(gain.shape) != (n,) or gain.dtype != torch.float32:
        raise ValueError(f"pack_gradients: gain is ({n},) float32, got {tuple(gain.shape)} {gain.dtype}")
    return torch.cat([kind.reshape(n, 1).to(torch.int32), v6.contiguous().view(torch.int32),
                      colors.contiguous().view(torch.int32).reshape(n, 4),
                      gain.contiguous().view(torch.int32).reshape(n, 1)], dim=1)


def gradients_from_shapes(shapes):
    """The (n, 12) gradients_device list that paints what the (n, 8) shapes_device list `shapes` paints: words 0 .. 6
    as they are, the colour of word 7 in all four colour words, gain 1.0 (GRAD_* are SHAPE_*'s values).  Torch ops
    alone on the input's device."""
    import torch

    if shapes.dim() != 2 or shapes.shape[1] != 8 or shapes.dtype != torch.int32:
        raise ValueError(f"gradients_from_shapes: shapes is (n, 8) int32, got {tuple(shapes.shape)} {shapes.dtype}")
    one = torch.full_like(shapes[:, :1], 0x3F800000)  # the bits of 1.0f
    return torch.cat([shapes[:, :7], shapes[:, 7:8].expand(-1, 4), one], dim=1).contiguous()


def soft_lights(xy, radius, rgb, gain=None):
    """The (n, 12) gradients_device list of n round lights, bright at the centre and fading to nothing at the rim
    (raylib's DrawCircleGradient(centre, radius, (rgb, 255), (rgb, 0))): GRAD_CIRCLE records with c[0] = (rgb, 255) and
    c[1] = (rgb, 0).  xy (n, 2) float32 the centres, radius (n,) float32, rgb (n, 3) uint8, gain (n,) float32 (None: 1)
    the HDR factor on r, g, b.  Torch ops alone on the inputs' device: a particle system kept as tensors becomes lights
    without leaving it."""
    import torch

    if xy.dim() != 2 or xy.shape[1] != 2 or xy.dtype != torch.float32:
        raise ValueError(f"soft_lights: xy is (n, 2) float32, got {tuple(xy.shape)} {xy.dtype}")
    n = int(xy.shape[0])
    if tuple(radius.shape) != (n,) or radius.dtype != torch.float32:
        raise ValueError(f"soft_lights: radius is ({n},) float32, got {tuple(radius.shape)} {radius.dtype}")
    if tuple(rgb.shape) != (n, 3) or rgb.dtype != torch.uint8:
        raise ValueError(f"soft_lights: rgb is ({n}, 3) uint8, got {tuple(rgb.shape)} {rgb.dtype}")
    v6 = torch.cat([xy, radius.reshape(n, 1), torch.zeros((n, 3), dtype=torch.float32, device=xy.device)], dim=1)
    alpha = torch.tensor([255, 0, 0, 0], dtype=torch.uint8, device=xy.device).reshape(1, 4, 1).expand(n, 4, 1)
    colors = torch.cat([rgb.reshape(n, 1, 3).expand(n, 4, 3), alpha], dim=2)
    kind = torch.full((n,), GRAD_CIRCLE, dtype=torch.int32, device=xy.device)
    return pack_gradients(kind, v6, colors, gain)


def pack_sprites(src_xywh, dst_xy, tint=None, flags=None):
    """The (n, 8) int32 tensor RC2DGI.sprites_device takes, with torch ops alone on the inputs' device (nothing
    waits): src_xywh (n, 4) int32, the source rectangles of the atlas; dst_xy (n, 2) int32, where each top-left pixel
    goes (raylib screen coordinates); tint (n, 4) uint8, None: white; flags (n,) of any integer dtype (SPRITE_*), None:
    0.  The four tint bytes go little-endian into word 6, as rc2dgi_sprite lays them out."""
    import torch

    if src_xywh.dim() != 2 or src_xywh.shape[1] != 4 or src_xywh.dtype != torch.int32:
        raise ValueError(f"pack_sprites: src_xywh is (n, 4) int32, got {tuple(src_xywh.shape)} {src_xywh.dtype}")
    n = int(src_xywh.shape[0])
    if tuple(dst_xy.shape) != (n, 2) or dst_xy.dtype != torch.int32:
        raise ValueError(f"pack_sprites: dst_xy is ({n}, 2) int32, got {tuple(dst_xy.shape)} {dst_xy.dtype}")
    if tint is None:
        tint = torch.full((n, 4), 255, dtype=torch.uint8, device=src_xywh.device)
    if tuple(tint.shape) != (n, 4) or tint.dtype != torch.uint8:
        raise ValueError(f"pack_sprites: tint is ({n}, 4) uint8, got {tuple(tint.shape)} {tint.dtype}")
    if flags is None:
        flags = torch.zeros(n, dtype=torch.int32, device=src_xywh.device)
    if tuple(flags.shape) != (n,) or flags.dtype.is_floating_point or flags.dtype == torch.bool:
        raise ValueError(f"pack_sprites: flags is ({n},) of an integer dtype, got {tuple(flags.shape)} {flags.dtype}")
    return torch.cat([src_xywh, dst_xy, tint.contiguous().view(torch.int32), flags.reshape(n, 1).to(torch.int32)], dim=1)


def tilemap_set_cols(atlas_w: int, tile_w: int, margin: int = 0, spacing: int = 0) -> int:
    """Tiled's column count of a tile set image: (AW - 2 * margin + spacing) // (tile_w + spacing)"""
    return (int(atlas_w) - 2 * int(margin) + int(spacing)) // (int(tile_w) + int(spacing))


def tilemap_sprites(cells, tile, origin, atlas_size, screen_size, set_cols=None, margin=0, spacing=0, tint=None,
                    replace=False):
    """The (n, 8) int32 sprite list (pack_sprites' layout) of the cells RC2DGI.tilemap_device draws: the visible,
    non-empty, accepted cells of `cells` ((rows, cols) int32, on any device) in row-major order, with torch ops alone on
    that device.  tile = (tile_w, tile_h), origin = (ox, oy), atlas_size = (AW, AH), screen_size = (W, H); the other
    arguments as for tilemap_device.  sprites_device on the list leaves the bits tilemap_device leaves: the fallback for
    layers that need a tint a cell (overwrite column 6) or, through sprites_xf_device, a zoomed camera."""
    import torch

    if cells.dim() != 2 or cells.dtype != torch.int32:
        raise ValueError(f"tilemap_sprites: cells is (rows, cols) int32, got {tuple(cells.shape)} {cells.dtype}")
    (tw, th), (ox, oy), (AW, AH), (W, H) = ((int(v[0]), int(v[1])) for v in (tile, origin, atlas_size, screen_size))
    margin, spacing = int(margin), int(spacing)
    if tw < 1 or th < 1 or margin < 0 or spacing < 0 or margin + tw > AW or margin + th > AH:
        raise ValueError("tilemap_sprites: tile 0 does not fit the atlas")
    set_cols = tilemap_set_cols(AW, tw, margin, spacing) if set_cols is None else int(set_cols)
    if set_cols < 1:
        raise ValueError(f"tilemap_sprites: set_cols is at least 1, got {set_cols}")
    rows, cols = int(cells.shape[0]), int(cells.shape[1])
    # the visible cells: ox + c * tw + tw - 1 >= 0 and ox + c * tw <= W - 1 (floor divisions), and rows alike
    c0, c1 = max(-ox // tw, 0), min((W - 1 - ox) // tw, cols - 1)
    r0, r1 = max(-oy // th, 0), min((H - 1 - oy) // th, rows - 1)
    if c0 > c1 or r0 > r1:
        return torch.zeros((0, 8), dtype=torch.int32, device=cells.device)
    g = cells[r0:r1 + 1, c0:c1 + 1].to(torch.int64) & 0xFFFFFFFF
    t = (g & TILE_ID_MASK) - 1
    tx, ty = t % set_cols, t // set_cols
    ok = (g != 0) & ((g & TILE_UNSUPPORTED) == 0) & (t >= 0)
    ok &= (tx <= (AW - margin - tw) // (tw + spacing)) & (ty <= (AH - margin - th) // (th + spacing))
    r, c = torch.nonzero(ok, as_tuple=True)  # row-major
    g, tx, ty = g[r, c], tx[r, c], ty[r, c]
    n = int(r.numel())
    flags = ((g >> 31) & 1) * SPRITE_FLIP_X + ((g >> 30) & 1) * SPRITE_FLIP_Y + (SPRITE_REPLACE if replace else 0)
    rgba = (255, 255, 255, 255) if tint is None else tuple(int(v) & 255 for v in tint)
    word = rgba[0] | rgba[1] << 8 | rgba[2] << 16 | rgba[3] << 24
    word -= (1 << 32) if word >= (1 << 31) else 0
    out = torch.stack([margin + tx * (tw + spacing), margin + ty * (th + spacing), torch.full_like(tx, tw),
                       torch.full_like(tx, th), ox + (c + c0) * tw, oy + (r + r0) * th, torch.full_like(tx, word),
                       flags], dim=1)
    return out.to(torch.int32).reshape(n, 8)


def pack_sprites_xf(src_xywh, p_xy, a_xy, b_xy, tint=None, flags=None):
    """The (n, 12) int32 tensor RC2DGI.sprites_xf_device takes, with torch ops alone on the inputs' device (nothing
    waits): src_xywh (n, 4) int32, the source rectangles of the atlas; p_xy, a_xy, b_xy (n, 2) float32, where each
    rectangle's top-left corner lands and the images of its top and left edges (screen pixels, y down); tint (n, 4)
    uint8, None: white; flags (n,) of any integer dtype (SPRITE_REPLACE | SPRITE_LINEAR), None: 0.  The float bits are
    reinterpreted; the four tint bytes go little-endian into word 10, as rc2dgi_sprite_xf lays them out."""
    import torch

    if src_xywh.dim() != 2 or src_xywh.shape[1] != 4 or src_xywh.dtype != torch.int32:
        raise ValueError(f"pack_sprites_xf: src_xywh is (n, 4) int32, got {tuple(src_xywh.shape)} {src_xywh.dtype}")
    n = int(src_xywh.shape[0])
    for name, t in (("p_xy", p_xy), ("a_xy", a_xy), ("b_xy", b_xy)):
        if tuple(t.shape) != (n, 2) or t.dtype != torch.float32:
            raise ValueError(f"pack_sprites_xf: {name} is ({n}, 2) float32, got {tuple(t.shape)} {t.dtype}")
    if tint is None:
        tint = torch.full((n, 4), 255, dtype=torch.uint8, device=src_xywh.device)
    if tuple(tint.shape) != (n, 4) or tint.dtype != torch.uint8:
        raise ValueError(f"pack_sprites_xf: tint is ({n}, 4) uint8, got {tuple(tint.shape)} {tint.dtype}")
    if flags is None:
        flags = torch.zeros(n, dtype=torch.int32, device=src_xywh.device)
    if tuple(flags.shape) != (n,) or flags.dtype.is_floating_point or flags.dtype == torch.bool:
        raise ValueError(f"pack_sprites_xf: flags is ({n},) of an integer dtype, got {tuple(flags.shape)} {flags.dtype}")
    return torch.cat([src_xywh, p_xy.contiguous().view(torch.int32), a_xy.contiguous().view(torch.int32),
                      b_xy.contiguous().view(torch.int32), tint.contiguous().view(torch.int32),
                      flags.reshape(n, 1).to(torch.int32)], dim=1)


def sprites_xf_from_pro(dest_xywh, origin_xy, rotation_deg):
    """(p_xy, a_xy, b_xy) float32 tensors for pack_sprites_xf from DrawTexturePro's geometry, with torch ops alone:
    dest_xywh (n, 4) float32, origin_xy (n, 2) float32, rotation_deg (n,) float32 (clockwise on the y-down screen, as
    raylib turns).  With c, s the cosine and sine of the rotation and R = [[c, -s], [s, c]]:
    P = dest.xy + R (-origin), A = R (dest.w, 0), B = R (0, dest.h).  The trigonometry is torch's and no part of the
    exact contract: the device consumes the record as given."""
    import torch

    n = int(dest_xywh.shape[0])
    if tuple(dest_xywh.shape) != (n, 4) or dest_xywh.dtype != torch.float32:
        raise ValueError(f"sprites_xf_from_pro: dest_xywh is (n, 4) float32, got {tuple(dest_xywh.shape)} {dest_xywh.dtype}")
    if tuple(origin_xy.shape) != (n, 2) or origin_xy.dtype != torch.float32:
        raise ValueError(f"sprites_xf_from_pro: origin_xy is ({n}, 2) float32, got {tuple(origin_xy.shape)} {origin_xy.dtype}")
    if tuple(rotation_deg.shape) != (n,) or rotation_deg.dtype != torch.float32:
        raise ValueError(f"sprites_xf_from_pro: rotation_deg is ({n},) float32, got {tuple(rotation_deg.shape)} "
                         f"{rotation_deg.dtype}")
    rad = torch.deg2rad(rotation_deg)
    c, s = torch.cos(rad), torch.sin(rad)
    ox, oy = origin_xy[:, 0], origin_xy[:, 1]
    p = torch.stack([dest_xywh[:, 0] - (c * ox - s * oy), dest_xywh[:, 1] - (s * ox + c * oy)], dim=1)
    a = torch.stack([c * dest_xywh[:, 2], s * dest_xywh[:, 2]], dim=1)
    b = torch.stack([-s * dest_xywh[:, 3], c * dest_xywh[:, 3]], dim=1)
    return p, a, b


def paint_device_limits(W: int, H: int):
    """Host-only: (batch_prims, work_bytes) of RC2DGI.paint_device on a W x H screen (rc2dgi_paint_device_limits): how
    many primitives one batch holds and the working memory the context allocates at the first call."""
    L = load_library()
    cfg = _Config(screen_width=W, screen_height=H)  # (the only fields rc2dgi_paint_device_limits reads)
    batch, work = ctypes.c_int(), ctypes.c_longlong()
    rc = L.rc2dgi_paint_device_limits(ctypes.byref(cfg), ctypes.byref(batch), ctypes.byref(work))
    if rc != 0:
        raise RC2DGIError(rc, f"rc2dgi_paint_device_limits({W}x{H})")
    return batch.value, work.value


def check_edges(edges) -> bool:
    """Host-only: whether `edges` is a valid edge table (rc2dgi_check_edges): at least one float32, ascending (repeats,
    +-inf and -0.0 allowed), no NaN."""
    e, p = _edge_array(edges)
    return load_library().rc2dgi_check_edges(p if e.size else None, int(e.size)) == 0


def curve_q8() -> np.ndarray:
    """Host-only: the 255 edges whose bin() is q8(x) = rint(clamp(x, 0, 1) * 255) for every float (rc2dgi_curve_q8)."""
    e = np.empty(CURVE_EDGES, np.float32)
    rc = load_library().rc2dgi_curve_q8(_fp(e))
    if rc != 0:
        raise RC2DGIError(rc, "rc2dgi_curve_q8")
    return e


def curve_from(fn) -> np.ndarray:
    """Host-only: the 255 edges of the tone curve byte(x) = q8(fn(x)) for a monotone (non-decreasing) fn, evaluated in
    float64 on arrays: edge k - 1 is the smallest non-negative float32 x with rint(255 * fn(x)) >= k, found by
    bisection over float bit patterns (the bits of a non-negative float order as the float does); +inf where no finite
    x reaches k.  fn's float64 result is rounded to float32 and the product with 255 is the float32 one, as q8 forms
    it, so that the curve shows exactly the byte the untoned path would show for fn(x): curve_from(lambda x: x) is
    curve_q8()."""
    k = np.arange(1, CURVE_EDGES + 1, dtype=np.float64)
    top = 0x7F800000  # +inf: the answer when no finite float reaches k
    lo, hi = np.zeros(CURVE_EDGES, np.int64), np.full(CURVE_EDGES, top, np.int64)
    while (lo < hi).any():
        mid = (lo + hi) // 2
        x = mid.astype(np.uint32).view(np.float32).astype(np.float64)
        with np.errstate(all="ignore"):
            y = np.asarray(fn(np.where(np.isfinite(x), x, np.finfo(np.float32).max)), np.float64)
        y32 = np.clip(y, 0.0, 1.0).astype(np.float32)  # (a NaN of fn stays one and reaches no k)
        ok = (np.rint(y32 * np.float32(255.0)) >= k) | (mid >= top)
        hi = np.where(ok & (lo < hi), mid, hi)
        lo = np.where(~ok & (lo < hi), mid + 1, lo)
    return lo.astype(np.uint32).view(np.float32).copy()


def percentile(hist_record, edges, p: float) -> float:
    """The value below which the fraction p (0 .. 1) of a histogram's non-NaN texels lie, to the resolution of the
    edges: the edge at which the running count of the bins first reaches p of texels - nan.  hist_record: one row of
    RC2DGI.histogram.  Bin 0 lies below every edge (it returns edges[0]); the last bin has no upper edge (edges[-1]).
    NaN for a record without a counted texel."""
    rec = np.asarray(hist_record).reshape(-1).astype(np.int64)
    e = np.asarray(edges, np.float32).reshape(-1)
    if rec.size != e.size + 4:
        raise ValueError(f"percentile: a record of {e.size} edges has {e.size + 4} words, got {rec.size}")
    total = int(rec[1] - rec[2])
    if rec[0] != STATS_OK or total <= 0:
        return float("nan")
    run = np.cumsum(rec[HIST_HEAD:])
    b = int(np.searchsorted(run, max(p * total, 1e-300), side="left"))
    return float(e[min(b, e.size - 1)])


def plan_rows(W: int, H: int, N: int, blur_radius: float, rank: int, world: int, pass_id: int,
              render_scale: float = 1.0):
    """Host-only planner: [(begin, end), ...] rows shard `rank` of `world` computes for a pass
    (PLAN_JFA + step, PLAN_LEVEL + level, PLAN_BLUR, PLAN_MERGE)."""
    L = load_library()
    cfg = _Config(W, H, N, render_scale, 2.0, 0, 0, 0, (ctypes.c_int * 4)())
    buf = (ctypes.c_int * 64)()
    n = L.rc2dgi_plan_rows(ctypes.byref(cfg), float(blur_radius), rank, world, pass_id, buf, 32)
    if n < 0:
        raise RC2DGIError(n, "rc2dgi_plan_rows")
    if n > 32:
        buf = (ctypes.c_int * (2 * n))()
        n = L.rc2dgi_plan_rows(ctypes.byref(cfg), float(blur_radius), rank, world, pass_id, buf, n)
    return [(buf[2 * k], buf[2 * k + 1]) for k in range(n)]


JFA_INFO = ("m", "hmax", "mg_max", "halo", "sh_minus", "sh_zero", "sh_plus", "mg", "same_block")


def plan_jfa_exchange(W: int, H: int, N: int, world: int, step: int, render_scale: float = 1.0):
    """Host-only JumpFlood exchange plan of row-strip shards for JFA step `step` (>= 1): a dict of
    JFA_INFO and the transfers [(src, src_window_row, rows, dst, dst_buf, dst_row), ...] in the order
    every shard issues them (rc2dgi_plan_jfa_exchange)."""
    L = load_library()
    cfg = _Config(W, H, N, render_scale, 2.0, 0, 0, 0, (ctypes.c_int * 4)())
    info = (ctypes.c_int * 9)()
    n = L.rc2dgi_plan_jfa_exchange(ctypes.byref(cfg), world, step, info, None, 0)
    if n < 0:
        raise RC2DGIError(n, "rc2dgi_plan_jfa_exchange")
    buf = (ctypes.c_int * max(6 * n, 1))()
    L.rc2dgi_plan_jfa_exchange(ctypes.byref(cfg), world, step, info, buf, n)
    return dict(zip(JFA_INFO, list(info))), [tuple(buf[6 * k:6 * k + 6]) for k in range(n)]


def plan_group_waits(W: int, H: int, N: int, world: int, rank: int, step: int, render_scale: float = 1.0):
    """Host-only: the peers shard `rank` of a group frame awaits (their step step-1 done) before JFA step
    `step` (rc2dgi_plan_group_waits): (readers of its J_{step-2}, senders of the J_{step-1} rows it copies)."""
    L = load_library()
    cfg = _Config(W, H, N, render_scale, 2.0, 0, 0, 0, (ctypes.c_int * 4)())
    buf = (ctypes.c_int * max(2 * world, 1))()
    n = L.rc2dgi_plan_group_waits(ctypes.byref(cfg), world, rank, step, buf, 2 * world)
    if n < 0:
        raise RC2DGIError(n, "rc2dgi_plan_group_waits")
    got = list(buf[:n])
    return sorted(q for q in got if q >= 0), sorted(-1 - q for q in got if q < 0)


def plan_jfa_window(W: int, H: int, N: int, rank: int, world: int, step: int, render_scale: float = 1.0):
    """Where shard `rank` reads tap y of JFA step `step`: ([buffer per tap], [global row of each
    buffer's local row 0]) (rc2dgi_plan_jfa_window)."""
    L = load_library()
    cfg = _Config(W, H, N, render_scale, 2.0, 0, 0, 0, (ctypes.c_int * 4)())
    buf, row0 = (ctypes.c_int * 3)(), (ctypes.c_int * 3)()
    rc = L.rc2dgi_plan_jfa_window(ctypes.byref(cfg), rank, world, step, buf, row0)
    if rc < 0:
        raise RC2DGIError(rc, "rc2dgi_plan_jfa_window")
    return list(buf), list(row0)


__all__ = ["RC2DGI", "RC2DGIError", "load_library", "abi_version", "RT", "PASS_NAMES", "shard_unique_id", "do_group",
           "plan_rows", "plan_jfa_exchange", "plan_jfa_window", "PLAN_JFA", "PLAN_LEVEL", "PLAN_BLUR", "PLAN_MERGE",
           "View", "display_layout", "FILTER_RT", "FILTER_POINT", "FILTER_LINEAR", "MAX_VIEWS", "Ray", "RayHit",
           "RAY_DTYPE", "HIT_DTYPE", "hit_floats", "RAY_INVALID", "RAY_RANGE", "RAY_EDGE", "RAY_EMISSIVE", "RAY_SURFACE",
           "RAY_STEPS", "Rect", "Stats", "RECT_DTYPE", "STATS_DTYPE", "stats_view", "STATS_OK", "STATS_INVALID",
           "STATS_WORDS", "REDUCE_MAX", "Tone", "CURVE_EDGES", "MAX_CURVES", "HIST_MAX_EDGES", "CHANNELS", "HIST_HEAD",
           "check_edges", "curve_q8", "curve_from", "percentile"]
