"""One script of frames as a host drives them back to back, for tests/test_pipeline_script_cpu.py and
test_gpu_pipeline.py: every step is "input changes, uniform changes, a curve for tone slot 1, one frame, captures", and
every input change can be made from device memory (an `upload` of the whole texture or a `write` of a rectangle).

    step  input change                                                        uniform change
    0     COLOR and EMISSIVE of scenes.demo(W, H), whole, by upload           -
    1     an emissive sprite: RGBA32F, 24 x 16, written flipped over the box  _Reflectivity 0.7
    2     an RGBA16F image blended into COLOR (an occluder in empty space)    _RayRange 200
    3     a patch of EMISSIVE with NaN and +inf on that image's corner        -
    4     the same patch with finite values                                   _RayRange 2, _BlurRadius 1.0
    5     -                                                                   -

The curve of tone slot 1 is the q8 table from step 0, a gamma curve from step 2 and Reinhard from step 4.

Nothing here touches a GPU: the texture every step's frame reads is worked out with tests/write_ref.c over the step
before (ref_write of test_write_cpu.py), and oracle.frame runs on that texture and that step's parameters alone, so a
frame that picked up anything of its neighbours differs from its oracle frame."""
import copy
import functools
from dataclasses import dataclass, field

import numpy as np

import oracle
import wild_inputs as wi
from test_write_cpu import ref_write

f32, f16 = np.float32, np.float16
ALL_STEPS = (0, 1, 2, 3, 4, 5)
SPRITE_W, SPRITE_H = 24, 16
BLEND_W, BLEND_H = 40, 20
PATCH_W, PATCH_H = 20, 12
N_POINTS, N_RAYS, N_EDGES = 256, 64, 15
GAMMA = 2.2


@dataclass
class Change:
    """One input change: kind "upload" (img: the whole texture) or "write" (img into rect, flipped and / or blended)."""
    kind: str
    which: str
    img: np.ndarray
    rect: tuple = None
    flip: bool = False
    blend: bool = False


@dataclass
class Step:
    index: int                     # the row of the table above
    changes: list
    uniforms: list                 # [(name, value)] in the order they are set
    curve: np.ndarray              # the 255 edges set into slot 1 before this frame, or None
    curve_name: str                # the curve in slot 1 while this frame's captures are composed
    params: oracle.Params          # this frame's parameters
    color: np.ndarray = None       # the textures this frame reads, as download returns them
    emis: np.ndarray = None


@dataclass
class Script:
    W: int
    H: int
    N: int
    storage: str
    steps: list
    CW: int = 0
    CH: int = 0
    sprite: tuple = None           # the rectangles of steps 1, 2 and 3 / 4 (x, y, w, h), GL rows
    blend: tuple = None
    patch: tuple = None
    uv: np.ndarray = None          # (256, 2) points sampled LINEAR on FINAL_GI
    rays: np.ndarray = None        # (64, 6) rays
    reduce_rects: list = None      # 3 rectangles of FINAL_GI: the inline plan
    hist_rects: list = None        # 2 rectangles of FINAL_GI
    hist_edges: np.ndarray = None  # 15 edges of the luma
    dist_crop: tuple = None        # the crop of DIST read as RGBA8, flipped
    tones: list = None             # one (exposure, 1) a view of display_layout(W, H)
    curves: dict = field(default_factory=dict)
    _frames: list = None


def gamma_curve(x):
    return np.power(np.maximum(x, 0.0), 1.0 / GAMMA)


def reinhard(x):
    return x / (1.0 + x)


@functools.lru_cache(maxsize=None)
def curves():
    """{name: 255 float32 edges} of the three curves slot 1 holds in turn; the host computes them (curve_q8, curve_from)"""
    from radiancecascade2dglobalillumination_amd import rc2dgi as R

    out = {"q8": R.curve_q8(), "gamma": R.curve_from(gamma_curve), "reinhard": R.curve_from(reinhard)}
    for e in out.values():
        e.setflags(write=False)
    return out


def tone_bytes(edges, values, exposure=1.0):
    """bin(v * exposure) over the edges as rc2dgi_tone states it: the number of edges <= the float32 product (a NaN
    counts none); tests/test_pipeline_script_cpu.py holds it against tone_ref.c's tone_bin."""
    v = (np.asarray(values, f32) * f32(exposure)).astype(f32)
    b = np.searchsorted(np.asarray(edges, f32), v, side="right")
    return np.where(np.isnan(v), 0, b).astype(np.uint8)


def box_of(W, H):
    """the demo's square wall (RC2DGI.cs:114) at W x H: (x0, y0, x1, y1), GL rows, as scenes.demo rounds it"""
    from radiancecascade2dglobalillumination_amd import scenes

    x, y, w, h = scenes.DEMO_WALLS[2]
    sx, sy = W / 1200.0, H / 900.0
    x0, x1 = int(round(x * sx)), int(round((x + w) * sx))
    t0, t1 = int(round(y * sy)), int(round((y + h) * sy))  # screen rows, y down
    return x0, H - t1, x1, H - t0


def seed_error(n):
    """per texel of an axis of n texels: how far the texel's centre lies from its 8-bit texture coordinate, in
    texture coordinates -- RGBA8 storage keeps the JumpFlood seeds in 8 bits, so a texel inside an occluder reads a
    distance of this size, not 0"""
    d = (np.arange(n) + 0.5) * 255.0 / n
    return np.abs(d - np.rint(d)) / 255.0


def place_blend(W, H):
    """Where the blended image goes: in empty space of the demo scene (4 texels clear all round), and of such
    places the one where most texels of its lower left corner pass the march's hit test (distance < 0.001) on RGBA8
    storage too -- there the 8-bit seeds decide it (seed_error): at 128 x 128 no texel of the demo's box passes, at
    256 x 256 none of columns 0 .. 60."""
    from radiancecascade2dglobalillumination_amd import scenes

    occ = np.any(scenes.demo(W, H)[0][..., :3] > 0, -1)
    hit = np.hypot(seed_error(H)[:, None], seed_error(W)[None, :]) < 0.0008
    step = max(4, min(W, H) // 32)
    best, where = -1, None
    for y in range(4, H - BLEND_H - 4, step):
        for x in range(4, W - BLEND_W - 4, step):
            if occ[y - 4:y + BLEND_H + 4, x - 4:x + BLEND_W + 4].any():
                continue
            score = int(hit[y:y + PATCH_H - 2, x:x + BLEND_W // 3].sum())
            if score > best:
                best, where = score, (x, y)
    assert where is not None
    return where + (BLEND_W, BLEND_H)


def rectangles(W, H, blended=True):
    """(sprite, blend, patch): the sprite centred on the box (the only texels of EMISSIVE rays hit are those of an
    occluder), the blended image in empty space (place_blend), the patch across the lower left corner of the blended
    image (texels of an occluder's edge, which rays from outside hit, and texels outside it) -- in a script without
    step 2 across the box's."""
    x0, y0, x1, y1 = box_of(W, H)
    cx, cy = (x0 + x1) // 2, (y0 + y1) // 2
    sprite = (cx - SPRITE_W // 2, cy - SPRITE_H // 2, SPRITE_W, SPRITE_H)
    blend = place_blend(W, H)
    patch = (blend[0] - 2, blend[1] - 2, PATCH_W, PATCH_H) if blended else (x0 - 2, y0 - 2, PATCH_W, PATCH_H)
    for x, y, w, h in (sprite, blend, patch):
        assert 0 <= x and x + w <= W and 0 <= y and y + h <= H, (W, H, (x, y, w, h))
    return sprite, blend, patch


def sprite_image():
    """RGBA32F emission, different in every row and column (a flip or a shift shows)"""
    j, i = np.mgrid[0:SPRITE_H, 0:SPRITE_W]
    img = np.empty((SPRITE_H, SPRITE_W, 4), f32)
    img[..., 0] = 0.5 + j / 32.0
    img[..., 1] = 0.25 + i / 48.0
    img[..., 2] = ((i + 2 * j) % 5) / 4.0
    img[..., 3] = 1.0
    return img


def blend_image():
    """RGBA16F: alpha 1 in the left third, 0.5 in the middle, 0 on the right (which leaves the texels as they were);
    every value is a multiple of 1 / 64, so a half holds it"""
    j, i = np.mgrid[0:BLEND_H, 0:BLEND_W]
    img = np.empty((BLEND_H, BLEND_W, 4), f32)
    img[..., 0] = (16 + i) / 64.0
    img[..., 1] = (60 - 2 * j) / 64.0
    img[..., 2] = ((3 * i + j) % 32) / 64.0 + 0.25
    img[..., 3] = np.where(i < BLEND_W // 3, 1.0, np.where(i < 2 * BLEND_W // 3, 0.5, 0.0))
    h = img.astype(f16)
    assert np.array_equal(h.astype(f32), img)
    return h


def odd_patch():
    """RGBA32F emission with a NaN in every third texel and +inf in every third (one channel each), the rest finite
    and dark where the sprite under it is bright (RGBA8 storage turns the NaN into 0 and clamps the rest: its frames
    still have to differ from the step before)"""
    j, i = np.mgrid[0:PATCH_H, 0:PATCH_W]
    img = np.empty((PATCH_H, PATCH_W, 4), f32)
    img[..., 0] = (1 + i) / 32.0
    img[..., 1] = (1 + j) / 32.0
    img[..., 2] = 0.0625
    img[..., 3] = 1.0
    k = (i + j) % 3
    img[..., 0] = np.where(k == 0, f32(np.nan), img[..., 0])
    img[..., 1] = np.where(k == 1, f32(np.inf), img[..., 1])
    return img


def finite_patch():
    j, i = np.mgrid[0:PATCH_H, 0:PATCH_W]
    img = np.empty((PATCH_H, PATCH_W, 4), f32)
    img[..., 0] = (1 + i) / 8.0
    img[..., 1] = (6 - j) / 8.0
    img[..., 2] = ((i * j) % 4) / 4.0
    img[..., 3] = 1.0
    return img


_cache = {}


def build(ref_lib, W, H, N, storage="f32", steps=ALL_STEPS, render_scale=1.0):
    """The script at W x H with N cascades on `storage`, `steps` a subset of the table's rows in order (each applies its
    own changes to what the listed steps before it left).  ref_lib: tests/write_ref.c (build_write_ref).  Cached: the
    arrays are shared and read-only."""
    from radiancecascade2dglobalillumination_amd import rc2dgi as R
    from radiancecascade2dglobalillumination_amd import scenes

    key = (W, H, N, storage, tuple(steps), render_scale)
    if key in _cache:
        return _cache[key]
    assert steps[0] == 0 and list(steps) == sorted(steps)
    u8 = storage == "rgba8"
    p = oracle.Params(W=W, H=H, N=N, render_scale=render_scale, gi_f16=storage == "f16", rgba8=u8)
    CW, CH, _ = oracle.dims(p)
    sprite, blend, patch = rectangles(W, H, 2 in steps)
    cv = curves()
    color, emis = scenes.demo(W, H)
    if u8:  # (the texels an RGBA8 texture holds after the upload)
        color, emis = wi.as_rgba8(color), wi.as_rgba8(emis)
    demo_color, demo_emis = color, emis
    out, curve_name = [], None
    for n in steps:
        changes, uniforms, curve = [], [], None
        if n == 0:
            changes = [Change("upload", "color", demo_color), Change("upload", "emissive", demo_emis)]
            curve = "q8"
        elif n == 1:
            changes = [Change("write", "emissive", sprite_image(), sprite, flip=True)]
            uniforms = [("_Reflectivity", 0.7)]
        elif n == 2:
            changes = [Change("write", "color", blend_image(), blend, blend=True)]
            uniforms = [("_RayRange", 200.0)]
            curve = "gamma"
        elif n == 3:
            changes = [Change("write", "emissive", odd_patch(), patch)]
        elif n == 4:
            changes = [Change("write", "emissive", finite_patch(), patch)]
            uniforms = [("_RayRange", 2.0), ("_BlurRadius", 1.0)]
            curve = "reinhard"
        for ch in changes:
            if ch.kind == "write":
                tex = color if ch.which == "color" else emis
                tex = ref_write(ref_lib, tex, ch.img, ch.rect, ch.flip, ch.blend, u8=u8)
                if ch.which == "color":
                    color = tex
                else:
                    emis = tex
            ch.img.setflags(write=False)
        for name, v in uniforms:
            setattr(p, {"_Reflectivity": "reflectivity", "_RayRange": "ray_range", "_BlurRadius": "blur_radius"}[name], v)
        curve_name = curve or curve_name
        for a in (color, emis):
            a.setflags(write=False)
        out.append(Step(n, changes, uniforms, None if curve is None else cv[curve], curve_name, copy.copy(p), color, emis))
    rng = np.random.default_rng(W * 7 + H)
    uv = rng.uniform(-0.1, 1.1, (N_POINTS, 2)).astype(f32)
    sx, sy, sw, sh = sprite
    near = N_POINTS // 4  # a quarter of the points around the sprite, where consecutive frames differ most
    uv[:near, 0] = (sx + rng.uniform(-sw, 2 * sw, near)) / W
    uv[:near, 1] = (sy + rng.uniform(-sh, 2 * sh, near)) / H
    rays = np.empty((N_RAYS, 6), f32)
    rays[:, 0:2] = rng.uniform(0.0, 1.0, (N_RAYS, 2))
    ang = rng.uniform(0, 2 * np.pi, N_RAYS)
    rays[:, 2], rays[:, 3] = np.cos(ang), np.sin(ang)
    rays[:, 4] = 0.0
    rays[:, 5] = rng.choice(f32([0.25, 1.0, 3.0]), N_RAYS)
    rays[:N_RAYS // 4, 0] = (sx + sw / 2) / W + rng.uniform(-0.2, 0.2, N_RAYS // 4)  # towards the box and the sprite
    rays[:N_RAYS // 4, 1] = (sy + sh / 2) / H - 0.3
    rays[:N_RAYS // 4, 2:4] = (0.0, 1.0)
    cs = (min(CW - 1, sx * CW // W), min(CH - 1, sy * CH // H))  # the sprite's corner in the cascade's texels
    around = (max(0, cs[0] - 8), max(0, cs[1] - 8), min(48, CW - max(0, cs[0] - 8)), min(40, CH - max(0, cs[1] - 8)))
    s = Script(W, H, N, storage, out, CW, CH, sprite, blend, patch, uv, rays,
               reduce_rects=[(0, 0, CW, CH), around, (1, 2, CW - 3, CH // 2 - 1)],
               hist_rects=[(0, 0, CW, CH), around],
               hist_edges=(2.0 ** np.arange(-10, N_EDGES - 10)).astype(f32),
               dist_crop=(W // 5, H // 6, W // 2 + 3, H // 3 + 1),
               tones=[(1.0, 1)] + [(2.0, 1)] * (len(R.display_layout(W, H)) - 1), curves=cv)
    for a in (s.uv, s.rays, s.hist_edges):
        a.setflags(write=False)
    _cache[key] = s
    return s


def frames(script):
    """oracle.frame of every step on that step's parameters and inputs alone, level 0 kept; computed once a script"""
    if script._frames is None:
        script._frames = [oracle.frame(st.params, st.color, st.emis, keep_levels=True) for st in script.steps]
    return script._frames


def captured_textures(script, fr):
    """what the four read captures of a step hold, from its oracle frame: FINAL_GI, the merged COLOR and BLUR as
    floats, the crop of DIST as the bytes of its texels, top row first"""
    x, y, w, h = script.dist_crop
    return dict(final_gi=fr.gi_final, color=fr.color_out, blur=fr.blur,
                dist=np.ascontiguousarray(oracle.to_u8(fr.dist)[y:y + h, x:x + w][::-1]))


def same_bits(a, b):
    """bit equality of two float32 arrays, a NaN equal to any NaN in the same place: wild_inputs.bits_equal where
    neither holds a NaN (payloads are nowhere specified: tests/test_gpu_inputs.py, tests/test_write_cpu.py)"""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not na.any() and not nb.any():
        return wi.bits_equal(a, b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def differ(a, b):
    return not same_bits(a, b)
