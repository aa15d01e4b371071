"""numpy restatement of rc2dgi_sprites_device as include/rc2dgi.h states it (written from the header, not from the
kernel): the refusal rule, the pixel mapping, rc2dgi_write's values, the tint, the two blends and the replacement, each
float operation one float32 operation, the 8-bit ones with the header's q8 and mul8.

A texture is (H, W, 4) in GL row order: float32 in F32 / F16 storage, the uint8 texels in RGBA8_COMPAT storage (a texel
k reads as k * (1/255)).  A sprite list is an (n, 8) int32 array, a row the words of rc2dgi_sprite."""
import numpy as np

f32 = np.float32
INV255 = f32(1) / f32(255)
LIM = 1 << 22
FLIP_X, FLIP_Y, REPLACE = 1, 2, 4


def words(sprites):
    """(n, 8) int32 of (sx, sy, w, h, dx, dy, (r, g, b, a), flags) tuples"""
    out = np.zeros((len(sprites), 8), np.int64)
    for k, (sx, sy, w, h, dx, dy, tint, flags) in enumerate(sprites):
        r, g, b, a = (int(v) for v in tint)
        out[k] = [sx, sy, w, h, dx, dy, r | g << 8 | b << 16 | a << 24, flags]
    return (out & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def accepted(wd, AW, AH):
    """the header's rule, a bool a record: not refused"""
    q = np.ascontiguousarray(wd, np.int32).astype(np.int64)
    sx, sy, w, h, dx, dy = (q[:, k] for k in range(6))
    flags = q[:, 7] & 0xFFFFFFFF
    bad = (flags & ~np.int64(7)) != 0
    bad |= (w < 1) | (h < 1) | (sx < 0) | (sy < 0) | (w > AW - sx) | (h > AH - sy)
    bad |= (dx < -LIM) | (dx > LIM) | (dy < -LIM) | (dy > LIM)
    return ~bad


def q8(x):
    """rint(clamp(x, 0, 1) * 255), NaN -> 0, as integers"""
    with np.errstate(invalid="ignore"):
        x = np.asarray(x, f32)
        c = np.where(np.isnan(x), f32(0), np.minimum(np.maximum(x, f32(0)), f32(1))).astype(f32)
        return np.rint((c * f32(255)).astype(f32)).astype(np.int64)


def mul8(x, y):
    return (x * y * 257 + 32768) >> 16


def values(atlas, rgba8):
    """rc2dgi_write's "Values" for every atlas pixel: (AH, AW, 4) float32"""
    a = np.asarray(atlas)
    if a.dtype == np.uint8:
        k = a.astype(f32)
        return (k * INV255).astype(f32) if rgba8 else (k / f32(255)).astype(f32)
    v = a.astype(f32)  # (a half widens exactly)
    return (q8(v).astype(f32) * INV255).astype(f32) if rgba8 else v


def tint_of(word, rgba8):
    k = np.array([(int(word) >> s) & 255 for s in (0, 8, 16, 24)]).astype(f32)
    return (k * INV255).astype(f32) if rgba8 else (k / f32(255)).astype(f32)


def draw(tex, atlas, wd, rgba8=False, clear=None, m=None):
    """the texture after rc2dgi_sprites_device(tex's target, clear, atlas, wd, count -> m); tex is not changed"""
    img = np.array(tex, np.uint8 if rgba8 else f32)
    H, W = img.shape[:2]
    if clear is not None:
        img[:] = np.array(clear, np.uint8) if rgba8 else (np.array(clear, f32) / f32(255)).astype(f32)
    wd = np.ascontiguousarray(wd, np.int32).reshape(-1, 8)
    n = len(wd) if m is None else min(max(int(m), 0), len(wd))
    AH, AW = np.asarray(atlas).shape[:2]
    val = values(atlas, rgba8)
    ok = accepted(wd[:n], AW, AH)
    with np.errstate(all="ignore"):
        for k in np.nonzero(ok)[0]:
            sx, sy, w, h, dx, dy = (int(v) for v in wd[k, :6])
            flags = int(wd[k, 7])
            X0, X1, Y0, Y1 = max(dx, 0), min(dx + w - 1, W - 1), max(dy, 0), min(dy + h - 1, H - 1)
            if X0 > X1 or Y0 > Y1:
                continue
            X, Y = np.arange(X0, X1 + 1), np.arange(Y0, Y1 + 1)
            i, j = X - dx, Y - dy
            iu = sx + (w - 1 - i if flags & FLIP_X else i)
            jv = sy + (h - 1 - j if flags & FLIP_Y else j)
            src = (val[np.ix_(jv, iu)] * tint_of(wd[k, 6], rgba8)).astype(f32)
            at = np.ix_(H - 1 - Y, X)
            if rgba8:
                s8 = q8(src)
                if flags & REPLACE:
                    img[at] = s8.astype(np.uint8)
                else:
                    a8 = s8[..., 3:4]
                    img[at] = np.minimum(mul8(s8, a8) + mul8(img[at].astype(np.int64), 255 - a8), 255).astype(np.uint8)
            elif flags & REPLACE:
                img[at] = src
            else:
                a = src[..., 3:4]
                ia = (f32(1) - a).astype(f32)
                img[at] = ((src * a).astype(f32) + (img[at] * ia).astype(f32)).astype(f32)
    return img
