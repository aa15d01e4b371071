"""numpy restatement of rc2dgi_sprites_xf_device as include/rc2dgi.h states it (written from the header, not from the
kernel): the refusal rule, the set-up (the inverse of (A, B) and the pixel box), the map of a pixel centre into the
source rectangle, POINT and LINEAR, rc2dgi_write's values, the tint, the two blends and the replacement.  Each float
operation is one float32 operation (numpy float32 arithmetic rounds once an operation and keeps denormals); the 8-bit
ones use sprites_ref's q8 and mul8.

A texture is (H, W, 4) in GL row order: float32 in F32 / F16 storage, the uint8 texels in RGBA8_COMPAT storage.  A
sprite list is an (n, 12) int32 array, a row the words of rc2dgi_sprite_xf."""
import numpy as np

from sprites_ref import mul8, q8, tint_of, values

f32 = np.float32
REPLACE, LINEAR = 4, 8
LIM, DET = f32(2.0 ** 20), f32(2.0 ** -20)
HALF = f32(0.5)


def words(sprites):
    """(n, 12) int32 of (sx, sy, w, h, px, py, ax, ay, bx, by, (r, g, b, a), flags) tuples"""
    out = np.zeros((len(sprites), 12), np.int32)
    for k, (sx, sy, w, h, px, py, ax, ay, bx, by, tint, flags) in enumerate(sprites):
        r, g, b, a = (int(v) for v in tint)
        ints = np.array([sx, sy, w, h, r | g << 8 | b << 16 | a << 24, flags], np.int64) & 0xFFFFFFFF
        out[k, [0, 1, 2, 3, 10, 11]] = ints.astype(np.uint32).view(np.int32)
        out[k, 4:10] = np.array([px, py, ax, ay, bx, by], f32).view(np.int32)
    return out


def floats(wd):
    """words 4 .. 9 of every record as float32: px, py, ax, ay, bx, by"""
    return np.ascontiguousarray(np.ascontiguousarray(wd, np.int32).reshape(-1, 12)[:, 4:10]).view(f32)


def refusal_terms(wd, AW, AH):
    """the four terms of the header's rule, a bool a record each: flags, source rectangle, component bound, determinant"""
    wd = np.ascontiguousarray(wd, np.int32).reshape(-1, 12)
    q = wd.astype(np.int64)
    sx, sy, w, h = (q[:, k] for k in range(4))
    flags = q[:, 11] & 0xFFFFFFFF
    bad_flags = (flags & ~np.int64(REPLACE | LINEAR)) != 0
    bad_src = (w < 1) | (h < 1) | (sx < 0) | (sy < 0) | (w > AW - sx) | (h > AH - sy)
    with np.errstate(all="ignore"):
        c = floats(wd)
        bad_comp = ~np.all(np.abs(c) <= LIM, axis=1)  # (false for a NaN and an infinity)
        det = (c[:, 2] * c[:, 5]).astype(f32) - (c[:, 3] * c[:, 4]).astype(f32)
        bad_det = ~(np.abs(det) >= DET)
    return bad_flags, bad_src, bad_comp, bad_det


def accepted(wd, AW, AH):
    """the header's rule, a bool a record: not refused"""
    t = refusal_terms(wd, AW, AH)
    return ~(t[0] | t[1] | t[2] | t[3])


def box(rec, W, H):
    """(X0, X1, Y0, Y1) of an accepted record, screen pixels (y down), inclusive; empty when X0 > X1 or Y0 > Y1"""
    px, py, ax, ay, bx, by = floats(rec)[0]
    xs = [px, px + ax, px + bx, (px + ax) + bx]
    ys = [py, py + ay, py + by, (py + ay) + by]
    return (max(int(np.floor(min(xs))) - 1, 0), min(int(np.floor(max(xs))) + 1, W - 1),
            max(int(np.floor(min(ys))) - 1, 0), min(int(np.floor(max(ys))) + 1, H - 1))


def lerp(p, q, f):
    return (p + (f * (q - p).astype(f32)).astype(f32)).astype(f32)


def draw(tex, atlas, wd, rgba8=False, clear=None, m=None):
    """the texture after rc2dgi_sprites_xf_device(tex's target, clear, atlas, wd, count -> m); tex is not changed"""
    img = np.array(tex, np.uint8 if rgba8 else f32)
    H, W = img.shape[:2]
    if clear is not None:
        img[:] = np.array(clear, np.uint8) if rgba8 else (np.array(clear, f32) / f32(255)).astype(f32)
    wd = np.ascontiguousarray(wd, np.int32).reshape(-1, 12)
    n = len(wd) if m is None else min(max(int(m), 0), len(wd))
    AH, AW = np.asarray(atlas).shape[:2]
    val = values(atlas, rgba8)
    ok = accepted(wd[:n], AW, AH)
    with np.errstate(all="ignore"):
        for k in np.nonzero(ok)[0]:
            sx, sy, w, h = (int(v) for v in wd[k, :4])
            flags = int(wd[k, 11])
            px, py, ax, ay, bx, by = floats(wd[k:k + 1])[0]
            det = ax * by - ay * bx  # (numpy float32 scalars: each operation rounds once)
            i00, i01, i10, i11 = by / det, (-bx) / det, (-ay) / det, ax / det
            X0, X1, Y0, Y1 = box(wd[k:k + 1], W, H)
            if X0 > X1 or Y0 > Y1:
                continue
            X, Y = np.arange(X0, X1 + 1), np.arange(Y0, Y1 + 1)
            dxp = ((X.astype(f32) + HALF) - px)[None, :]
            dyp = ((Y.astype(f32) + HALF) - py)[:, None]
            a = (dxp * i00).astype(f32) + (dyp * i01).astype(f32)
            b = (dxp * i10).astype(f32) + (dyp * i11).astype(f32)
            cov = (a >= 0) & (a < 1) & (b >= 0) & (b < 1)
            if not cov.any():
                continue
            s = np.where(cov, a * f32(w), f32(0)).astype(f32)
            t = np.where(cov, b * f32(h), f32(0)).astype(f32)
            sub = val[sy:sy + h, sx:sx + w]  # the source rectangle: no tap leaves it
            if flags & LINEAR:
                xs, ys = s - HALF, t - HALF
                i0, j0 = np.floor(xs).astype(np.int64), np.floor(ys).astype(np.int64)
                fx, fy = (xs - i0.astype(f32))[..., None], (ys - j0.astype(f32))[..., None]
                c0, c1 = np.clip(i0, 0, w - 1), np.clip(i0 + 1, 0, w - 1)
                r0, r1 = np.clip(j0, 0, h - 1), np.clip(j0 + 1, 0, h - 1)
                v = lerp(lerp(sub[r0, c0], sub[r0, c1], fx), lerp(sub[r1, c0], sub[r1, c1], fx), fy)
            else:
                v = sub[np.minimum(t.astype(np.int64), h - 1), np.minimum(s.astype(np.int64), w - 1)]
            src = (v * tint_of(wd[k, 10], rgba8)).astype(f32)
            at = np.ix_(H - 1 - Y, X)
            cur = img[at]
            if rgba8:
                s8 = q8(src)
                if flags & REPLACE:
                    new = s8.astype(np.uint8)
                else:
                    a8 = s8[..., 3:4]
                    new = np.minimum(mul8(s8, a8) + mul8(cur.astype(np.int64), 255 - a8), 255).astype(np.uint8)
            elif flags & REPLACE:
                new = src
            else:
                al = src[..., 3:4]
                ia = (f32(1) - al).astype(f32)
                new = ((src * al).astype(f32) + (cur * ia).astype(f32)).astype(f32)
            img[at] = np.where(cov[..., None], new, cur)
    return img
