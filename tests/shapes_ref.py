"""TEST INFRASTRUCTURE ONLY: numpy restatement of rc2dgi_shapes_device, written from include/rc2dgi.h.  The vertex lists
are float32 arithmetic, one rounding an operation; the window transform, the snap, the coverage rule, the RGBA8 blend
and the circle table are oracle.paint_ref's (pinned against llvmpipe).  A shape covers a texel when one of its
triangles does and blends over it once, in list order."""
import numpy as np

from oracle.paint_ref import _blend8, _cover, _snap, _window, circle_table

f32 = np.float32
RECT, CIRCLE, TRIANGLE, LINE, ELLIPSE = 0, 1, 2, 3, 4
NV = {RECT: 4, CIRCLE: 3, TRIANGLE: 6, LINE: 5, ELLIPSE: 4}  # the words of v[] a kind reads
LIM_PRIM, LIM = f32(4194304.0), f32(1048576.0)
_TABLE = None


def table():
    global _TABLE
    if _TABLE is None:
        _TABLE = circle_table()
    return _TABLE


def words(shapes):
    """(n, 8) int32 records from (kind, v (up to 6 floats), (r, g, b, a)) tuples; words not given are zero."""
    out = np.zeros((len(shapes), 8), np.int32)
    for k, (kind, v, rgba) in enumerate(shapes):
        out[k, 0] = kind
        vv = np.zeros(6, f32)
        vv[:len(v)] = np.asarray(v, f32)
        out[k, 1:7] = vv.view(np.int32)
        out[k, 7] = np.array(rgba, np.uint8).view(np.int32)[0]
    return out


def refused(rec):
    """the header's "Refused" paragraph on one record of eight int32 words"""
    kind = int(rec[0])
    if kind not in NV:
        return True
    with np.errstate(all="ignore"):
        v = np.asarray(rec[1:7], np.int32).view(f32)
        ok = lambda c, lim: bool(np.abs(f32(c)) < lim)  # noqa: E731  (false for a NaN and for an infinity)
        if kind == RECT:
            return not (ok(v[0], LIM_PRIM) and ok(v[1], LIM_PRIM) and ok(v[2], LIM_PRIM) and ok(v[3], LIM_PRIM) and
                        ok(f32(v[0] + v[2]), LIM_PRIM) and ok(f32(v[1] + v[3]), LIM_PRIM))
        if kind == CIRCLE:
            return not (ok(v[0], LIM_PRIM) and ok(v[1], LIM_PRIM) and ok(v[2], LIM_PRIM) and
                        bool(f32(np.abs(v[0]) + np.abs(v[2])) < LIM_PRIM) and
                        bool(f32(np.abs(v[1]) + np.abs(v[2])) < LIM_PRIM))
        return not all(ok(v[i], LIM) for i in range(NV[kind]))


def vertices(rec):
    """the triangles of an accepted record, as lists of three (x, y) float32 pairs in screen coordinates"""
    kind = int(rec[0])
    v = np.asarray(rec[1:7], np.int32).view(f32)
    with np.errstate(all="ignore"):
        if kind == RECT:
            x, y, xr, yb = v[0], v[1], f32(v[0] + v[2]), f32(v[1] + v[3])
            tl, tr, bl, br = (x, y), (xr, y), (x, yb), (xr, yb)
            return [(tl, bl, br), (tl, br, tr)]
        if kind in (CIRCLE, ELLIPSE):
            if kind == CIRCLE:
                rh = rv = v[2] if v[2] > 0 else f32(0.1)
            else:
                rh, rv = v[2], v[3]
            cs = table()
            T = [(f32(v[0] + f32(cs[k][0] * rh)), f32(v[1] + f32(cs[k][1] * rv))) for k in range(37)]
            return [((v[0], v[1]), T[k + 1], T[k]) for k in range(36)]
        if kind == TRIANGLE:
            return [((v[0], v[1]), (v[2], v[3]), (v[4], v[5]))]
        dx, dy, thick = f32(v[2] - v[0]), f32(v[3] - v[1]), v[4]
        ln = f32(np.sqrt(f32(f32(dx * dx) + f32(dy * dy))))
        if not (ln > 0 and thick > 0):
            return []
        scale = f32(thick / f32(f32(2.0) * ln))
        rx, ry = f32(f32(-scale) * dy), f32(scale * dx)
        s0, s1 = (f32(v[0] - rx), f32(v[1] - ry)), (f32(v[0] + rx), f32(v[1] + ry))
        s2, s3 = (f32(v[2] - rx), f32(v[3] - ry)), (f32(v[2] + rx), f32(v[3] + ry))
        return [(s0, s1, s2), (s1, s2, s3)]


def snapped(rec, W, H):
    """the record's triangles in window coordinates, 1/256 pixel, as Python ints"""
    return [[tuple(_snap(c) for c in _window(px, py, W, H)) for px, py in t] for t in vertices(rec)]


def coverage(rec, W, H):
    """(H, W) bool, GL rows: the texels one of the record's triangles covers"""
    cov = np.zeros((H, W), bool)
    for t in snapped(rec, W, H):
        m = _cover(t, W, H)
        if m is not None:
            cov |= m
    return cov


def paint(W, H, recs, clear=None, base=None, rgba8=False, count=None):
    """-> (texture (H, W, 4) in GL rows -- float32, or uint8 texels with rgba8 -- , m, refused) after
    rc2dgi_shapes_device(which, clear, recs, n, count): base is the texture before the call (zeros if None)."""
    recs = np.asarray(recs, np.int32).reshape(-1, 8)
    n = len(recs)
    m = n if count is None else min(max(int(count), 0), n)
    if rgba8:
        img = np.zeros((H, W, 4), np.uint8) if base is None else np.array(base, np.uint8)
        if clear is not None:
            img[:] = np.array(clear, np.uint8)
    else:
        img = np.zeros((H, W, 4), f32) if base is None else np.array(base, f32)
        if clear is not None:
            img[:] = np.array(clear, f32) / f32(255)
    inv = f32(f32(1) / f32(255))
    nref = 0
    for rec in recs[:m]:
        if refused(rec):
            nref += 1
            continue
        cov = coverage(rec, W, H)
        if not cov.any():
            continue
        rgba = np.array([rec[7]], np.int32).view(np.uint8)
        if rgba8:
            src = np.broadcast_to(rgba, img.shape)
            img = np.where(cov[..., None], _blend8(src, img), img)
            continue
        col = rgba.astype(f32) * inv
        a = col[3]
        blended = (col[None, None, :] * a + img * (f32(1) - a)).astype(f32)
        img = np.where(cov[..., None], blended, img)
    return img, m, nref
