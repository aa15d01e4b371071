"""TEST INFRASTRUCTURE ONLY: numpy restatement of rc2dgi_gradients_device, written from include/rc2dgi.h.  The geometry
(the refusal test, the vertex lists, the snap) is tests/shapes_ref.py's and the RGBA8 blend oracle.paint_ref's; the edge
functions are int64 with _cover's orientation, the first covering triangle in listed order supplies the colour, the
interpolation is float32 with one rounding an operation, and the blends are rc2dgi_write's."""
import numpy as np

import shapes_ref as S
from oracle.paint_ref import _blend8

f32 = np.float32
RECT, CIRCLE, TRIANGLE, LINE, ELLIPSE = S.RECT, S.CIRCLE, S.TRIANGLE, S.LINE, S.ELLIPSE
GAIN_LIM = f32(1048576.0)
INV255 = f32(f32(1) / f32(255))
# the colour index of each listed vertex, triangle by triangle ("Colours by kind")
FAN = [(0, 1, 1)] * 36
COLOURS = {RECT: [(0, 1, 2), (0, 2, 3)], CIRCLE: FAN, ELLIPSE: FAN, TRIANGLE: [(0, 1, 2)], LINE: [(0, 0, 1), (0, 1, 1)]}


def words(grads):
    """(n, 12) int32 records from (kind, v (up to 6 floats), colours (up to four (r, g, b, a)), gain) tuples; words not
    given are zero."""
    out = np.zeros((len(grads), 12), np.int32)
    for k, (kind, v, cols, gain) in enumerate(grads):
        out[k, 0] = kind
        vv = np.zeros(6, f32)
        vv[:len(v)] = np.asarray(v, f32)
        out[k, 1:7] = vv.view(np.int32)
        cc = np.zeros((4, 4), np.uint8)
        cc[:len(cols)] = np.asarray(cols, np.uint8).reshape(-1, 4)
        out[k, 7:11] = cc.reshape(16).view(np.int32)
        out[k, 11] = np.array([gain], f32).view(np.int32)[0]
    return out


def from_shapes(recs):
    """the equal-colour, gain-1 records of (n, 8) shapes_ref.words records (the header's first consequence)"""
    recs = np.asarray(recs, np.int32).reshape(-1, 8)
    one = np.full((len(recs), 1), np.array([1.0], f32).view(np.int32)[0], np.int32)
    return np.concatenate([recs[:, :7], np.repeat(recs[:, 7:8], 4, axis=1), one], axis=1)


def gain_of(rec):
    return np.asarray(rec[11:12], np.int32).view(f32)[0]


def refused(rec):
    """the header's "Refused" paragraph on one record of twelve int32 words"""
    if S.refused(rec[:8]):
        return True
    with np.errstate(all="ignore"):
        return not bool(np.abs(gain_of(rec)) <= GAIN_LIM)  # (false for a NaN and for an infinity)


def edge_functions(t, W, H):
    """t: three snapped vertices in listed order.  None for a zero area; otherwise (E0, E1, E2, cov): E_k (H, W) int64,
    the edge function of the edge joining the other two vertices with the inside positive, and the coverage mask."""
    (x0, y0), (x1, y1), (x2, y2) = t
    area = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
    if area == 0:
        return None
    P = [(x0, y0), (x1, y1), (x2, y2)]
    order = [0, 1, 2] if area > 0 else [0, 2, 1]  # counter-clockwise, as _cover swaps
    X = (np.arange(W, dtype=np.int64) * 256 + 128)[None, :]
    Y = (np.arange(H, dtype=np.int64) * 256 + 128)[:, None]
    E = [None, None, None]
    cov = np.ones((H, W), bool)
    for e in range(3):
        ia, ib, opp = order[e], order[(e + 1) % 3], order[(e + 2) % 3]
        (ax, ay), (bx, by) = P[ia], P[ib]
        dx, dy = bx - ax, by - ay
        Ee = dx * (Y - ay) - dy * (X - ax)
        incl = dy < 0 or (dy == 0 and dx > 0)
        cov &= (Ee > 0) | ((Ee == 0) & incl)
        E[opp] = Ee  # the edge that joins the other two vertices of listed vertex `opp`
    return E[0], E[1], E[2], cov


def unorm(c):
    return (np.asarray(c, np.uint8).astype(f32) * INV255).astype(f32)


def interpolate(E0, E1, E2, q0, q1, q2, gain):
    """the header's "Interpolation": E_k int64 arrays of one shape, q_k four floats -> src (..., 4) float32"""
    with np.errstate(all="ignore"):
        fa = (E0 + E1 + E2).astype(f32)  # int64 -> float32: one round-to-nearest-even conversion
        w1 = (E1.astype(f32) / fa).astype(f32)[..., None]
        w2 = (E2.astype(f32) / fa).astype(f32)[..., None]
        q0, q1, q2 = (np.asarray(q, f32) for q in (q0, q1, q2))
        d1, d2 = (q1 - q0).astype(f32), (q2 - q0).astype(f32)
        p1, p2 = (w1 * d1).astype(f32), (w2 * d2).astype(f32)
        col = ((q0 + p1).astype(f32) + p2).astype(f32)
        col[..., :3] = (col[..., :3] * f32(gain)).astype(f32)
    return col


def shade(rec, W, H):
    """-> (cov (H, W) bool, src (H, W, 4) float32, tri (H, W) int: the index in listed order of the triangle that
    supplied the colour, -1 where none) of an accepted record"""
    kind = int(rec[0])
    cols = np.asarray(rec[7:11], np.int32).view(np.uint8).reshape(4, 4)
    gain = gain_of(rec)
    cov = np.zeros((H, W), bool)
    src = np.zeros((H, W, 4), f32)
    tri = np.full((H, W), -1, np.int64)
    for idx, t in enumerate(S.snapped(rec[:8], W, H)):
        ef = edge_functions(t, W, H)
        if ef is None:
            continue
        E0, E1, E2, m = ef
        new = m & ~cov  # the first covering triangle supplies the colour
        if new.any():
            i0, i1, i2 = COLOURS[kind][idx]
            col = interpolate(E0[new], E1[new], E2[new], unorm(cols[i0]), unorm(cols[i1]), unorm(cols[i2]), gain)
            src[new] = col
            tri[new] = idx
            cov |= new
    return cov, src, tri


def q8(x):
    """fragment output -> unorm8 (NaN -> 0): clamp, times 255, round to nearest even"""
    with np.errstate(all="ignore"):
        c = np.fmin(np.fmax(np.asarray(x, f32), f32(0)), f32(1))  # (fmaxf(NaN, 0) is 0)
        return np.rint((c * f32(255)).astype(f32)).astype(np.uint8)


def paint(W, H, recs, clear=None, base=None, rgba8=False, count=None):
    """-> (texture (H, W, 4) in GL rows -- float32, or uint8 texels with rgba8 -- , m, refused) after
    rc2dgi_gradients_device(which, clear, recs, n, count): base is the texture before the call (zeros if None)."""
    recs = np.asarray(recs, np.int32).reshape(-1, 12)
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
    nref = 0
    for rec in recs[:m]:
        if refused(rec):
            nref += 1
            continue
        cov, src, _ = shade(rec, W, H)
        if not cov.any():
            continue
        if rgba8:
            img = np.where(cov[..., None], _blend8(q8(src), img), img)
            continue
        with np.errstate(all="ignore"):
            a = src[..., 3:4]
            blended = ((src * a).astype(f32) + (img * (f32(1) - a).astype(f32)).astype(f32)).astype(f32)
        img = np.where(cov[..., None], blended, img)
    return img, m, nref
