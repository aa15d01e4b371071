#!/usr/bin/env python3
"""What rc2dgi_sprites_xf_device costs beside rc2dgi_sprites_device, the 1:1 call (f32 storage, draws blended into COLOR
at 4096 x 4096 from an RGBA8 atlas), per case:
  a  one rc2dgi_sprites_device call of the case's sprites at identity (each source rectangle 1:1 at its place): the
     yardstick, the only earlier way to draw such pixels from a list
  b  one rc2dgi_sprites_xf_device call of the same sprites transformed as the case says
HIP events around each call for the device time, the wall clock until it returns (both only enqueue).  a and b alternate
run by run in one process; each figure is the mean and the minimum of --runs runs after --warmup warm-up runs.
Cases, from a 512 x 512 atlas unless said: 1024 and 16384 16 x 16 sprites at seeded random places -- at identity (POINT;
the two textures are compared in bits, after one application each over the same upload), turned by 30 degrees about
their centres (POINT, then LINEAR), scaled 4 x about their centres (LINEAR); `full`, one 4096 x 4096 sprite of a
4096 x 4096 atlas at identity (compared in bits); `full_scaled`, the 512 x 512 atlas over the whole target (LINEAR)
beside the same yardstick; `diagonal`, a 512 x 16 rectangle stretched along the target's diagonal, 11 pixels thick,
whose box and so whose mask bits cover the whole target, beside its 1:1 draw.
Prints one JSON line and writes it to --out.
Usage: sprites_xf_cost.py [--out FILE] [--runs 20]"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from radiancecascade2dglobalillumination_amd import RC2DGI, rc2dgi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--runs", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--counts", default="1024,16384")
args = ap.parse_args()


def stats(t):
    return {"mean_ms": float(np.mean(t)), "min_ms": float(np.min(t))}


assert torch.cuda.is_available(), "sprites_xf_cost.py measures on the GPU"
W = H = 4096
SW = SH = 16
rng = np.random.default_rng(1)
base = rng.uniform(0.0, 1.0, (H, W, 4)).astype(np.float32)


def about_centre(src, dst, deg, k):
    """(p, a, b) of the sprites (src rectangles at dst, 1:1) turned by `deg` and scaled by k about their centres"""
    w, h = src[:, 2].astype(np.float64), src[:, 3].astype(np.float64)
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    a = np.stack([c * w * k, s * w * k], 1)
    b = np.stack([-s * h * k, c * h * k], 1)
    centre = dst.astype(np.float64) + np.stack([w, h], 1) / 2
    return (centre - (a + b) / 2).astype(np.float32), a.astype(np.float32), b.astype(np.float32)


cases = []  # (name, atlas size, src (n, 4), dst (n, 2) of the yardstick, (p, a, b) of the transformed list, flags, bits)
for n in (int(v) for v in args.counts.split(",")):
    src = np.stack([rng.integers(0, 512 - SW + 1, n), rng.integers(0, 512 - SH + 1, n), np.full(n, SW), np.full(n, SH)],
                   1).astype(np.int32)
    dst = np.stack([rng.integers(0, W - SW + 1, n), rng.integers(0, H - SH + 1, n)], 1).astype(np.int32)
    cases += [(f"identity_{n}", 512, src, dst, about_centre(src, dst, 0.0, 1.0), 0, True),
              (f"rot30_point_{n}", 512, src, dst, about_centre(src, dst, 30.0, 1.0), 0, False),
              (f"rot30_linear_{n}", 512, src, dst, about_centre(src, dst, 30.0, 1.0), rc2dgi.SPRITE_LINEAR, False),
              (f"scale4_linear_{n}", 512, src, dst, about_centre(src, dst, 0.0, 4.0), rc2dgi.SPRITE_LINEAR, False)]
one = np.zeros((1, 2), np.int32)
full = np.array([[0, 0, W, H]], np.int32)
cases.append(("full", 4096, full, one, about_centre(full, one, 0.0, 1.0), 0, True))
whole = np.array([[0, 0, 512, 512]], np.int32)
f = np.float32
cases.append(("full_scaled", 4096, full, one, (f([[0, 0]]), f([[W, 0]]), f([[0, H]])), rc2dgi.SPRITE_LINEAR, False))
strip = np.array([[0, 0, 512, 16]], np.int32)
cases.append(("diagonal", 512, strip, one, (f([[8, 0]]), f([[W - 16, H - 16]]), f([[-8, 8]])), 0, False))

result = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "warmup": args.warmup, "W": W, "H": H,
          "cases": []}
for name, asize, src, dst, (p, a, b), flags, bits in cases:
    n = len(src)
    atlas_np = rng.integers(0, 256, (asize, asize, 4)).astype(np.uint8)
    xsrc = whole if name == "full_scaled" else src  # (the transformed list's source; the yardstick keeps `src`)
    stream = torch.cuda.Stream()
    ctx_a, ctx_b = RC2DGI(W, H, cascade_count=2), RC2DGI(W, H, cascade_count=2)
    L, which = ctx_a._L, rc2dgi.RT["color"]
    for c in (ctx_a, ctx_b):
        c.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        atlas = torch.from_numpy(atlas_np).to("cuda")
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda")  # noqa: E731
        words_a = rc2dgi.pack_sprites(t(src), t(dst))
        words_b = rc2dgi.pack_sprites_xf(t(xsrc), t(p), t(a), t(b), None,
                                         torch.full((n,), flags, dtype=torch.int32, device="cuda"))
        status = torch.zeros((2, 2), dtype=torch.int32, device="cuda")
        stream.synchronize()
        at = rc2dgi.Atlas(atlas.data_ptr(), asize, asize, 0, rc2dgi.FMT_RGBA8)
        at_p = ctypes.byref(at)
        pa, pb = ctypes.c_void_p(words_a.data_ptr()), ctypes.c_void_p(words_b.data_ptr())
        sa, sb = ctypes.c_void_p(status[0].data_ptr()), ctypes.c_void_p(status[1].data_ptr())

        def draw_a():
            rc = L.rc2dgi_sprites_device(ctx_a._h, which, None, at_p, pa, n, None, sa)
            assert rc == 0, rc

        def draw_b():
            rc = L.rc2dgi_sprites_xf_device(ctx_b._h, which, None, at_p, pb, n, None, sb)
            assert rc == 0, rc

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            fn()
            wall = (time.perf_counter() - t0) * 1e3
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1), wall

        for _ in range(args.warmup):
            draw_a()
            draw_b()
        stream.synchronize()
        a_dev, a_wall, b_dev, b_wall = [], [], [], []
        for _ in range(args.runs):  # the two calls alternate
            d, w = timed(draw_a)
            a_dev.append(d)
            a_wall.append(w)
            d, w = timed(draw_b)
            b_dev.append(d)
            b_wall.append(w)
        stream.synchronize()
        for c in (ctx_a, ctx_b):  # one application each over the same texels
            c.upload("color", base)
        draw_a()
        draw_b()
        stream.synchronize()
    got_a, got_b = ctx_a.download("color"), ctx_b.download("color")
    same = bool(np.array_equal(got_a.view(np.uint32), got_b.view(np.uint32)))
    touched = int(np.count_nonzero(np.any(got_b != base, axis=-1)))
    r = {"case": name, "sprites": n, "atlas": [asize, asize], "flags": int(flags), "status": status.cpu().numpy().tolist(),
         "texels_changed_by_b": touched, "textures_compared_in_bits": bits,
         "textures_equal_in_bits": same if bits else None,
         "a_sprites_device_device_time": stats(a_dev), "a_sprites_device_host_returns": stats(a_wall),
         "b_sprites_xf_device_device_time": stats(b_dev), "b_sprites_xf_device_host_returns": stats(b_wall),
         "b_over_a_device_time": float(np.mean(b_dev) / np.mean(a_dev))}
    for c in (ctx_a, ctx_b):
        c.set_stream(None)
        c.close()
    del atlas, words_a, words_b
    result["cases"].append(r)
    print(json.dumps(r), flush=True)
    assert not bits or same, f"case {name}: the two textures differ"
    assert status.cpu().numpy().tolist() == [[n, 0], [n, 0]], f"case {name}: a record was refused"

line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
