#!/usr/bin/env python3
"""What rc2dgi_shapes_device costs at 4096 x 4096 (f32 storage, paints to COLOR with a clear), the method of
scripts/paint_cost.py: HIP events around the call, the wall clock until the call returns (it only enqueues), the two
callers of a comparison alternating run by run in one process, mean and minimum of --runs runs after --warmup.
  one          one TRIANGLE of a few pixels: what a call costs at this size whatever it draws (b alone)
  redraw1024, redraw16384  random RedrawSceneToRTs shapes (10 x 10 squares and radius-10 discs, half of each, seeded)
               through rc2dgi_paint_device (a) and, as RECT / CIRCLE records, through rc2dgi_shapes_device (b); the
               two textures are compared in bits
  lines16384   16384 LINEs of length 64, thick 2, random direction (b alone)
  tris16384    16384 random TRIANGLEs of about 16 pixels (b alone)
  diagonal     one LINE thick 4 along the whole diagonal (b) against the same quad as one rc2dgi_sprites_xf_device
               sprite from a 1 x 1 white atlas (a), which is binned by its box: what the tile rejection buys
Prints one JSON line a case and writes the whole result to --out, with the name of the machine it ran on.
Usage: shapes_cost.py [--out FILE] [--runs 20]"""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from radiancecascade2dglobalillumination_amd import RC2DGI, rc2dgi, scenes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--runs", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--cases", default="one,redraw1024,redraw16384,lines16384,tris16384,diagonal")
args = ap.parse_args()

W = H = 4096
CLEAR = (0, 0, 0, 255)
f32 = np.float32


def redraw_words(n, seed=1):
    """paint_cost.py's list, as (n, 6) rc2dgi_prim words"""
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], 1)
    cols = rng.integers(0, 256, (n, 3))
    walls, lamps = scenes.redraw_prims([tuple(p) for p in pts[: n // 2]],
                                       [(tuple(p), tuple(int(v) for v in c) + (255,)) for p, c in zip(pts[n // 2:], cols)])
    both = walls + lamps
    prims = [both[k] for k in rng.permutation(n)]
    arr = (rc2dgi.Prim * n)()
    for k, p in enumerate(prims):
        arr[k] = rc2dgi.Prim(int(p[0]), float(p[1]), float(p[2]), float(p[3]), float(p[4]), *(int(v) for v in p[5:9]))
    return np.frombuffer(bytes(arr), np.int32).reshape(-1, 6).copy()


def shape_words(kind, v, rgba):
    n = len(v)
    out = np.zeros((n, 8), np.int32)
    out[:, 0] = kind
    vv = np.zeros((n, 6), f32)
    vv[:, :v.shape[1]] = v
    out[:, 1:7] = vv.view(np.int32)
    out[:, 7] = np.ascontiguousarray(rgba, np.uint8).view(np.int32)[:, 0]
    return out


def stats(t):
    return {"mean_ms": float(np.mean(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t))}


assert torch.cuda.is_available(), "shapes_cost.py measures on the GPU"
result = {"device": torch.cuda.get_device_name(0), "box": platform.node(), "W": W, "H": H, "runs": args.runs,
          "cases": []}
stream = torch.cuda.Stream()
for case in args.cases.split(","):
    rng = np.random.default_rng(7)
    ctx_a, ctx_b = RC2DGI(W, H, cascade_count=2), RC2DGI(W, H, cascade_count=2)
    for c in (ctx_a, ctx_b):
        c.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        status = torch.zeros((2, 2), dtype=torch.int32, device="cuda")
        call_a = None
        if case.startswith("redraw"):
            n = int(case[6:])
            prims = torch.from_numpy(redraw_words(n)).to("cuda")
            shapes = rc2dgi.shapes_from_prims(prims)
            call_a, name_a = (lambda: ctx_a.paint_device("color", prims, CLEAR, None, status[0])), "paint_device"
        elif case == "one":
            n = 1
            shapes = torch.from_numpy(shape_words(rc2dgi.SHAPE_TRIANGLE, f32([[100, 100, 104, 101, 101, 104]]),
                                                  np.array([[255, 255, 255, 255]], np.uint8))).to("cuda")
        elif case.startswith("lines"):
            n = int(case[5:])
            p, ang = rng.uniform(0, W, (n, 2)), rng.uniform(0, 2 * np.pi, n)
            v = np.stack([p[:, 0], p[:, 1], p[:, 0] + 64 * np.cos(ang), p[:, 1] + 64 * np.sin(ang), np.full(n, 2.0)], 1)
            shapes = torch.from_numpy(shape_words(rc2dgi.SHAPE_LINE, v.astype(f32), rng.integers(0, 256, (n, 4)))).to("cuda")
        elif case.startswith("tris"):
            n = int(case[4:])
            p = rng.uniform(0, W, (n, 1, 2)) + rng.uniform(-8, 8, (n, 3, 2))
            shapes = torch.from_numpy(shape_words(rc2dgi.SHAPE_TRIANGLE, p.reshape(n, 6).astype(f32),
                                                  rng.integers(0, 256, (n, 4)))).to("cuda")
        else:  # the diagonal: LINE (0, 0) -> (W, H) thick 4, and the same quad as a sprite of a 1 x 1 white atlas
            n = 1
            white = np.array([[255, 255, 255, 255]], np.uint8)
            shapes = torch.from_numpy(shape_words(rc2dgi.SHAPE_LINE, f32([[0, 0, W, H, 4]]), white)).to("cuda")
            atlas = torch.full((1, 1, 4), 255, dtype=torch.uint8, device="cuda")
            r = 2.0 / np.sqrt(2.0)  # the half thickness along each axis: s0 = (r, -r), s1 = (-r, r)
            xf = rc2dgi.pack_sprites_xf(torch.tensor([[0, 0, 1, 1]], dtype=torch.int32, device="cuda"),
                                        torch.tensor([[r, -r]], dtype=torch.float32, device="cuda"),
                                        torch.tensor([[float(W), float(H)]], dtype=torch.float32, device="cuda"),
                                        torch.tensor([[-2 * r, 2 * r]], dtype=torch.float32, device="cuda"))
            call_a = lambda: ctx_a.sprites_xf_device("color", atlas, xf, CLEAR, None, status[0])  # noqa: E731
            name_a = "sprites_xf_device"
        call_b = lambda: ctx_b.shapes_device("color", shapes, CLEAR, None, status[1])  # noqa: E731
        stream.synchronize()

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            fn()
            wall = (time.perf_counter() - t0) * 1e3
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1), wall

        calls = ([call_a] if call_a else []) + [call_b]
        for _ in range(args.warmup):
            for fn in calls:
                fn()
        stream.synchronize()
        dev = {id(fn): [] for fn in calls}
        wall = {id(fn): [] for fn in calls}
        for _ in range(args.runs):  # the two callers alternate
            for fn in calls:
                d, w = timed(fn)
                dev[id(fn)].append(d)
                wall[id(fn)].append(w)
    r = {"case": case, "shapes": n, "status": status.cpu().numpy().tolist(),
         "paint_tile_h": ctx_b.get_tuning("paint_tile_h"), "paint_batch": ctx_b.get_tuning("paint_batch"),
         "b_shapes_device_device_time": stats(dev[id(call_b)]), "b_shapes_device_host_returns": stats(wall[id(call_b)])}
    if call_a:
        r["a_call"] = name_a
        r["a_device_time"] = stats(dev[id(call_a)])
        r["a_host_returns"] = stats(wall[id(call_a)])
        r["b_over_a_device_time"] = float(np.mean(dev[id(call_b)]) / np.mean(dev[id(call_a)]))
    if case.startswith("redraw"):
        same = bool(np.array_equal(ctx_a.download("color").view(np.uint32), ctx_b.download("color").view(np.uint32)))
        assert same, f"{case}: shapes_device and paint_device left different bits"
        r["textures_equal_in_bits"] = same
    elif call_a:  # the diagonal: how many texels each call touched (the two coverage rules differ at the rim)
        a, b = ctx_a.download("color"), ctx_b.download("color")
        r["texels_drawn"] = {"a": int(np.count_nonzero(a[..., 0])), "b": int(np.count_nonzero(b[..., 0]))}
    for c in (ctx_a, ctx_b):
        c.set_stream(None)
        c.close()
    result["cases"].append(r)
    print(json.dumps(r), flush=True)

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
