#!/usr/bin/env python3
"""What rc2dgi_gradients_device costs at 4096 x 4096 (f32 storage, paints to EMISSIVE with a clear, the default plan),
the method of scripts/shapes_cost.py: HIP events around the call, the wall clock until the call returns (it only
enqueues), the two callers of a row alternating run by run in one process, mean and [min - max] of --runs runs after
--warmup.  The yardstick of rows b and c is rc2dgi_shapes_device on the same shapes in the same run; the two textures
are compared in bits BEFORE anything is timed.
  a_one          one TRIANGLE of 4 pixels: what a call costs at this size whatever it draws
  b_small16384   16384 ten-pixel equal-colour CIRCLEs and RECTs (radius-5 discs and 10 x 10 squares, half of each)
                 through rc2dgi_shapes_device (s) and, as gradients_from_shapes records, through
                 rc2dgi_gradients_device (g)
  c_discs1024    1024 equal-colour CIRCLEs of radius 100, the raster-dominated case, through both
  d_lights1024   1024 soft_lights of radius 100 (g alone)
  e_lines16384   16384 gradient LINEs of length 64, thick 2, random direction (g alone)
Prints one JSON line a row and writes the whole result to --out, with the name of the machine it ran on.
Usage: gradients_cost.py [--out FILE] [--runs 20]"""
import argparse
import json
import os
import platform
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
ap.add_argument("--cases", default="a_one,b_small16384,c_discs1024,d_lights1024,e_lines16384")
args = ap.parse_args()

W = H = 4096
CLEAR = (0, 0, 0, 255)
f32 = np.float32


def stats(t):
    return {"mean_ms": float(np.mean(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t))}


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to("cuda")


assert torch.cuda.is_available(), "gradients_cost.py measures on the GPU"
result = {"device": torch.cuda.get_device_name(0), "box": platform.node(), "W": W, "H": H, "runs": args.runs,
          "warmup": args.warmup, "which": "emissive", "clear": list(CLEAR), "cases": []}
stream = torch.cuda.Stream()
for case in args.cases.split(","):
    rng = np.random.default_rng(7)
    ctx_s, ctx_g = RC2DGI(W, H, cascade_count=2), RC2DGI(W, H, cascade_count=2)
    for c in (ctx_s, ctx_g):
        c.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        status = torch.zeros((2, 2), dtype=torch.int32, device="cuda")
        shapes = None
        if case == "a_one":
            n = 1
            grads = rc2dgi.pack_gradients(dev([rc2dgi.GRAD_TRIANGLE], np.int32), dev([[100, 100, 104, 100, 100, 102]], f32),
                                          dev([[[255, 0, 0, 255], [0, 255, 0, 255], [0, 0, 255, 255], [0, 0, 0, 0]]], np.uint8))
        elif case in ("b_small16384", "c_discs1024"):
            n = 16384 if case.startswith("b") else 1024
            p = rng.uniform(0, W, (n, 2))
            v6 = np.zeros((n, 6), f32)
            if case.startswith("b"):  # ten-pixel discs and squares, half of each, in a seeded order
                kind = rng.permutation(np.arange(n) % 2)
                disc = kind == rc2dgi.SHAPE_CIRCLE
                v6[disc, :3] = np.concatenate([p[disc], np.full((disc.sum(), 1), 5.0)], 1)
                v6[~disc, :4] = np.concatenate([p[~disc] - 5.0, np.full(((~disc).sum(), 2), 10.0)], 1)
            else:
                kind = np.full(n, rc2dgi.SHAPE_CIRCLE)
                v6[:, :3] = np.concatenate([p, np.full((n, 1), 100.0)], 1)
            rgba = rng.integers(0, 256, (n, 4))
            rgba[:, 3] = rng.integers(60, 256, n)
            shapes = rc2dgi.pack_shapes(dev(kind, np.int32), dev(v6, f32), dev(rgba, np.uint8))
            grads = rc2dgi.gradients_from_shapes(shapes)
        elif case == "d_lights1024":
            n = 1024
            grads = rc2dgi.soft_lights(dev(rng.uniform(0, W, (n, 2)), f32), dev(np.full(n, 100.0), f32),
                                       dev(rng.integers(0, 256, (n, 3)), np.uint8), dev(rng.uniform(0.5, 8, n), f32))
        else:  # e_lines16384
            n = 16384
            p, ang = rng.uniform(0, W, (n, 2)), rng.uniform(0, 2 * np.pi, n)
            v6 = np.stack([p[:, 0], p[:, 1], p[:, 0] + 64 * np.cos(ang), p[:, 1] + 64 * np.sin(ang), np.full(n, 2.0),
                           np.zeros(n)], 1)
            grads = rc2dgi.pack_gradients(dev(np.full(n, rc2dgi.GRAD_LINE), np.int32), dev(v6, f32),
                                          dev(rng.integers(0, 256, (n, 4, 4)), np.uint8), dev(rng.uniform(0.5, 8, n), f32))
        call_s = None
        if shapes is not None:
            call_s = lambda: ctx_s.shapes_device("emissive", shapes, CLEAR, None, status[0])  # noqa: E731
        call_g = lambda: ctx_g.gradients_device("emissive", grads, CLEAR, None, status[1])  # noqa: E731
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

        calls = ([call_s] if call_s else []) + [call_g]
        for _ in range(args.warmup):
            for fn in calls:
                fn()
        stream.synchronize()
        r = {"case": case, "records": n, "paint_tile_h": ctx_g.get_tuning("paint_tile_h"),
             "paint_batch": ctx_g.get_tuning("paint_batch")}
        if call_s:  # the equal-bit rows: asserted equal before anything is timed
            a, b = ctx_s.download("emissive"), ctx_g.download("emissive")
            same = bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
            assert same, f"{case}: gradients_device and shapes_device left different bits"
            r["textures_equal_in_bits"] = same
            r["texels_drawn"] = int(np.count_nonzero(np.any(b != (f32(CLEAR) / f32(255)), axis=-1)))
        dev_t = {id(fn): [] for fn in calls}
        wall_t = {id(fn): [] for fn in calls}
        for _ in range(args.runs):  # the two callers alternate
            for fn in calls:
                d, w = timed(fn)
                dev_t[id(fn)].append(d)
                wall_t[id(fn)].append(w)
    r["status"] = status.cpu().numpy().tolist()
    r["g_gradients_device_device_time"] = stats(dev_t[id(call_g)])
    r["g_gradients_device_host_returns"] = stats(wall_t[id(call_g)])
    if call_s:
        r["s_shapes_device_device_time"] = stats(dev_t[id(call_s)])
        r["s_shapes_device_host_returns"] = stats(wall_t[id(call_s)])
        r["g_over_s_device_time"] = float(np.mean(dev_t[id(call_g)]) / np.mean(dev_t[id(call_s)]))
    for c in (ctx_s, ctx_g):
        c.set_stream(None)
        c.close()
    result["cases"].append(r)
    print(json.dumps(r), flush=True)

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
