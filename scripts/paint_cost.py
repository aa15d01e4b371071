#!/usr/bin/env python3
"""What painting a primitive list costs through the two painters (f32 storage, paints to COLOR with a clear), per list:
  a  rc2dgi_paint of the host list: HIP events around the call (its copies and its kernel; the call ends in a stream
     synchronise, so the events enclose all of its device work) and the wall clock until it returns
  b  rc2dgi_paint_device of the same list in device memory: HIP events around the call, and the wall clock until the
     call returns (it only enqueues) -- with the device idle, and again behind a torch.cuda._sleep of a few
     milliseconds (the call does not wait for it)
Lists: the demo's own colour list at 1200 x 900 (RenderScene, 8 primitives) and, at 4096 x 4096, 1024, 16384 and 262144
random RedrawSceneToRTs shapes (10 x 10 squares and radius-10 discs, half of each, seeded).  a and b alternate run by
run in one process; each figure is the mean and the minimum of --runs runs after --warmup warm-up runs (lists from
--few-from primitives up: --few-runs runs after one).  Both painters' textures are compared in bits once a list.
Prints one JSON line and writes it to --out.
Usage: paint_cost.py [--out FILE] [--runs 20]"""
import argparse
import ctypes
import json
import os
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
ap.add_argument("--few-from", type=int, default=100000, help="lists this long are timed --few-runs times")
ap.add_argument("--few-runs", type=int, default=4)
ap.add_argument("--lists", default="demo,1024,16384,262144")
args = ap.parse_args()


def prim_array(prims):
    arr = (rc2dgi.Prim * max(len(prims), 1))()
    for k, p in enumerate(prims):
        arr[k] = rc2dgi.Prim(int(p[0]), float(p[1]), float(p[2]), float(p[3]), float(p[4]), *(int(v) for v in p[5:9]))
    return arr


def redraw_list(W, H, n, seed=1):
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], 1)
    cols = rng.integers(0, 256, (n, 3))
    walls, lamps = scenes.redraw_prims([tuple(p) for p in pts[: n // 2]],
                                       [(tuple(p), tuple(int(v) for v in c) + (255,)) for p, c in zip(pts[n // 2:], cols)])
    both = walls + lamps
    return [both[k] for k in rng.permutation(n)]


def stats(t):
    return {"mean_ms": float(np.mean(t)), "min_ms": float(np.min(t))}


assert torch.cuda.is_available(), "paint_cost.py measures on the GPU"
result = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "few_runs": args.few_runs, "lists": []}
for spec in args.lists.split(","):
    if spec == "demo":
        W, H = 1200, 900
        clear, prims, _, _ = scenes.demo_prims(W, H)
    else:
        W = H = 4096
        clear, prims = (0, 0, 0, 255), redraw_list(W, H, int(spec))
    n = len(prims)
    runs, warmup = (args.few_runs, 1) if n >= args.few_from else (args.runs, args.warmup)
    arr = prim_array(prims)
    words = np.frombuffer(bytes(arr), np.int32).reshape(-1, 6)[:n].copy()
    cl = (ctypes.c_ubyte * 4)(*clear)
    stream = torch.cuda.Stream()
    host_ctx, dev_ctx = RC2DGI(W, H, cascade_count=2), RC2DGI(W, H, cascade_count=2)
    L, which = host_ctx._L, rc2dgi.RT["color"]
    for c in (host_ctx, dev_ctx):
        c.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        t = torch.from_numpy(words).to("cuda")
        status = torch.zeros(2, dtype=torch.int32, device="cuda")
        stream.synchronize()

        def host_paint():
            rc = L.rc2dgi_paint(host_ctx._h, which, cl, arr, n)
            assert rc == 0, rc

        def dev_paint():
            rc = L.rc2dgi_paint_device(dev_ctx._h, which, cl, ctypes.c_void_p(t.data_ptr()), n, None,
                                       ctypes.c_void_p(status.data_ptr()))
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

        for _ in range(warmup):
            host_paint()
            dev_paint()
        stream.synchronize()
        a_dev, a_wall, b_dev, b_wall, b_busy = [], [], [], [], []
        for _ in range(runs):  # the two painters alternate
            d, w = timed(host_paint)
            a_dev.append(d)
            a_wall.append(w)
            d, w = timed(dev_paint)
            b_dev.append(d)
            b_wall.append(w)
        for _ in range(runs):  # the enqueue behind a busy device
            torch.cuda._sleep(5_000_000)
            t0 = time.perf_counter()
            dev_paint()
            b_busy.append((time.perf_counter() - t0) * 1e3)
            stream.synchronize()
    same = bool(np.array_equal(host_ctx.download("color").view(np.uint32), dev_ctx.download("color").view(np.uint32)))
    batch, work = rc2dgi.paint_device_limits(W, H)
    r = {"W": W, "H": H, "list": spec, "prims": n, "runs": runs, "batch_prims": batch, "work_bytes": work,
         "status": status.cpu().numpy().tolist(), "textures_equal_in_bits": same,
         "a_paint_device_time": stats(a_dev), "a_paint_host_returns": stats(a_wall),
         "b_paint_device_device_time": stats(b_dev), "b_paint_device_host_returns": stats(b_wall),
         "b_paint_device_host_returns_busy_device": stats(b_busy),
         "b_over_a_device_time": float(np.mean(b_dev) / np.mean(a_dev))}
    for c in (host_ctx, dev_ctx):
        c.set_stream(None)
        c.close()
    result["lists"].append(r)
    print(json.dumps(r), flush=True)

line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
