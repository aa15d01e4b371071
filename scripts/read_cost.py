#!/usr/bin/env python3
"""What reading a texture as an image costs (rc2dgi_read / rc2dgi_read_device), per configuration (f32 storage):
  a  rc2dgi_read_device of the whole FINAL_GI as RGBA32F / RGBA16F / RGBA8, HIP events
  b  the same for a 64 x 64 rectangle, HIP events
  c  hipMemcpyDtoDAsync of as many bytes as each image of (a) holds, HIP events (the yardstick of present_cost.py)
  d  rc2dgi_read of the whole FINAL_GI to host memory as RGBA32F and RGBA16F, wall clock
  e  rc2dgi_download of FINAL_GI, wall clock, in the same run
Each figure is the mean and the minimum of --runs runs after --warmup warm-up runs; a, b and c are timed one launch per
pair of events on a stream of their own.  Prints one JSON line and writes it to --out.
Usage: read_cost.py [--out FILE] [--runs 30]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from radiancecascade2dglobalillumination_amd import RC2DGI, scenes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--runs", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--host-runs", type=int, default=5, help="runs of the wall-clock host routes d and e")
ap.add_argument("--configs", default="4096x4096x6,1200x900x6")
args = ap.parse_args()
FORMATS = [("rgba32f", torch.float32, np.float32, 16), ("rgba16f", torch.float16, np.float16, 8),
           ("rgba8", torch.uint8, np.uint8, 4)]


def hip_runtime():
    """The HIP runtime this process already holds (torch's), for hipMemcpyDtoDAsync."""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert paths, "no HIP runtime loaded"
    lib = ctypes.CDLL(sorted(paths)[0])
    lib.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.hipMemcpyDtoDAsync.restype = ctypes.c_int
    return lib


def event_ms(stream, fn):
    """Mean and minimum HIP-event time of fn() on `stream`, one launch per event pair."""
    with torch.cuda.stream(stream):
        for _ in range(args.warmup):
            fn()
        stream.synchronize()
        t = []
        for _ in range(args.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
    return {"mean_ms": float(np.mean(t)), "min_ms": float(np.min(t))}


def wall_ms(fn, runs):
    fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"mean_ms": float(np.mean(t)), "min_ms": float(np.min(t))}


assert torch.cuda.is_available(), "read_cost.py measures on the GPU"
hip = hip_runtime()
result = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "host_runs": args.host_runs, "configs": []}
for spec in args.configs.split(","):
    W, H, N = (int(v) for v in spec.split("x"))
    ctx = RC2DGI(W, H, cascade_count=N)
    cc, cp, ec, ep = scenes.demo_prims(W, H)
    ctx.paint("color", cp, cc)
    ctx.paint("emissive", ep, ec)
    ctx.do_rc2dgi()
    ctx.sync()
    cw, ch = ctx.cascade_resolution
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    r = {"W": W, "H": H, "N": N, "storage": "f32", "cascade_w": cw, "cascade_h": ch}
    spot = (cw // 2 - 32, ch // 2 - 32, 64, 64)
    for name, tdt, ndt, px in FORMATS:
        whole = torch.empty((ch, cw, 4), dtype=tdt, device="cuda")
        small = torch.empty((64, 64, 4), dtype=tdt, device="cuda")
        nbytes = cw * ch * px
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def d2d():
            rc = hip.hipMemcpyDtoDAsync(dst.data_ptr(), src.data_ptr(), nbytes, stream.cuda_stream)
            assert rc == 0, rc

        a = event_ms(stream, lambda: ctx.read_into(whole, "final_gi"))
        b = event_ms(stream, lambda: ctx.read_into(small, "final_gi", spot))
        c = event_ms(stream, d2d)
        r[name] = {"image_bytes": nbytes, "a_read_device_whole": a, "b_read_device_64x64": b, "c_memcpy_dtod": c,
                   "a_over_c": a["mean_ms"] / c["mean_ms"], "a_GBps_read_and_written": (cw * ch * 16 + nbytes) / (a["mean_ms"] * 1e6)}
        if px != 4:
            r[name]["d_read_host_whole"] = wall_ms(lambda: ctx.read("final_gi", dtype=ndt), args.host_runs)
        del whole, small, src, dst
    e = wall_ms(lambda: ctx.download("final_gi"), args.host_runs)
    r["e_download"] = e
    r["e_over_d_rgba32f"] = e["mean_ms"] / r["rgba32f"]["d_read_host_whole"]["mean_ms"]
    r["e_over_d_rgba16f"] = e["mean_ms"] / r["rgba16f"]["d_read_host_whole"]["mean_ms"]
    ctx.set_stream(None)
    ctx.close()
    result["configs"].append(r)

line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
