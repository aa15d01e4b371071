#!/usr/bin/env python3
"""What the display frame costs (rc2dgi_compose / rc2dgi_compose_device), per configuration:
  a  rc2dgi_compose_device of the display layout (main blit + seven thumbnails), HIP events
  b  the same with view 0 only (the main blit), HIP events
  c  hipMemcpyDtoDAsync of W*H*20 bytes, the bytes the blit moves a pixel (16 read + 4 written), HIP events
     (c_half: W*H*10 bytes, a copy that moves W*H*20 bytes of traffic in all)
  d  rc2dgi_compose to host memory, wall clock
  e  the eight rc2dgi_download calls it replaces, wall clock
Each figure is the median of --runs runs after --warmup warm-up runs; a, b and c are timed one launch per pair of
events on a stream of their own.  Prints one JSON line and writes it to --out.
Usage: present_cost.py [--out FILE] [--runs 30] [--only-kernel]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from radiancecascade2dglobalillumination_amd import RC2DGI, display_layout, scenes  # noqa: E402
from radiancecascade2dglobalillumination_amd.rc2dgi import RT  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--runs", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--host-runs", type=int, default=3, help="runs of the wall-clock host routes d and e")
ap.add_argument("--only-kernel", action="store_true", help="a and b only (A/B of two builds)")
ap.add_argument("--configs", default="4096x4096x6,1200x900x6")
args = ap.parse_args()
assert args.runs >= 20, "the median of at least 20 runs"


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
    """Median HIP-event time of fn() on `stream`, one launch per event pair."""
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
    return float(np.median(t)), float(np.min(t))


def wall_ms(fn, runs):
    fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


assert torch.cuda.is_available(), "present_cost.py measures on the GPU"
hip = hip_runtime()
result = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "configs": []}
for spec in args.configs.split(","):
    W, H, N = (int(v) for v in spec.split("x"))
    ctx = RC2DGI(W, H, cascade_count=N)
    cc, cp, ec, ep = scenes.demo_prims(W, H)
    ctx.paint("color", cp, cc)
    ctx.paint("emissive", ep, ec)
    ctx.do_rc2dgi()
    ctx.sync()
    views = display_layout(W, H)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    frame = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    a_ms, a_min = event_ms(stream, lambda: ctx.compose_into(frame, views))
    b_ms, b_min = event_ms(stream, lambda: ctx.compose_into(frame, views[:1]))
    r = {"W": W, "H": H, "N": N, "storage": "f32", "a_compose_layout_ms": a_ms, "b_compose_blit_ms": b_ms,
         "a_min_ms": a_min, "b_min_ms": b_min, "blit_GBps": W * H * 20 / (b_ms * 1e6)}
    if not args.only_kernel:
        nbytes = W * H * 20
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def d2d(n):
            rc = hip.hipMemcpyDtoDAsync(dst.data_ptr(), src.data_ptr(), n, stream.cuda_stream)
            assert rc == 0, rc

        c_ms, _ = event_ms(stream, lambda: d2d(nbytes))
        ch_ms, _ = event_ms(stream, lambda: d2d(nbytes // 2))
        d_ms = wall_ms(lambda: ctx.compose(views), args.host_runs)
        names = {v: k for k, v in RT.items()}
        e_ms = wall_ms(lambda: [ctx.download(names[v.which], np.uint8) for v in views], args.host_runs)
        r.update({"c_memcpy_dtod_ms": c_ms, "c_half_memcpy_dtod_ms": ch_ms, "d_compose_host_ms": d_ms,
                  "e_eight_downloads_ms": e_ms, "b_over_c": b_ms / c_ms, "b_over_c_half": b_ms / ch_ms,
                  "a_minus_b_ms": a_ms - b_ms, "e_over_d": e_ms / d_ms})
    ctx.set_stream(None)
    ctx.close()
    result["configs"].append(r)

line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
