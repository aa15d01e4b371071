#!/usr/bin/env python3
"""What writing an image into an input texture costs (rc2dgi_write / rc2dgi_write_device), per configuration (f32
storage, the demo scene painted, writes to COLOR):
  a  rc2dgi_write_device of the whole texture as RGBA32F / RGBA16F / RGBA8, HIP events
  b  the same for a 64 x 64 rectangle, HIP events
  c  the whole texture with RC2DGI_WRITE_BLEND, HIP events
  d  hipMemcpyDtoDAsync of the float image (W * H * 16 bytes), HIP events, measured twice: the yardstick, and how far
     two runs of it lie apart
  e  rc2dgi_upload_device of the same images (RGBA32F, RGBA8), HIP events: the whole-texture call there was before
     (rc2dgi_upload* are the code of the commit before rc2dgi_write)
  f  rc2dgi_write of the whole texture and of a 64 x 64 rectangle from host memory as RGBA8 and RGBA32F, wall clock
  g  rc2dgi_upload of the same whole images from host memory, wall clock, in the same run
Bytes moved by a device write: the source (16 / 8 / 4 a pixel) plus 16 a texel written, plus 16 a texel read with the
blend.  Each figure is the mean and the minimum of --runs runs after --warmup warm-up runs (the wall-clock routes: of
--host-runs runs after one); a .. e are timed one launch per pair of events on a stream of their own.  Prints one JSON
line and writes it to --out.
Usage: write_cost.py [--out FILE] [--runs 30]"""
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
ap.add_argument("--host-runs", type=int, default=5, help="runs of the wall-clock host routes f and g")
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


def tbps(nbytes, ms):
    return nbytes / (ms * 1e9)


assert torch.cuda.is_available(), "write_cost.py measures on the GPU"
hip = hip_runtime()
result = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "host_runs": args.host_runs, "configs": []}
for spec in args.configs.split(","):
    W, H, N = (int(v) for v in spec.split("x"))
    ctx = RC2DGI(W, H, cascade_count=N)
    cc, cp, ec, ep = scenes.demo_prims(W, H)
    ctx.paint("color", cp, cc)
    ctx.paint("emissive", ep, ec)
    ctx.sync()
    image = ctx.download("color")  # the demo scene's colour: k / 255 values, alpha 1
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    r = {"W": W, "H": H, "N": N, "storage": "f32", "texels": W * H}
    spot = (W // 2 - 32, H // 2 - 32, 64, 64)
    fbytes = W * H * 16

    # d: the yardstick, twice
    src = torch.empty(fbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty(fbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def d2d():
        rc = hip.hipMemcpyDtoDAsync(dst.data_ptr(), src.data_ptr(), fbytes, stream.cuda_stream)
        assert rc == 0, rc

    d1, d2 = event_ms(stream, d2d), event_ms(stream, d2d)
    r["d_memcpy_dtod"] = {"bytes": fbytes, "first": d1, "second": d2,
                          "runs_differ_ms": abs(d1["mean_ms"] - d2["mean_ms"]),
                          "TBps_read_and_written": tbps(2 * fbytes, min(d1["mean_ms"], d2["mean_ms"]))}
    del src, dst

    for name, tdt, ndt, px in FORMATS:
        host_whole = (np.rint(image * 255).astype(np.uint8) if px == 4 else image.astype(ndt))
        host_small = np.ascontiguousarray(host_whole[spot[1]:spot[1] + 64, spot[0]:spot[0] + 64])
        whole = torch.from_numpy(host_whole).to("cuda")
        small = torch.from_numpy(host_small).to("cuda")
        torch.cuda.synchronize()
        a = event_ms(stream, lambda: ctx.write("color", whole))
        b = event_ms(stream, lambda: ctx.write("color", small, spot))
        c = event_ms(stream, lambda: ctx.write("color", whole, blend=True))
        moved = W * H * (px + 16)
        r[name] = {"image_bytes": W * H * px, "a_write_device_whole": a, "b_write_device_64x64": b,
                   "c_write_device_whole_blend": c, "a_bytes_moved": moved, "a_TBps": tbps(moved, a["mean_ms"]),
                   "c_bytes_moved": moved + W * H * 16, "c_TBps": tbps(moved + W * H * 16, c["mean_ms"]),
                   "a_over_d": a["mean_ms"] / min(d1["mean_ms"], d2["mean_ms"])}
        if px != 8:
            e = event_ms(stream, lambda: ctx.upload("color", whole))
            r[name]["e_upload_device_whole"] = e
            r[name]["a_over_e"] = a["mean_ms"] / e["mean_ms"]
            ctx.sync()
            f = wall_ms(lambda: ctx.write("color", host_whole), args.host_runs)
            fs = wall_ms(lambda: ctx.write("color", host_small, spot), args.host_runs)
            g = wall_ms(lambda: ctx.upload("color", host_whole), args.host_runs)
            r[name].update({"f_write_host_whole": f, "f_write_host_64x64": fs, "g_upload_host_whole": g,
                            "g_over_f": g["mean_ms"] / f["mean_ms"]})
        ctx.sync()
        del whole, small
    ctx.set_stream(None)
    ctx.close()
    result["configs"].append(r)

line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
