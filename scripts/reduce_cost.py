#!/usr/bin/env python3
"""What the region statistics cost (rc2dgi_reduce / rc2dgi_reduce_device, include/rc2dgi.h), per configuration, demo
scene:
  a  rc2dgi_reduce_device, one rectangle, the whole FINAL_GI, HIP events -- f32, and f16 and rgba8 beside it
  b  in the f32 process, hipMemcpyDtoDAsync of W*H*8 bytes (CW*CH*8 of the cascade texture): the copy that moves the
     traffic a's f32 read moves (8 bytes read and 8 written a texel), HIP events
  c  rc2dgi_reduce_device, 65 536 rectangles of 32 x 32 at random positions of the same texture, HIP events (the plan's
     upload is part of the call and of the time); texels/s beside a's
  d  host rc2dgi_reduce of one 64 x 64 rectangle, wall clock, against rc2dgi_download of that texture plus the numpy
     reduction of the same rectangle
Each figure is the median of --runs runs after --warmup warm-up runs, one call per pair of events on a stream of its
own.  Every (configuration, storage) is measured by a child process of its own under `timeout`; the first one that
fails ends the script, nothing more is started.  Prints one JSON line and writes it to --out (default
profiles/reduce/reduce_cost.json).
Usage: reduce_cost.py [--out FILE] [--runs 30]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reduce", "reduce_cost.json"))
ap.add_argument("--runs", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--host-runs", type=int, default=3, help="runs of the wall-clock rc2dgi_download")
ap.add_argument("--configs", default="4096x4096x6,1200x900x6")
ap.add_argument("--step-timeout", type=int, default=240, help="seconds a child process may take")
ap.add_argument("--child", default="", help="internal: WxHxN:storage, measure that and print one JSON line")
args = ap.parse_args()
assert args.runs >= 20, "the median of at least 20 runs"
NSPRITES, SPRITE = 1 << 16, 32


def measure(spec, storage):
    import torch

    from radiancecascade2dglobalillumination_amd import RC2DGI, scenes
    from radiancecascade2dglobalillumination_amd.rc2dgi import RT, stats_view

    def event_ms(stream, fn):
        """Median HIP-event time of fn() on `stream`, one call per event pair."""
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

    assert torch.cuda.is_available(), "reduce_cost.py measures on the GPU"
    W, H, N = (int(v) for v in spec.split("x"))
    ctx = RC2DGI(W, H, cascade_count=N, ray_range=2.0, storage=storage)
    cc, cp, ec, ep = scenes.demo_prims(W, H)
    ctx.paint("color", cp, cc)
    ctx.paint("emissive", ep, ec)
    ctx.do_rc2dgi()
    ctx.sync()
    CW, CH = ctx.cascade_resolution
    L, h = ctx._L, ctx._h
    vp = ctypes.c_void_p
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    texel_bytes = {"f32": 16, "f16": 8, "rgba8": 4}[storage]

    whole = np.int32([[0, 0, CW, CH]])
    out_a = torch.zeros((1, 22), dtype=torch.int32, device="cuda")

    def run_a():
        assert L.rc2dgi_reduce_device(h, RT["final_gi"], whole.ctypes.data, 1, vp(out_a.data_ptr())) == 0

    torch.cuda.synchronize()
    a_ms, a_min = event_ms(stream, run_a)
    rec = stats_view(out_a)[0]
    r = {"W": W, "H": H, "N": N, "storage": storage, "cascade": [CW, CH], "device": torch.cuda.get_device_name(0),
         "a_reduce_whole_final_gi_ms": a_ms, "a_min_ms": a_min, "a_read_MB": CW * CH * texel_bytes / 1e6,
         "a_GBps": CW * CH * texel_bytes / (a_ms * 1e6), "a_Gtexels_per_s": CW * CH / (a_ms * 1e6),
         "a_mean": [float(rec["sum"][c] / max(1, rec["texels"] - rec["nonfinite"][c])) for c in range(4)],
         "a_max": [float(v) for v in rec["max"]]}
    if storage != "f32":
        ctx.close()
        return r

    # b: the copy that moves the same traffic
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert paths, "no HIP runtime loaded"
    hip = ctypes.CDLL(sorted(paths)[0])
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    hip.hipMemcpyDtoDAsync.restype = ctypes.c_int
    nbytes = CW * CH * 8
    src = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def d2d():
        rc = hip.hipMemcpyDtoDAsync(dst.data_ptr(), src.data_ptr(), nbytes, stream.cuda_stream)
        assert rc == 0, rc

    b_ms, b_min = event_ms(stream, d2d)
    del src, dst

    # c: sprites
    rng = np.random.default_rng(1)
    sprites = np.stack([rng.integers(0, CW - SPRITE + 1, NSPRITES), rng.integers(0, CH - SPRITE + 1, NSPRITES),
                        np.full(NSPRITES, SPRITE), np.full(NSPRITES, SPRITE)], 1).astype(np.int32)
    out_c = torch.zeros((NSPRITES, 22), dtype=torch.int32, device="cuda")

    def run_c():
        assert L.rc2dgi_reduce_device(h, RT["final_gi"], sprites.ctypes.data, NSPRITES, vp(out_c.data_ptr())) == 0

    torch.cuda.synchronize()
    c_ms, c_min = event_ms(stream, run_c)
    assert (stats_view(out_c)["texels"] == SPRITE * SPRITE).all()
    ctx.set_stream(None)

    # d: the host call against the download
    x0, y0 = CW // 3, CH // 3
    one = np.int32([[x0, y0, 64, 64]])
    d_ms = wall_ms(lambda: ctx.reduce("final_gi", one), args.runs)

    def by_download():
        t = ctx.download("final_gi")[y0:y0 + 64, x0:x0 + 64].reshape(-1, 4)
        fin = np.isfinite(t)
        return np.where(fin, t, 0).sum(0, dtype=np.float64), t.min(0), t.max(0), (~fin).sum(0)

    dl_ms = wall_ms(by_download, args.host_runs)
    r.update({"b_memcpy_dtod_8_bytes_a_texel_ms": b_ms, "b_min_ms": b_min, "b_bytes": nbytes,
              "a_over_b": a_ms / b_ms, "accepted_a_le_1p5_b": bool(a_ms <= 1.5 * b_ms),
              "c_reduce_65536_sprites_32x32_ms": c_ms, "c_min_ms": c_min,
              "c_Gtexels_per_s": NSPRITES * SPRITE * SPRITE / (c_ms * 1e6), "c_ns_per_rectangle": c_ms * 1e6 / NSPRITES,
              "d_reduce_host_64x64_ms": d_ms, "d_download_and_numpy_ms": dl_ms, "d_download_over_reduce": dl_ms / d_ms})
    ctx.close()
    return r


if args.child:
    spec, storage = args.child.split(":")
    print("RESULT " + json.dumps(measure(spec, storage)), flush=True)
    sys.exit(0)

result = {"runs": args.runs, "warmup": args.warmup, "sprites": NSPRITES, "sprite": [SPRITE, SPRITE], "configs": []}
for spec in args.configs.split(","):
    for storage in ("f32", "f16", "rgba8"):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child",
               f"{spec}:{storage}", "--runs", str(args.runs), "--warmup", str(args.warmup), "--host-runs",
               str(args.host_runs)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            sys.exit(f"reduce_cost.py: {spec} {storage} ended with status {p.returncode}: nothing more is started")
        result["configs"].append(json.loads(lines[-1][7:]))
result["device"] = result["configs"][0]["device"]

line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
