#!/usr/bin/env python3
"""What the queries cost (rc2dgi_sample / rc2dgi_raycast, include/rc2dgi.h), per configuration, demo scene, f32:
  a  rc2dgi_sample_device, 2^20 uniformly random points, FINAL_GI LINEAR, HIP events
  b  rc2dgi_sample_device, COLOR POINT, the W*H texel centres in row-major order, HIP events
  c  rc2dgi_raycast_device, 2^20 rays drawn at random from level 4's own ray set (origins, directions and interval
     as RadianceCascades.fs main() derives them), HIP events; c_rows: the first 2^20 rays of that set in texel order
  d  host rc2dgi_sample of one point and of 1000 points, wall clock
and beside them what they replace or resemble:
  rc2dgi_download of the same texture, wall clock (the only other route to those values)
  hipMemcpyDtoDAsync of W*H*40 bytes, the bytes b moves a point (8 + 16 read, 16 written), HIP events
     (half: W*H*20 bytes, a copy that moves W*H*40 bytes of traffic in all)
  level 4's time from rc2dgi_pass_times mode 1, divided by its ray count
Each figure is the median of --runs runs after --warmup warm-up runs; a, b, c and the copies are timed one launch
per pair of events on a stream of their own.  Prints one JSON line and writes it to --out (default
profiles/query/query_cost.json).
Usage: query_cost.py [--out FILE] [--runs 30]"""
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
from radiancecascade2dglobalillumination_amd.rc2dgi import FILTER_LINEAR, FILTER_POINT, RT  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "query",
                                             "query_cost.json"))
ap.add_argument("--runs", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--host-runs", type=int, default=3, help="runs of the wall-clock rc2dgi_download")
ap.add_argument("--configs", default="4096x4096x6,1200x900x6")
ap.add_argument("--level", type=int, default=4)
args = ap.parse_args()
assert args.runs >= 20, "the median of at least 20 runs"
f32 = np.float32
NQ = 1 << 20


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


def level_rays(N, level, CW, CH, ray_range, i, j, r):
    """Ray r of the probe at cascade texel (i, j) of a level, as RadianceCascades.fs:96-121 derives it (float32)."""
    CRx, CRy, bsc = f32(CW), f32(CH), 1 << level
    max_value = (1 << (N * 2)) - 1
    t0 = (f32((1 << (level * 2)) - 1) / f32(max_value)) * f32(ray_range)
    t1 = (f32((1 << (level * 2 + 2)) - 1) / f32(max_value)) * f32(ray_range)
    bdx, bdy = CRx / f32(bsc), CRy / f32(bsc)
    pix = np.floor(((i.astype(f32) + f32(0.5)) / CRx) * CRx)
    piy = np.floor(((j.astype(f32) + f32(0.5)) / CRy) * CRy)
    blkx, blky = np.floor(pix / bdx), np.floor(piy / bdy)
    cx, cy = pix - bdx * blkx, piy - bdy * blky
    block = (blkx + blky * f32(bsc) + f32(0.5)).astype(np.int64)
    angle = ((block * 4 + r).astype(f32) + f32(0.5)) * (f32(6.28318530718) / f32(bsc * bsc * 4))
    rays = np.empty((len(i), 6), f32)
    rays[:, 0] = ((cx + f32(0.5)) * f32(bsc)) / CRx
    rays[:, 1] = ((cy + f32(0.5)) * f32(bsc)) / CRy
    rays[:, 2] = np.cos(angle.astype(np.float64)).astype(f32)
    rays[:, 3] = np.sin(angle.astype(np.float64)).astype(f32)
    rays[:, 4], rays[:, 5] = t0, t1
    return rays


assert torch.cuda.is_available(), "query_cost.py measures on the GPU"
hip = hip_runtime()
result = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "queries": NQ, "configs": []}
for spec in args.configs.split(","):
    W, H, N = (int(v) for v in spec.split("x"))
    ray_range = 2.0
    ctx = RC2DGI(W, H, cascade_count=N, ray_range=ray_range)
    cc, cp, ec, ep = scenes.demo_prims(W, H)
    ctx.paint("color", cp, cc)
    ctx.paint("emissive", ep, ec)
    ctx.set_timing(1)
    lv = []
    for _ in range(5):
        ctx.do_rc2dgi()
        ctx.sync()
        lv.append(ctx.pass_times(levels=N)["levels"][args.level])
    ctx.set_timing(0)
    ctx.do_rc2dgi()
    ctx.sync()
    CW, CH = ctx.cascade_resolution
    level_ray_count = CW * CH * 4
    L, h = ctx._L, ctx._h
    rng = np.random.default_rng(1)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    vp = ctypes.c_void_p

    # a: random points, the final GI with the LINEAR filter
    uv_a = torch.from_numpy(rng.random((NQ, 2), dtype=f32)).cuda()
    out_a = torch.empty((NQ, 4), dtype=torch.float32, device="cuda")

    def run_a():
        assert L.rc2dgi_sample_device(h, RT["final_gi"], FILTER_LINEAR, vp(uv_a.data_ptr()), NQ, vp(out_a.data_ptr())) == 0

    # b: every texel centre of colorRT in row-major order, POINT
    u = (np.arange(W, dtype=f32) + f32(0.5)) / f32(W)
    v = (np.arange(H, dtype=f32) + f32(0.5)) / f32(H)
    uv_b = torch.from_numpy(np.ascontiguousarray(np.stack(np.broadcast_arrays(u[None, :], v[:, None]), -1).reshape(-1, 2))).cuda()
    nb = W * H
    out_b = torch.empty((nb, 4), dtype=torch.float32, device="cuda")

    def run_b():
        assert L.rc2dgi_sample_device(h, RT["color"], FILTER_POINT, vp(uv_b.data_ptr()), nb, vp(out_b.data_ptr())) == 0

    # c: rays of level `level`: a random draw, and the first NQ in texel order
    nc = min(NQ, level_ray_count)
    pick = rng.integers(0, level_ray_count, nc)
    rows = np.arange(nc)
    rays_c, rays_rows = (torch.from_numpy(level_rays(N, args.level, CW, CH, ray_range, (k // 4) % CW, k // (4 * CW), k % 4)).cuda()
                         for k in (pick, rows))
    hits = torch.empty((nc, 11), dtype=torch.int32, device="cuda")

    def run_c(rays):
        assert L.rc2dgi_raycast_device(h, vp(rays.data_ptr()), nc, vp(hits.data_ptr())) == 0

    torch.cuda.synchronize()
    a_ms, a_min = event_ms(stream, run_a)
    b_ms, b_min = event_ms(stream, run_b)
    c_ms, c_min = event_ms(stream, lambda: run_c(rays_c))
    st = hits[:, 0].cpu().numpy()
    steps = hits[:, 1].cpu().numpy()
    cr_ms, cr_min = event_ms(stream, lambda: run_c(rays_rows))
    steps_rows = hits[:, 1].cpu().numpy()

    nbytes = nb * 40
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def d2d(n):
        rc = hip.hipMemcpyDtoDAsync(dst.data_ptr(), src.data_ptr(), n, stream.cuda_stream)
        assert rc == 0, rc

    m_ms, _ = event_ms(stream, lambda: d2d(nbytes))
    mh_ms, _ = event_ms(stream, lambda: d2d(nbytes // 2))
    del src, dst
    ctx.set_stream(None)
    one, thousand = rng.random((1, 2), dtype=f32), rng.random((1000, 2), dtype=f32)
    d1_ms = wall_ms(lambda: ctx.sample("final_gi", one, FILTER_LINEAR), args.runs)
    d1000_ms = wall_ms(lambda: ctx.sample("final_gi", thousand, FILTER_LINEAR), args.runs)
    dl_ms = wall_ms(lambda: ctx.download("final_gi"), args.host_runs)
    level_ms = float(np.median(lv))
    result["configs"].append({
        "W": W, "H": H, "N": N, "storage": "f32", "cascade": [CW, CH],
        "a_sample_final_gi_linear_ms": a_ms, "a_min_ms": a_min, "a_ns_per_point": a_ms * 1e6 / NQ,
        "b_sample_color_point_ms": b_ms, "b_min_ms": b_min, "b_points": nb, "b_GBps": nb * 40 / (b_ms * 1e6),
        "c_raycast_level_random_ms": c_ms, "c_min_ms": c_min, "c_rays": nc, "c_ns_per_ray": c_ms * 1e6 / nc,
        "c_mean_steps": float(steps.mean()), "c_max_steps": int(steps.max()),
        "c_exits": {str(s): int(np.count_nonzero(st == s)) for s in range(-1, 5)},
        "c_rows_raycast_level_in_order_ms": cr_ms, "c_rows_min_ms": cr_min, "c_rows_ns_per_ray": cr_ms * 1e6 / nc,
        "c_rows_mean_steps": float(steps_rows.mean()),
        "d_sample_host_1_ms": d1_ms, "d_sample_host_1000_ms": d1000_ms,
        "download_final_gi_ms": dl_ms, "download_over_d1": dl_ms / d1_ms,
        "memcpy_dtod_b_bytes_ms": m_ms, "memcpy_dtod_half_ms": mh_ms, "b_over_memcpy": b_ms / m_ms,
        "b_over_memcpy_half": b_ms / mh_ms,
        "level": args.level, "level_ms": level_ms, "level_rays": level_ray_count,
        "level_ns_per_ray": level_ms * 1e6 / level_ray_count})
    ctx.close()

line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
