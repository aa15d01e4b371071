#!/usr/bin/env python3
"""What the edge tables cost (rc2dgi_compose_tone / rc2dgi_histogram, include/rc2dgi.h), per configuration, demo scene,
f32:
  a  rc2dgi_compose_tone_device of the display layout, the main blit with an exposure and an sRGB curve, HIP events
  b  rc2dgi_compose_device of the same views in the same run (k_present, the kernel rc2dgi_compose keeps); the bar is
     a <= 2 b.  Beside them the host call rc2dgi_compose_tone (wall clock) against rc2dgi_download of COLOR plus a numpy
     tone map (searchsorted over the same edges)
  c  rc2dgi_histogram_device, luma, 256 log-spaced edges, one rectangle: the whole FINAL_GI, HIP events
  d  rc2dgi_reduce_device of the same rectangle in the same run; the bar is c <= 2 d
  e  c on a constant texture of the same size and format (COLOR of a second context): every texel in one bin; e / c
  f  rc2dgi_histogram_device of 65 536 rectangles of 32 x 32 at random positions, the same edges (the plan's upload is
     part of the call and of the time)
  g  host rc2dgi_histogram of one 64 x 64 rectangle, wall clock, against rc2dgi_download of that texture plus
     numpy.histogram of the same rectangle
b and d are measured before and after a and c (b0 / b1, d0 / d1), so that drift shows.  Each figure is the median of
--runs runs after --warmup warm-up runs, one call per pair of events on a stream of its own.  Every configuration is
measured by a child process of its own under `timeout`; the first one that fails ends the script, nothing more is
started.  Prints one JSON line and writes it to --out (default profiles/tone/tone_cost.json).
Usage: tone_cost.py [--out FILE] [--runs 30]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tone", "tone_cost.json"))
ap.add_argument("--runs", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--host-runs", type=int, default=3, help="runs of the wall-clock rc2dgi_download")
ap.add_argument("--configs", default="4096x4096x6,1200x900x6")
ap.add_argument("--step-timeout", type=int, default=240, help="seconds a child process may take")
ap.add_argument("--child", default="", help="internal: WxHxN, measure that and print one JSON line")
args = ap.parse_args()
assert args.runs >= 20, "the median of at least 20 runs"
NSPRITES, SPRITE, EXPOSURE = 1 << 16, 32, 1.6


def srgb(x):
    return np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(np.maximum(x, 0.0031308), 1 / 2.4) - 0.055)


def measure(spec):
    import torch

    from radiancecascade2dglobalillumination_amd import RC2DGI, scenes
    from radiancecascade2dglobalillumination_amd import rc2dgi as R

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

    assert torch.cuda.is_available(), "tone_cost.py measures on the GPU"
    W, H, N = (int(v) for v in spec.split("x"))
    ctx = RC2DGI(W, H, cascade_count=N, ray_range=2.0, storage="f32")
    cc, cp, ec, ep = scenes.demo_prims(W, H)
    ctx.paint("color", cp, cc)
    ctx.paint("emissive", ep, ec)
    ctx.do_rc2dgi()
    ctx.sync()
    CW, CH = ctx.cascade_resolution
    curve = R.curve_from(srgb)
    ctx.set_curve(1, curve)
    views = R.display_layout(W, H)
    tones = [(EXPOSURE, 1)] + [(1.0, 0)] * (len(views) - 1)
    edges = (2.0 ** np.linspace(-16, 16, 256)).astype(np.float32)
    whole = np.int32([[0, 0, CW, CH]])
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    img = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    out_c = torch.zeros((1, 260), dtype=torch.int32, device="cuda")
    out_d = torch.zeros((1, 22), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    run_a = lambda: ctx.compose_into(img, views, tones=tones)  # noqa: E731
    run_b = lambda: ctx.compose_into(img, views)  # noqa: E731
    run_c = lambda: ctx.histogram_into(out_c, "final_gi", edges, "luma", whole)  # noqa: E731
    run_d = lambda: ctx.reduce_into(out_d, "final_gi", whole)  # noqa: E731

    b0, b0_min = event_ms(stream, run_b)
    d0, d0_min = event_ms(stream, run_d)
    a, a_min = event_ms(stream, run_a)
    c, c_min = event_ms(stream, run_c)
    rec_c = out_c.cpu().numpy().view(np.uint32)[0]
    assert rec_c[0] == 0 and rec_c[1] == CW * CH and rec_c[2:].sum() == CW * CH

    # e: every texel in one bin -- COLOR of a second context of the cascade's size, constant, no frame
    flat = RC2DGI(CW, CH, cascade_count=1, storage="f32")
    flat.upload("color", torch.full((CH, CW, 4), 0.25, dtype=torch.float32, device="cuda"))
    flat.sync()
    flat.set_stream(stream.cuda_stream)
    out_e = torch.zeros((1, 260), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    e, e_min = event_ms(stream, lambda: flat.histogram_into(out_e, "color", edges, "luma", whole))
    rec_e = out_e.cpu().numpy().view(np.uint32)[0]
    assert rec_e[3:].max() == CW * CH
    flat.set_stream(None)
    flat.close()

    # f: sprites
    rng = np.random.default_rng(1)
    sprites = np.stack([rng.integers(0, CW - SPRITE + 1, NSPRITES), rng.integers(0, CH - SPRITE + 1, NSPRITES),
                        np.full(NSPRITES, SPRITE), np.full(NSPRITES, SPRITE)], 1).astype(np.int32)
    out_f = torch.zeros((NSPRITES, 260), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    f, f_min = event_ms(stream, lambda: ctx.histogram_into(out_f, "final_gi", edges, "luma", sprites))
    assert (out_f[:, 1] == SPRITE * SPRITE).all().item()
    del out_f

    b1, b1_min = event_ms(stream, run_b)
    d1, d1_min = event_ms(stream, run_d)
    ctx.set_stream(None)

    # the host calls against a download and numpy
    tone_host = wall_ms(lambda: ctx.compose(views, tones=tones), args.host_runs)

    def tone_by_download():
        t = ctx.download("color")[::-1]
        rgb = np.searchsorted(curve, (t[..., :3] * np.float32(EXPOSURE)).reshape(-1), side="right").astype(np.uint8)
        return rgb.reshape(H, W, 3)

    tone_dl = wall_ms(tone_by_download, args.host_runs)
    x0, y0 = CW // 3, CH // 3
    one = np.int32([[x0, y0, 64, 64]])
    g = wall_ms(lambda: ctx.histogram("final_gi", edges, "luma", one), args.runs)

    def hist_by_download():
        t = ctx.download("final_gi")[y0:y0 + 64, x0:x0 + 64].reshape(-1, 4)
        luma = (np.float32(0.2126) * t[:, 0] + np.float32(0.7152) * t[:, 1]) + np.float32(0.0722) * t[:, 2]
        return np.histogram(luma, np.concatenate([[-np.inf], edges, [np.inf]]))[0]

    g_dl = wall_ms(hist_by_download, args.host_runs)
    bb, dd = max(b0, b1), max(d0, d1)
    r = {"W": W, "H": H, "N": N, "storage": "f32", "cascade": [CW, CH], "device": torch.cuda.get_device_name(0),
         "exposure": EXPOSURE, "curve": "sRGB by curve_from, the main blit only", "edges": 256,
         "a_compose_tone_ms": a, "a_min_ms": a_min, "b0_compose_ms": b0, "b0_min_ms": b0_min, "b1_compose_ms": b1,
         "b1_min_ms": b1_min, "a_over_b": a / bb, "accepted_a_le_2_b": bool(a <= 2 * bb),
         "compose_tone_host_ms": tone_host, "download_and_numpy_tone_ms": tone_dl,
         "c_histogram_whole_final_gi_ms": c, "c_min_ms": c_min, "d0_reduce_ms": d0, "d0_min_ms": d0_min,
         "d1_reduce_ms": d1, "d1_min_ms": d1_min, "c_over_d": c / dd, "accepted_c_le_2_d": bool(c <= 2 * dd),
         "c_GBps": CW * CH * 16 / (c * 1e6), "c_bins_filled": int((rec_c[3:] > 0).sum()),
         "e_histogram_constant_ms": e, "e_min_ms": e_min, "e_over_c": e / c,
         "f_histogram_65536_sprites_32x32_ms": f, "f_min_ms": f_min, "f_ns_per_rectangle": f * 1e6 / NSPRITES,
         "g_histogram_host_64x64_ms": g, "g_download_and_numpy_ms": g_dl, "g_download_over_histogram": g_dl / g}
    ctx.close()
    return r


if args.child:
    print("RESULT " + json.dumps(measure(args.child)), flush=True)
    sys.exit(0)

result = {"runs": args.runs, "warmup": args.warmup, "sprites": NSPRITES, "sprite": [SPRITE, SPRITE], "configs": []}
for spec in args.configs.split(","):
    cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", spec,
           "--runs", str(args.runs), "--warmup", str(args.warmup), "--host-runs", str(args.host_runs)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        sys.exit(f"tone_cost.py: {spec} ended with status {p.returncode}: nothing more is started")
    result["configs"].append(json.loads(lines[-1][7:]))
result["device"] = result["configs"][0]["device"]

line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
