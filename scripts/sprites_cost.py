#!/usr/bin/env python3
"""What drawing a sprite list costs through the two ways the library offers (f32 storage, draws blended into COLOR), per
list:
  a  one rc2dgi_write_device(.., FLIP | BLEND) call a sprite, the sub-image of the atlas into its rectangle: HIP events
     around the loop and the wall clock until the last call returns (each call only enqueues)
  b  one rc2dgi_sprites_device call of the same list in device memory: HIP events around the call, and the wall clock
     until it returns (it only enqueues)
Lists, at 4096 x 4096 from a 512 x 512 RGBA8 atlas: 64, 1024 and 16384 white 16 x 16 sprites at seeded random places
inside the target; and `full`, one 4096 x 4096 sprite from a 4096 x 4096 RGBA8 atlas against rc2dgi_write_device of the
whole texture.  a and b alternate run by run in one process; each figure is the mean and the minimum of --runs runs
after --warmup warm-up runs (lists from --few-from sprites up: --few-runs runs after one).  Both textures start from
the same upload and are compared in bits once a list, after one application each.
Prints one JSON line and writes it to --out.
Usage: sprites_cost.py [--out FILE] [--runs 20]"""
import argparse
import ctypes
import json
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
ap.add_argument("--few-from", type=int, default=10000, help="lists this long are timed --few-runs times")
ap.add_argument("--few-runs", type=int, default=4)
ap.add_argument("--lists", default="64,1024,16384,full")
args = ap.parse_args()


def stats(t):
    return {"mean_ms": float(np.mean(t)), "min_ms": float(np.min(t))}


assert torch.cuda.is_available(), "sprites_cost.py measures on the GPU"
W = H = 4096
SW = SH = 16
FLAGS = rc2dgi.WRITE_FLIP | rc2dgi.WRITE_BLEND
result = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "few_runs": args.few_runs, "W": W, "H": H,
          "lists": []}
rng = np.random.default_rng(1)
base = rng.uniform(0.0, 1.0, (H, W, 4)).astype(np.float32)
for spec in args.lists.split(","):
    if spec == "full":
        aw = ah = 4096
        sprites = np.array([[0, 0, W, H, 0, 0]], np.int32)
    else:
        aw = ah = 512
        n = int(spec)
        sprites = np.stack([rng.integers(0, aw - SW + 1, n), rng.integers(0, ah - SH + 1, n), np.full(n, SW),
                            np.full(n, SH), rng.integers(0, W - SW + 1, n), rng.integers(0, H - SH + 1, n)], 1).astype(np.int32)
    n = len(sprites)
    runs, warmup = (args.few_runs, 1) if n >= args.few_from else (args.runs, args.warmup)
    atlas_np = rng.integers(0, 256, (ah, aw, 4)).astype(np.uint8)
    stream = torch.cuda.Stream()
    loop_ctx, list_ctx = RC2DGI(W, H, cascade_count=2), RC2DGI(W, H, cascade_count=2)
    L, which = loop_ctx._L, rc2dgi.RT["color"]
    for c in (loop_ctx, list_ctx):
        c.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        atlas = torch.from_numpy(atlas_np).to("cuda")
        src, dst = torch.from_numpy(sprites[:, :4]).to("cuda"), torch.from_numpy(sprites[:, 4:6]).to("cuda")
        words = rc2dgi.pack_sprites(src, dst)
        status = torch.zeros(2, dtype=torch.int32, device="cuda")
        stream.synchronize()
        # a's arguments, made once: the rectangle (GL rows) and the address of the sub-image of every sprite
        rects = (rc2dgi.Rect * n)(*[rc2dgi.Rect(int(s[4]), H - int(s[5]) - int(s[3]), int(s[2]), int(s[3])) for s in sprites])
        rect_ps = [ctypes.byref(rects[k]) for k in range(n)]
        subs = [ctypes.c_void_p(atlas.data_ptr() + (int(s[1]) * aw + int(s[0])) * 4) for s in sprites]
        apitch = aw * 4
        fn_write, fn_sprites = L.rc2dgi_write_device, L.rc2dgi_sprites_device
        at = rc2dgi.Atlas(atlas.data_ptr(), aw, ah, 0, rc2dgi.FMT_RGBA8)
        at_p, words_p, status_p = ctypes.byref(at), ctypes.c_void_p(words.data_ptr()), ctypes.c_void_p(status.data_ptr())

        def loop_draw():
            h = loop_ctx._h
            for k in range(n):
                rc = fn_write(h, which, rect_ps[k], rc2dgi.FMT_RGBA8, FLAGS, subs[k], apitch)
                assert rc == 0, rc

        def list_draw():
            rc = fn_sprites(list_ctx._h, which, None, at_p, words_p, n, None, status_p)
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
            loop_draw()
            list_draw()
        stream.synchronize()
        a_dev, a_wall, b_dev, b_wall = [], [], [], []
        for _ in range(runs):  # the two ways alternate
            d, w = timed(loop_draw)
            a_dev.append(d)
            a_wall.append(w)
            d, w = timed(list_draw)
            b_dev.append(d)
            b_wall.append(w)
        stream.synchronize()
        for c in (loop_ctx, list_ctx):  # one application each over the same texels
            c.upload("color", base)
        loop_draw()
        list_draw()
        stream.synchronize()
    got_a, got_b = loop_ctx.download("color"), list_ctx.download("color")
    same = bool(np.array_equal(got_a.view(np.uint32), got_b.view(np.uint32)))
    changed = bool(not np.array_equal(got_b, base))
    batch, work = rc2dgi.paint_device_limits(W, H)
    r = {"list": spec, "sprites": n, "sprite_w": int(sprites[0, 2]), "sprite_h": int(sprites[0, 3]), "atlas": [aw, ah],
         "runs": runs, "batch": batch, "work_bytes": work, "status": status.cpu().numpy().tolist(),
         "textures_equal_in_bits": same, "texture_changed": changed,
         "a_write_loop_device_time": stats(a_dev), "a_write_loop_host_returns": stats(a_wall),
         "b_sprites_device_device_time": stats(b_dev), "b_sprites_device_host_returns": stats(b_wall),
         "a_over_b_device_time": float(np.mean(a_dev) / np.mean(b_dev))}
    for c in (loop_ctx, list_ctx):
        c.set_stream(None)
        c.close()
    del atlas, words
    result["lists"].append(r)
    print(json.dumps(r), flush=True)
    assert same, f"list {spec}: the two textures differ"

line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
