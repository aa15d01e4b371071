#!/usr/bin/env python3
"""What drawing a tile layer costs through the three ways the library offers (f32 storage, blended into COLOR), a case:
  tilemap  one rc2dgi_tilemap_device call on the grid of cell words
  sprites  one rc2dgi_sprites_device call on the list rc2dgi.tilemap_sprites expands the grid into (made once, outside
           the timing: the yardstick is the existing raster alone, not the expansion)
  write    one rc2dgi_write_device(FLIP | BLEND) call of the layer assembled beforehand into one image as large as the
           target: the floor, timed where the layer covers the target (with a white tint the three leave equal bits)
HIP events around the call give the device's work, the wall clock until the call returns the host's (through the
Python binding).  The callers of a case alternate run by run in one process; each figure is the mean, the minimum and
the maximum of --runs runs after --warmup warm-up runs.  The textures of a case start from the same upload and are
asserted equal in bits, after one application each, before anything is timed.
Cases: 4096 x 4096 with 16 x 16 tiles from a 512 x 512 RGBA8 set, every cell non-empty (`full`) and one in eight
(`eighth`); tiles of 8 and of 64; 1200 x 900 with 32 x 32 tiles; an RGBA32F set.
Prints one JSON line a case and writes all to --out.
Usage: tilemap_cost.py [--out FILE] [--runs 20] [--cases full,eighth,tile8,tile64,window,f32set]"""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from radiancecascade2dglobalillumination_amd import RC2DGI, rc2dgi  # noqa: E402

CASES = {  # W, H, tile, set pixels, set dtype, share of non-empty cells
    "full": (4096, 4096, 16, 512, "uint8", 1.0),
    "eighth": (4096, 4096, 16, 512, "uint8", 0.125),
    "tile8": (4096, 4096, 8, 512, "uint8", 1.0),
    "tile64": (4096, 4096, 64, 512, "uint8", 1.0),
    "window": (1200, 900, 32, 512, "uint8", 1.0),
    "f32set": (4096, 4096, 16, 512, "float32", 1.0),
}

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--runs", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--cases", default=",".join(CASES))
args = ap.parse_args()


def stats(t):
    return {"mean_ms": float(np.mean(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t))}


def assemble(atlas, cells, tile, W, H):
    """the layer as one (H, W, 4) image, row 0 the top: what the cells show at origin (0, 0); every cell is non-empty
    and accepted (torch ops on the device)"""
    set_cols = atlas.shape[1] // tile
    Y, X = torch.arange(H, device="cuda"), torch.arange(W, device="cuda")
    g = cells.to(torch.int64)[(Y // tile)[:, None], (X // tile)[None, :]] & 0xFFFFFFFF
    t = (g & rc2dgi.TILE_ID_MASK) - 1
    ox, oy = (X % tile)[None, :].expand(H, W), (Y % tile)[:, None].expand(H, W)
    u = (t % set_cols) * tile + torch.where((g & rc2dgi.TILE_FLIP_X) != 0, tile - 1 - ox, ox)
    v = (t // set_cols) * tile + torch.where((g & rc2dgi.TILE_FLIP_Y) != 0, tile - 1 - oy, oy)
    return atlas[v, u].contiguous()


assert torch.cuda.is_available(), "tilemap_cost.py measures on the GPU"
result = {"device": torch.cuda.get_device_name(0), "box": socket.gethostname(), "runs": args.runs,
          "warmup": args.warmup, "storage": "f32", "cases": []}
rng = np.random.default_rng(1)
for name in args.cases.split(","):
    W, H, tile, aw, dtype, share = CASES[name]
    cols, rows = -(-W // tile), -(-H // tile)
    ntiles = (aw // tile) ** 2
    g = rng.integers(1, ntiles + 1, (rows, cols)).astype(np.uint32) | (rng.integers(0, 4, (rows, cols)).astype(np.uint32) << 30)
    if share < 1.0:
        g[rng.random((rows, cols)) >= share] = 0
    atlas_np = (rng.integers(0, 256, (aw, aw, 4)).astype(np.uint8) if dtype == "uint8"
                else rng.uniform(0.0, 1.0, (aw, aw, 4)).astype(np.float32))
    base = rng.uniform(0.0, 1.0, (H, W, 4)).astype(np.float32)
    routes = ["tilemap", "sprites"] + (["write"] if share == 1.0 else [])
    stream = torch.cuda.Stream()
    ctx = {r: RC2DGI(W, H, cascade_count=2) for r in routes}
    for c in ctx.values():
        c.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        atlas = torch.from_numpy(atlas_np).to("cuda")
        cells = torch.from_numpy(g.view(np.int32)).to("cuda")
        status = torch.zeros((2, 2), dtype=torch.int32, device="cuda")
        sprites = rc2dgi.tilemap_sprites(cells, (tile, tile), (0, 0), (aw, aw), (W, H)).contiguous()
        image = assemble(atlas, cells, tile, W, H) if "write" in routes else None
        stream.synchronize()
        draw = {"tilemap": lambda: ctx["tilemap"].tilemap_device("color", atlas, cells, (tile, tile), status=status[0]),
                "sprites": lambda: ctx["sprites"].sprites_device("color", atlas, sprites, status=status[1]),
                "write": lambda: ctx["write"].write("color", image, flip=True, blend=True)}

        # equal in bits first: one application each over the same upload
        for r in routes:
            ctx[r].upload("color", base)
            draw[r]()
        stream.synchronize()
        tex = {r: ctx[r].download("color").view(np.uint32) for r in routes}
        same = all(bool(np.array_equal(tex["tilemap"], tex[r])) for r in routes)
        changed = bool(not np.array_equal(tex["tilemap"], base.view(np.uint32)))
        st = status.cpu().numpy().tolist()
        assert same, f"case {name}: the textures differ"
        assert changed and st[0][0] == st[1][0] == int(sprites.shape[0]) and st[0][1] == 0, (name, st)
        del tex

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            fn()
            wall = (time.perf_counter() - t0) * 1e3
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1), wall

        for _ in range(args.warmup):
            for r in routes:
                draw[r]()
        stream.synchronize()
        dev, wall = {r: [] for r in routes}, {r: [] for r in routes}
        for _ in range(args.runs):  # the callers alternate
            for r in routes:
                d, w = timed(draw[r])
                dev[r].append(d)
                wall[r].append(w)
        stream.synchronize()
    rec = {"case": name, "W": W, "H": H, "tile": tile, "grid": [cols, rows], "set": [aw, aw], "set_dtype": dtype,
           "non_empty_share": share, "cells_drawn": st[0][0], "textures_equal_in_bits": same, "texture_changed": changed}
    for r in routes:
        rec[r + "_device_time"] = stats(dev[r])
        rec[r + "_host_returns"] = stats(wall[r])
    rec["sprites_min_over_tilemap_mean"] = rec["sprites_device_time"]["min_ms"] / rec["tilemap_device_time"]["mean_ms"]
    if "write" in routes:
        rec["tilemap_over_write_mean"] = rec["tilemap_device_time"]["mean_ms"] / rec["write_device_time"]["mean_ms"]
    if name == "full":  # the bar: below the minimum of the expanded list's runs
        rec["bar_tilemap_mean_below_sprites_min"] = bool(rec["tilemap_device_time"]["mean_ms"] < rec["sprites_device_time"]["min_ms"])
    for c in ctx.values():
        c.set_stream(None)
        c.close()
    del atlas, cells, sprites, image
    result["cases"].append(rec)
    print(json.dumps(rec), flush=True)

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
