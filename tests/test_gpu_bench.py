"""bench.py on the GPU: a plain run times its steps and prints the headline line only, and
--dump-outputs writes what the timed path left a caller -- the same arrays the same frames give through
the Python binding in this process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from radiancecascade2dglobalillumination_amd import RC2DGI, scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_last_timed_frame(tmp_path):
    W, H, N, steps, warmup = 320, 192, 4, 3, 1
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--size", str(W), "--height", str(H), "--cascades", str(N),
                        "--no-autotune", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == steps and line["warmup"] == warmup and line["ms_per_step"] > 0
    assert line["value"] > 0 and line["unit"] == "Mpixel*cascades/s" and line["higher_is_better"] is True
    # what takes runs of its own is behind --full
    for k in ("rc_level_ms", "gather_roofline", "valu_roofline", "inputs", "cpu_baseline"):
        assert k not in line

    color, emis = scenes.demo(W, H, t=3.0)  # the bench's scene of rank 0
    ctx = RC2DGI(W, H, cascade_count=N, ray_range=2.0)
    ctx.upload("color", color)
    ctx.upload("emissive", emis)
    for _ in range(warmup + steps):
        ctx.do_rc2dgi()
    ctx.sync()
    for name in ("dist", "final_gi", "color"):
        got = np.load(tmp_path / f"{name}.npy")
        want = ctx.download(name)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.isfinite(want).all() and np.array_equal(got, want), f"{name}: {np.count_nonzero(got != want)} values differ"
    ctx.close()
