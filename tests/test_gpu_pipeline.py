"""GPU: frames and device calls back to back without a host sync, as a game loop or a torch producer and consumer drive
the library -- the script of tests/pipeline_script.py (an input change from device memory, uniform changes, a curve for
tone slot 1, one frame, nine captures into device memory; six steps) enqueued whole and synchronised once
(run_pipelined), against the same calls with a sync after every one and the captures taken by the host variants
(run_stepwise).

Every step's FINAL_GI, COLOR, BLUR and DIST capture of both runs is compared with oracle.frame of that step's
parameters and inputs alone, in bits (a NaN equal to a NaN in the same place: step 3 plants some on f32 and f16); the
pipelined run's reduce, histogram, sample, ray cast and composed image with the stepwise twin's, in bits.  What the
context changes on the host at enqueue time while the device may still work on the frame before -- the spare texture
the fused blur + merge swaps, what COLOR and FINAL_GI resolve to, the non-finite redo's flag and epoch, the split
records pass's alternating counters, the chain's epoch flags, the block fills keyed on _RayRange, the scratch of reduce
and histogram, the tone curve table -- must not show in any of them.

(a) the context's own stream, three storages, three shapes; (b) a caller's stream shared with torch, which makes each
input right before the call that consumes it and overwrites it right after, clones each capture before the next step
overwrites it, and keeps the device provably busy while the host enqueues; (c) the cascade chain; (d) 4096^2 on the
default schedule against a fresh context per step; (e) rc2dgi_set_stream itself.

Calls found to wait for the stream although they only enqueue: none at these shapes after one warm-up frame (case (b)
asks torch's event after every call).  The first frame of a context, and a frame after a sky uniform or a table
changed, uploads the tables and waits: by design ("Back-to-back frames")."""
import ctypes
import time

import numpy as np
import pytest

import pipeline_script as ps
import wild_inputs as wi
from test_write_cpu import build_write_ref

pytestmark = pytest.mark.gpu

STORAGES = ["f32", "f16", "rgba8"]
SHAPES = [(256, 256, 4), (128, 128, 3), (200, 120, 3)]
TEXTURES = ("final_gi", "color", "blur")
ACCESSORY = ("reduce", "hist", "sample", "rays", "image")
FILL_STEPS = (2, 3)  # the steps at _RayRange 200


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def R(torch):
    from radiancecascade2dglobalillumination_amd import rc2dgi

    return rc2dgi


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return build_write_ref(tmp_path_factory)


# ------------------------------------------------------------------ the calls of a step
def make_ctx(R, s, tuning=()):
    ctx = R.RC2DGI(s.W, s.H, cascade_count=s.N, storage=s.storage)
    for k, v in tuning:
        ctx.set_tuning(k, v)
    return ctx


def staged_inputs(torch, s):
    """every image of the script in device memory, and the points and rays: made before the script starts"""
    dev = {(k, j): torch.from_numpy(np.array(ch.img)).to("cuda") for k, st in enumerate(s.steps)
           for j, ch in enumerate(st.changes)}
    dev["uv"] = torch.from_numpy(np.array(s.uv)).to("cuda")
    dev["rays"] = torch.from_numpy(np.array(s.rays)).to("cuda")
    torch.cuda.synchronize()
    return dev


def alloc_captures(torch, R, s):
    """one step's capture tensors, filled with a pattern no capture holds"""
    x, y, w, h = s.dist_crop
    full = lambda shape, dt, v: torch.full(shape, v, dtype=dt, device="cuda")  # noqa: E731
    return dict(final_gi=full((s.CH, s.CW, 4), torch.float32, -7.0), color=full((s.H, s.W, 4), torch.float32, -7.0),
                blur=full((s.CH, s.CW, 4), torch.float32, -7.0), dist=full((h, w, 4), torch.uint8, 0xA5),
                reduce=full((len(s.reduce_rects), R.STATS_WORDS), torch.int32, -7),
                hist=full((len(s.hist_rects), len(s.hist_edges) + 4), torch.int32, -7),
                sample=full((len(s.uv), 4), torch.float32, -7.0), rays=full((len(s.rays), 11), torch.int32, -7),
                image=full((s.H, s.W, 4), torch.uint8, 0xA5))


def device_captures(R, ctx, s, dev, cap, lib):
    """the nine captures of a step through the device variants into the tensors of `cap`; lib(name, fn) makes a call"""
    L, h, vp = ctx._L, ctx._h, ctypes.c_void_p
    lib("read_into final_gi", lambda: ctx.read_into(cap["final_gi"], "final_gi"))
    lib("read_into color", lambda: ctx.read_into(cap["color"], "color"))
    lib("read_into blur", lambda: ctx.read_into(cap["blur"], "blur"))
    lib("read_into dist", lambda: ctx.read_into(cap["dist"], "dist", s.dist_crop, flip=True))
    lib("reduce_into", lambda: ctx.reduce_into(cap["reduce"], "final_gi", s.reduce_rects))
    lib("histogram_into", lambda: ctx.histogram_into(cap["hist"], "final_gi", s.hist_edges, "luma", s.hist_rects))
    # (RC2DGI.sample / raycast make their result tensor themselves: the C calls, into tensors made beforehand)
    lib("sample_device", lambda: ctx._check(L.rc2dgi_sample_device(
        h, R.RT["final_gi"], R.FILTER_LINEAR, vp(dev["uv"].data_ptr()), len(s.uv), vp(cap["sample"].data_ptr())), "sample"))
    lib("raycast_device", lambda: ctx._check(L.rc2dgi_raycast_device(
        h, vp(dev["rays"].data_ptr()), len(s.rays), vp(cap["rays"].data_ptr())), "raycast"))
    lib("compose_into", lambda: ctx.compose_into(cap["image"], R.display_layout(s.W, s.H), tones=s.tones))


def host_captures(R, ctx, s):
    """the same nine captures through the host variants, as the arrays as_arrays makes of the device's"""
    return as_arrays(dict(
        final_gi=ctx.read("final_gi"), color=ctx.read("color"), blur=ctx.read("blur"),
        dist=ctx.read("dist", s.dist_crop, np.uint8, flip=True), reduce=ctx.reduce("final_gi", s.reduce_rects),
        hist=ctx.histogram("final_gi", s.hist_edges, "luma", s.hist_rects), sample=ctx.sample("final_gi", s.uv, R.FILTER_LINEAR),
        rays=ctx.raycast(s.rays), image=ctx.compose(R.display_layout(s.W, s.H), tones=s.tones)))


def as_arrays(cap):
    """captures as numpy arrays a comparison in bits can take: the floats of the textures as they are, every record
    and the sampled values as 32-bit words, the images as bytes"""
    out = {}
    for k, v in cap.items():
        a = v.cpu().numpy() if hasattr(v, "data_ptr") else np.ascontiguousarray(v)
        if k in ("reduce", "hist", "sample", "rays"):
            a = np.ascontiguousarray(a).reshape(len(a), -1).view(np.int32).reshape(len(a), -1)
        out[k] = a
    return out


def step_calls(ctx, st, inputs, lib):
    """a step up to its frame: the input changes from the device tensors inputs(j), the uniforms, the curve, the frame"""
    for j, ch in enumerate(st.changes):
        t = inputs(j)
        if ch.kind == "upload":
            lib(f"upload {ch.which}", lambda: ctx.upload(ch.which, t))
        else:
            lib(f"write {ch.which}", lambda: ctx.write(ch.which, t, ch.rect, ch.flip, ch.blend))
    for name, v in st.uniforms:
        ctx.set_shader_value(name, v)
    if st.curve is not None:
        lib("set_curve", lambda: ctx.set_curve(1, st.curve))
    lib("do", ctx.do_rc2dgi)


def run_pipelined(R, torch, ctx, s, dev):
    """The whole script enqueued: no sync, no download and no host-variant call between the first step and the last
    capture, then one sync.  Returns every step's captures and what rc_fill_levels said after its frame was enqueued
    (a value the host keeps: asking does not wait)."""
    caps = [alloc_captures(torch, R, s) for _ in s.steps]
    torch.cuda.synchronize()
    fills = []
    lib = lambda name, fn: fn()  # noqa: E731
    for k, st in enumerate(s.steps):
        step_calls(ctx, st, lambda j: dev[(k, j)], lib)
        fills.append(ctx.get_tuning("rc_fill_levels"))
        device_captures(R, ctx, s, dev, caps[k], lib)
    ctx.sync()
    return [as_arrays(c) for c in caps], fills


def run_stepwise(R, torch, ctx, s, dev, after_step=None):
    """The twin: the same calls with ctx.sync() after every one, the captures by the host variants."""
    def lib(name, fn):
        fn()
        ctx.sync()

    caps, fills = [], []
    for k, st in enumerate(s.steps):
        step_calls(ctx, st, lambda j: dev[(k, j)], lib)
        fills.append(ctx.get_tuning("rc_fill_levels"))
        caps.append(host_captures(R, ctx, s))
        if after_step:
            after_step(k, st)
    return caps, fills


# ------------------------------------------------------------------ the comparisons
def assert_textures(s, caps, what):
    """every step's FINAL_GI, COLOR, BLUR and DIST capture holds the bits of its oracle frame"""
    for st, cap, fr in zip(s.steps, caps, ps.frames(s)):
        want = ps.captured_textures(s, fr)
        odd = any(np.isnan(want[k]).any() for k in TEXTURES)
        assert odd == (st.index == 3 and s.storage != "rgba8")
        for k in TEXTURES:
            tag = f"{what}, step {st.index}"
            if odd:  # (wi.assert_bits but for the payload of a NaN)
                assert cap[k].shape == want[k].shape, (tag, k)
                assert np.array_equal(np.isnan(cap[k]), np.isnan(want[k])), f"{tag}: {k}: NaN in other texels than the oracle's"
                assert ps.same_bits(cap[k], want[k]), f"{tag}: {k}: {wi.bits_differ(cap[k], want[k])} values differ in bits"
            else:
                wi.assert_bits(cap, want, tag, names=(k,))
        assert np.array_equal(cap["dist"], want["dist"]), \
            f"{what}, step {st.index}: dist: {np.count_nonzero(cap['dist'] != want['dist'])} bytes differ"


def assert_accessory(s, got, want, what):
    for st, a, b in zip(s.steps, got, want):
        for k in ACCESSORY:
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, st.index, k, a[k].shape, b[k].shape)
            assert np.array_equal(a[k], b[k]), \
                f"{what}, step {st.index}: {k}: {np.count_nonzero(a[k] != b[k])} words differ from the stepwise twin's"


_twins = {}


def twin_captures(R, torch, s, tuning=(), after_step=None):
    """the stepwise twin on a context of its own, its textures held against the oracle: (captures, fills, seconds its
    calls took on the host, syncs and host variants included); run once a script and shared"""
    key = (s.W, s.H, s.N, s.storage, tuning)
    if key not in _twins:
        _twins[key] = run_twin(R, torch, s, tuning, after_step)
    return _twins[key]


def run_twin(R, torch, s, tuning, after_step):
    ctx = make_ctx(R, s, tuning)
    dev = staged_inputs(torch, s)
    t0 = time.perf_counter()
    caps, fills = run_stepwise(R, torch, ctx, s, dev, after_step and (lambda k, st: after_step(ctx, k, st)))
    seconds = time.perf_counter() - t0
    ctx.close()
    assert_textures(s, caps, f"{s.W}x{s.H} {s.storage} stepwise")
    return caps, fills, seconds


# ------------------------------------------------------------------ (a) the context's own stream
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("W,H,N", SHAPES)
def test_script_on_the_own_stream(R, torch, ref_lib, W, H, N, storage):
    """256^2, N = 4: the fused blur + merge with its spare swap, FINAL_GI = giRT2; 128^2, N = 3: the same with FINAL_GI =
    giRT1; 200 x 120, N = 3: float JumpFlood keys, separate blur, copy-back and merge."""
    s = ps.build(ref_lib, W, H, N, storage)
    want, twin_fills, _ = twin_captures(R, torch, s)
    ctx = make_ctx(R, s)
    assert ctx.final_gi == (2 if N % 2 == 0 else 1) and ctx.cascade_resolution == (s.CW, s.CH)
    got, fills = run_pipelined(R, torch, ctx, s, staged_inputs(torch, s))
    ctx.close()
    what = f"{W}x{H} {storage} pipelined"
    assert_textures(s, got, what)
    assert_accessory(s, got, want, what)
    for f in (fills, twin_fills):
        if storage == "f32":  # the block fills follow _RayRange both ways
            assert [v != 0 for v in f] == [st.index in FILL_STEPS for st in s.steps], f
        else:
            assert f == [0] * len(s.steps), f


# ------------------------------------------------------------------ (b) a caller's stream, shared with torch
SLEEP_PROBE_CYCLES = 4_000_000
POISON = 0.375  # what torch overwrites an input with once the call that consumes it has returned


def sleep_cycles_per_ms(torch, stream):
    """how long torch.cuda._sleep spins per cycle of its argument, from two events around a known count"""
    with torch.cuda.stream(stream):
        torch.cuda._sleep(1000)  # (the kernel's first launch)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(SLEEP_PROBE_CYCLES)
        e1.record()
        e1.synchronize()
    ms = e0.elapsed_time(e1)
    assert ms > 0
    return SLEEP_PROBE_CYCLES / ms


@pytest.mark.parametrize("storage", ["f32", "rgba8"])
@pytest.mark.parametrize("W,H,N", [(256, 256, 4), (200, 120, 3)])
def test_script_on_a_callers_stream_with_torch_producing_and_consuming(R, torch, ref_lib, W, H, N, storage):
    """Producer: under torch.cuda.stream(s) torch makes each input on the stream right before the call that consumes it
    and overwrites it in place right after that call has returned.  Consumer: the library reads every step into one
    reused tensor a kind, torch clones it on the stream before the next step overwrites it.  Busy device: after one
    warm-up frame a torch.cuda._sleep sized to three times the stepwise twin's host time (measured, as is the sleep's
    rate) runs ahead of the script; an event behind it has not completed when the script's last call returns, nor
    after any call before."""
    s = ps.build(ref_lib, W, H, N, storage)
    want, _, twin_seconds = twin_captures(R, torch, s)
    stream = torch.cuda.Stream()
    ctx = make_ctx(R, s)
    ctx.set_stream(stream.cuda_stream)
    ctx.do_rc2dgi()  # the warm-up frame, on the cleared inputs: it uploads the tables and waits
    ctx.sync()
    staged = staged_inputs(torch, s)
    rate = sleep_cycles_per_ms(torch, stream)
    sleep_ms = 3.0 * twin_seconds * 1e3
    assert sleep_ms < 5000.0, f"the stepwise twin took {twin_seconds:.3f} s on the host"
    queried = []
    clones = []
    with torch.cuda.stream(stream):
        cap = alloc_captures(torch, R, s)
        stream.synchronize()
        plug = torch.cuda.Event()
        torch.cuda._sleep(int(sleep_ms * rate))
        plug.record()
        t0 = time.perf_counter()

        def lib(name, fn):
            fn()
            queried.append((name, plug.query()))

        for k, st in enumerate(s.steps):
            made = {}

            def inputs(j):
                made[j] = staged[(k, j)].clone()
                return made[j]

            def lib_then_overwrite(name, fn):
                lib(name, fn)
                if made:
                    made.popitem()[1].fill_(POISON)

            step_calls(ctx, st, inputs, lib_then_overwrite)
            device_captures(R, ctx, s, staged, cap, lib)
            clones.append({name: t.clone() for name, t in cap.items()})
        enqueue_seconds = time.perf_counter() - t0
        still_busy = not plug.query()
    ctx.sync()
    ctx.set_stream(None)
    ctx.close()
    print(f"\n{W}x{H} {storage}: stepwise twin {twin_seconds * 1e3:.1f} ms on the host, pipelined enqueue "
          f"{enqueue_seconds * 1e3:.1f} ms, sleep {sleep_ms:.1f} ms = {int(sleep_ms * rate)} cycles at {rate:.0f} cycles / ms, "
          f"event complete after the last call: {not still_busy}")
    waited = [name for name, done in queried if done]
    assert not waited, f"the plug had run out after {waited[0]} (call {[n for n, _ in queried].index(waited[0])} of {len(queried)})"
    assert still_busy, "the device was idle before the script's last call returned"
    got = [as_arrays(c) for c in clones]
    what = f"{W}x{H} {storage} on torch's stream"
    assert_textures(s, got, what)
    assert_accessory(s, got, want, what)


# ------------------------------------------------------------------ (c) the cascade chain
def test_script_on_the_cascade_chain(R, torch, ref_lib):
    """rc_chain 1 on f32 at 256^2, N = 4, the smallest shape of the ladder: the chain really ran where rc_chain is still
    1, no workgroup timed out and no level was a fill (a chained frame never fills; a quiet fallback to one launch a
    level would have, at _RayRange 200), after every step of the twin and of the pipelined run."""
    s = ps.build(ref_lib, 256, 256, 4, "f32")
    tuning = (("rc_chain", 1),)

    def chained(ctx, k, st):
        assert ctx.get_tuning("rc_chain") == 1 and ctx.get_tuning("rc_chain_timeouts") == 0, f"twin, step {st.index}"

    want, twin_fills, _ = twin_captures(R, torch, s, tuning, chained)
    ctx = make_ctx(R, s, tuning)
    got, fills = run_pipelined(R, torch, ctx, s, staged_inputs(torch, s))
    assert ctx.get_tuning("rc_chain") == 1 and ctx.get_tuning("rc_chain_timeouts") == 0
    ctx.close()
    assert fills == [0] * len(s.steps) and twin_fills == [0] * len(s.steps), (fills, twin_fills)
    assert_textures(s, got, "256x256 chained pipelined")
    assert_accessory(s, got, want, "256x256 chained pipelined")


# ------------------------------------------------------------------ (d) 4096^2 on the default schedule
def big_captures(torch, R, s):
    crops = big_crops(s)
    full = lambda shape, dt, v: torch.full(shape, v, dtype=dt, device="cuda")  # noqa: E731
    cap = {f"{name} {k}": full((64, 64, 4), torch.float32, -7.0) for name in ("final_gi", "color") for k in crops}
    cap["dist"] = full((s.H, s.W, 4), torch.uint8, 0xA5)
    cap["reduce"] = full((3, R.STATS_WORDS), torch.int32, -7)
    return cap


def big_crops(s):
    sx, sy = s.sprite[:2]
    return {"near": (sx - 20, sy - 24, 64, 64), "far": (s.W // 8, s.H // 2, 64, 64)}


def test_script_at_4096_on_the_default_schedule(R, torch, ref_lib):
    """4096^2, N = 6, f32: the only size with the split records pass's alternating list counters and the palettes.
    Steps 0, 1 and 4, pipelined; 64 x 64 crops of FINAL_GI and COLOR around the sprite and far from it, the whole DIST
    as bytes and three reduced rectangles equal those of a fresh context a step, given that step's whole input and
    drained (tests/test_gpu_live.py holds such a context against oracle rows at this size)."""
    W = H = 4096
    s = ps.build(ref_lib, W, H, 6, "f32", steps=(0, 1, 4))
    crops = big_crops(s)
    rects = [(0, 0, s.CW, s.CH), crops["near"], (1, 2, s.CW - 3, s.CH // 2 - 1)]

    def capture(ctx, cap):
        for name in ("final_gi", "color"):
            for k, r in crops.items():
                ctx.read_into(cap[f"{name} {k}"], name, r)
        ctx.read_into(cap["dist"], "dist")
        ctx.reduce_into(cap["reduce"], "final_gi", rects)

    live = make_ctx(R, s)
    dev = staged_inputs(torch, s)
    caps = [big_captures(torch, R, s) for _ in s.steps]
    torch.cuda.synchronize()
    lib = lambda name, fn: fn()  # noqa: E731
    for k, st in enumerate(s.steps):
        step_calls(live, st, lambda j: dev[(k, j)], lib)
        capture(live, caps[k])
    live.sync()
    live.close()
    del dev
    got = [as_arrays(c) for c in caps]
    for k, st in enumerate(s.steps):
        fresh = make_ctx(R, s)
        for name, v in (("_Reflectivity", st.params.reflectivity), ("_RayRange", st.params.ray_range),
                        ("_BlurRadius", st.params.blur_radius)):
            fresh.set_shader_value(name, v)
        fresh.frame(st.color, st.emis)
        fresh.sync()
        capture(fresh, caps[k])  # (the tensors the live context filled: copied to the host above)
        fresh.sync()
        want = as_arrays(caps[k])
        fresh.close()
        for name in want:
            a, b = got[k][name], want[name]
            same = np.array_equal(a, b) if a.dtype != np.float32 else wi.bits_equal(a, b)
            assert same, f"step {st.index}: {name} differs from a fresh context's"
        if k:
            assert not wi.bits_equal(got[k]["final_gi near"], got[k - 1]["final_gi near"]), "consecutive steps differ"


# ------------------------------------------------------------------ (e) rc2dgi_set_stream itself
def test_set_stream_drains_the_stream_it_leaves(R, torch, ref_lib):
    """A frame enqueued on stream A behind a sleep, set_stream(B), a read on B without a sync: the read sees that
    frame, because rc2dgi_set_stream waits for the stream it leaves (B knows nothing of A).  set_stream(None) returns
    to the own stream the same way."""
    s = ps.build(ref_lib, 128, 128, 3, "f32")
    fr = ps.frames(s)
    dev = staged_inputs(torch, s)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    ctx = make_ctx(R, s)
    ctx.set_stream(a.cuda_stream)
    ctx.do_rc2dgi()  # (the tables)
    ctx.sync()
    cycles = int(20.0 * sleep_cycles_per_ms(torch, a))
    lib = lambda name, fn: fn()  # noqa: E731
    outs = [torch.full((s.CH, s.CW, 4), -7.0, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    with torch.cuda.stream(a):
        torch.cuda._sleep(cycles)
        behind = torch.cuda.Event()
        behind.record()
    step_calls(ctx, s.steps[0], lambda j: dev[(0, j)], lib)
    assert not behind.query(), "stream A was idle already: the sleep is too short to show a drain"
    ctx.set_stream(b.cuda_stream)
    assert a.query(), "set_stream returned with work left on the stream it leaves"
    ctx.read_into(outs[0], "final_gi")
    with torch.cuda.stream(b):
        torch.cuda._sleep(cycles)
        behind = torch.cuda.Event()
        behind.record()
    step_calls(ctx, s.steps[1], lambda j: dev[(1, j)], lib)
    assert not behind.query(), "stream B was idle already"
    ctx.set_stream(None)
    assert b.query(), "set_stream(None) returned with work left on the stream it leaves"
    ctx.read_into(outs[1], "final_gi")
    ctx.sync()
    b.synchronize()
    for k in range(2):
        wi.assert_bits({"final_gi": outs[k].cpu().numpy()}, {"final_gi": fr[k].gi_final}, f"step {k} read on the next stream")
    ctx.close()
