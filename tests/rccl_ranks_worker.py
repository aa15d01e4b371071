"""The child process of test_gpu_rccl_ranks.py (not collected by pytest): rc2dgi_do over a communicator at world > 1,
the ranks as threads of this process over the stand-in transport (fake_rccl.cpp) that RC2DGI_RCCL_LIB names.

    python rccl_ranks_worker.py OUT.jsonl

Runs every case in turn and appends one JSON record per case to OUT.jsonl; stops at the first case that returns a
device error.  A record holds, per frame and rank, None or the first difference from the unsharded frame
(shard_compare.assert_shard_matches_whole), strip_tables_active and the stand-in's log of that frame; the parent
asserts on it.  Importing this module runs nothing (the parent takes the case lists from it)."""
import ctypes
import json
import os
import sys
import threading
import time

# W, H, N, rayRange, renderScale, blur, world, scene, storage, strip_tables knob
CASES = [
    (2, 2, 1, 2.0, 1.0, 1.5, 2, "full", "f32", 1),         # S = 1: no JumpFlood exchange, broadcasts only
    (3, 2, 1, 2.0, 1.0, 1.5, 2, "full", "f32", 1),         # the smallest frame with an exchange step (S = 2)
    (64, 64, 2, 8.0, 1.0, 1.5, 2, "rand:31", "f32", 1),
    (256, 256, 5, 3.0, 1.0, 1.5, 8, "demo", "f32", 1),     # integer key; block buffers 1 and 2 in use
    (512, 256, 4, 2.0, 1.0, 1.5, 3, "rand:32", "f32", 1),  # uneven strips, float key
    (200, 120, 3, 2.0, 1.0, 2.5, 4, "rand:33", "f32", 1),  # not a power of two
    (320, 256, 4, 8.0, 0.5, 1.37, 3, "rand:34", "f32", 1),
    (128, 128, 3, 4.0, 1.0, 0.0, 5, "rand:35", "f32", 1),  # blur off
    (512, 384, 5, 2.0, 1.0, 1.5, 3, "rand:36", "f16", 1),
    (512, 384, 5, 2.0, 1.0, 1.5, 3, "rand:36", "rgba8", 1),
    # H = 2 mod 4: a step's offset of H / 4 rows ends in .5, its float taps round to the margin row, and that row is
    # one a shard copies from its own window into a block buffer (at 200 x 120 nothing reads those rows)
    (200, 122, 3, 2.0, 1.0, 2.5, 4, "rand:39", "f32", 1),
    # thin strips (tests/test_shard_edges_cpu.py): one and two rows, every step a block step, a block request received
    # from three ranks, a step whose taps share one block; two-row strips of a power-of-two screen
    (64, 12, 2, 2.0, 1.0, 1.5, 8, "rand:37", "f32", 1),
    (128, 16, 2, 2.0, 1.0, 1.5, 8, "rand:38", "f32", 1),
    (4096, 4096, 6, 2.0, 1.0, 1.5, 2, "demo", "f32", 1),      # strip tables, the smallest size at which they apply
    (4096, 4096, 6, 2.0, 1.0, 1.5, 4, "demo", "f32", 0),      # strip_tables 0: distRT all-broadcast at that size
    (4096, 4096, 6, 2.0, 1.0, 1.5, 8, "speckled", "f32", 1),  # strip tables; records derived from the inputs
]
RECONNECT = (64, 64, 2, 8.0, 1.0, 1.5, "rand:31")  # world 2, then the same frame at world 4 on a new communicator
STANDIN_CASES = ["move", "bytes", "roots", "overlap", "unmatched"]
WAIT_LIMIT_MS = 10000  # of the stand-in's host-side waits while the product runs (its default is 30 s)


def standin_library(tmp_dir):
    """Path of the built stand-in: the one build() left in the tree, else built into tmp_dir."""
    from radiancecascade2dglobalillumination_amd import _build

    if os.path.exists(_build.FAKE_RCCL_LIB) and \
            os.path.getmtime(_build.FAKE_RCCL_LIB) >= os.path.getmtime(_build.FAKE_RCCL_SRC):
        return _build.FAKE_RCCL_LIB
    return _build.build_fake_rccl(out=os.path.join(str(tmp_dir), "libfake_rccl.so"))


def case_id(case):
    W, H, N, rr, rs, blur, world, scene, storage, stk = case
    return f"{W}x{H}-N{N}-rr{rr:g}-rs{rs:g}-blur{blur:g}-w{world}-{scene}-{storage}-st{stk}"


def scene_of(spec, W, H):
    import numpy as np
    from radiancecascade2dglobalillumination_amd import scenes

    if spec == "full":  # every texel an occluder, one of them an emitter (as test_gpu_parity's scene of that name)
        color = np.ones((H, W, 4), np.float32)
        emis = np.zeros((H, W, 4), np.float32)
        emis[0, 0] = (1.0, 0.5, 0.25, 1.0)
        return color, emis
    if spec == "demo":
        return scenes.demo(W, H)
    if spec == "speckled":
        from test_gpu_parity import speckled_scene

        return speckled_scene(W, H)
    return scenes.random_scene(W, H, int(spec.split(":")[1]))


class Fake:
    """The stand-in's entry points through ctypes (the same library instance librc2dgi opened by that path)."""

    class UniqueId(ctypes.Structure):
        _fields_ = [("internal", ctypes.c_char * 128)]

    def __init__(self, path):
        L = self.L = ctypes.CDLL(path)
        vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        L.ncclGetUniqueId.argtypes = [ctypes.POINTER(self.UniqueId)]
        L.ncclCommInitRank.argtypes = [ctypes.POINTER(vp), i, self.UniqueId, i]
        L.ncclCommDestroy.argtypes = [vp]
        L.ncclSend.argtypes = [vp, sz, i, i, vp, vp]
        L.ncclRecv.argtypes = [vp, sz, i, i, vp, vp]
        L.ncclBroadcast.argtypes = [vp, vp, sz, i, i, vp, vp]
        L.ncclGetErrorString.argtypes = [i]
        L.ncclGetErrorString.restype = ctypes.c_char_p
        L.fake_rccl_set_wait_limit_ms.argtypes = [ctypes.c_long]
        L.fake_rccl_set_wait_limit_ms.restype = ctypes.c_long
        L.fake_rccl_log.argtypes = [ctypes.c_char_p, i, ctypes.c_char_p, ctypes.c_long]
        L.fake_rccl_log.restype = ctypes.c_long

    def log(self, uid: bytes, rank: int):
        n = self.L.fake_rccl_log(uid, rank, None, 0)
        assert n >= 0, "fake_rccl_log: unknown id or rank"
        buf = ctypes.create_string_buffer(n + 1)
        assert self.L.fake_rccl_log(uid, rank, buf, n + 1) == n
        return json.loads(buf.value.decode())


TRANSPORT_ERRORS = ("JumpFlood exchange: ", "ncclBroadcast", "ncclCommInitRank: ")


def run_ranks(fns):
    """fns[k]() on one thread per rank (ctypes releases the GIL; a group's end blocks until the peers post);
    returns one None or exception per rank."""
    errs = [None] * len(fns)

    def body(k):
        try:
            fns[k]()
        except BaseException as e:  # noqa: BLE001  (reported in the record)
            errs[k] = e

    ts = [threading.Thread(target=body, args=(k,)) for k in range(len(fns))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return errs


class DeviceError(Exception):
    pass


def frames_on_ranks(R, fake, ctxs, uid, want, W, H, blur, expect_st, frames, seen):
    """`frames` frames of do_rc2dgi() on the connected contexts; per frame and rank: the comparison with the whole
    frame, strip_tables_active and the frame's slice of the stand-in's log (`seen`: log entries already consumed).
    Raises DeviceError on anything that is not an error the transport returned."""
    out = []
    for _ in range(frames):
        errs = run_ranks([c.do_rc2dgi for c in ctxs])
        for e in errs:
            if e is not None and not (isinstance(e, R.RC2DGIError) and any(m in str(e) for m in TRANSPORT_ERRORS)):
                raise DeviceError(f"do_rc2dgi: {e!r}")
        try:
            for c in ctxs:
                c.sync()
        except R.RC2DGIError as e:
            raise DeviceError(f"sync: {e!r}")
        fr = {"errors": [None if e is None else str(e) for e in errs], "differs": [], "st": [], "log": []}
        for k, c in enumerate(ctxs):
            diff = None
            if all(e is None for e in errs):
                try:
                    assert_shard_matches_whole(c, want, W, H, blur, expect_strip_tables=expect_st)
                except AssertionError as e:
                    diff = str(e) or "assertion failed"
            fr["differs"].append(diff)
            fr["st"].append(c.get_tuning("strip_tables_active"))
            log = fake.log(uid, k)
            fr["log"].append(log[seen[k]:])
            seen[k] = len(log)
        out.append(fr)
        if any(e is not None for e in errs):
            break  # (the ranks are out of step after a transport error: no further frame on this communicator)
    return out


def make_ctx(R, W, H, N, rr, rs, blur, storage):
    kw = {} if storage == "f32" else {"storage": storage}
    c = R.RC2DGI(W, H, cascade_count=N, render_scale=rs, ray_range=rr, **kw)
    c.set_shader_value("_BlurRadius", blur)
    return c


def shard_ctx(c, k, world, stk, color, emis):
    c.set_shard(k, world)
    c.set_tuning("poison", 1)
    if not stk:
        c.set_tuning("strip_tables", 0)
    c.upload("color", color)
    c.upload("emissive", emis)


_whole = {}


def whole_of(R, W, H, N, rr, rs, blur, scene, storage):
    key = (W, H, N, rr, rs, blur, scene, storage)
    if key not in _whole:
        if W >= 4096:
            _whole.clear()  # (one 4096^2 frame's textures at a time)
        color, emis = scene_of(scene, W, H)
        _whole[key] = (color, emis, whole_frame(R, W, H, N, rr, rs, blur, color, emis,
                                                None if storage == "f32" else storage))
    return _whole[key]


def run_case(R, fake, case):
    W, H, N, rr, rs, blur, world, scene, storage, stk = case
    color, emis, want = whole_of(R, W, H, N, rr, rs, blur, scene, storage)
    expect_st = bool(stk) and W == H and W >= 4096 and storage == "f32"
    ctxs = []
    try:
        for k in range(world):
            c = make_ctx(R, W, H, N, rr, rs, blur, storage)
            ctxs.append(c)
            shard_ctx(c, k, world, stk, color, emis)
        uid = R.shard_unique_id()
        for c in ctxs:
            c.connect(uid)
        pitch = ctxs[0].device_buffer("dist")[1]
        frames = frames_on_ranks(R, fake, ctxs, uid, want, W, H, blur, expect_st, 2, [0] * world)
        return {"frames": frames, "dist_pitch_bytes": pitch, "expect_st": expect_st}
    finally:
        for c in ctxs:
            c.close()


def run_reconnect(R, fake):
    W, H, N, rr, rs, blur, scene = RECONNECT
    color, emis, want = whole_of(R, W, H, N, rr, rs, blur, scene, "f32")
    ctxs = []
    try:
        for k in range(2):
            ctxs.append(make_ctx(R, W, H, N, rr, rs, blur, "f32"))
            shard_ctx(ctxs[k], k, 2, 1, color, emis)
        uid2 = R.shard_unique_id()
        for c in ctxs:
            c.connect(uid2)
        first = frames_on_ranks(R, fake, ctxs, uid2, want, W, H, blur, False, 1, [0, 0])
        for k in range(2):
            ctxs.append(make_ctx(R, W, H, N, rr, rs, blur, "f32"))
        for k, c in enumerate(ctxs):  # set_shard drops the first two contexts' communicator and windows
            shard_ctx(c, k, 4, 1, color, emis)
        uid4 = R.shard_unique_id()
        assert uid4 != uid2
        for c in ctxs:
            c.connect(uid4)
        second = frames_on_ranks(R, fake, ctxs, uid4, want, W, H, blur, False, 1, [0] * 4)
        return {"frames": first + second, "dist_pitch_bytes": ctxs[0].device_buffer("dist")[1], "expect_st": False,
                "old_log_after": [len(fake.log(uid2, k)) for k in range(2)],
                "old_log_first": [len(first[0]["log"][k]) for k in range(2)]}
    finally:
        for c in ctxs:
            c.close()


# --- the stand-in itself, driven directly on two threads with small device buffers ------------------------------------
NCCL_UINT8, NCCL_FLOAT32 = 1, 7
NCCL_INTERNAL_ERROR, NCCL_INVALID_ARGUMENT, NCCL_INVALID_USAGE = 3, 4, 5


def standin_comms(fake, n=2):
    uid = Fake.UniqueId()
    assert fake.L.ncclGetUniqueId(ctypes.byref(uid)) == 0
    comms = []
    for k in range(n):
        h = ctypes.c_void_p()
        assert fake.L.ncclCommInitRank(ctypes.byref(h), n, uid, k) == 0
        comms.append(h)
    return uid, comms


def run_standin(fake, which):
    import torch

    L = fake.L
    dev = torch.device("cuda:0")
    uid, comms = standin_comms(fake)
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    st = [ctypes.c_void_p(s.cuda_stream) for s in streams]
    g = torch.Generator(device="cpu").manual_seed(5)
    a = torch.randint(0, 256, (1000,), dtype=torch.uint8, generator=g).to(dev)
    b = torch.zeros(1000, dtype=torch.uint8, device=dev)
    f0 = torch.zeros(128, dtype=torch.float32, device=dev)
    f1 = torch.randn(128, generator=g).to(dev)
    torch.cuda.synchronize()
    rec = {}
    res = [None, None]
    msg = [None, None]

    def call(k, fn):  # the result and, on the same thread, the stand-in's description of a failure
        res[k] = fn()
        msg[k] = L.ncclGetErrorString(res[k]).decode()

    try:
        if which == "move":  # a send and its receive, then an in-place broadcast from rank 1 (float32: count x 4 B)
            def rank0():
                call(0, lambda: L.ncclSend(a.data_ptr() + 8, 900, NCCL_UINT8, 1, comms[0], st[0])
                     or L.ncclBroadcast(f0.data_ptr(), f0.data_ptr(), 128, NCCL_FLOAT32, 1, comms[0], st[0]))

            def rank1():
                call(1, lambda: L.ncclRecv(b.data_ptr() + 16, 900, NCCL_UINT8, 0, comms[1], st[1])
                     or L.ncclBroadcast(f1.data_ptr(), f1.data_ptr(), 128, NCCL_FLOAT32, 1, comms[1], st[1]))

            errs = run_ranks([rank0, rank1])
            for s in streams:
                s.synchronize()
            want_b = torch.zeros_like(b)
            want_b[16:916] = a[8:908]
            rec = {"results": res, "moved": bool(torch.equal(b, want_b)), "broadcast": bool(torch.equal(f0, f1)),
                   "log": [fake.log(bytes(uid), k) for k in range(2)]}
        elif which == "bytes":  # a count that differs: both sides
            errs = run_ranks([lambda: call(0, lambda: L.ncclSend(a.data_ptr(), 100, NCCL_UINT8, 1, comms[0], st[0])),
                              lambda: call(1, lambda: L.ncclRecv(b.data_ptr(), 96, NCCL_UINT8, 0, comms[1], st[1]))])
            rec = {"results": res, "messages": msg}
        elif which == "roots":  # a broadcast whose roots disagree: every rank
            errs = run_ranks([lambda: call(0, lambda: L.ncclBroadcast(a.data_ptr(), a.data_ptr(), 64, NCCL_UINT8, 0,
                                                                       comms[0], st[0])),
                              lambda: call(1, lambda: L.ncclBroadcast(b.data_ptr(), b.data_ptr(), 64, NCCL_UINT8, 1,
                                                                       comms[1], st[1]))])
            rec = {"results": res, "messages": msg}
        elif which == "overlap":  # two receives of one group into overlapping rows: refused before anything is posted
            def rank0():
                L.ncclGroupStart()
                r1 = L.ncclRecv(b.data_ptr(), 64, NCCL_UINT8, 1, comms[0], st[0])
                r2 = L.ncclRecv(b.data_ptr() + 32, 64, NCCL_UINT8, 1, comms[0], st[0])
                call(0, L.ncclGroupEnd)
                res[1] = [r1, r2]

            errs = run_ranks([rank0])
            rec = {"results": res, "messages": msg}
        else:  # an unmatched receive: an error once the wait limit (1 s for this call) has passed, naming it
            def rank0():
                old = L.fake_rccl_set_wait_limit_ms(1000)
                t0 = time.monotonic()
                try:
                    call(0, lambda: L.ncclRecv(b.data_ptr(), 64, NCCL_UINT8, 1, comms[0], st[0]))
                finally:
                    L.fake_rccl_set_wait_limit_ms(old)
                res[1] = time.monotonic() - t0

            errs = run_ranks([rank0])
            rec = {"results": res, "messages": msg}
        rec["exceptions"] = [repr(e) for e in errs if e is not None]
        torch.cuda.synchronize()
        rec["untouched"] = bool(which == "move" or int(b.count_nonzero()) == 0)
        return rec
    finally:
        for h in comms:
            L.ncclCommDestroy(h)


def main(out_path):
    import conftest  # noqa: F401  (puts the repository root on sys.path)
    import torch

    global assert_shard_matches_whole, whole_frame
    from shard_compare import assert_shard_matches_whole, whole_frame

    from radiancecascade2dglobalillumination_amd import rc2dgi as R

    assert torch.cuda.is_available(), "the ranks need a HIP device"
    path = os.environ["RC2DGI_RCCL_LIB"]
    fake = Fake(path)
    fake.L.fake_rccl_set_wait_limit_ms(WAIT_LIMIT_MS)
    jobs = [("standin:" + w, lambda w=w: run_standin(fake, w)) for w in STANDIN_CASES]
    jobs += [(case_id(c), lambda c=c: run_case(R, fake, c)) for c in CASES]
    jobs += [("reconnect", lambda: run_reconnect(R, fake))]
    only = os.environ.get("RCCL_RANKS_ONLY")  # (substrings of the ids to run, comma-separated: one case by hand)
    with open(out_path, "a") as out:
        for name, job in jobs:
            if only and not any(o in name for o in only.split(",")):
                continue
            t0 = time.monotonic()
            rec = {"case": name}
            stop = False
            try:
                rec.update(job())
            except DeviceError as e:
                rec["device_error"] = str(e)
                stop = True
            except Exception as e:  # noqa: BLE001  (a failing case is its record; the next one still runs)
                rec["exception"] = repr(e)
                stop = isinstance(e, R.RC2DGIError) and not any(m in str(e) for m in TRANSPORT_ERRORS)
            rec["seconds"] = round(time.monotonic() - t0, 3)
            out.write(json.dumps(rec) + "\n")
            out.flush()
            print(f"{name}: {rec['seconds']} s" + (" STOP" if stop else ""), flush=True)
            if stop:
                return 3
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
