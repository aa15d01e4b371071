"""GPU: rc2dgi_do over a communicator at world 2 to 8 -- the JumpFlood send / receive groups, the distRT broadcasts
and the strip-table broadcasts of rc2dgi_group.cpp / rc2dgi_frame.cpp -- bit for bit against the unsharded frame.

Real RCCL puts one rank on one device, so the ranks run as threads of one child process over fake_rccl.cpp, a
stand-in with RCCL's calling semantics that RC2DGI_RCCL_LIB names (the variable is read once per process, and this
process may already hold the real library: hence the child).  rccl_ranks_worker.py runs every case there and writes
one record per case; the tests below assert on their case's record: every rank's textures equal the whole frame in
both frames, and -- so that a pass cannot be vacuous -- the stand-in's log of each rank and frame equals the exchange
derived here from plan_jfa_exchange and the strip rows.  The stand-in itself is driven directly in the same child
(test_standin_*), to show that it moves the right bytes and refuses what it must."""
import json
import os
import subprocess
import sys

import pytest

from rccl_ranks_worker import (CASES, NCCL_INTERNAL_ERROR, NCCL_INVALID_ARGUMENT, NCCL_INVALID_USAGE, RECONNECT,
                               case_id, standin_library)

pytestmark = pytest.mark.gpu

# The child's wall time on an MI355X: 30 s (imports 4 s, the three 4096^2 cases 25 s, everything else 1.5 s); the
# limit is four times that.
MEASURED_SECONDS = 30
CHILD_TIMEOUT = 4 * MEASURED_SECONDS


@pytest.fixture(scope="module")
def R():
    from radiancecascade2dglobalillumination_amd import rc2dgi

    return rc2dgi


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    """One run of the worker in a fresh process; {case id: record} and how the process ended."""
    tmp = tmp_path_factory.mktemp("rccl_ranks")
    out = tmp / "records.jsonl"
    env = dict(os.environ, RC2DGI_RCCL_LIB=standin_library(tmp))
    env.pop("RCCL_RANKS_ONLY", None)
    here = os.path.dirname(os.path.abspath(__file__))
    ended = {}
    try:
        p = subprocess.run([sys.executable, os.path.join(here, "rccl_ranks_worker.py"), str(out)], env=env, cwd=here,
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        ended = {"returncode": p.returncode, "tail": (p.stdout + p.stderr)[-3000:]}
    except subprocess.TimeoutExpired as e:
        ended = {"returncode": None, "tail": f"no end after {CHILD_TIMEOUT} s: {(e.stdout or b'')[-2000:]!r}"}
    records = {}
    if out.exists():
        for line in out.read_text().splitlines():
            rec = json.loads(line)
            records[rec["case"]] = rec
    return records, ended


def record_of(child, name):
    records, ended = child
    assert name in records, f"the worker wrote no record of {name}; it ended with {ended}"
    rec = records[name]
    assert "device_error" not in rec, rec["device_error"]
    assert "exception" not in rec, rec["exception"]
    return rec


def strip_rows(H, q, world):  # rc2dgi_shard_rows, restated
    return q * H // world, (q + 1) * H // world


def strip_table_pieces(W, H, q, world, dist_pitch_bytes):
    """Bytes of shard q's four strip-table pieces (4096^2 and up: bound-table cells of 2^csh texels, 64 a row): its
    march-field rows at 2 B a texel, its cell rows of the bound table (1 B a cell), of the hit flags (1 B) and of the
    palettes (16 entries of 16 B)."""
    csh = 0
    while ((W - 1) >> csh) >= 64 or ((H - 1) >> csh) >= 64:
        csh += 1
    y0, y1 = strip_rows(H, q, world)
    assert y0 % (1 << csh) == 0 and y1 % (1 << csh) == 0
    ncr = (y1 - y0) >> csh
    return [(y1 - y0) * dist_pitch_bytes, ncr * 64, ncr * 64, ncr * 64 * 16 * 16]


def expected_groups(R, W, H, N, rs, world, rank, dist_pitch_bytes, st):
    """The groups of one frame on `rank`, each a list of [kind, peer or root, bytes] in the order posted: one per
    JumpFlood step with a transfer to or from another rank (a transfer appears once on each side, a transfer of a
    shard to itself on neither), then the broadcasts."""
    jump_row = 2 * dist_pitch_bytes  # (jumpRT: 4 B a texel at distRT's pitch in texels, distRT 2 B)
    groups = []
    step = 1
    while True:
        try:
            _, xfers = R.plan_jfa_exchange(W, H, N, world, step, rs)
        except R.RC2DGIError:
            break  # (step == S)
        ops = []
        for src, _src_row, rows, dst, _dst_buf, _dst_row in xfers:
            if src == rank and dst != rank:
                ops.append(["send", dst, rows * jump_row])
            elif dst == rank and src != rank:
                ops.append(["recv", src, rows * jump_row])
        if ops:
            groups.append(ops)
        step += 1
    if st:
        groups.append([["bcast", 0, dist_pitch_bytes]])  # row 0 of distRT
        groups.append([["bcast", q, b] for q in range(world)
                       for b in strip_table_pieces(W, H, q, world, dist_pitch_bytes)])
    else:
        groups.append([["bcast", q, (strip_rows(H, q, world)[1] - strip_rows(H, q, world)[0]) * dist_pitch_bytes]
                       for q in range(world)])
    return groups, step - 1  # (and the number of exchange steps planned)


def logged_groups(log):
    """[[kind, peer, bytes, group], ...] -> the groups in order, and their indices."""
    groups, idx = [], []
    for kind, peer, nbytes, g in log:
        if not idx or idx[-1] != g:
            groups.append([])
            idx.append(g)
        groups[-1].append([kind, peer, nbytes])
    return groups, idx


def check_frames(R, rec, W, H, N, rs, world, n_frames, first_group=None):
    frames = rec["frames"]
    assert len(frames) == n_frames
    st = rec["expect_st"]
    next_group = list(first_group or [0] * world)
    for f, fr in enumerate(frames):
        assert fr["errors"] == [None] * world, f"frame {f}: {fr['errors']}"
        assert fr["differs"] == [None] * world, f"frame {f}: {fr['differs']}"
        assert fr["st"] == [int(st)] * world, f"frame {f}: strip_tables_active {fr['st']}"
        for k in range(world):
            want, _ = expected_groups(R, W, H, N, rs, world, k, rec["dist_pitch_bytes"], st)
            got, idx = logged_groups(fr["log"][k])
            assert got == want, f"frame {f} rank {k}: the transport ran {got}, the plan says {want}"
            assert idx == list(range(next_group[k], next_group[k] + len(want))), (f, k, idx)
            next_group[k] += len(want)
            n_bcast = sum(1 for e in fr["log"][k] if e[0] == "bcast")
            assert n_bcast == (1 + 4 * world if st else world), (f, k, n_bcast)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_ranks_match_whole_frame(R, child, case):
    W, H, N, _rr, rs, _blur, world, _scene, storage, stk = case
    rec = record_of(child, case_id(case))
    assert rec["expect_st"] == (bool(stk) and W == H and W >= 4096 and storage == "f32")
    check_frames(R, rec, W, H, N, rs, world, 2)


def test_the_cases_reach_the_exchange_steps(R):
    """The plan behind the log assertions is not empty where the cases say so: no step at 2 x 2, one at 3 x 2, a
    transfer between ranks in every other case, a transfer into a block buffer (dst_buf 1 or 2) at 256^2 / 8, and a
    transfer of a shard to itself (a device copy inside the open group) in the cases chosen for it."""
    for case in CASES:
        W, H, N, _rr, rs, _blur, world, *_ = case
        bufs, between, steps, own = set(), 0, 0, 0
        for step in range(1, 16):
            try:
                _, xfers = R.plan_jfa_exchange(W, H, N, world, step, rs)
            except R.RC2DGIError:
                break
            steps += 1
            bufs |= {x[4] for x in xfers}
            between += sum(1 for x in xfers if x[0] != x[3])
            own += sum(1 for x in xfers if x[0] == x[3])
        if (W, H) == (2, 2):
            assert steps == 0
        else:
            assert steps >= 1 and between > 0, case
        if (W, H, world) == (256, 256, 8):
            assert {1, 2} <= bufs, bufs
        if (W, H) in ((200, 122), (200, 120), (3, 2)):
            assert own > 0, case


def test_reconnect_to_a_larger_world(R, child):
    """A frame at world 2, then set_shard(k, 4) on four contexts (two of them new), a new id and a frame: the dropped
    communicator and the reallocated windows leave nothing behind, and the old communicator sees no further call."""
    W, H, N, _rr, rs, _blur, _scene = RECONNECT
    rec = record_of(child, "reconnect")
    first = dict(rec, frames=rec["frames"][:1])
    second = dict(rec, frames=rec["frames"][1:])
    check_frames(R, first, W, H, N, rs, 2, 1)
    check_frames(R, second, W, H, N, rs, 4, 1)
    assert rec["old_log_after"] == rec["old_log_first"]


def test_standin_moves_the_right_bytes(child):
    rec = record_of(child, "standin:move")
    assert rec["exceptions"] == [] and rec["results"] == [0, 0]
    assert rec["moved"], "ncclSend / ncclRecv: the receiver's buffer differs from the sender's rows"
    assert rec["broadcast"], "ncclBroadcast: the non-root buffer differs from the root's"
    assert rec["log"] == [[["send", 1, 900, 0], ["bcast", 1, 512, 1]], [["recv", 0, 900, 0], ["bcast", 1, 512, 1]]]


def test_standin_refuses_a_differing_byte_count(child):
    rec = record_of(child, "standin:bytes")
    assert rec["exceptions"] == [] and rec["results"] == [NCCL_INVALID_ARGUMENT] * 2, rec
    assert "100 bytes" in rec["messages"][0] and "96 bytes" in rec["messages"][0]
    assert rec["untouched"]


def test_standin_refuses_disagreeing_roots(child):
    rec = record_of(child, "standin:roots")
    assert rec["exceptions"] == [] and rec["results"] == [NCCL_INVALID_ARGUMENT] * 2, rec
    assert rec["untouched"]


def test_standin_refuses_an_overlapping_receive(child):
    rec = record_of(child, "standin:overlap")
    assert rec["exceptions"] == [] and rec["results"] == [NCCL_INVALID_USAGE, [0, 0]], rec
    assert "overlapping" in rec["messages"][0]
    assert rec["untouched"]


def test_standin_names_an_unmatched_receive(child):
    rec = record_of(child, "standin:unmatched")
    assert rec["exceptions"] == [] and rec["results"][0] == NCCL_INTERNAL_ERROR, rec
    assert 0.9 <= rec["results"][1] < 5.0, f"waited {rec['results'][1]} s at a limit of 1 s"
    assert "recv on rank 0, peer 1, 64 bytes" in rec["messages"][0], rec["messages"]
    assert rec["untouched"]


def test_worker_ran_to_its_end(child):
    records, ended = child
    assert ended["returncode"] == 0, ended
    assert len(records) == 5 + len(CASES) + 1, sorted(records)
