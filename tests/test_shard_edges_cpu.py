"""CPU: the shapes of tests/test_gpu_shard_edges.py reach what they are chosen for, asserted with the host-only
planners of the C ABI (rc2dgi_plan_rows, rc2dgi_plan_jfa_exchange, rc2dgi_plan_group_waits): no device.

A thin-strip shape is there for the JumpFlood exchange of strips of one to four rows: block steps up to the last one,
a step whose shifted taps share a block, block requests gathered from several owners, ranks that await many peers.  A
schedule shape is there for level plans whose row windows start at odd rows, end off the tiles' grid and wrap."""
import pytest

import oracle
from radiancecascade2dglobalillumination_amd import rc2dgi as R
from rccl_ranks_worker import CASES as RANK_CASES
from shard_edge_cases import FILL, SWEEPS, THIN, strip, thin_id


def exchange(W, H, N, world, rs=1.0):
    """{step: (info, transfers)} of every exchange step 1 .. S-1"""
    S = oracle.dims(oracle.Params(W=W, H=H, N=N, render_scale=rs))[2]
    assert S >= 2, (W, H, S)
    return {t: R.plan_jfa_exchange(W, H, N, world, t, rs) for t in range(1, S)}


def block_sources(xfers):
    """{(receiver, block buffer): the shards its rows come from} of one step's transfers"""
    req = {}
    for src, _src_row, _rows, dst, dst_buf, _dst_row in xfers:
        if dst_buf > 0:
            req.setdefault((dst, dst_buf), set()).add(src)
    return req


def reached(W, H, N, world, rs=1.0):
    """What the exchange plan of a shape shows: the names of shard_edge_cases.Thin.reaches that hold, "block_step",
    and "four_peers"."""
    plan = exchange(W, H, N, world, rs)
    got = set()
    if all(info["halo"] == 0 for info, _ in plan.values()):
        got.add("all_block")
    if any(info["halo"] == 0 for info, _ in plan.values()):
        got.add("block_step")
    if any(info["same_block"] == 1 for info, _ in plan.values()):
        got.add("same_block")
    if any(len(srcs) >= 3 for _, xf in plan.values() for srcs in block_sources(xf).values()):
        got.add("three_sources")
    for t in plan:
        for k in range(world):
            readers, senders = R.plan_group_waits(W, H, N, world, k, t, rs)
            if len(set(readers) | set(senders)) >= 4:
                got.add("four_peers")
    return got


@pytest.mark.parametrize("case", THIN, ids=thin_id)
def test_thin_shapes_reach_their_exchange_paths(case):
    heights = {b - a for a, b in (strip(case.H, r, case.world) for r in range(case.world))}
    assert heights == case.heights, heights
    got = reached(case.W, case.H, case.N, case.world, case.rs)
    assert "block_step" in got and "four_peers" in got, got
    # every step 1 .. S-1 a block step, the last included: what one-row strips do, and only they (the last step's
    # shift is one row, which a taller strip takes as a halo of its window)
    assert ("all_block" in got) == (case.heights == {1}), (got, heights)
    assert got - {"block_step", "four_peers"} == set(case.reaches), got


def test_thin_shapes_cover_every_exchange_path():
    """Each path is reached by some shape the GPU test runs; the one-row shapes are block steps throughout."""
    union = set().union(*(t.reaches for t in THIN))
    assert union == {"all_block", "same_block", "three_sources"}
    for t in THIN:
        if t.heights == {1}:
            assert all(info["halo"] == 0 for info, _ in exchange(t.W, t.H, t.N, t.world, t.rs).values()), thin_id(t)


def test_the_uneven_thin_shape_has_two_strip_heights_and_a_padded_cascade():
    t = next(t for t in THIN if (t.W, t.H, t.rs) == (96, 50, 1.0))
    assert {b - a for a, b in (strip(t.H, r, t.world) for r in range(t.world))} == {3, 4}
    CW, CH, _ = oracle.dims(oracle.Params(W=t.W, H=t.H, N=t.N, render_scale=t.rs))
    assert (CW, CH) == (96, 56)


def test_cascade_sizes_of_the_scaled_thin_shapes():
    sizes = {(t.W, t.H, t.rs): oracle.dims(oracle.Params(W=t.W, H=t.H, N=t.N, render_scale=t.rs))[:2] for t in THIN}
    assert sizes[(128, 64, 0.5)] == (64, 32)     # coarser than the screen
    assert sizes[(96, 50, 1.7)] == (168, 88)     # finer than the screen
    assert sizes[(128, 64, 1.0)] == (128, 64)    # the fused blur + merge: cascades the size of the screen


@pytest.mark.parametrize("case", SWEEPS + [FILL], ids=lambda s: f"{s.W}x{s.H}-N{s.N}-w{s.world}")
def test_schedule_shapes_cut_the_tiles(case):
    W, H, N, _rr, blur, world = case
    plans = [[R.plan_rows(W, H, N, blur, r, world, R.PLAN_LEVEL + L) for r in range(world)] for L in range(N)]
    for L in range(N - 1):  # a tile origin at an odd row, at every level below the top
        assert any(a % 2 == 1 for ivs in plans[L] for a, _ in ivs), (L, plans[L])
    # a last tile cut short: an interval that ends off the 8-row grid of the smallest tiles
    assert any(b % 8 for lv in plans for ivs in lv for _, b in ivs)
    # the wrap: a set of two intervals on the first or the last rank
    assert any(len(plans[L][r]) == 2 for L in range(N) for r in (0, world - 1))
    for lv in plans:  # (every rank computes some row of every level)
        assert all(ivs for ivs in lv)


def test_sweep_strips_are_uneven():
    W, H, _N, _rr, _blur, world = SWEEPS[0]
    assert [b - a for a, b in (strip(H, r, world) for r in range(world))] == [85, 85, 86]


def test_thin_cases_over_the_communicator_have_block_steps():
    """The two thin cases of rccl_ranks_worker.CASES: strips of one and two rows whose long steps are block steps; one
    of them serves a block request from three owners and has a step on one shared block."""
    thin = [c for c in RANK_CASES if (c[0], c[1]) in ((64, 12), (128, 16))]
    assert len(thin) == 2
    got = {(c[0], c[1]): reached(c[0], c[1], c[2], c[6], c[4]) for c in thin}
    assert all("block_step" in g and "four_peers" in g for g in got.values()), got
    assert {"three_sources", "same_block"} <= got[(64, 12)], got
    heights = {(c[0], c[1]): {b - a for a, b in (strip(c[1], r, c[6]) for r in range(c[6]))} for c in thin}
    assert heights == {(64, 12): {1, 2}, (128, 16): {2}}
