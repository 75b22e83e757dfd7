"""The record-per-lane read-off's chunk pipeline (DESIGN.md section 3a''', the kLaneQuery loop of
hub_lane_memo_kernel and LaneHub::emit_q): a wave loads the source cells and destinations two
chunks ahead and the two gathers one chunk ahead, every lane of a chunk's wave goes through one
store block (the result and, in plans of up to four command slots, a row assembled in registers
and stored through a buffer of the chunk's exact size), and the look-aheads past a wave's last
chunk read the plan's last record.  MR_LANE_QUERY=require against MR_LANE_QUERY=0 with
MR_LANE_WIN=require, byte for byte (results, pool, record order, fallback list, stats), and the
oracle's labels, on 21^2 seed 7 and 65^2 seed 2024 with MR_HUB_LANE=1.  On both maps every
label has one to four commands (a source asking for itself: one), and no pair is without a path."""
import numpy as np
import pytest

from marshrutka_amd.abi import MR_OK, Params
from marshrutka_amd.mapgen import random_query_cells
from oracle_raw import RESULT, differing, labels_raw
from test_gpu_lane_query import _query_vs_ref, _run_plan, _switches
from test_gpu_lane_stage import _bound, _decoded, hip  # noqa: F401  (hip: a fixture)
from test_gpu_lane_winner import World, _oracle, _same

pytestmark = pytest.mark.gpu

LANE_MAX_QUERIES = 32  # a source with more queries runs on hub_kernel
LONGEST = 4            # commands of the longest label on either map


@pytest.fixture(scope="module")
def eng():
    from marshrutka_amd import build, pathfinder
    build.build()
    if not pathfinder.device_available():
        pytest.fail("no gfx950 device visible to the GPU tests")
    return pathfinder


@pytest.fixture(scope="module")
def w21(eng, oracle_lib):
    return World(eng, oracle_lib, 21, 7)


@pytest.fixture(scope="module")
def w65(eng, oracle_lib):
    return World(eng, oracle_lib, 65, 2024)


def _records(w, n, seed):
    """Exactly n lane records: sources of 1, 32, 1, 5, 2, 1, 3, ... queries (so a chunk holds
    sources of one query beside one of 32), every third source a special cell until they run
    out; destinations random, every fifth a special, every eleventh the record's own source."""
    rng = np.random.default_rng(seed)
    sp = list(w.specials)
    plain = [int(v) for v in rng.permutation(w.V) if int(v) not in set(sp)]
    counts, cells, left, i = [], [], n, 0
    while left:
        c = min(left, (1, LANE_MAX_QUERIES, 1, 5, 2, 1, 3)[i % 7])
        cells.append(sp.pop() if (i % 3 == 1 and sp) else plain.pop())
        counts.append(c)
        left -= c
        i += 1
    src = np.concatenate([np.full(c, s, dtype=np.int64) for s, c in zip(cells, counts)])
    dst = rng.integers(0, w.V, size=n)
    dst[::5] = np.resize(np.array(w.specials), len(dst[::5]))
    dst[::11] = src[::11]
    order = rng.permutation(n)
    return src[order], dst[order], len(cells)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 767, 769, 1025])
def test_pipeline_edges(eng, oracle_lib, monkeypatch, w21, n):
    """n records on 21^2 under one workgroup (MR_LANE_QUERY_GRID=1: four waves walk the chunks
    at stride four, so a wave walks 0, 1, 2, 3 or 5 chunks, the chunks one and two ahead fall
    past the end in every combination and the last chunk is full, partial or one record), the
    default grid, and a wave per chunk (=full)."""
    w = w21
    src, dst, k = _records(w, n, 100 + n)
    a = _query_vs_ref(eng, monkeypatch, w, Params(), src, dst, grids=(1, None, "full"), max_cmds=4)
    assert a["stats"]["lane_sources"] == a["stats"]["num_sources"] == k
    _oracle(oracle_lib, w, Params(), a, src, dst)


@pytest.mark.parametrize("mc", [1, 2, 3, 4, 8, 16])
def test_row_shapes(eng, oracle_lib, monkeypatch, w65, mc):
    """Rows of 1, 2, 3 (48 bytes: they straddle lines), 4, 8 and 16 slots on 65^2: labels of
    every length the map has (1 .. 4), so at 1, 2 and 3 slots some go to the overflow pool with
    their tag in slot 0; specials as sources and as destinations among plain records; one
    workgroup and the default grid."""
    w, p = w65, Params()
    src, dst = random_query_cells(w.m, 2500, 70 + mc)
    sp = np.array(w.specials)
    src = np.concatenate([src, sp, src[:len(sp)], src[:40]])
    dst = np.concatenate([dst, dst[:len(sp)], sp, src[-40:]])
    order = np.random.default_rng(mc).permutation(len(src))
    src, dst = src[order], dst[order]
    a = _query_vs_ref(eng, monkeypatch, w, p, src, dst, grids=(None, 1), max_cmds=mc)
    lens = a["res"].view(RESULT)["n"]
    assert set(lens.tolist()) == set(range(1, LONGEST + 1))
    assert (a["res"].view(RESULT)["status"] == MR_OK).all()
    _oracle(oracle_lib, w, p, a, src, dst, pick=range(0, len(src), 4))


@pytest.mark.parametrize("mc,offset", [(1, 0), (3, 16), (4, 48)])
def test_bound_rows(eng, oracle_lib, hip, monkeypatch, w21, mc, offset):  # noqa: F811
    """257 records (four full chunks and one record) into a caller's buffers filled with 0xA5,
    the record bases `offset` bytes past a 256-byte boundary and the pool of the plan's own
    size: nothing outside the records is written (the last chunk's store block covers one
    record), the records decode to the oracle's labels, the slots from n_commands on of every
    row are zero where the plan has at most four (a long label's: from slot 1 on), every pad
    word written is zero, and a second pass leaves the same bytes."""
    w, p, n = w21, Params(), 257
    src, dst, _ = _records(w, n, 9)
    q = w.m.query_array(src, dst, w.arr)
    ores, ocmds = labels_raw(oracle_lib, w.og, p, q)
    _switches(monkeypatch, "query", (("MR_LANE_QUERY_GRID", "1"),))
    plan = eng.Plan(w.g, p, None, max_cmds=mc, query_array=q)
    blk, rr, cr, orr = _bound(hip, plan, n, mc, max(4096, 8 * n), offset, 0xA5)
    try:
        snaps = []
        for _ in range(2):
            plan.run()
            plan.wait()
            snaps.append(blk.read())
        host = snaps[0]
        assert (snaps[1] == host).all(), "a second pass wrote other bytes"
        outside = np.ones(len(host), dtype=bool)
        for lo, hi in (rr, cr, orr):
            outside[lo:hi] = False
        assert (host[outside] == 0xA5).all(), "bytes outside the records were written"
        q_of = np.array(plan.record_queries())
        res, cmds = _decoded(eng, w, p, host, rr, cr, orr, n, mc)
    finally:
        plan.__del__()
        blk.free()
    assert (res["status"] == MR_OK).all()
    assert len(differing(res, cmds, ores[q_of], ocmds)) == 0
    slots = host[cr[0]:cr[1]].view(np.uint32).reshape(n, mc, 4)
    ncmd = host[rr[0]:rr[1]].view(np.uint32).reshape(n, 4)[:, 3] & 0xFFFF
    assert (ncmd > mc).any() == (mc < LONGEST)
    used = np.where(ncmd > mc, 1, ncmd)  # (a longer label keeps its tag in slot 0)
    past = np.arange(mc)[None, :] >= used[:, None]
    assert not slots[past].any(), "a row has non-zero bytes past n_commands"
    assert not slots[:, :, 3].any(), "a pad word is not zero"


def test_three_passes(eng, oracle_lib, monkeypatch, w65):
    """Three passes of one plan, then the fetch: the persistent waves leave nothing in LDS or
    in the counters (the overflow pool's offsets start again each pass: max_cmds 2 sends the
    longer labels there).  Same bytes as one pass of the reference mode."""
    w, p, mc = w65, Params(), 2
    src, dst, _ = _records(w, 1500, 3)
    q = w.m.query_array(src, dst, w.arr)

    def make():
        plan = eng.Plan(w.g, p, None, max_cmds=mc, query_array=q)
        plan.run()
        plan.run()
        return plan

    ref = _run_plan(eng, monkeypatch, lambda: eng.Plan(w.g, p, None, max_cmds=mc, query_array=q), len(q), "ref")
    for env in ((), (("MR_LANE_QUERY_GRID", "2"),)):
        a = _run_plan(eng, monkeypatch, make, len(q), "query", env=env)
        assert (a["res"].view(RESULT)["n"] > mc).any()
        _same(a, ref)
    _oracle(oracle_lib, w, p, ref, src, dst, pick=range(0, len(src), 3))
