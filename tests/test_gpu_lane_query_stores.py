"""The record stores of the record-per-lane read-off (DESIGN.md section 3a''', LaneHub::emit_q)
and the sources' region rows (LaneHub::query_record).  A chunk's five stores, the result and the
four command slots, carry a cache policy of their own: they are written through the L2 instead
of kept in it, which changes no byte of the output.  Everything here runs under
MR_LANE_QUERY=require and compares the raw result, slot and pool bytes with the same plan under
MR_LANE_QUERY=0 (the source-per-lane read-off, whose stores are plain ones), and the labels
with the oracle: after several passes over the same buffers, beside records another kernel of
the pass writes with plain stores, over lines a device fill left dirty just before the pass,
and read by the wire encoder on another stream right after it.  Every case sets MR_HUB_LANE=1
so that small plans take the lane path."""
import ctypes as C

import numpy as np
import pytest

import irregular_maps as im
from golden_util import as_expected
from marshrutka_amd.abi import MR_NOT_FOUND, MR_OK, Params
from marshrutka_amd.mapgen import random_query_cells
from oracle_raw import differing, labels_raw
from test_gpu_lane_query import NONSTD, _query_vs_ref, _run_plan, _switches
from test_gpu_lane_stage import DeviceBytes, _bound, _decoded, hip  # noqa: F401  (hip: a fixture)
from test_gpu_lane_winner import World, _oracle, _same

pytestmark = pytest.mark.gpu

ROW_SLOTS = 4  # the widest row the kernel assembles in registers (kLaneRowSlots): rows of 4 leave whole
LANE_MAX_QUERIES = 32  # a source with more queries runs on hub_kernel
D2H = 2


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
    """Exactly n lane records on w: distinct sources of one query each, the specials among them
    as sources and as destinations (tests/test_gpu_lane_query.py::test_chunk_edges)."""
    rng = np.random.default_rng(seed)
    cells = w.specials + [int(v) for v in rng.permutation(w.V) if int(v) not in set(w.specials)]
    src = np.array(cells[:n], dtype=np.int64)
    dst = rng.integers(0, w.V, size=n)
    dst[:len(w.specials)] = w.specials[::-1]
    dst[len(w.specials)] = src[len(w.specials)]  # (a source asking for itself)
    assert len(src) == n
    return src, dst


def _bound_passes(eng, hip, monkeypatch, w, params, src, dst, mode, mc, passes=3):  # noqa: F811
    """The plan under `mode` with its outputs bound to a zeroed device block and a pool that
    holds every label (in record order after each pass, so byte-deterministic): `passes` passes
    back to back, then the block's bytes, the record order, the decoded records and the stats."""
    _switches(monkeypatch, mode)
    n = len(src)
    plan = eng.Plan(w.g, params, None, max_cmds=mc, query_array=w.m.query_array(src, dst, w.arr))
    blk, rr, cr, orr = _bound(hip, plan, n, mc, max(4096, 8 * n))
    try:
        for _ in range(passes):
            plan.run()
        plan.wait()
        host = blk.read()
        out = {"host": host, "ranges": (rr, cr, orr), "order": np.array(plan.record_queries()), "stats": plan.stats(),
               "decoded": _decoded(eng, w, params, host, rr, cr, orr, n, mc)}
    finally:
        plan.__del__()
        blk.free()
    return out


@pytest.mark.parametrize("mc", [1, 2, 3, 4])
@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_rows_whole_and_narrow(eng, oracle_lib, hip, monkeypatch, w21, n, mc):  # noqa: F811
    """n records (a partial chunk, a full one, one record in a chunk of its own, four chunks and
    one record) at 1 to 4 command slots: rows of 4 leave as whole lines, four lanes a row, the
    narrower ones by their own lanes; at 1 and 2 some labels go to the pool.  Three passes, then
    every byte of the bound results, slots and pool equals the reference read-off's, and the
    decoded records are the oracle's."""
    w, p = w21, Params()
    src, dst = _records(w, n, 100 * n + mc)
    ref = _bound_passes(eng, hip, monkeypatch, w, p, src, dst, "ref", mc)
    got = _bound_passes(eng, hip, monkeypatch, w, p, src, dst, "query", mc)
    assert got["stats"]["lane_sources"] == got["stats"]["num_sources"] == n
    assert (got["order"] == ref["order"]).all()
    for name, (a, b) in zip(("results", "slots", "pool"), got["ranges"]):
        assert np.array_equal(got["host"][a:b], ref["host"][a:b]), f"{name}: bytes differ from the reference read-off's"
    assert np.array_equal(got["host"], ref["host"])
    ores, ocmds = labels_raw(oracle_lib, w.og, p, w.m.query_array(src, dst, w.arr))
    res, cmds = got["decoded"]
    assert np.isin(res["status"], (MR_OK, MR_NOT_FOUND)).all()
    assert len(differing(res, cmds, ores[got["order"]], ocmds)) == 0
    if mc <= 2:
        assert (ores["n"] > mc).any()


@pytest.mark.parametrize("mc", [2, 4])
def test_beside_plain_stores(eng, oracle_lib, monkeypatch, w65, mc):
    """Lane sources of 1 to 3 queries and one source of 40, which stays on hub_kernel: its
    records, written with plain stores in the same pass, lie among the lane records' lines.
    The fetched bytes equal the reference read-off's, and the labels the oracle's."""
    w = w65
    rng = np.random.default_rng(40 + mc)
    plain = [int(v) for v in rng.permutation(w.V) if int(v) not in set(w.specials)]
    counts = [1] * 50 + [2] * 30 + [3] * 21 + [40]
    cells = w.specials[:7] + plain[:len(counts) - 7]
    src = np.concatenate([np.full(c, s) for s, c in zip(cells, counts)])
    dst = rng.integers(0, w.V, size=len(src))
    dst[::9] = np.resize(np.array(w.specials), len(dst[::9]))
    order = rng.permutation(len(src))
    src, dst = src[order], dst[order]
    a = _query_vs_ref(eng, monkeypatch, w, Params(), src, dst, grids=(None, 1), max_cmds=mc)
    assert a["stats"]["lane_sources"] == len(counts) - 1 < a["stats"]["num_sources"] == len(counts)
    _oracle(oracle_lib, w, Params(), a, src, dst)


def _stream_calls(hip):  # noqa: F811
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]


@pytest.mark.parametrize("mc", [3, 4])
def test_over_dirty_lines(eng, oracle_lib, hip, monkeypatch, w21, mc):  # noqa: F811
    """Outputs bound with mr_plan_bind_outputs_ex.  Before each of two passes a device fill on
    the pass's stream sets the whole block to 0xFF, which leaves its lines dirty in the cache
    under the pass's stores; the block is read back on that stream right after the pass.
    Nothing outside the records is written, the records decode to the oracle's labels, every
    slot of a lane record's row is written (zeros from n_commands on, zero pad words), and both
    passes leave the same bytes."""
    w, p = w21, Params()
    n = 257
    src, dst = _records(w, n, 7 + mc)
    _stream_calls(hip)
    s = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s)) == 0
    _switches(monkeypatch, "query")
    plan = eng.Plan(w.g, p, None, max_cmds=mc, query_array=w.m.query_array(src, dst, w.arr))
    blk, rr, cr, orr = _bound(hip, plan, n, mc, max(4096, 8 * n), fill=0xFF)
    try:
        snaps = []
        for _ in range(2):
            assert hip.hipMemsetAsync(C.c_void_p(blk.ptr), 0xFF, blk.nbytes, s) == 0
            plan.run(s.value)
            host = np.zeros(blk.nbytes, dtype=np.uint8)
            assert hip.hipMemcpyAsync(host.ctypes.data, C.c_void_p(blk.ptr), blk.nbytes, D2H, s) == 0
            assert hip.hipStreamSynchronize(s) == 0
            snaps.append(host)
        host = snaps[0]
        assert (snaps[1] == host).all(), "a second pass left other bytes"
        outside = np.ones(len(host), dtype=bool)
        for a, b in (rr, cr, orr):
            outside[a:b] = False
        assert (host[outside] == 0xFF).all(), "bytes outside the records were written"
        q_of = np.array(plan.record_queries())
        ores, ocmds = labels_raw(oracle_lib, w.og, p, w.m.query_array(src, dst, w.arr))
        res, cmds = _decoded(eng, w, p, host, rr, cr, orr, n, mc)
        assert len(differing(res, cmds, ores[q_of], ocmds)) == 0
        assert plan.stats()["lane_sources"] == n
    finally:
        plan.__del__()
        blk.free()
        hip.hipStreamSynchronize(s)
        hip.hipStreamDestroy(s)
    slots = host[cr[0]:cr[1]].view(np.uint32).reshape(n, mc, 4)
    ncmd = host[rr[0]:rr[1]].view(np.uint32).reshape(n, 4)[:, 3] & 0xFFFF
    used = np.where(ncmd > mc, 1, ncmd)  # (a longer label keeps its tag in slot 0)
    past = np.arange(mc)[None, :] >= used[:, None]
    assert not slots[past].any(), "a row has bytes that are not zero past n_commands"
    assert not slots[:, :, 3].any(), "a pad word is not zero"


@pytest.mark.parametrize("mc", [2, 4])
def test_wire_on_second_stream(eng, hip, monkeypatch, w65, mc):  # noqa: F811
    """mr_plan_wire_records on a second stream right after a pass on the first (the encoder
    reads the records the pass's stores wrote, behind the wait for the pass's end event): the
    rows, decoded on the host, are the plan's own fetch.  Whole rows (4 slots) and narrow ones
    (2, where some labels go through the pools)."""
    from marshrutka_amd.pathfinder import result_from_c
    w, p = w65, Params()
    src, dst = random_query_cells(w.m, 2500, 77)
    sp = np.array(w.specials)
    src, dst = np.concatenate([src, sp, src[:len(sp)]]), np.concatenate([dst, dst[:len(sp)], sp])
    n, pcap = len(src), 8 * len(src)
    rw = eng.wire_row_words(mc)
    _stream_calls(hip)
    sa, sb = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(sa)) == 0 and hip.hipStreamCreate(C.byref(sb)) == 0
    _switches(monkeypatch, "query")
    plan = eng.Plan(w.g, p, None, max_cmds=mc, query_array=w.m.query_array(src, dst, w.arr))
    wbuf = DeviceBytes(hip, n * rw * 4 + pcap * 8)
    try:
        plan.run(sa.value)
        assert plan.stats()["fallback_sources"] == 0  # (the passes from here on are one launch each)
        plan.run(sa.value)
        plan.wire_records(wbuf.ptr, wbuf.ptr + n * rw * 4, pcap, stream=sb.value)
        assert hip.hipStreamSynchronize(sb) == 0
        words = wbuf.read().view(np.uint32)
        out, cmds = eng.decode_wire_raw(w.g, p, words[:n * rw], n, mc, words[n * rw:])
        q_of = plan.record_queries()
        got = [None] * n
        for k in range(n):
            assert out[k].status in (0, 1), (k, out[k].status)
            got[q_of[k]] = as_expected(result_from_c(out[k], cmds)) if out[k].status == 0 else None
        assert got == [as_expected(x) for x in plan.fetch()]
        if mc == 2:
            assert any(x is not None and len(x[3]) > mc for x in got)  # some labels went through the wire pool
    finally:
        plan.__del__()
        wbuf.free()
        for s in (sa, sb):
            hip.hipStreamSynchronize(s)
            hip.hipStreamDestroy(s)


def test_sources_of_every_region(eng, oracle_lib, monkeypatch, w65):
    """A record's source decides its region row (the winner table's region byte of the source's
    cell) and so the bits of the winner word it reads.  Sources: every special cell, and
    plain cells of all four homelands (their corners, among them the map's first cell and its
    last one, the highest cell index, and their middles), of the four borders between them (the
    axes' ends and middles) and round every campfire, so that every region row and a cell of no
    campfire's neighbourhood is among them.  Each has five destinations: a source's records span
    lanes and chunks."""
    w = w65
    S, H = w.m.size, w.m.h
    at = lambda x, y: (y + H) * S + (x + H)  # noqa: E731
    spread = [at(sx * a, sy * b) for sx in (-1, 1) for sy in (-1, 1) for a, b in ((H, H), (H // 2, H // 2), (1, H), (H, 1))]
    spread += [at(sx * a, 0) for sx in (-1, 1) for a in (H, H // 2, 2)] + [at(0, sy * a) for sy in (-1, 1) for a in (H, H // 2, 2)]
    near = [c + d for c in w.campfires for d in (1, -1, S, -S, 2 * S + 2, -2 * S - 2) if 0 <= c + d < w.V]
    cells = list(dict.fromkeys(w.specials + [v for v in spread + near if v not in set(w.specials)]))
    assert 0 in cells and w.V - 1 in cells
    rng = np.random.default_rng(29)
    src = np.repeat(np.array(cells, dtype=np.int64), 5)
    dst = rng.integers(0, w.V, size=len(src))
    dst[::5] = np.resize(np.array(w.specials + [0, w.V - 1]), len(dst[::5]))
    for mc in (4, 8):
        a = _query_vs_ref(eng, monkeypatch, w, Params(), src, dst, grids=(None, 1), max_cmds=mc)
        assert a["stats"]["lane_sources"] == a["stats"]["num_sources"] == len(cells)
        _oracle(oracle_lib, w, Params(), a, src, dst)


def test_nonstandard_layout_rows(eng, monkeypatch):
    """The catalogued irregular map of tests/test_gpu_lane_query.py in its transposed
    orientation (the cells' ranks are not the closed form of their positions) at 4 command
    slots: three passes, the bytes of the reference read-off, and py_ref's labels."""
    name, k, pi = NONSTD
    m = im.get_map(name)
    params = im.params_for(m)[pi]
    g = eng.MapGrid(im.oriented(name, k).cells())
    qs = im.capped_queries(name, 200)

    def make():
        plan = eng.Plan(g, params, qs, max_cmds=ROW_SLOTS)
        plan.run()
        plan.run()  # (_run_plan runs the third)
        return plan
    ref = _run_plan(eng, monkeypatch, make, len(qs), "ref")
    assert ref["stats"]["lanes_per_source"] == 1 and ref["stats"]["lane_sources"] > 0
    a = _run_plan(eng, monkeypatch, make, len(qs), "query", labels=True)
    _same(a, ref)
    assert a["labels"] == im.py_ref_labels(name, k, pi, 200)
