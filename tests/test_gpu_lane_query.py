"""The lane memo with a record per lane (DESIGN.md section 3a''', LaneHub::query_record):
where a plan reads its destinations off the winner table and no memo row has a blocker,
hub_lane_memo_kernel<.., kLaneQuery> gives each lane one record of the plan's grouped order
(its source's cell from KArgs::q_srcv), and persistent waves walk the chunks of 64 records at
the grid's stride.  MR_LANE_QUERY=require makes plan creation fail where that kernel is not
used, so a plan created under it ran it; MR_LANE_QUERY=0 with MR_LANE_WIN=require is the
source-per-lane read-off.  Both must give the same bytes (results, command pool, record
order, fallback list, stats), and the oracle's labels.  MR_LANE_QUERY_GRID caps the launch's
workgroups, so that a small plan's waves walk several chunks.  Every case sets MR_HUB_LANE=1
so that small plans take the lane path."""
import numpy as np
import pytest

import irregular_maps as im
from golden_util import as_expected
from marshrutka_amd.abi import MR_ERR_CAPACITY, MR_ERR_INVALID_ARG, SORT_LEGS, SORT_MONEY, SORT_TIME, Params
from marshrutka_amd.mapgen import random_query_cells
from oracle_raw import RESULT, differing, labels_raw
from test_gpu_lane_stage import _bound, _decoded, hip  # noqa: F401  (hip: a fixture)
from test_gpu_lane_winner import World, _live, _oracle, _same

pytestmark = pytest.mark.gpu

# mode -> (MR_LANE_MEMO, MR_LANE_WIN, MR_LANE_QUERY)
MODES = {"query": ("require", "require", "require"), "ref": ("require", "require", "0"), "default": (None, None, None),
         "off": (None, None, "0")}
SWITCHES = ("MR_LANE_MEMO", "MR_LANE_WIN", "MR_LANE_QUERY")
LANE_MAX_QUERIES = 32  # a source with more queries runs on hub_kernel


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


def _switches(monkeypatch, mode, env=()):
    monkeypatch.setenv("MR_HUB_LANE", "1")
    for k in ("MR_DEV_GROUP", "MR_LANE_WIN_BUDGET", "MR_LANE_STAGE", "MR_LANE_LDS_PAD", "MR_LANE_QUERY_GRID"):
        monkeypatch.delenv(k, raising=False)
    for k, v in zip(SWITCHES, MODES[mode]):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    for k, v in env:
        monkeypatch.setenv(k, v)


def _run_plan(eng, monkeypatch, make_plan, n, mode, env=(), labels=False):
    """make_plan() under the mode's switches; the plan's raw bytes, order, fallback list and stats."""
    _switches(monkeypatch, mode, env)
    plan = make_plan()
    plan.run()
    res, pool = plan.fetch_raw()
    r = np.frombuffer(res, dtype=np.uint8, count=n * 32).copy()
    ncmd = int(r.view(RESULT)["n"].astype(np.int64).sum())
    p = np.frombuffer(pool, dtype=np.uint8, count=ncmd * 40).copy()
    out = {"res": r, "pool": p, "order": plan.record_queries(), "fallback": [str(c) for c in plan.fallback_sources()],
           "stats": plan.stats()}
    if labels:
        out["labels"] = [as_expected(x) for x in plan.fetch()]
    plan.__del__()
    return out


def _run(eng, monkeypatch, w, params, src, dst, mode, max_cmds=8, env=()):
    q = w.m.query_array(src, dst, w.arr)
    return _run_plan(eng, monkeypatch, lambda: eng.Plan(w.g, params, None, max_cmds=max_cmds, query_array=q), len(q), mode, env)


def _query_vs_ref(eng, monkeypatch, w, params, src, dst, grids=(None,), **kw):
    """The record-per-lane kernel (once per entry of `grids`: a MR_LANE_QUERY_GRID value, None
    for the default grid) against the source-per-lane read-off."""
    env = tuple(kw.pop("env", ()))
    ref = _run(eng, monkeypatch, w, params, src, dst, "ref", env=env, **kw)
    assert ref["stats"]["lanes_per_source"] == 1 and ref["stats"]["lane_sources"] > 0
    for grid in grids:
        e = env + ((("MR_LANE_QUERY_GRID", str(grid)),) if grid is not None else ())
        _same(_run(eng, monkeypatch, w, params, src, dst, "query", env=e, **kw), ref)
    return ref


def test_all_pairs_21(eng, oracle_lib, monkeypatch, w21):
    """21^2 seed 7: all 441 x 441 (source, destination) pairs in 14 plans of 441 sources x at
    most 32 destinations (tests/test_gpu_lane_winner.py's construction).  Every source has 32
    queries (the last plan: 25), so a wave's 64 records span two or three sources.  Every
    plan's bytes equal the reference mode's, and every label is the oracle's."""
    w, V, p = w21, w21.V, Params()
    src_all, dst_all, res_all, pool_all, base = [], [], [], [], 0
    for d0 in range(0, V, 32):
        d = np.arange(d0, min(V, d0 + 32))
        src, dst = np.repeat(np.arange(V), len(d)), np.tile(d, V)
        a = _query_vs_ref(eng, monkeypatch, w, p, src, dst)
        r = a["res"].view(RESULT).copy()
        r["off"] += base
        base += len(a["pool"]) // 40
        src_all.append(src), dst_all.append(dst), res_all.append(r.view(np.uint8)), pool_all.append(a["pool"])
    src, dst = np.concatenate(src_all), np.concatenate(dst_all)
    assert len(src) == V * V
    _oracle(oracle_lib, w, p, {"res": np.concatenate(res_all), "pool": np.concatenate(pool_all)}, src, dst)


@pytest.mark.parametrize("sort_by", [(SORT_LEGS, SORT_MONEY), (SORT_LEGS, SORT_TIME)])
def test_random_queries_65(eng, oracle_lib, monkeypatch, w65, sort_by):
    """65^2 seed 2024, both Legs-first orders: 6 000 random queries plus every special as a
    source and as a destination, with the default grid and with two workgroups (eight waves
    walk the ~95 chunks); 500 labels against the oracle."""
    w, p = w65, Params(sort_by=sort_by)
    src, dst = random_query_cells(w.m, 6000, 65)
    sp = np.array(w.specials)
    src = np.concatenate([src, src[:len(sp)], sp, sp])
    dst = np.concatenate([dst, sp, dst[:len(sp)], sp[::-1]])
    a = _query_vs_ref(eng, monkeypatch, w, p, src, dst, grids=(None, 2))
    extra = list(range(6000, len(src)))
    pick = sorted(set(np.linspace(0, 5999, 500 - len(extra)).astype(int).tolist())) + extra
    assert len(pick) == 500
    _oracle(oracle_lib, w, p, a, src, dst, pick=pick)


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 513])
def test_chunk_edges(eng, oracle_lib, monkeypatch, w21, n):
    """Exactly n lane records on 21^2: distinct sources of one query each (the specials among
    them), and where n is more than the map's 441 cells, 441 sources of which n - 441 have
    two.  One workgroup (MR_LANE_QUERY_GRID=1: its four waves wrap round the chunks) and the
    default grid; a partial last chunk, a full one, and one record in a chunk of its own."""
    w = w21
    rng = np.random.default_rng(n)
    cells = w.specials + [int(v) for v in rng.permutation(w.V) if int(v) not in set(w.specials)]
    k = min(n, w.V)
    src = np.array(cells[:k] + cells[:n - k], dtype=np.int64)
    dst = rng.integers(0, w.V, size=n)
    dst[:len(w.specials)] = w.specials[::-1]
    dst[len(w.specials)] = src[len(w.specials)]  # (a source asking for itself)
    assert len(src) == n and np.bincount(src).max() <= 2
    a = _query_vs_ref(eng, monkeypatch, w, Params(), src, dst, grids=(1, None))
    assert a["stats"]["lane_sources"] == a["stats"]["num_sources"] == k
    _oracle(oracle_lib, w, Params(), a, src, dst)


def test_mixed_counts_65(eng, oracle_lib, monkeypatch, w65):
    """Sources of 1, 2, 3, 5, 31 and 32 queries in uneven numbers: the count classes change in
    the middle of a wave, and a chunk holds the end of one source and the start of the next.
    A source of 40 queries beside them stays on hub_kernel."""
    w = w65
    rng = np.random.default_rng(11)
    plain = [int(v) for v in rng.permutation(w.V) if int(v) not in set(w.specials)]
    counts = [1] * 37 + [2] * 21 + [3] * 10 + [5] * 7 + [31] * 3 + [32] * 5 + [40]
    cells = w.specials[:9] + plain[:len(counts) - 9]
    src = np.concatenate([np.full(c, s) for s, c in zip(cells, counts)])
    dst = rng.integers(0, w.V, size=len(src))
    dst[::7] = np.resize(np.array(w.specials), len(dst[::7]))
    order = rng.permutation(len(src))
    src, dst = src[order], dst[order]
    a = _query_vs_ref(eng, monkeypatch, w, Params(), src, dst, grids=(None, 1))
    assert a["stats"]["lane_sources"] == len(counts) - 1 < a["stats"]["num_sources"] == len(counts)
    _oracle(oracle_lib, w, Params(), a, src, dst)


@pytest.mark.parametrize("mc", [1, 2, 4, 16])
def test_max_cmds(eng, oracle_lib, monkeypatch, w65, mc):
    """Command rows of 1, 2, 4 and 16 slots; at 1 and 2 some labels go to the overflow pool
    (the fetch lays the pool out in query order, so its bytes do not depend on the order in
    which the lanes took their pool offsets)."""
    w, p = w65, Params()
    src, dst = random_query_cells(w.m, 2500, 40 + mc)
    sp = np.array(w.specials)
    src, dst = np.concatenate([src, sp, src[:len(sp)]]), np.concatenate([dst, dst[:len(sp)], sp])
    a = _query_vs_ref(eng, monkeypatch, w, p, src, dst, grids=(None, 3), max_cmds=mc)
    if mc <= 2:
        assert (a["res"].view(RESULT)["n"] > mc).any()
    _oracle(oracle_lib, w, p, a, src, dst, pick=range(0, len(src), 5))


@pytest.mark.parametrize("case", ["sfm", "route_guru_0", "route_guru_6", "hq_on_campfire", "hq_off_campfire", "homeland_2",
                                  "dev_group_0", "dev_group_1"])
def test_params_variants(eng, oracle_lib, monkeypatch, case):
    """tests/test_gpu_lane_winner.py's six parameter sets on 21^2 seed 11 (3 campfires per
    homeland), and the host's and the device's grouping of the queries (the record sources
    are expanded from either's block)."""
    w = World(eng, oracle_lib, 21, 11, cf=3)
    plain = next(v for v in range(w.V) if v not in set(w.specials))
    p = {"sfm": Params(use_sfm=True),
         "route_guru_0": Params(route_guru=0, scroll_of_escape_cost=7),
         "route_guru_6": Params(route_guru=6),
         "hq_on_campfire": Params(hq_position=w.m.index_at(w.campfires[2])),
         "hq_off_campfire": Params(hq_position=w.m.index_at(plain)),
         "homeland_2": Params(homeland=2)}.get(case, Params())
    src, dst = random_query_cells(w.m, 1500, 6)
    hq = [w.m.cell_of(p.hq_position)] if p.hq_position is not None else []
    src = np.concatenate([src, np.array(hq + w.specials, dtype=np.int64)])
    dst = np.concatenate([dst, np.array((hq + w.specials)[::-1], dtype=np.int64)])
    env = (("MR_DEV_GROUP", case[-1]),) if case.startswith("dev_group") else ()
    a = _query_vs_ref(eng, monkeypatch, w, p, src, dst, grids=(None, 2), env=env)
    _oracle(oracle_lib, w, p, a, src, dst)


NONSTD = ("ties", 5, 0)  # (catalogued map, a transposed orientation, parameter set): 6 regions, 17 specials


def test_nonstandard_layout(eng, monkeypatch):
    """A catalogued irregular map in a transposed orientation (mr_grid rank_std false: a
    source's and a destination's rank and special entry come from the grid's {sinfo, rank}
    record, LaneHub::cell_word's other branch), with a parameter set whose plan passes every
    gate under `require`: the bytes of the reference mode, and py_ref's labels."""
    name, k, pi = NONSTD
    m = im.get_map(name)
    params = im.params_for(m)[pi]
    g = eng.MapGrid(im.oriented(name, k).cells())
    qs = im.capped_queries(name, 200)
    make = lambda: eng.Plan(g, params, qs)  # noqa: E731
    ref = _run_plan(eng, monkeypatch, make, len(qs), "ref")
    assert ref["stats"]["lanes_per_source"] == 1 and ref["stats"]["lane_sources"] > 0
    for env in ((), (("MR_LANE_QUERY_GRID", "1"),)):
        a = _run_plan(eng, monkeypatch, make, len(qs), "query", env=env, labels=True)
        _same(a, ref)
        assert a["labels"] == im.py_ref_labels(name, k, pi, 200)


def test_switch(eng, oracle_lib, monkeypatch, w21):
    """Under `require` a plan outside the gate fails with MR_ERR_INVALID_ARG and the reason: a
    Money-first order (no lane memo), and MR_LANE_WIN=0 (no winner table).  With nothing set
    the same plans run, and give the bytes of MR_LANE_QUERY=0."""
    w = w21
    src, dst = random_query_cells(w.m, 1500, 21)
    money = Params(sort_by=(SORT_MONEY, SORT_LEGS))
    q = w.m.query_array(src, dst, w.arr)
    make = lambda p: (lambda: eng.Plan(w.g, p, None, max_cmds=8, query_array=q))  # noqa: E731
    for p, env, word in ((money, (("MR_LANE_MEMO", "1"), ("MR_LANE_WIN", "1")), "no winner table"),
                         (Params(), (("MR_LANE_WIN", "0"),), "no winner table")):
        with pytest.raises(eng.EngineError) as ei:
            _run_plan(eng, monkeypatch, make(p), len(q), "query", env=env)
        assert ei.value.status == MR_ERR_INVALID_ARG and "MR_LANE_QUERY=require" in str(ei.value) and word in str(ei.value)
        a = _run_plan(eng, monkeypatch, make(p), len(q), "default", env=env[-1:])
        _same(a, _run_plan(eng, monkeypatch, make(p), len(q), "off", env=env[-1:]))
        _oracle(oracle_lib, w, p, a, src, dst, pick=range(0, len(src), 3))
    _same(_run(eng, monkeypatch, w, Params(), src, dst, "default"), _run(eng, monkeypatch, w, Params(), src, dst, "ref"))


def test_bound_overflow_pool(eng, oracle_lib, hip, monkeypatch, w65):
    """max_cmds 2 and a caller's overflow pool.  Which labels fit a pool that is too small
    depends on the order in which they take their space: a plan bound to a pool smaller than
    its own keeps the source-per-lane read-off, where a source's records take theirs in
    record order (tests/test_gpu_lane_stage.py's construction: every long label belongs to
    one source, so record j of it fits exactly when the lengths up to it do).  With a pool of
    the plan's own size every label fits whatever the order, the record-per-lane kernel runs,
    and the decoded records are the oracle's."""
    w, p, mc = w65, Params(), 2
    rng = np.random.default_rng(5)
    plain = [int(v) for v in rng.permutation(w.V) if int(v) not in set(w.specials)]
    others = np.array(plain[1:200] + w.specials)
    src = np.concatenate([np.full(LANE_MAX_QUERIES, plain[0]), others])
    dst = np.concatenate([np.array(plain[200:200 + LANE_MAX_QUERIES]), others])
    n = len(src)
    q = w.m.query_array(src, dst, w.arr)
    ores, ocmds = labels_raw(oracle_lib, w.og, p, q)
    for small in (True, False):
        _switches(monkeypatch, "query")
        plan = eng.Plan(w.g, p, None, max_cmds=mc, query_array=q)
        q_of = np.array(plan.record_queries())
        lens = ores["n"][q_of].astype(np.int64)
        longs = np.flatnonzero(lens > mc)
        assert len(longs) >= 12 and (src[q_of[longs]] == plain[0]).all()
        cap = int(lens[longs][:len(longs) // 2].sum()) if small else max(4096, 8 * n)
        fits = np.ones(n, dtype=bool)
        fits[longs] = np.cumsum(lens[longs]) <= cap
        assert fits[longs].sum() == (len(longs) // 2 if small else len(longs))
        blk, rr, cr, orr = _bound(hip, plan, n, mc, cap)
        try:
            plan.run()
            plan.wait()
            res, cmds = _decoded(eng, w, p, blk.read(), rr, cr, orr, n, mc)
        finally:
            plan.__del__()
            blk.free()
        assert ((res["status"] == MR_ERR_CAPACITY) == ~fits).all(), small
        ok = np.flatnonzero(fits)
        assert len(differing(res[ok], cmds, ores[q_of[ok]], ocmds)) == 0, small


def test_plans_give_their_blocks_back(eng, oracle_lib, monkeypatch, w21):
    """tests/test_gpu_plan_lifetime.py's pattern with the record sources' buffer in the plan:
    the live device blocks after mr_cache_trim repeat from round to round, and a creation
    that fails late under `require` (the staged kernel asked for as well: the refusal comes
    after the memo, the winner table and every other buffer) leaves nothing behind."""
    src, dst = random_query_cells(w21.m, 1500, 14)
    first = _run(eng, monkeypatch, w21, Params(), src, dst, "query")  # (warm: the memo and its table exist from here)
    before = _live(eng)
    for _ in range(2):
        _same(first, _run(eng, monkeypatch, w21, Params(), src, dst, "query"))
        assert _live(eng) == before
    with pytest.raises(eng.EngineError) as ei:
        _run(eng, monkeypatch, w21, Params(), src, dst, "query", max_cmds=4, env=(("MR_LANE_STAGE", "1"),))
    assert "MR_LANE_QUERY=require" in str(ei.value) and "staged" in str(ei.value)
    assert _live(eng) == before
