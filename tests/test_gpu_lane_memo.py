"""The lane memo (DESIGN.md section 3a''', mr_k_lane_memo.hip): where the specials' labels
depend on a non-special source only through its SoE region, a lane plan reads every
source's destinations off rows built once per (grid, params) instead of running the
Dijkstra per source.  MR_LANE_MEMO=require makes plan creation fail where the gate is
false, so a plan that was created under it ran the memo kernel; =0 runs hub_lane_kernel.
Both must give the same bytes, and the oracle's labels.  Every case sets MR_HUB_LANE=1 so
that small plans take the lane path."""
import numpy as np
import pytest

from golden_util import as_expected
from marshrutka_amd.abi import (MR_ERR_INVALID_ARG, SORT_LEGS, SORT_MONEY, SORT_TIME, Params)
from marshrutka_amd.mapgen import SyntheticMap, index_to_geo, random_query_cells

pytestmark = pytest.mark.gpu

ONE_LEG = (1, 0, 180)  # legs, money, time of a one-leg walk (linear run time)


@pytest.fixture(scope="module")
def eng():
    from marshrutka_amd import build, pathfinder
    build.build()
    if not pathfinder.device_available():
        pytest.fail("no gfx950 device visible to the GPU tests")
    return pathfinder


class World:
    """A map with its engine grid, oracle grid and special cells (row-major numbers)."""

    def __init__(self, eng, oracle_lib, size, seed, cf=4):
        self.m = SyntheticMap(size, campfires_per_homeland=cf, seed=seed)
        self.arr = self.m.cells_array()
        self.g = eng.MapGrid.from_array(self.arr)
        self.og = oracle_lib.OracleGrid.from_array(self.arr)
        m, H = self.m, self.m.h
        self.V = m.size * m.size
        self.center = H * m.size + H
        self.border1 = [self.center - 1, self.center + 1, self.center - m.size, self.center + m.size]
        self.campfires = [m.cell_of(c) for c in m.campfires()]
        self.specials = [self.center] + self.border1 + self.campfires

    def regions(self, homeland):
        """One plain cell per SoE region of `homeland` (the oracle's nearest campfire)."""
        reps = {}
        sp = set(self.specials)
        for v in range(self.V):
            if v in sp:
                continue
            c = self.og.nearest_campfire(v, homeland)
            if c is not None and str(c) not in reps:
                reps[str(c)] = v
        return list(reps.values())


@pytest.fixture(scope="module")
def w21(eng, oracle_lib):
    return World(eng, oracle_lib, 21, 7)


@pytest.fixture(scope="module")
def w65(eng, oracle_lib):
    return World(eng, oracle_lib, 65, 2024)


def _run(eng, monkeypatch, w, params, src, dst, memo, max_cmds=8, env=()):
    """memo: "require", "0" or None (the variable unset)."""
    monkeypatch.setenv("MR_HUB_LANE", "1")
    monkeypatch.delenv("MR_DEV_GROUP", raising=False)
    if memo is None:
        monkeypatch.delenv("MR_LANE_MEMO", raising=False)
    else:
        monkeypatch.setenv("MR_LANE_MEMO", memo)
    for k, v in env:
        monkeypatch.setenv(k, v)
    q = w.m.query_array(src, dst, w.arr)
    plan = eng.Plan(w.g, params, None, max_cmds=max_cmds, query_array=q)
    plan.run()
    res, pool = plan.fetch_raw()
    n = len(q)
    r = np.frombuffer(res, dtype=np.uint8, count=n * 32).copy()
    ncmd = int(np.frombuffer(res, dtype=np.uint32, count=n * 8).reshape(n, 8)[:, 4].astype(np.int64).sum())
    p = np.frombuffer(pool, dtype=np.uint8, count=ncmd * 40).copy()
    return {"res": r, "pool": p, "order": plan.record_queries(), "plan": plan,
            "fallback": [str(c) for c in plan.fallback_sources()], "stats": plan.stats()}


def _same(a, b):
    assert np.array_equal(a["res"], b["res"])
    assert np.array_equal(a["pool"], b["pool"])
    assert a["order"] == b["order"]
    assert a["fallback"] == b["fallback"]
    for k in ("solver", "num_sources", "lane_sources", "lanes_per_source", "fallback_sources"):
        assert a["stats"][k] == b["stats"][k], (k, a["stats"][k], b["stats"][k])


def _oracle(w, params, run, src, dst, pick=None):
    """The plan's labels of queries `pick` (all) against the oracle's, every field."""
    idx = range(len(src)) if pick is None else pick
    got = run["plan"].fetch()
    pairs = [(w.m.index_at(int(src[i])), w.m.index_at(int(dst[i]))) for i in idx]
    exp = w.og.find_path_batch(params, pairs, threads=16)
    bad = [(str(p[0]), str(p[1])) for i, p, e in zip(idx, pairs, exp) if as_expected(e) != as_expected(got[i])]
    assert not bad, f"{len(bad)}/{len(pairs)} labels differ from the oracle; first {bad[0]}"


def _memo_vs_plain(eng, monkeypatch, w, params, src, dst, env=()):
    a = _run(eng, monkeypatch, w, params, src, dst, "require", env=env)
    b = _run(eng, monkeypatch, w, params, src, dst, "0", env=env)
    assert a["stats"]["lanes_per_source"] == 1 and a["stats"]["lane_sources"] > 0
    _same(a, b)
    return a


def _gate_by_oracle(w, params):
    """The gate's predicate from the reference alone: from a plain source of every region,
    every special's label is strictly below the one-leg walk on the metrics in the plan's
    order.  (A label below the one-leg walk uses no position-dependent own edge, each of
    which is componentwise >= that walk; so this is the predicate on the built rows.)"""
    order = list(params.sort_by) + [k for k in (SORT_LEGS, SORT_MONEY, SORT_TIME) if k not in params.sort_by]
    col = {SORT_LEGS: 0, SORT_MONEY: 1, SORT_TIME: 2}
    leg = tuple(ONE_LEG[col[k]] for k in order)
    reps = w.regions(params.homeland)
    pairs = [(w.m.index_at(s), w.m.index_at(t)) for s in reps for t in w.specials]
    labs = w.og.find_path_batch(params, pairs, threads=16)
    return all(tuple((lab.legs, lab.money, lab.time_s)[col[k]] for k in order) < leg for lab in labs)


def test_every_cell_as_source_21(eng, oracle_lib, monkeypatch, w21):
    """21^2, 4 campfires per homeland (21 specials), default params.  Every cell is a source
    with 3 destinations (the Center, the border-1 cells, every campfire and cells of every
    region among them); from one plain source per region and from two specials every cell is
    a destination.  Memo bytes = lane-kernel bytes, and every label is the oracle's."""
    w = w21
    V = w.V
    rng = np.random.default_rng(21)
    src = np.repeat(np.arange(V), 3)
    dst = rng.integers(0, V, size=len(src))
    every = w.regions(Params().homeland) + [w.center, w.campfires[5]]
    assert len(every) == 4 + 2
    src = np.concatenate([src] + [np.full(V, s) for s in every])
    dst = np.concatenate([dst] + [np.arange(V) for _ in every])
    a = _memo_vs_plain(eng, monkeypatch, w, Params(), src, dst)
    _oracle(w, Params(), a, src, dst)


def test_random_queries_65(eng, oracle_lib, monkeypatch, w65):
    """65^2, seed 2024: 4 000 random queries, dst == src, special destinations from plain and
    special sources; 500 of them against the oracle."""
    w = w65
    src, dst = random_query_cells(w.m, 4000, 65)
    sp = np.array(w.specials)
    extra_s = np.concatenate([src[:100], src[100:100 + len(sp)], sp, sp])
    extra_d = np.concatenate([src[:100], sp, sp[::-1], sp])
    src, dst = np.concatenate([src, extra_s]), np.concatenate([dst, extra_d])
    a = _memo_vs_plain(eng, monkeypatch, w, Params(), src, dst)
    pick = list(range(0, 4000, 10)) + list(range(4000, len(src)))[:100]
    _oracle(w, Params(), a, src, dst, pick=pick)


@pytest.mark.parametrize("sort_by", [(SORT_LEGS, SORT_MONEY), (SORT_LEGS, SORT_TIME)])
def test_legs_first_orders_create(eng, oracle_lib, monkeypatch, w21, sort_by):
    src, dst = random_query_cells(w21.m, 1500, 3)
    p = Params(sort_by=sort_by)
    assert _gate_by_oracle(w21, p)
    a = _memo_vs_plain(eng, monkeypatch, w21, p, src, dst)
    _same(_run(eng, monkeypatch, w21, p, src, dst, None), a)
    _oracle(w21, p, a, src, dst, pick=range(0, 1500, 5))


@pytest.mark.parametrize("sort_by", [(SORT_MONEY, SORT_LEGS), (SORT_MONEY, SORT_TIME), (SORT_TIME, SORT_LEGS),
                                     (SORT_TIME, SORT_MONEY)])
def test_other_orders_follow_the_gate(eng, oracle_lib, monkeypatch, w21, sort_by):
    """The gate is what the reference says about the regions' tables (false on this map for
    every order that does not lead with Legs); creation under `require` follows it, and the
    default run matches the lane kernel either way."""
    src, dst = random_query_cells(w21.m, 1500, 4)
    p = Params(sort_by=sort_by)
    gate = _gate_by_oracle(w21, p)
    assert not gate
    with pytest.raises(eng.EngineError) as ei:
        _run(eng, monkeypatch, w21, p, src, dst, "require")
    assert ei.value.status == MR_ERR_INVALID_ARG and "MR_LANE_MEMO=require" in str(ei.value)
    _same(_run(eng, monkeypatch, w21, p, src, dst, None), _run(eng, monkeypatch, w21, p, src, dst, "0"))


@pytest.mark.parametrize("case", ["no_caravans", "no_soe", "five_campfires"])
def test_plans_without_a_memo_raise(eng, oracle_lib, monkeypatch, w21, case):
    w, p = w21, Params()
    if case == "no_caravans":
        p = Params(use_caravans=False)
    elif case == "no_soe":
        p = Params(use_soe=False)
    else:  # 5 + 20 specials: a 32-entry table
        w = World(eng, oracle_lib, 21, 7, cf=5)
    src, dst = random_query_cells(w.m, 1500, 5)
    with pytest.raises(eng.EngineError) as ei:
        _run(eng, monkeypatch, w, p, src, dst, "require")
    assert ei.value.status == MR_ERR_INVALID_ARG and "MR_LANE_MEMO=require" in str(ei.value)
    a = _run(eng, monkeypatch, w, p, src, dst, None)
    _same(a, _run(eng, monkeypatch, w, p, src, dst, "0"))
    _oracle(w, p, a, src, dst, pick=range(0, 1500, 10))


@pytest.mark.parametrize("case", ["sfm", "route_guru_0", "route_guru_6", "hq_on_campfire", "hq_off_campfire"])
def test_params_variants(eng, oracle_lib, monkeypatch, case):
    """(3 campfires per homeland: 17 specials, so an HQ off a campfire still fits 22 entries)"""
    w = World(eng, oracle_lib, 21, 11, cf=3)
    plain = next(v for v in range(w.V) if v not in set(w.specials) and v != w.center)
    p = {"sfm": Params(use_sfm=True),
         "route_guru_0": Params(route_guru=0, scroll_of_escape_cost=7),
         "route_guru_6": Params(route_guru=6),
         "hq_on_campfire": Params(hq_position=w.m.index_at(w.campfires[2])),
         "hq_off_campfire": Params(hq_position=w.m.index_at(plain))}[case]
    src, dst = random_query_cells(w.m, 1500, 6)
    hq = [w.m.cell_of(p.hq_position)] if p.hq_position is not None else []
    src = np.concatenate([src, np.array(hq + w.specials, dtype=np.int64)])
    dst = np.concatenate([dst, np.array((hq + w.specials)[::-1], dtype=np.int64)])
    a = _memo_vs_plain(eng, monkeypatch, w, p, src, dst)
    _oracle(w, p, a, src, dst, pick=range(0, len(src), 4))


def test_blockers(eng, oracle_lib, monkeypatch):
    """A blocker is a boundary special whose settled label a walk candidate tied on all three
    metrics.  Under the gate every special is reached at 0 legs and every walk has at least
    one, so no row of a gated plan has a blocker; and tests/hub_model.py, run on the CPU
    over the maps of sizes 21, 25, 29 and 33 with seeds 1..40 (4 campfires per homeland,
    default params), records no tie from any special source either: no seed in that range
    exercises a nonzero blocker mask or an invalid row under the default order.  What is
    left to check here is that the masks read from a row (zero) go through the same
    read-off as the lane kernel's on the largest of those maps."""
    w = World(eng, oracle_lib, 33, 5)
    src, dst = random_query_cells(w.m, 3000, 8)
    a = _memo_vs_plain(eng, monkeypatch, w, Params(), src, dst)
    assert a["fallback"] == []
    _oracle(w, Params(), a, src, dst, pick=range(0, 3000, 10))


def test_host_and_device_grouping(eng, oracle_lib, monkeypatch, w65):
    src, dst = random_query_cells(w65.m, 6000, 9)
    a = _run(eng, monkeypatch, w65, Params(), src, dst, "require", env=(("MR_DEV_GROUP", "1"),))
    b = _run(eng, monkeypatch, w65, Params(), src, dst, "require", env=(("MR_DEV_GROUP", "0"),))
    c = _run(eng, monkeypatch, w65, Params(), src, dst, "0", env=(("MR_DEV_GROUP", "0"),))
    _same(a, b)
    _same(b, c)
