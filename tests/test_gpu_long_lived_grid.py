"""One grid that lives long (DESIGN.md "Who owns what", what a grid shares between its plans).
The reference keeps one parsed map while the user changes settings and asks again; behind
the ABI that is one mr_grid that sees hundreds of parameter sets, from more than one host
thread.  A grid is immutable to its callers, but inside it collects lazily built, bounded,
shared state: the rank and special tables per (homeland, HQ cell) (8 keys, then a plan
uploads copies of its own), the region tables, the lane memos (64 keys, then the cache is
cleared) and their winner tables.  A stale or mis-keyed entry gives labels that are
plausible, deterministic and wrong, and only a grid's later uses would show it.  Every
other module looks at a grid's first few uses; this one looks at the later ones.

Expected labels are the oracle's, never the engine's.  Where bytes are compared between two
engine runs, the reference run is a plan on a fresh MapGrid of the same cells.

Not covered here: the memo cache's 256 MB byte bound (it needs the workload's own map size),
and Time-first orders combined with Fleetfoot 1..3 in the tests that keep several plans or
threads busy at once (their certificate's tile sweep assumes all its workgroups are
resident and can stall up to its spin limit beside other kernels: mr_cert_tile.hpp; a
separate piece of work, not a correctness fault)."""
import copy
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from host_threads_child import hq_keys
from marshrutka_amd.abi import SORT_LEGS, SORT_MONEY, SORT_TIME, Params
from marshrutka_amd.mapgen import SyntheticMap, random_query_cells
from oracle_raw import RESULT, command_rows, differing, labels_raw
from test_gpu_lane_memo import World as MemoWorld
from test_gpu_lane_memo import _gate_by_oracle
from test_gpu_lane_stage import _bound, _decoded, hip  # noqa: F401 (hip: a fixture)
from test_gpu_lane_winner import World as WinWorld
from test_gpu_lane_winner import _live, _oracle, _same

pytestmark = pytest.mark.gpu

SWITCHES = ("MR_HUB_LANE", "MR_LANE_MEMO", "MR_LANE_WIN", "MR_LANE_QUERY", "MR_LANE_STAGE", "MR_DEV_GROUP", "MR_LANE_WIN_BUDGET",
            "MR_HUB_GROUP", "MR_HUB_GROUP_FORCE", "MR_ALGO", "MR_HUB_FALLBACK_ALL", "MR_FETCH_WIRE", "MR_HOST_DECODE")
GRID_KEYS = 8  # (homeland, HQ cell) keys a grid keeps device tables for (grid_tables)
MEMO_KEYS = 64  # keys the memo cache holds before it is cleared (lane_memo_rows)
OWN_TABLES = 4  # own_sinfo, own_cell, own_rank, own_rank_inv (plan_tables)


@pytest.fixture(scope="module")
def eng():
    from marshrutka_amd import build, pathfinder
    build.build()
    if not pathfinder.device_available():
        pytest.fail("no gfx950 device visible to the GPU tests")
    return pathfinder


class World(WinWorld):
    """test_gpu_lane_winner's World (w.g is the long-lived grid) with test_gpu_lane_memo's
    regions(), on a clustered map where asked for."""
    regions = MemoWorld.regions

    def __init__(self, eng, oracle_lib, size, seed, cf=4, clustered=False):
        if not clustered:
            super().__init__(eng, oracle_lib, size, seed, cf)
            return
        self.m = SyntheticMap(size, campfires_per_homeland=cf, seed=seed, clustered=True)
        self.arr = self.m.cells_array()
        self.g = eng.MapGrid.from_array(self.arr)
        self.og = oracle_lib.OracleGrid.from_array(self.arr)
        self.V = size * size
        self.center = self.m.h * size + self.m.h
        self.campfires = [self.m.cell_of(c) for c in self.m.campfires()]
        self.specials = [self.center, self.center - 1, self.center + 1, self.center - size, self.center + size] + self.campfires

    def fresh_grid(self, eng):
        return eng.MapGrid.from_array(self.arr)


def _env(monkeypatch, **env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _gate(w, params):
    """_gate_by_oracle with the HQ cell among the specials."""
    hq = [] if params.hq_position is None else [w.m.cell_of(params.hq_position)]
    v = copy.copy(w)
    v.specials = w.specials + [c for c in hq if c not in w.specials]
    return _gate_by_oracle(v, params)


def _taken(plan, n):
    """What test_gpu_lane_winner._run keeps of a plan that has run (for _same and _oracle)."""
    res, pool = plan.fetch_raw()
    r = np.frombuffer(res, dtype=np.uint8, count=n * 32).copy()
    ncmd = int(r.view(RESULT)["n"].astype(np.int64).sum())
    p = np.frombuffer(pool, dtype=np.uint8, count=ncmd * 40).copy()
    return {"res": r, "pool": p, "order": plan.record_queries(), "fallback": [str(c) for c in plan.fallback_sources()],
            "stats": plan.stats()}


def _blocks(eng):
    """The cache-managed device blocks that live objects hold (no collection and no trim, which
    _live does: in a process that has run the whole suite each costs half a second)."""
    blocks = C.c_uint64()
    eng.lib().mr_cache_live(C.byref(blocks), None)
    return blocks.value


def _once(eng, grid, w, params, src, dst, max_cmds=8):
    """A plan created, run, fetched and destroyed: (_taken, cache blocks it held while alive)."""
    n0 = _blocks(eng)
    plan = eng.Plan(grid, params, None, max_cmds=max_cmds, query_array=w.m.query_array(src, dst, w.arr))
    try:
        plan.run()
        out = _taken(plan, len(src))
        held = _blocks(eng) - n0
    finally:
        plan.__del__()
    return out, held


def _agrees(w, run, src, dst, ores, ocmds, pick=None):
    """A run's labels against oracle labels computed before (labels_raw of the same queries)."""
    idx = np.arange(len(src)) if pick is None else np.asarray(pick)
    bad = differing(run["res"].view(RESULT)[idx], command_rows(run["pool"].tobytes()), ores[idx], ocmds)
    assert len(bad) == 0, f"{len(bad)}/{len(idx)} labels differ from the oracle; first (src, dst) = " \
                          f"{(int(src[idx[bad[0]]]), int(dst[idx[bad[0]]]))}"


def _with_specials(w, params, src, dst):
    hq = [w.m.cell_of(params.hq_position)] if params.hq_position is not None else []
    sp = np.array(hq + w.specials, dtype=np.int64)
    return np.concatenate([src, src[:len(sp)], sp, sp]), np.concatenate([dst, sp, dst[:len(sp)], sp[::-1]])


# ---- 1. more (homeland, HQ) keys than the grid keeps ---------------------------------------

@pytest.fixture(scope="module")
def keys12(eng, oracle_lib):
    """21^2 seed 11, 3 campfires per homeland (17 specials: an HQ off a campfire still fits
    the 22-entry tables), the 12 keys' parameters and queries, and the oracle's labels."""
    w = World(eng, oracle_lib, 21, 11, cf=3)
    cases = []
    for i, (h, hq) in enumerate(hq_keys(w)):
        p = Params(homeland=h, hq_position=hq)
        src, dst = _with_specials(w, p, *random_query_cells(w.m, 600, 50 + i))
        ores, ocmds = labels_raw(oracle_lib, w.og, p, w.m.query_array(src, dst, w.arr))
        cases.append({"params": p, "src": src, "dst": dst, "ores": ores, "ocmds": ocmds})
    return w, cases


def test_the_twelve_keys_pass_the_memo_gate(keys12):
    """The reference-side predicate of the memo's gate holds for all 12 keys, each with 3
    regions: under MR_HUB_LANE=1 they all run the memo kernels."""
    w, cases = keys12
    assert len(cases) == 12 and len({(c["params"].homeland, c["params"].hq_position) for c in cases}) == 12
    for c in cases:
        assert len(w.regions(c["params"].homeland)) == 3
        assert _gate(w, c["params"]), c["params"]


@pytest.mark.parametrize("mode", ["lane", "group"])
def test_more_keys_than_the_grid_keeps(eng, oracle_lib, monkeypatch, keys12, mode):
    """12 keys in order on one grid, then in reverse.  Every plan equals the same plan on a
    fresh grid (results, pool, record order, fallback list, stats) and the oracle, and the
    second walk repeats the first one's bytes.  The grid keeps tables for the first 8 keys
    it sees; plans of the others upload their own four, which shows in the cache blocks a
    live plan holds (the grid's tables are plain allocations the cache does not count):
    four more than the same plan on a fresh grid holds, and as many for the first 8."""
    w, cases = keys12
    if mode == "lane":
        _env(monkeypatch, MR_HUB_LANE="1", MR_LANE_MEMO="require", MR_LANE_WIN="require")
    else:
        _env(monkeypatch)
    grid = w.fresh_grid(eng)  # the long-lived one of this mode
    first = []
    for i, c in enumerate(cases):
        a, held = _once(eng, grid, w, c["params"], c["src"], c["dst"])
        b, held_fresh = _once(eng, w.fresh_grid(eng), w, c["params"], c["src"], c["dst"])
        _same(a, b)
        if mode == "lane":
            assert a["stats"]["lanes_per_source"] == 1 and a["stats"]["lane_sources"] > 0
        else:
            assert a["stats"]["lanes_per_source"] in (8, 16, 32) and a["stats"]["lane_sources"] == 0
        _agrees(w, a, c["src"], c["dst"], c["ores"], c["ocmds"])
        own = OWN_TABLES if i >= GRID_KEYS else 0
        assert held == held_fresh + own, f"key {i + 1}: {held} blocks on the long-lived grid, {held_fresh} on a fresh one"
        first.append(a)
    for i in reversed(range(len(cases))):
        c = cases[i]
        a, held = _once(eng, grid, w, c["params"], c["src"], c["dst"])
        _same(a, first[i])
        _, held_fresh = _once(eng, w.fresh_grid(eng), w, c["params"], c["src"], c["dst"])
        own = OWN_TABLES if i >= GRID_KEYS else 0
        assert held == held_fresh + own, f"key {i + 1}, second walk: {held} blocks against {held_fresh}"
    # an all-destinations plan on a key past the eighth: every cell of every source
    c = cases[10]
    if mode == "lane":
        _env(monkeypatch, MR_HUB_LANE="1")  # (no lane plan: `require` would refuse it)
    sources =[next(v for v in range(w.V) if v not in set(w.specials)), w.campfires[0], w.center]
    n0 = _blocks(eng)
    plan = eng.SSSPPlan(grid, c["params"], [w.m.index_at(s) for s in sources])
    try:
        plan.run()
        held = _blocks(eng) - n0
        for i, s in enumerate(sources):
            ores, ocmds = labels_raw(oracle_lib, w.og, c["params"], w.m.query_array(np.full(w.V, s), np.arange(w.V), w.arr))
            res, pool, used = plan.labels_raw(i)
            bad = differing(np.frombuffer(res, dtype=RESULT), command_rows(pool, used), ores, ocmds)
            assert len(bad) == 0, f"source {s}: {len(bad)} cells differ from the oracle, first {bad[0]}"
            rec = plan.records(i)
            assert (rec[:, 0] == ores["legs"]).all() and (rec[:, 1] == ores["money"]).all() and \
                (rec[:, 2] == ores["time_s"]).all(), f"source {s}: device records differ from the oracle's metrics"
    finally:
        plan.__del__()
    fresh = eng.SSSPPlan(w.fresh_grid(eng), c["params"], [w.m.index_at(s) for s in sources])
    fresh.run()
    held_fresh = _blocks(eng) - n0
    fresh.__del__()
    assert held == held_fresh + OWN_TABLES, (held, held_fresh)


# ---- 2. memo cache turnover ----------------------------------------------------------------

@pytest.fixture(scope="module")
def w21(eng, oracle_lib):
    return World(eng, oracle_lib, 21, 7)


def test_memo_cache_turnover(eng, oracle_lib, monkeypatch, w21):
    """160 memo keys on one grid (scroll prices 0..79 in both Legs-first orders) beside two
    anchor plans that stay alive.  The cache is cleared at its 64th key, so the anchors'
    memos leave it while the anchors hold them: their later passes repeat their first
    bytes, new plans with their parameters rebuild the memo and give the same bytes, and
    plans of other max_cmds (the same key: they share the memo) give the oracle's labels.
    Every plan of the walk is created under MR_LANE_MEMO=require and MR_LANE_WIN=require
    and gives the oracle's labels.  Whether a row has a blocker is decided on the device; a
    key refused for that reason runs under the default switches and is not counted (on an
    MI355X none is: 160 of 160 are created under `require`; the test needs more than 64)."""
    w = w21
    before = _live(eng)
    orders = [(SORT_LEGS, SORT_MONEY), (SORT_LEGS, SORT_TIME)]
    require = dict(MR_HUB_LANE="1", MR_LANE_MEMO="require", MR_LANE_WIN="require")

    def plan_of(params, src, dst, max_cmds=8):
        return eng.Plan(w.g, params, None, max_cmds=max_cmds, query_array=w.m.query_array(src, dst, w.arr))

    _env(monkeypatch, MR_LANE_QUERY="require", **require)
    asrc, adst = _with_specials(w, Params(), *random_query_cells(w.m, 1500, 90))
    anchors = []
    for sort_by in orders:
        p = Params(sort_by=sort_by)
        assert _gate(w, p)
        plan = plan_of(p, asrc, adst)
        plan.run()
        anchors.append({"params": p, "plan": plan, "first": _taken(plan, len(asrc))})
        _oracle(oracle_lib, w, p, anchors[-1]["first"], asrc, adst)
    required = set()
    for cost in range(80):
        for sort_by in orders:
            p = Params(scroll_of_escape_cost=cost, sort_by=sort_by)
            assert _gate(w, p), p
            src, dst = _with_specials(w, p, *random_query_cells(w.m, 300 - 3 * len(w.specials), 1000 + cost))
            _env(monkeypatch, **require)
            try:
                plan = plan_of(p, src, dst)
                required.add((cost, sort_by))
            except eng.EngineError as e:
                if "blockers" not in str(e):
                    raise
                _env(monkeypatch, MR_HUB_LANE="1")
                plan = plan_of(p, src, dst)
            try:
                plan.run()
                run = _taken(plan, len(src))
            finally:
                plan.__del__()
            assert run["stats"]["lanes_per_source"] == 1 and run["stats"]["lane_sources"] > 0
            _oracle(oracle_lib, w, p, run, src, dst)
    print(f"{len(required)} of 160 keys created under require")
    assert len(required) > MEMO_KEYS, f"{len(required)} keys created under require: the {MEMO_KEYS}-key clear is not certain"
    _env(monkeypatch, MR_LANE_QUERY="require", **require)
    for a in anchors:
        a["plan"].run()
        _same(_taken(a["plan"], len(asrc)), a["first"])  # (its memo left the cache; the plan holds it)
        again = plan_of(a["params"], asrc, adst)  # (rebuilds the memo)
        again.run()
        _same(_taken(again, len(asrc)), a["first"])
        again.__del__()
        _env(monkeypatch, **require)
        for mc in (1, 16):  # the same memo key as max_cmds 8
            other = plan_of(a["params"], asrc, adst, max_cmds=mc)
            other.run()
            run = _taken(other, len(asrc))
            other.__del__()
            assert run["stats"]["lanes_per_source"] == 1 and run["stats"]["lane_sources"] > 0
            _oracle(oracle_lib, w, a["params"], run, asrc, adst)
            if mc == 1:
                assert (run["res"].view(RESULT)["n"] > mc).any()
        _env(monkeypatch, MR_LANE_QUERY="require", **require)
    for a in anchors:
        a["plan"].__del__()
    assert _live(eng) == before


# ---- 3. plans alive together, passes interleaved -------------------------------------------

def _stream_api(hip):
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]


def _all_cells_agree(oracle_lib, w, params, plan, sources):
    for i, s in enumerate(sources):
        ores, ocmds = labels_raw(oracle_lib, w.og, params, w.m.query_array(np.full(w.V, s), np.arange(w.V), w.arr))
        res, pool, used = plan.labels_raw(i)
        bad = differing(np.frombuffer(res, dtype=RESULT), command_rows(pool, used), ores, ocmds)
        assert len(bad) == 0, f"source {s}: {len(bad)} cells differ from the oracle, first {bad[0]}"


def test_plans_alive_together(eng, oracle_lib, hip, monkeypatch):  # noqa: F811
    """Nine plans of different kinds on one 33^2 grid (clustered, 5 campfires per homeland:
    a Time-first order hands sources to the SSSP kernel), all created before any runs, three
    rounds of passes taken round-robin, each plan on its own stream and, in the second
    round, every second plan on a caller stream; fetched in reverse creation order.  Every
    plan gives the bytes of the same plan created, run and fetched alone on a fresh grid,
    and the oracle's labels (300 per plan, every cell for the all-destinations plan)."""
    _env(monkeypatch, MR_HUB_LANE="1")
    _stream_api(hip)
    w = World(eng, oracle_lib, 33, 5, cf=5, clustered=True)
    plain = [v for v in range(w.V) if v not in set(w.specials)]
    src, dst = random_query_cells(w.m, 1000, 33)
    sp = np.array(w.specials, dtype=np.int64)
    src, dst = np.concatenate([src, src[:len(sp)], sp]), np.concatenate([dst, sp, dst[:len(sp)]])
    busy = (np.full(40, plain[7]), np.concatenate([np.arange(100, 130), sp[:10]]))
    hq2 = Params(homeland=2, hq_position=w.m.index_at(w.campfires[2]))
    sssp_sources = [plain[3], w.campfires[1], w.center]
    # name -> (params, sources, destinations, max_cmds); "sssp" and "bound" are special below
    kinds = {
        "legs": (Params(), src, dst, 8),
        "legs_mc2": (Params(), src, dst, 2),
        "money": (Params(sort_by=(SORT_MONEY, SORT_LEGS)), src, dst, 8),
        "fleetfoot2": (Params(fleetfoot=2), src, dst, 8),
        "time": (Params(sort_by=(SORT_TIME, SORT_MONEY)), src, dst, 8),
        "one_source": (Params(), busy[0], busy[1], 8),
        "homeland2_hq": (hq2, np.concatenate([src, [w.campfires[2]]]), np.concatenate([dst, [plain[0]]]), 8),
        "sssp": (Params(), None, None, 0),
        "bound": (Params(sort_by=(SORT_LEGS, SORT_TIME)), src, dst, 4),
    }

    def create(grid, name):
        p, s, d, mc = kinds[name]
        if name == "sssp":
            return eng.SSSPPlan(grid, p, [w.m.index_at(v) for v in sssp_sources]), None
        plan = eng.Plan(grid, p, None, max_cmds=mc, query_array=w.m.query_array(s, d, w.arr))
        if name != "bound":
            return plan, None
        blk, rr, cr, orr = _bound(hip, plan, len(s), mc, 8 * len(s))
        # (the block's fill is queued on the null stream, which the plan's stream does not wait for)
        assert hip.hipStreamSynchronize(None) == 0
        return plan, (blk, rr, cr, orr)

    def take(name, plan, bound):
        p, s, d, mc = kinds[name]
        if name == "sssp":
            return {"rec": [plan.records(i).copy() for i in range(len(sssp_sources))]}
        out = _taken(plan, len(s))
        if bound:
            blk, rr, cr, orr = bound
            plan.wait()
            host = blk.read()
            out["records"] = np.concatenate([host[rr[0]:rr[1]], host[cr[0]:cr[1]]])
            out["decoded"] = _decoded(eng, w, p, host, rr, cr, orr, len(s), mc)
        return out

    alone = {}
    for name in kinds:  # each plan alone on a fresh grid
        plan, bound = create(w.fresh_grid(eng), name)
        try:
            plan.run()
            alone[name] = take(name, plan, bound)
        finally:
            plan.__del__()
            if bound:
                bound[0].free()

    before = _live(eng)
    streams = [C.c_void_p() for _ in range(2)]
    for s in streams:
        assert hip.hipStreamCreate(C.byref(s)) == 0
    live = {}
    try:
        for name in kinds:
            live[name] = create(w.g, name)
        names = list(kinds)
        for rnd in range(3):
            for k, name in enumerate(names):
                caller = streams[k // 2 % 2].value if rnd == 1 and k % 2 else 0
                live[name][0].run(caller)
        got = {name: take(name, *live[name]) for name in reversed(names)}
        for name in names:
            p, s, d, mc = kinds[name]
            if name == "sssp":
                for a, b in zip(got[name]["rec"], alone[name]["rec"]):
                    assert np.array_equal(a, b), name
                _all_cells_agree(oracle_lib, w, p, live[name][0], sssp_sources)
                continue
            try:
                _same(got[name], alone[name])
            except AssertionError as e:
                raise AssertionError(f"{name}: differs from the same plan alone on a fresh grid: {e}") from e
            pick = np.unique(np.concatenate([np.linspace(0, len(s) - 1, 290).astype(int), np.arange(len(s) - 10, len(s))]))
            assert len(pick) <= 300
            _oracle(oracle_lib, w, p, got[name], s, d, pick=pick)
            if name == "bound":
                assert np.array_equal(got[name]["records"], alone[name]["records"])
                (ra, ca), (rb, cb) = got[name]["decoded"], alone[name]["decoded"]
                assert len(differing(ra, ca, rb, cb)) == 0
        st = {name: got[name]["stats"] for name in names if name != "sssp"}
        assert st["time"]["fallback_sources"] > 0
        assert (got["legs_mc2"]["res"].view(RESULT)["n"] > 2).any()
        for name in ("legs", "legs_mc2", "money", "fleetfoot2", "bound"):
            assert st[name]["lanes_per_source"] == 1 and st[name]["lane_sources"] > 0, (name, st[name])
        assert st["one_source"]["lane_sources"] == 0 and st["one_source"]["num_sources"] == 1
    finally:
        for name in sorted(live):  # (not the creation order)
            plan, bound = live[name]
            plan.__del__()
            if bound:
                bound[0].free()
        for s in streams:
            hip.hipStreamSynchronize(s)
            hip.hipStreamDestroy(s)
    assert _live(eng) == before


# ---- 4. host threads -----------------------------------------------------------------------

@pytest.mark.parametrize("hub_lane", ["1", None])
def test_host_threads(eng, hub_lane):
    """tests/host_threads_child.py in a fresh process (its docstring says what it does), once
    with MR_HUB_LANE=1 and once without: exit status 0 and a final "ok" line.  Measured on an
    MI355X: 0.9 s a run, of which the threads' six rounds take 0.08 s (the child joins them
    against an 80 s deadline of its own), beside the 120 s limit of each run.

    A pass proves little about races the run did not happen to hit: no sanitizer watches the
    library here.  What the test does produce, and no other test does, is the concurrent first
    use of a grid's tables, memos and winner tables, and mr_cache_trim beside running plans."""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    if hub_lane:
        env["MR_HUB_LANE"] = hub_lane
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_threads_child.py")
    r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=120)
    print(r.stdout[-300:])
    assert r.returncode == 0, f"exit status {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert r.stdout.strip().splitlines()[-1] == "ok", r.stdout[-2000:]
