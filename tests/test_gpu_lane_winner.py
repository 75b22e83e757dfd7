"""The lane memo's winner table (DESIGN.md section 3a''', hub_lane_win_kernel): under the
memo's gate the best boundary walk into a plain cell depends on a plain source only through
its region row, so it is built once per (grid, params) and hub_lane_memo_kernel compares one
boundary's walk with the source's own instead of running the 20 candidates per query.
MR_LANE_WIN=require makes plan creation fail where the table is not used, so a plan created
under it read its destinations off the table; MR_LANE_WIN=0 runs the candidates inside the
memo kernel; MR_LANE_MEMO=0 runs hub_lane_kernel.  All three must give the same bytes, and
the oracle's labels.  Every case sets MR_HUB_LANE=1 so that small plans take the lane path."""
import ctypes as C
import gc

import numpy as np
import pytest

from marshrutka_amd.abi import MR_ERR_INVALID_ARG, SORT_LEGS, SORT_MONEY, SORT_TIME, Params
from marshrutka_amd.mapgen import SyntheticMap, random_query_cells
from oracle_raw import RESULT, command_rows, differing, labels_raw

pytestmark = pytest.mark.gpu

# mode -> (MR_LANE_MEMO, MR_LANE_WIN)
MODES = {"win": ("require", "require"), "candidates": ("require", "0"), "lane": ("0", None), "default": (None, None)}


@pytest.fixture(scope="module")
def eng():
    from marshrutka_amd import build, pathfinder
    build.build()
    if not pathfinder.device_available():
        pytest.fail("no gfx950 device visible to the GPU tests")
    return pathfinder


class World:
    def __init__(self, eng, oracle_lib, size, seed, cf=4):
        self.m = SyntheticMap(size, campfires_per_homeland=cf, seed=seed)
        self.arr = self.m.cells_array()
        self.g = eng.MapGrid.from_array(self.arr)
        self.og = oracle_lib.OracleGrid.from_array(self.arr)
        m, H = self.m, self.m.h
        self.V = m.size * m.size
        self.center = H * m.size + H
        self.campfires = [m.cell_of(c) for c in m.campfires()]
        self.specials = [self.center, self.center - 1, self.center + 1, self.center - m.size,
                         self.center + m.size] + self.campfires


@pytest.fixture(scope="module")
def w21(eng, oracle_lib):
    return World(eng, oracle_lib, 21, 7)


@pytest.fixture(scope="module")
def w65(eng, oracle_lib):
    return World(eng, oracle_lib, 65, 2024)


def _run(eng, monkeypatch, w, params, src, dst, mode, max_cmds=8, env=()):
    memo, win = MODES[mode]
    monkeypatch.setenv("MR_HUB_LANE", "1")
    for k in ("MR_DEV_GROUP", "MR_LANE_WIN_BUDGET"):
        monkeypatch.delenv(k, raising=False)
    for k, v in (("MR_LANE_MEMO", memo), ("MR_LANE_WIN", win)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    for k, v in env:
        monkeypatch.setenv(k, v)
    q = w.m.query_array(src, dst, w.arr)
    plan = eng.Plan(w.g, params, None, max_cmds=max_cmds, query_array=q)
    plan.run()
    res, pool = plan.fetch_raw()
    n = len(q)
    r = np.frombuffer(res, dtype=np.uint8, count=n * 32).copy()
    ncmd = int(r.view(RESULT)["n"].astype(np.int64).sum())
    p = np.frombuffer(pool, dtype=np.uint8, count=ncmd * 40).copy()
    out = {"res": r, "pool": p, "order": plan.record_queries(), "fallback": [str(c) for c in plan.fallback_sources()],
           "stats": plan.stats()}
    plan.__del__()
    return out


def _same(a, b):
    assert np.array_equal(a["res"], b["res"])
    assert np.array_equal(a["pool"], b["pool"])
    assert a["order"] == b["order"]
    assert a["fallback"] == b["fallback"]
    for k in ("solver", "num_sources", "lane_sources", "lanes_per_source", "fallback_sources"):
        assert a["stats"][k] == b["stats"][k], (k, a["stats"][k], b["stats"][k])


def _three_modes(eng, monkeypatch, w, params, src, dst, **kw):
    a = _run(eng, monkeypatch, w, params, src, dst, "win", **kw)
    assert a["stats"]["lanes_per_source"] == 1 and a["stats"]["lane_sources"] > 0
    _same(a, _run(eng, monkeypatch, w, params, src, dst, "candidates", **kw))
    _same(a, _run(eng, monkeypatch, w, params, src, dst, "lane", **kw))
    return a


def _win_vs_candidates(eng, monkeypatch, w, params, src, dst, **kw):
    a = _run(eng, monkeypatch, w, params, src, dst, "win", **kw)
    assert a["stats"]["lanes_per_source"] == 1 and a["stats"]["lane_sources"] > 0
    _same(a, _run(eng, monkeypatch, w, params, src, dst, "candidates", **kw))
    return a


def _oracle(oracle_lib, w, params, run, src, dst, pick=None):
    """The run's labels of queries `pick` (all) against the oracle's, every field and command."""
    idx = np.arange(len(src)) if pick is None else np.asarray(list(pick))
    ores, ocmds = labels_raw(oracle_lib, w.og, params, w.m.query_array(np.asarray(src)[idx], np.asarray(dst)[idx], w.arr))
    bad = differing(run["res"].view(RESULT)[idx], command_rows(run["pool"].tobytes()), ores, ocmds)
    assert len(bad) == 0, f"{len(bad)}/{len(idx)} labels differ from the oracle; first (src, dst) = " \
                          f"{(int(src[idx[bad[0]]]), int(dst[idx[bad[0]]]))}"


def test_all_pairs_21(eng, oracle_lib, monkeypatch, w21):
    """21^2 seed 7: all 441 x 441 (source, destination) pairs.  A source with more than 32
    queries runs on hub_kernel, not on a lane, so the pairs go in 14 plans of 441 sources x
    at most 32 destinations each; every plan's bytes agree between the three modes, and every
    label is the oracle's."""
    w, V, p = w21, w21.V, Params()
    src_all, dst_all, res_all, pool_all, base = [], [], [], [], 0
    for d0 in range(0, V, 32):
        d = np.arange(d0, min(V, d0 + 32))
        src, dst = np.repeat(np.arange(V), len(d)), np.tile(d, V)
        a = _three_modes(eng, monkeypatch, w, p, src, dst)
        r = a["res"].view(RESULT).copy()
        r["off"] += base
        base += len(a["pool"]) // 40
        src_all.append(src), dst_all.append(dst), res_all.append(r.view(np.uint8)), pool_all.append(a["pool"])
    src, dst = np.concatenate(src_all), np.concatenate(dst_all)
    assert len(src) == V * V
    _oracle(oracle_lib, w, p, {"res": np.concatenate(res_all), "pool": np.concatenate(pool_all)}, src, dst)


@pytest.mark.parametrize("sort_by", [(SORT_LEGS, SORT_MONEY), (SORT_LEGS, SORT_TIME)])
def test_random_queries_65(eng, oracle_lib, monkeypatch, w65, sort_by):
    """65^2 seed 2024: 6 000 random queries plus every special as a source and as a
    destination; 500 labels against the oracle."""
    w, p = w65, Params(sort_by=sort_by)
    src, dst = random_query_cells(w.m, 6000, 65)
    sp = np.array(w.specials)
    src = np.concatenate([src, src[:len(sp)], sp, sp])
    dst = np.concatenate([dst, sp, dst[:len(sp)], sp[::-1]])
    a = _three_modes(eng, monkeypatch, w, p, src, dst)
    extra = list(range(6000, len(src)))
    pick = sorted(set(np.linspace(0, 5999, 500 - len(extra)).astype(int).tolist())) + extra
    assert len(pick) == 500
    _oracle(oracle_lib, w, p, a, src, dst, pick=pick)


@pytest.mark.parametrize("case", ["sfm", "route_guru_0", "route_guru_6", "hq_on_campfire", "hq_off_campfire", "homeland_2"])
def test_params_variants(eng, oracle_lib, monkeypatch, case):
    """tests/test_gpu_lane_memo.py's variants on 21^2 seed 11 (3 campfires per homeland: 3
    regions, 17 specials), and a homeland other than the default."""
    w = World(eng, oracle_lib, 21, 11, cf=3)
    plain = next(v for v in range(w.V) if v not in set(w.specials))
    p = {"sfm": Params(use_sfm=True),
         "route_guru_0": Params(route_guru=0, scroll_of_escape_cost=7),
         "route_guru_6": Params(route_guru=6),
         "hq_on_campfire": Params(hq_position=w.m.index_at(w.campfires[2])),
         "hq_off_campfire": Params(hq_position=w.m.index_at(plain)),
         "homeland_2": Params(homeland=2)}[case]
    assert Params().homeland != 2
    src, dst = random_query_cells(w.m, 1500, 6)
    hq = [w.m.cell_of(p.hq_position)] if p.hq_position is not None else []
    src = np.concatenate([src, np.array(hq + w.specials, dtype=np.int64)])
    dst = np.concatenate([dst, np.array((hq + w.specials)[::-1], dtype=np.int64)])
    a = _win_vs_candidates(eng, monkeypatch, w, p, src, dst)
    _oracle(oracle_lib, w, p, a, src, dst)


@pytest.mark.parametrize("case", ["max_cmds_2", "dev_group_0", "dev_group_1", "busy_source"])
def test_other_settings(eng, oracle_lib, monkeypatch, w65, case):
    """max_cmds = 2 (longer labels go to the overflow pool), the host's and the device's
    grouping of the queries, and a source with more than 32 queries (it runs on hub_kernel
    beside the lanes)."""
    w = w65
    src, dst = random_query_cells(w.m, 3000, 12)
    kw = {}
    if case == "max_cmds_2":
        kw["max_cmds"] = 2
    elif case.startswith("dev_group"):
        kw["env"] = (("MR_DEV_GROUP", case[-1]),)
    else:
        src = np.concatenate([src, np.full(40, src[0])])
        dst = np.concatenate([dst, np.arange(100, 140)])
    a = _win_vs_candidates(eng, monkeypatch, w, Params(), src, dst, **kw)
    if case == "max_cmds_2":
        assert (a["res"].view(RESULT)["n"] > 2).any()
    if case == "busy_source":
        assert a["stats"]["lane_sources"] < a["stats"]["num_sources"]


def test_budget(eng, oracle_lib, monkeypatch, w21):
    """A byte budget of zero leaves no room for the table: `require` fails, and the default
    run reads off the candidates and gives the same bytes."""
    src, dst = random_query_cells(w21.m, 1500, 13)
    a = _run(eng, monkeypatch, w21, Params(), src, dst, "win")
    with pytest.raises(eng.EngineError) as ei:
        _run(eng, monkeypatch, w21, Params(), src, dst, "win", env=(("MR_LANE_WIN_BUDGET", "0"),))
    assert ei.value.status == MR_ERR_INVALID_ARG and "MR_LANE_WIN=require" in str(ei.value)
    _same(a, _run(eng, monkeypatch, w21, Params(), src, dst, "default", env=(("MR_LANE_WIN_BUDGET", "0"),)))
    _same(a, _run(eng, monkeypatch, w21, Params(), src, dst, "default"))


def _live(eng):
    gc.collect()
    L = eng.lib()
    L.mr_cache_trim()
    blocks, nbytes = C.c_uint64(), C.c_uint64()
    L.mr_cache_live(C.byref(blocks), C.byref(nbytes))
    return blocks.value, nbytes.value


def test_plans_give_their_blocks_back(eng, oracle_lib, monkeypatch, w21):
    """tests/test_gpu_plan_lifetime.py's pattern: the live device blocks after mr_cache_trim
    repeat from round to round (the table belongs to the grid's memo, not to a plan), and a
    creation that fails late under `require` leaves nothing behind."""
    src, dst = random_query_cells(w21.m, 1500, 14)
    first = _run(eng, monkeypatch, w21, Params(), src, dst, "win")  # (warm: the memo and its table exist from here)
    before = _live(eng)
    for _ in range(2):
        _same(first, _run(eng, monkeypatch, w21, Params(), src, dst, "win"))
        assert _live(eng) == before
    with pytest.raises(eng.EngineError):
        _run(eng, monkeypatch, w21, Params(), src, dst, "win", env=(("MR_LANE_WIN_BUDGET", "0"),))
    assert _live(eng) == before
