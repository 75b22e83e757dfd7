"""Who gives device memory back (DESIGN.md "Who owns what"): every buffer of a plan is a
member that returns its block to the block cache when the plan goes.  mr_cache_live counts
the cache-managed blocks that live objects hold; "live" below is that count (blocks and
class bytes) after mr_cache_trim.  A plan family leaks if live differs between two rounds
of the same work, and a failed creation leaks if live differs across it."""
import ctypes as C
import gc

import numpy as np
import pytest

from golden_util import as_expected
from marshrutka_amd.abi import MR_ERR_INVALID_ARG, CellIndex, Params
from marshrutka_amd.mapgen import SyntheticMap, random_queries

pytestmark = pytest.mark.gpu

SWITCHES = ("MR_ALGO", "MR_HUB_FALLBACK_ALL", "MR_HUB_SPW", "MR_HUB_WIDE", "MR_HUB_NONLIN", "MR_GRID_STATE", "MR_HUB_LANE",
            "MR_HUB_LANE_MIN", "MR_HUB_GROUP", "MR_HUB_GROUP_FORCE", "MR_LANE_NONLIN", "MR_LANE_MEMO", "MR_CERT",
            "MR_CERT_SLOTS", "MR_DEV_GROUP", "MR_RANK_TABLE", "MR_FILL_GX", "MR_DBG_FLAGS", "MR_FILL_OVERLAP",
            "MR_FILL_FUSED", "MR_FILL_SLOTS", "MR_DBG_INJECT_SLOT", "MR_FETCH_WIRE", "MR_HOST_DECODE")


@pytest.fixture(scope="module")
def eng():
    from marshrutka_amd import build, pathfinder
    build.build()
    if not pathfinder.device_available():
        pytest.fail("no gfx950 device visible to the GPU tests")
    return pathfinder


@pytest.fixture(scope="module")
def world(eng, oracle_lib):
    """21^2, 4 campfires per homeland, seed 7 (the lane memo's gate holds for the default
    order, tests/test_gpu_lane_memo.py), with 60 queries and their oracle labels."""
    m = SyntheticMap(21, campfires_per_homeland=4, seed=7)
    qs = random_queries(m, 60, 3)
    og = oracle_lib.OracleGrid(m.cells())
    exp = {ff: [as_expected(e) for e in og.find_path_batch(Params(fleetfoot=ff), qs, threads=4)] for ff in (0, 1)}
    return {"m": m, "g": eng.MapGrid(m.cells()), "qs": qs, "exp": exp}


@pytest.fixture
def clean_env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def live(eng):
    gc.collect()
    L = eng.lib()
    L.mr_cache_trim()
    blocks, nbytes = C.c_uint64(), C.c_uint64()
    L.mr_cache_live(C.byref(blocks), C.byref(nbytes))
    return blocks.value, nbytes.value


def destroy(plan):
    plan.__del__()  # mr_plan_destroy now, not when the collector gets to it


# family -> (switches, fleetfoot, what stats() must say)
QUERY_FAMILIES = {
    "lane": ({"MR_HUB_LANE": "1", "MR_LANE_MEMO": "0"}, 0,
             lambda s: s["solver"] == "hub" and s["lanes_per_source"] == 1 and s["lane_sources"] > 0),
    "lane_fleetfoot": ({"MR_HUB_LANE": "1"}, 1,
                       lambda s: s["solver"] == "hub" and s["lanes_per_source"] == 1 and s["lane_sources"] > 0),
    # (creation under `require` succeeds only where the memo kernel runs)
    "memo": ({"MR_HUB_LANE": "1", "MR_LANE_MEMO": "require"}, 0,
             lambda s: s["solver"] == "hub" and s["lanes_per_source"] == 1 and s["lane_sources"] > 0),
    "group": ({}, 0, lambda s: s["solver"] == "hub" and s["lanes_per_source"] in (8, 16, 32) and s["lane_sources"] == 0),
    "hub_cert": ({"MR_HUB_LANE": "0", "MR_HUB_GROUP": "0"}, 0,
                 lambda s: s["solver"] == "hub" and s["lanes_per_source"] == 0),
    "hub_cert_fallback": ({"MR_HUB_LANE": "0", "MR_HUB_GROUP": "0", "MR_HUB_FALLBACK_ALL": "1"}, 0,
                          lambda s: s["solver"] == "hub" and s["lanes_per_source"] == 0 and
                          s["fallback_sources"] == s["num_sources"] and s["certified_sources"] > 0),
    "wide": ({"MR_HUB_WIDE": "1"}, 0, lambda s: s["solver"] == "hub_wide"),
    "sssp": ({"MR_ALGO": "sssp"}, 0, lambda s: s["solver"] in ("levels", "bucketed")),
}


@pytest.mark.parametrize("family", sorted(QUERY_FAMILIES))
def test_query_plans_give_their_blocks_back(eng, world, clean_env, family):
    env, ff, says = QUERY_FAMILIES[family]
    for k, v in env.items():
        clean_env.setenv(k, v)

    def one_round():
        plan = eng.Plan(world["g"], Params(fleetfoot=ff), world["qs"])
        plan.run()
        plan.run()
        got = [as_expected(r) for r in plan.fetch()]
        stats = plan.stats()
        destroy(plan)
        return got, stats

    one_round()  # (warm: the grid's shared tables, memo rows and the stages exist from here)
    before = live(eng)
    got, stats = one_round()
    assert says(stats), (family, stats)
    assert got == world["exp"][ff]
    assert live(eng) == before


FILL_MODES = {"serial": {"MR_FILL_OVERLAP": "0"}, "streams": {"MR_FILL_FUSED": "0"}, "fused": {"MR_FILL_FUSED": "1"}}


def sssp_sources(m):
    cells = m.all_indices()
    return [CellIndex.center(), m.campfires()[1], cells[5], cells[len(cells) // 2 + 3], cells[-2]]


@pytest.mark.parametrize("slots", [2, 3])
@pytest.mark.parametrize("mode", sorted(FILL_MODES))
def test_all_destinations_plans_give_their_blocks_back(eng, clean_env, mode, slots):
    clean_env.setenv("MR_FILL_SLOTS", str(slots))
    for k, v in FILL_MODES[mode].items():
        clean_env.setenv(k, v)
    m = SyntheticMap(33, campfires_per_homeland=3, seed=5)
    g = eng.MapGrid(m.cells())
    sources = sssp_sources(m)

    def one_round(passes):
        plan = eng.SSSPPlan(g, Params(), sources)
        for _ in range(passes):
            plan.run()
        rec = [plan.records(i) for i in range(len(sources))]
        stats = plan.stats()
        destroy(plan)
        return rec, stats

    want, _ = one_round(2)
    before = live(eng)
    rec, stats = one_round(slots + 1)  # the slots wrap
    assert stats["solver"] == "hub" and stats["fill_launch"] == mode, stats
    assert all((a == b).all() for a, b in zip(rec, want))
    assert live(eng) == before


def test_failed_creation_leaves_nothing_behind(eng, world, clean_env):
    """Two creations that fail late: `require` on a Fleetfoot lane plan (the memo gate is
    false for non-linear run times; the hub, certificate and lane buffers exist by then),
    and an all-destinations plan with a source that is no grid cell (refused after a
    complete creation)."""
    destroy(eng.Plan(world["g"], Params(fleetfoot=1), world["qs"]))  # (warm)
    before = live(eng)
    clean_env.setenv("MR_HUB_LANE", "1")
    clean_env.setenv("MR_LANE_MEMO", "require")
    with pytest.raises(eng.EngineError) as ei:
        eng.Plan(world["g"], Params(fleetfoot=1), world["qs"])
    assert ei.value.status == MR_ERR_INVALID_ARG and "non-linear run times" in str(ei.value)
    assert live(eng) == before
    clean_env.delenv("MR_LANE_MEMO")
    clean_env.delenv("MR_HUB_LANE")
    with pytest.raises(eng.EngineError) as ei:
        eng.SSSPPlan(world["g"], Params(), [CellIndex.center(), CellIndex.homeland(0, 200, 200)])
    assert "is not a grid cell" in str(ei.value)
    assert live(eng) == before
    plan = eng.Plan(world["g"], Params(fleetfoot=1), world["qs"])
    plan.run()
    assert [as_expected(r) for r in plan.fetch()] == world["exp"][1]
    destroy(plan)
    assert live(eng) == before


def test_rebinding_the_overflow_pool_replaces_its_staging(eng, world, clean_env):
    # device buffers from the HIP runtime the engine library runs on (as
    # test_overflow_pool_bound_in_record_order does)
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    qs, mc = world["qs"], 2
    destroy(eng.Plan(world["g"], Params(), qs, max_cmds=mc))  # (warm)
    before = live(eng)
    n, rw, cw = len(qs), 4, 4 * mc
    caps = (8 * n, 64 * n)  # (two size classes of staging)
    nw = n * (rw + cw) + max(caps) * 4
    dbuf = C.c_void_p()
    assert hip.hipMalloc(C.byref(dbuf), nw * 4) == 0
    try:
        plan = eng.Plan(world["g"], Params(), qs, max_cmds=mc)
        held = []
        for cap in caps:
            plan.bind_outputs(dbuf.value, dbuf.value + n * rw * 4, dbuf.value + n * (rw + cw) * 4, cap)
            held.append(live(eng))
        # the second binding holds one staging block, of its own class, not two
        assert held[1][0] == held[0][0] and held[1][1] > held[0][1]
        plan.run()
        assert [as_expected(r) for r in plan.fetch()] == world["exp"][0]
        destroy(plan)
    finally:
        hip.hipFree(dbuf)
    assert live(eng) == before


def test_destroy_with_passes_queued(eng, clean_env):
    """mr_plan_destroy waits for the passes still queued before the plan's blocks go back to
    the cache: the same plan created right after takes those blocks, and its records are
    a serial plan's."""
    m = SyntheticMap(33, campfires_per_homeland=3, seed=5)
    g = eng.MapGrid(m.cells())
    sources = sssp_sources(m)
    clean_env.setenv("MR_FILL_OVERLAP", "0")
    ref = eng.SSSPPlan(g, Params(), sources)
    ref.run()
    want = [ref.records(i) for i in range(len(sources))]
    assert ref.stats()["fill_launch"] == "serial"
    destroy(ref)
    clean_env.delenv("MR_FILL_OVERLAP")
    before = live(eng)
    plan = eng.SSSPPlan(g, Params(), sources)
    for _ in range(3):
        plan.run()  # (no host wait)
    destroy(plan)  # (no trim here: the next plan takes the blocks this one gave back)
    plan = eng.SSSPPlan(g, Params(), sources)
    assert plan.stats()["fill_launch"] == "fused"
    plan.run()
    for i in range(len(sources)):
        assert (plan.records(i) == want[i]).all(), i
    destroy(plan)
    assert live(eng) == before
