"""Pass timing bound to the dispatch (mr_plan_run): once a query plan had a
pass without fallback sources, a pass of it that is exactly one launch carries its pair of
timing events on that launch (hipExtLaunchKernel) instead of two records round it.  The end
event is still what mr_plan_wait, the fetches and a pass on another stream wait for, and
mr_plan_kernel_ms still counts every pass: those that were recorded round (the first pass, with
its fallback launches) and those that were bound, in one window.  Pairs past kMaxTimed (1 024)
are folded into the plan's totals while it runs, and their events are used again."""
import ctypes as C
import time

import numpy as np
import pytest

from marshrutka_amd.abi import Params
from marshrutka_amd.mapgen import random_query_cells
from test_gpu_lane_stage import hip  # noqa: F401  (a fixture)
from test_gpu_lane_winner import World, _oracle
from oracle_raw import RESULT

pytestmark = pytest.mark.gpu

# kind -> the switches that send a small plan to one kernel (the others unset)
KINDS = {"query": {"MR_HUB_LANE": "1", "MR_LANE_MEMO": "require", "MR_LANE_WIN": "require", "MR_LANE_QUERY": "require"},
         "group": {"MR_HUB_GROUP": "16"},
         "lane": {"MR_HUB_LANE": "1", "MR_LANE_MEMO": "0"},
         "hub": {"MR_HUB_LANE": "0", "MR_HUB_GROUP": "0"}}
SWITCHES = ("MR_HUB_LANE", "MR_HUB_GROUP", "MR_HUB_GROUP_FORCE", "MR_LANE_MEMO", "MR_LANE_WIN", "MR_LANE_QUERY", "MR_LANE_STAGE",
            "MR_DEV_GROUP", "MR_LANE_WIN_BUDGET", "MR_LANE_LDS_PAD", "MR_LANE_QUERY_GRID", "MR_HUB_FALLBACK_ALL")


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


def _plan(eng, monkeypatch, w, kind, src, dst, max_cmds=8):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in KINDS[kind].items():
        monkeypatch.setenv(k, v)
    plan = eng.Plan(w.g, Params(), None, max_cmds=max_cmds, query_array=w.m.query_array(src, dst, w.arr))
    st = plan.stats()
    # every source on the one kernel: a pass without fallback sources is then one launch
    want = {"query": (st["num_sources"], 1), "lane": (st["num_sources"], 1), "group": (0, 16), "hub": (0, 0)}[kind]
    assert (st["lane_sources"], st["lanes_per_source"]) == want, st
    return plan


def _settle(plan):
    """The first pass and its stats (the plan then knows that no source went to the fallback),
    and the timing window closed."""
    plan.run()
    assert plan.stats()["fallback_sources"] == 0
    plan.kernel_ms()


def _labels(plan, n):
    res, pool = plan.fetch_raw()
    r = np.frombuffer(res, dtype=np.uint8, count=n * 32).copy()
    ncmd = int(r.view(RESULT)["n"].astype(np.int64).sum())
    return {"res": r, "pool": np.frombuffer(pool, dtype=np.uint8, count=ncmd * 40).copy()}


@pytest.mark.parametrize("kind", ["query", "group", "lane", "hub"])
def test_five_passes(eng, oracle_lib, monkeypatch, w65, kind):
    """Five single-launch passes: kernel_ms counts five, their average is positive, and
    together they took no longer than the host saw the loop and its wait take."""
    w = w65
    src, dst = random_query_cells(w.m, 3000, 5)
    plan = _plan(eng, monkeypatch, w, kind, src, dst)
    try:
        _settle(plan)
        t0 = time.perf_counter()
        for _ in range(5):
            plan.run()
        plan.wait()
        wall_ms = (time.perf_counter() - t0) * 1e3
        ms, n = plan.kernel_ms()
        print(f"{kind}: {n} passes, {ms * 1e3:.2f} us a pass, loop {wall_ms * 1e3:.1f} us")
        assert n == 5 and ms > 0.0
        assert n * ms <= wall_ms
        _oracle(oracle_lib, w, Params(), _labels(plan, len(src)), src, dst, pick=range(0, len(src), 6))
    finally:
        plan.__del__()


@pytest.mark.parametrize("kind", ["query", "group"])
def test_window_of_both_kinds(eng, monkeypatch, w21, kind):
    """One window over the first pass (several launches, events recorded round them) and three
    single-launch passes: the count is the passes run, and a window with no pass counts none."""
    w = w21
    src, dst = random_query_cells(w.m, 500, 9)
    plan = _plan(eng, monkeypatch, w, kind, src, dst)
    try:
        plan.run()
        assert plan.stats()["fallback_sources"] == 0
        for _ in range(3):
            plan.run()
        ms, n = plan.kernel_ms()
        assert n == 4 and ms > 0.0
        assert plan.kernel_ms() == (0.0, 0)
    finally:
        plan.__del__()


@pytest.mark.parametrize("kind", ["query", "group"])
def test_two_streams_no_wait(eng, oracle_lib, hip, monkeypatch, w21, kind):  # noqa: F811
    """A pass on stream A and at once one on stream B, then a fetch with no wait before it: B's
    pass waits for the end event of A's (bound to A's launch), the fetch for B's.  The labels
    are the oracle's, and both passes are counted."""
    w = w21
    src, dst = random_query_cells(w.m, 1500, 3)
    sp = np.array(w.specials)
    src, dst = np.concatenate([src, sp]), np.concatenate([dst, sp[::-1]])
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    sa, sb = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(sa)) == 0 and hip.hipStreamCreate(C.byref(sb)) == 0
    plan = _plan(eng, monkeypatch, w, kind, src, dst)
    try:
        _settle(plan)
        plan.run(sa.value)
        plan.run(sb.value)
        got = _labels(plan, len(src))
        _oracle(oracle_lib, w, Params(), got, src, dst)
        ms, n = plan.kernel_ms()
        assert n == 2 and ms > 0.0
    finally:
        plan.__del__()
        for s in (sa, sb):
            hip.hipStreamSynchronize(s)
            hip.hipStreamDestroy(s)


def test_more_passes_than_pending_pairs(eng, oracle_lib, monkeypatch, w21):
    """1 100 passes of a tiny plan with no kernel_ms call between them: past 1 024 pending pairs
    mr_plan_run folds the oldest into the plan's totals and uses their events again.  Every pass
    is counted, and the labels after them are the oracle's."""
    w = w21
    src, dst = random_query_cells(w.m, 200, 4)
    plan = _plan(eng, monkeypatch, w, "query", src, dst)
    try:
        _settle(plan)
        for _ in range(1100):
            plan.run()
        ms, n = plan.kernel_ms()
        assert n == 1100 and ms > 0.0
        _oracle(oracle_lib, w, Params(), _labels(plan, len(src)), src, dst)
        for _ in range(3):  # (events that went through the fold, used again)
            plan.run()
        assert plan.kernel_ms()[1] == 3
    finally:
        plan.__del__()
