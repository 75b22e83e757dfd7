"""Every solver path at large scroll prices and at the 32-bit money limit.

Money is the one metric a caller can push to the top of 32 bits (large_costs.py).  Regime
A: prices at the lane kernels' gate cost G, one above it, and as large as the map allows
with nothing wrapping; the bar is the parity suite's, bit-exact equality of (legs, money,
time, every command) with the C++ oracle, on every grid_state mode, with the plan stats
proving at G that the gated lane and group kernels were the ones that ran.  The oracle
is only a reference where no u32 sum wraps, which large_costs.oracle_answers asserts
before it answers.  Regime B: prices whose sums pass 2^32; a plan reports MR_ERR_LIMIT
or returns labels equal to exact integer arithmetic (py_ref.Finder(wrap=False)), and
where a queried optimum itself passes 2^32 only MR_ERR_LIMIT is right.

Why regime B's passes end whatever the metric values are (csrc/, read before the first
such pass was run).  No loop below counts up to a metric or waits for one to reach a
value; a wrapped or saturated sum can change which label wins, never how often a loop
runs.

  * Which kernels run.  choose_kernel (mr_host.cpp:2131-2159) gives a plan to
    hub_lane_kernel or hub_group_kernel only if lane_bounds_ok (mr_host.cpp:1772-1779)
    holds; regime B's prices fail it ((2 NS + 4) * price > 2^32 - 2), so the lane, lanenl,
    lanetab and group* modes run hub_kernel there.  Their own loops are bounded by
    constants all the same (mr_hub_lane.hpp:464 guard < 4096, :872 guard <= TM + 1, :1009
    it < NS; mr_hub_group.hpp:205 guard <= TM, :381 it < n_it).
  * hub_kernel and hub_wide_kernel: one settle per iteration of `for it <= NS`
    (mr_device.hpp:2255, :2764); a special once settled (st == 2) is never selected again.
    Destinations are read off per query afterwards (emit_all), each a scan of at most
    NS + 1 boundaries.
  * specials_reg (mr_device.hpp:667-734), the Dijkstra over the specials inside the
    level and bucketed solvers: `for it <= NS`, leaving early when no tentative special
    has the bucket's key.  A key below the bucket (what a wrapped sum produces) raises
    kErrBucket and is otherwise ignored.
  * The level solver's main loop (mr_device.hpp:1117-1194) and the bucketed solver's
    (:1383-1421, with next_bucket :1335-1351) advance to the least pending key (the next
    list that holds cells, or min_special_key), never by counting through key values, and
    both carry `guard > V + NS + 64 -> kErrBucket, break`.  A cell enters a list on its
    first touch only, which its state word decides, not a metric (:1319), so no list
    outgrows V.  region_offer's loop (:1231) is a compare-and-swap retry: each retry means
    another thread's store went through.
  * solve_kernel (mr_device.hpp:3482, :3528) takes sources off a counter until it is past
    their number.
  * cmp_list (mr_device.hpp:386) walks at most 8192 commands; emit (:818-836) writes from
    position len - 1 downwards and stops at 0 whatever the parent chain holds, with len
    checked against max_cmds or the overflow pool's capacity first (:808-813).
  * The certificate (the fallback modes).  Money enters it only through unsigned
    comparisons: ranks among the table's boundaries (mr_cert_tile.hpp:296-308) and the
    candidate compares of cert_check_kernel, whose loops run over cells, hubs and table
    entries (mr_cert.hpp:203 it < 64, :251, :308, :358).  cert_sweep_kernel buckets cells by
    the first metric in comparator order that is not money (mr_cert.hpp:624), gives up above
    kSweepBuckets buckets (:661), visits each bucket once (:753) and drops a push into a
    full queue (:742-747).  cert_tile_kernel steps buckets of legs or time up to
    kTileMaxSteps (mr_cert_tile.hpp:452, :509) and exchanges up to kTileMaxSteps / kTileH
    (:589); a wait for a neighbour tile gives up after 2^22 polls (:561-567), and a tile
    that fails stores kTileDone so that its neighbours' waits end (:575).  Legs and time
    of a table label are sums over at most 2 NS + 4 commands bounded by the grid, whatever
    label wins.
  * The fill kernel serves all-destinations plans only; regime B makes none.
"""
import pytest

import large_costs as lc
from golden_util import as_expected
from marshrutka_amd.abi import MR_ERR_LIMIT, SORT_LEGS, SORT_MONEY, SORT_TIME, mr_command, mr_result, result_from_c
from test_gpu_decode_widths import DeviceWords, hip  # noqa: F401  (hip: a fixture)
from test_gpu_parity import eng, grid_state  # noqa: F401  (fixtures: the 19 solver modes)
from test_gpu_sssp import all_labels_match, mode  # noqa: F401  (mode: a fixture, auto / fallback / sssp)

pytestmark = pytest.mark.gpu

GROUP_LANES = {"group": 8, "group16": 16, "group32": 32}


def _mismatches(qs, exp, got):
    return [(q, e, as_expected(r)) for q, e, r in zip(qs, exp, got) if as_expected(r) != e]


@pytest.mark.parametrize("case,which", lc.CASE_COSTS, ids=[f"{c}-{w}" for c, w in lc.CASE_COSTS])
def test_parity_at_large_costs(eng, oracle_lib, grid_state, case, which):  # noqa: F811
    """Regime A.  At G, Fleetfoot 0 and the HQ on a campfire the plan must have run on the
    kernel the mode names (hub_lane_kernel: one lane a source; hub_group_kernel: the
    group's lanes), or the gated kernels would never see a large value; above G only
    exactness is asserted, whichever kernel the host picks."""
    ans = lc.oracle_answers(oracle_lib, case, which)  # (asserts that nothing wraps)
    m, hq = lc.case_map(case)
    g = eng.MapGrid(m.cells())
    qs, cost = lc.queries_of(case), lc.cost_of(case, which)
    algo = grid_state.split("-")[0]
    for sort_by in lc.ORDERS:
        for ff in lc.FLEETFOOT:
            params = lc.params_of(cost, sort_by, ff, hq)
            plan = eng.Plan(g, params, qs)
            plan.run()
            got = plan.fetch()
            st = plan.stats()
            bad = _mismatches(qs, ans[(sort_by, ff)], got)
            assert not bad, f"{case} C={cost} {sort_by} ff={ff}: {len(bad)}/{len(qs)} mismatches; first: {bad[0]}; {st}"
            assert st["num_specials"] == lc.num_specials(case), st
            if which == "G" and ff == 0 and case != "A3":
                if algo.startswith("lane"):
                    assert st["lanes_per_source"] == 1 and st["lane_sources"] > 0, (sort_by, st)
                if algo in GROUP_LANES:
                    assert st["lanes_per_source"] == GROUP_LANES[algo], (sort_by, st)


SSSP_PARAMS = [((SORT_LEGS, SORT_MONEY), 0), ((SORT_TIME, SORT_MONEY), 2), ((SORT_MONEY, SORT_LEGS), 0)]


@pytest.mark.parametrize("case", ["A1", "A2"])
def test_all_destinations_at_largest_cost(eng, oracle_lib, mode, case):  # noqa: F811
    """The all-destinations plans (fill kernel, sources handed over, the SSSP kernel alone)
    at the case's largest price: every cell's label and its record's three metrics."""
    lc.oracle_answers(oracle_lib, case, "top")  # (asserts that nothing wraps)
    m, hq = lc.case_map(case)
    src = lc.sources_of(case)
    for sort_by, ff in SSSP_PARAMS:
        all_labels_match(eng, oracle_lib, m, lc.params_of(lc.cost_of(case, "top"), sort_by, ff, hq),
                         [src[0], src[2], src[4], src[5]])


@pytest.mark.parametrize("max_cmds", [2, 16])
@pytest.mark.parametrize("case", ["A1", "A2"])
def test_fetch_routes_at_largest_cost(eng, oracle_lib, hip, monkeypatch, case, max_cmds):  # noqa: F811
    """The device decoder (pageable and page-locked arrays), the wire fetch, the host
    decoder and mr_plan_wire_records + mr_decode_wire at the case's largest price, each
    against the oracle (not against one another): at 2 slots most labels go through the
    overflow and wire pools.  The wire rows carry no metrics; mr_decode_wire sums them."""
    ans = lc.oracle_answers(oracle_lib, case, "top")
    for v in ("MR_HOST_DECODE", "MR_FETCH_WIRE", "MR_DEV_GROUP", "MR_GRID_STATE", "MR_ALGO"):
        monkeypatch.delenv(v, raising=False)
    m, hq = lc.case_map(case)
    g = eng.MapGrid(m.cells())
    qs = lc.queries_of(case)
    n, cap = len(qs), len(qs) * 24
    for sort_by, ff in (((SORT_TIME, SORT_MONEY), 2), ((SORT_LEGS, SORT_MONEY), 0)):
        params, exp = lc.params_of(lc.cost_of(case, "top"), sort_by, ff, hq), ans[(sort_by, ff)]
        assert any(len(e[3]) > max_cmds for e in exp) == (max_cmds == 2)
        for route in ("device", "pinned", "wire", "host"):
            if route == "host":
                monkeypatch.setenv("MR_HOST_DECODE", "1")
            else:
                monkeypatch.delenv("MR_HOST_DECODE", raising=False)
            monkeypatch.setenv("MR_FETCH_WIRE", "1" if route == "wire" else "0")
            plan = eng.Plan(g, params, qs, max_cmds=max_cmds)
            plan.run()
            res, pool = (mr_result * n)(), (mr_command * cap)()
            if route == "pinned":
                eng.pin_host(res)
                eng.pin_host(pool)
            try:
                st = eng.lib().mr_plan_fetch(plan.handle, res, pool, cap)
            finally:
                if route == "pinned":
                    eng.unpin_host(res)
                    eng.unpin_host(pool)
            assert st == 0, (route, st, eng.last_error())
            bad = _mismatches(qs, exp, [result_from_c(res[i], pool) for i in range(n)])
            assert not bad, f"{route} {sort_by} ff={ff}: {len(bad)}/{n} mismatches; first: {bad[0]}"
        monkeypatch.delenv("MR_HOST_DECODE", raising=False)
        monkeypatch.setenv("MR_FETCH_WIRE", "0")
        rw, pcap = eng.wire_row_words(max_cmds), 8 * n
        wbuf = DeviceWords(hip, n * rw + 2 * pcap)
        try:
            plan = eng.Plan(g, params, qs, max_cmds=max_cmds)
            plan.run()
            plan.wire_records(wbuf.ptr.value, wbuf.ptr.value + n * rw * 4, pcap)
            plan.wait()
            host = wbuf.read()
            out, cmds = eng.decode_wire_raw(g, params, host[:n * rw], n, max_cmds, host[n * rw:])
            q_of = plan.record_queries()
            got = [None] * n
            for k in range(n):
                assert out[k].status == 0, (k, out[k].status)
                got[q_of[k]] = result_from_c(out[k], cmds)
            bad = _mismatches(qs, exp, got)
            assert not bad, f"wire_records {sort_by} ff={ff}: {len(bad)}/{n} mismatches; first: {bad[0]}"
            del plan
        finally:
            wbuf.free()


@pytest.mark.parametrize("sort_by", lc.B_ORDERS, ids=["legs-money", "money-legs"])
@pytest.mark.parametrize("prices", lc.B_PRICES, ids=["3e9", "2^32-1"])
def test_regime_b_limit_or_exact(eng, grid_state, prices, sort_by):  # noqa: F811
    """Regime B: the plan reports MR_ERR_LIMIT (never MR_ERR_DEVICE, never another
    status) or returns; what it returns is exact: each label's money is the integer sum
    of its commands' money and the label is Finder(wrap=False)'s.  Where a queried
    optimum itself has money >= 2^32 (the (Legs, Money) order at price 2^32 - 1:
    test_large_costs.py asserts it has some), only MR_ERR_LIMIT is right."""
    exact = lc.exact_answers(prices, sort_by)
    m, _ = lc.case_map("A1")
    qs = lc.b_queries()
    must_limit = any(e[1] >= 1 << 32 for e in exact)
    if sort_by == (SORT_LEGS, SORT_MONEY) and prices[0] == 0xFFFFFFFF:
        assert must_limit
    try:
        plan = eng.Plan(eng.MapGrid(m.cells()), lc.b_params(prices, sort_by), qs)
        plan.run()
        got = plan.fetch()
    except eng.EngineError as e:
        assert e.status == MR_ERR_LIMIT, f"{grid_state}: status {e.status}: {e}"
        print(f"regime B {grid_state} {prices[0]} {sort_by}: MR_ERR_LIMIT")
        return
    print(f"regime B {grid_state} {prices[0]} {sort_by}: returned labels")
    assert not must_limit, f"{grid_state}: labels returned though an optimum's money passes 2^32"
    for q, r in zip(qs, got):
        assert r is not None and r.money == sum(c.money for c in r.commands), (grid_state, q, as_expected(r))
    bad = _mismatches(qs, exact, got)
    assert not bad, f"{grid_state}: {len(bad)}/{len(qs)} labels differ from exact arithmetic; first: {bad[0]}"
