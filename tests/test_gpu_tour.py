"""Tour plans (mr_tour_plan_create): the best visiting order of up to 10 stops per tour, reduced
on the device from the plan's own cost matrix.

The rule (DESIGN.md section 3b''''): the cost of an order pi of a tour's stops is the sum over its
legs of the metrics of FindPath::eval(from, to); the answer is the pi with the least
(m[q0], m[q1], m[q2], pi[0], .., pi[n-1]), (q0, q1, q2) the plan's metric order.  The host
references are tour_ref.brute_force (every permutation) and tour_ref.held_karp (the kernel's DP in
Python integers), over the oracle's labels or MatrixPlan.records() of the same cells.  Hub path,
sources handed to the SSSP kernel, and the SSSP kernel alone feed the matrix (the `mode`
fixture)."""
import ctypes as C
import random

import numpy as np
import pytest

import large_costs as lc
import tour_ref as tr
from golden_util import as_expected
from marshrutka_amd import abi
from marshrutka_amd.abi import (MR_ERR_INVALID_ARG, MR_ERR_LIMIT, MR_NOT_FOUND, MR_OK, SORT_LEGS, SORT_MONEY, SORT_TIME,
                                CellIndex, Params, mr_result, mr_tour_record)
from marshrutka_amd.mapgen import SyntheticMap
from test_gpu_nearest import matrix_records, plan_order
from test_gpu_sssp import PARAMS, _hip, _raw_words, eng, mode  # noqa: F401  (eng, mode: fixtures)

pytestmark = pytest.mark.gpu

TOUR_MODES = [abi.TOUR_OPEN, abi.TOUR_RETURN, abi.TOUR_TO_LAST]
SWITCHES = ("MR_ALGO", "MR_HUB_FALLBACK_ALL", "MR_DBG_FLAGS", "MR_MATRIX_GX", "MR_TOUR_GX", "MR_TOUR_WAVE_MAX")


@pytest.fixture(autouse=True)
def _clear(monkeypatch):
    """No kernel switch set but the test's own (autouse: before `mode` sets its two)."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def stops_of(tour, tmode):
    return len(tour) - (2 if tmode == abi.TOUR_TO_LAST else 1)


def legs_of(tour, tmode):
    return stops_of(tour, tmode) + (0 if tmode == abi.TOUR_OPEN else 1)


def tour_matrix(tour, tmode, metric):
    """tour_ref's M of a tour: metric(a, b) = (legs, money, time) of the leg a -> b, zeros from a
    cell to itself; under the modes without a fixed end the end's row and column are zeros."""
    n = stops_of(tour, tmode)
    M = np.zeros((n + 2, n + 2, 3), dtype=np.int64)
    for i, a in enumerate(tour):
        for j, b in enumerate(tour):
            if a != b:
                M[i, j] = metric(a, b)
    return M


def expected_record(tour, tmode, order, metric, solve=tr.held_karp):
    """(legs, money, time, status, n_stops, n_legs, order[10]) a plan must give for the tour."""
    n, L = stops_of(tour, tmode), legs_of(tour, tmode)
    M = tour_matrix(tour, tmode, metric)
    if not tr.limit_gate(M, L, tmode):
        return (0, 0, 0, MR_ERR_LIMIT, n, L) + (0xFF,) * 10
    cost, pi = solve(M, tmode, order)[:2]
    return tuple(cost) + (MR_OK, n, L) + tuple(pi) + (0xFF,) * (10 - n)


def record_tuple(r):
    assert int(r["reserved"]) == 0
    return (int(r["legs"]), int(r["money"]), int(r["time_s"]), int(r["status"]), int(r["n_stops"]), int(r["n_legs"])) + tuple(
        int(x) for x in r["order"])


def cell_sequence(tour, pi):
    return [tour[1 + k] for k in pi]


# ---- 1. the oracle end to end ------------------------------------------------------------------
_oracle = {}


def oracle_case(oracle_lib, pi):
    """(map, 30 pool cells, the oracle's labels of every ordered pair of them), once per PARAMS entry."""
    if pi not in _oracle:
        m = SyntheticMap(21, campfires_per_homeland=3, seed=210 + pi)
        rng = random.Random(2100 + pi)
        cells = m.all_indices()
        pool = [CellIndex.center(), m.campfires()[0], CellIndex.border(2, 1)] + rng.sample(cells, 27)
        pool = list(dict.fromkeys(pool))
        og = oracle_lib.OracleGrid(m.cells())
        pairs = [(a, b) for a in pool for b in pool]
        _oracle[pi] = (m, pool, dict(zip(pairs, og.find_path_batch(PARAMS[pi], pairs, threads=0))))
    return _oracle[pi]


_oracle_want = {}


def oracle_tours(oracle_lib, pi, tmode):
    """12 tours of 3-6 distinct random stops from the pool and their expected records by brute force."""
    m, pool, exp = oracle_case(oracle_lib, pi)
    if (pi, tmode) not in _oracle_want:
        rng = random.Random(31 * pi + tmode)
        extra = 2 if tmode == abi.TOUR_TO_LAST else 1
        tours = [rng.sample(pool, rng.randint(3, 6) + extra) for _ in range(12)]
        order = plan_order(PARAMS[pi])

        def metric(a, b):
            e = exp[a, b]
            return (e.legs, e.money, e.time_s)
        _oracle_want[pi, tmode] = (tours, [expected_record(t, tmode, order, metric, tr.brute_force) for t in tours])
    return _oracle_want[pi, tmode]


@pytest.mark.parametrize("pi", range(len(PARAMS)))
def test_records_and_legs_match_oracle(eng, oracle_lib, mode, pi):  # noqa: F811
    m, pool, exp = oracle_case(oracle_lib, pi)
    g = eng.MapGrid(m.cells())
    for tmode in TOUR_MODES:
        tours, want = oracle_tours(oracle_lib, pi, tmode)
        assert all(3 <= stops_of(t, tmode) <= 6 for t in tours)
        plan = eng.TourPlan(g, PARAMS[pi], tours, tmode)
        plan.run()
        rec = plan.records()
        assert [record_tuple(r) for r in rec] == want, (PARAMS[pi], tmode)
        orders = plan.orders()
        for t, tour in enumerate(tours):
            assert orders[t] == list(want[t][6:6 + stops_of(tour, tmode)])
            seq = [tour[0]] + cell_sequence(tour, orders[t])
            if tmode == abi.TOUR_RETURN:
                seq.append(tour[0])
            if tmode == abi.TOUR_TO_LAST:
                seq.append(tour[-1])
            assert len(seq) == int(rec[t]["n_legs"]) + 1
            sums = [0, 0, 0]
            for r in range(len(seq) - 1):
                leg = plan.leg(t, r)
                assert as_expected(leg) == as_expected(exp[seq[r], seq[r + 1]]), (PARAMS[pi], tmode, t, r)
                sums = [sums[0] + leg.legs, sums[1] + leg.money, sums[2] + leg.time_s]
            assert tuple(sums) == want[t][:3]
            with pytest.raises(eng.EngineError) as ei:
                plan.leg(t, len(seq) - 1)
            assert ei.value.status == MR_ERR_INVALID_ARG


# ---- 2. every size, both paths -----------------------------------------------------------------
_sizes = {}


def sizes_case(eng):  # noqa: F811
    """33 x 33, a pool of 24 cells: (grid, pool, the pool's matrix records per Params, tour index lists).
    A tour per n = 0..10 and 30 mixed ones, as indices into the pool with room for a fixed end."""
    if not _sizes:
        m = SyntheticMap(33, campfires_per_homeland=4, seed=33)
        rng = random.Random(330)
        pool = [CellIndex.center(), m.campfires()[2]] + rng.sample(m.all_indices(), 22)
        pool = list(dict.fromkeys(pool))
        idx = [[rng.randrange(len(pool)) for _ in range(n + 2)] for n in range(11)]
        idx += [[rng.randrange(len(pool)) for _ in range(rng.randint(0, 10) + 2)] for _ in range(30)]
        _sizes["case"] = (m, pool, idx, {})
    return _sizes["case"]


@pytest.mark.parametrize("tmode", TOUR_MODES)
@pytest.mark.parametrize("params", [Params(), Params(sort_by=(SORT_TIME, SORT_MONEY)), Params(sort_by=(SORT_MONEY, SORT_LEGS))])
def test_every_size_on_both_paths(eng, monkeypatch, params, tmode):  # noqa: F811
    """n = 0..10 in one plan: the wave path up to 5 stops, the two workgroup classes beyond (the
    class edges 5/6 and 8/9, the 120 KB table of n = 10).  MR_TOUR_WAVE_MAX=0: every tour on the
    workgroup path; =8: the wave path up to 8 stops (24 KB a wave); MR_TOUR_GX=1: one workgroup
    walks every tour of its class.  All four give the records of the host DP."""
    m, pool, idx, cache = sizes_case(eng)
    g = eng.MapGrid(m.cells())
    key = params.sort_by
    if key not in cache:
        cache[key] = matrix_records(eng, g, params, pool, pool)
    mrec = cache[key]
    where = {c: i for i, c in enumerate(pool)}
    tours = [[pool[i] for i in (ix if tmode == abi.TOUR_TO_LAST else ix[:-1])] for ix in idx]
    assert [stops_of(t, tmode) for t in tours[:11]] == list(range(11))
    order = plan_order(params)
    want = [expected_record(t, tmode, order, lambda a, b: mrec[where[a], where[b], :3]) for t in tours]
    assert all(w[3] == MR_OK for w in want)
    first = None
    for env in ({}, {"MR_TOUR_WAVE_MAX": "0"}, {"MR_TOUR_WAVE_MAX": "8"}, {"MR_TOUR_GX": "1"}):
        for k in ("MR_TOUR_WAVE_MAX", "MR_TOUR_GX"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        plan = eng.TourPlan(g, params, tours, tmode)
        assert plan.num_points == len({c for t in tours for c in t})
        plan.run()
        rec = plan.records()
        got = [record_tuple(r) for r in rec]
        bad = [t for t in range(len(tours)) if got[t] != want[t]]
        assert not bad, (env, params, tmode, len(bad), bad[0], got[bad[0]], want[bad[0]])
        ptr, nbytes = plan.device_records()
        assert nbytes == (len(tours) + 3) // 4 * 4 * 32
        raw = _raw_words(_hip(), ptr, nbytes).reshape(-1, 8)
        assert (raw[:len(tours)] == rec.view(np.uint32).reshape(-1, 8)).all() and (raw[len(tours):] == 0).all()
        if first is None:
            first = raw.copy()
        assert (raw == first).all(), env


# ---- 3. ties -----------------------------------------------------------------------------------
def test_ties_go_to_the_least_order(eng, mode):  # noqa: F811
    m = SyntheticMap(21, campfires_per_homeland=3, seed=5)
    cells = m.all_indices()
    rng = random.Random(55)
    a, b, c, d, e = rng.sample(cells, 5)
    g = eng.MapGrid(m.cells())
    params = Params()
    order = plan_order(params)
    pool = [a, b, c, d, e]
    mrec = matrix_records(eng, g, params, pool, pool)

    def metric(x, y):
        return mrec[pool.index(x), pool.index(y), :3]
    perm1, perm2 = [a, b, c, d, e], [a, d, b, e, c]
    tours = [[a, b, c, b, d, b],      # one cell listed three times
             [a, a, b, c, a],         # stops equal to the start
             [a, b, b, b, b, b],      # all stops the same cell: the identity order
             perm1, perm2]            # two tours that are permutations of each other
    for tmode in (abi.TOUR_OPEN, abi.TOUR_RETURN):
        want, n_best = [], []
        for t in tours:
            M = tour_matrix(t, tmode, metric)
            cost, pi, nb = tr.brute_force(M, tmode, order)
            want.append(tuple(cost) + (MR_OK, stops_of(t, tmode), legs_of(t, tmode)) + tuple(pi) + (0xFF,) * (10 - len(pi)))
            n_best.append(nb)
        assert all(nb >= 2 for nb in n_best[:3]), n_best  # the reference found ties in each
        assert want[2][6:11] == (0, 1, 2, 3, 4)
        plan = eng.TourPlan(g, params, tours, tmode)
        plan.run()
        rec = plan.records()
        assert [record_tuple(r) for r in rec] == want, tmode
        orders = plan.orders()
        assert record_tuple(rec[3])[:3] == record_tuple(rec[4])[:3]
        if n_best[3] == 1:  # a unique optimum: the same cells in the same order
            assert cell_sequence(perm1, orders[3]) == cell_sequence(perm2, orders[4])


# ---- 4. the limit gate -------------------------------------------------------------------------
def test_limit_gate_refuses_one_tour_only(eng, mode):  # noqa: F811
    """Scroll prices of 10^9 under (Legs, Money): a leg that uses a scroll costs 10^9 money, so five
    legs of a tour that holds such a pair could pass 2^32 - 1 and the tour is refused, four could
    not and the tour is answered exactly; a tour of neighbouring cells is cheap."""
    m, hq = lc.case_map("A2")
    params = lc.params_of(lc.cost_of("A2", "top"), (SORT_LEGS, SORT_MONEY), 0, hq)
    assert params.scroll_of_escape_cost == 1_000_000_000
    cells = m.all_indices()
    where = {c: i for i, c in enumerate(cells)}
    g = eng.MapGrid(m.cells())
    mrec = matrix_records(eng, g, params, cells, cells)
    order = plan_order(params)

    def metric(a, b):
        return mrec[where[a], where[b], :3]
    rng = random.Random(4)
    big = cheap = None
    for _ in range(2000):  # five cells with a scroll's leg among their pairs and none with two
        t = rng.sample(cells, 5)
        M = tour_matrix(t, abi.TOUR_OPEN, metric)
        if int(M[:5, :5, 1].max()) >= 999_999_990 and tr.limit_gate(M, 4, abi.TOUR_OPEN):
            big = t
            break
    for h in range(4):  # five neighbours: walks
        t = [CellIndex.homeland(h, x, y) for x, y in ((2, 2), (2, 3), (3, 2), (3, 3), (2, 4))]
        if int(tour_matrix(t, abi.TOUR_OPEN, metric)[:5, :5, 1].max()) < 1000:
            cheap = t
            break
    assert big is not None and cheap is not None
    refused = big + [cheap[0]]  # the same pairs and a fifth leg
    tours = [refused, cheap, big]
    want = [expected_record(t, abi.TOUR_OPEN, order, metric) for t in tours]
    assert want[0] == (0, 0, 0, MR_ERR_LIMIT, 5, 5) + (0xFF,) * 10
    assert want[1][3] == MR_OK and want[2][3] == MR_OK and want[2][1] >= 999_999_990
    plan = eng.TourPlan(g, params, tours, abi.TOUR_OPEN)
    plan.run()
    rec = plan.records()  # MR_OK: the refused tour is its record's business
    assert [record_tuple(r) for r in rec] == want
    assert plan.orders()[0] is None and plan.orders()[1] == list(want[1][6:10])
    assert plan.leg(0, 0) is None
    res = mr_result()
    assert eng.lib().mr_tour_leg_label(plan.handle, 0, 0, C.byref(res), None, 0) == MR_NOT_FOUND
    assert plan.leg(2, 3).money + plan.leg(2, 2).money + plan.leg(2, 1).money + plan.leg(2, 0).money == want[2][1]
    # under MR_TOUR_RETURN the four-stop tour has five legs: refused as well
    back = eng.TourPlan(g, params, tours, abi.TOUR_RETURN)
    back.run()
    want = [expected_record(t, abi.TOUR_RETURN, order, metric) for t in tours]
    assert want[2][3] == MR_ERR_LIMIT and want[1][3] == MR_OK
    assert [record_tuple(r) for r in back.records()] == want


# ---- 5. lifetime -------------------------------------------------------------------------------
def test_reruns_streams_and_plan_kinds(eng, mode):  # noqa: F811
    hip = _hip()
    L = eng.lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    try:
        m = SyntheticMap(33, campfires_per_homeland=3, seed=33)
        cells = m.all_indices()
        rng = random.Random(6)
        g = eng.MapGrid(m.cells())
        tours = [rng.sample(cells, rng.randint(1, 11)) for _ in range(20)] + [[cells[3], cells[3], cells[4]]]
        plan = eng.TourPlan(g, Params(), tours, abi.TOUR_RETURN)
        other = eng.TourPlan(g, Params(sort_by=(SORT_TIME, SORT_LEGS)), tours[:7], abi.TOUR_OPEN)
        mp = eng.MatrixPlan(g, Params(), cells[:3], cells[:10])
        assert plan.num_points == len({c for t in tours for c in t}) == plan.num_sources
        plan.run(stream.value)
        plan.wait()
        first = plan.records().copy()
        ptr, nbytes = plan.device_records()
        raw = _raw_words(hip, ptr, nbytes).copy()
        other.run()
        mp.run()
        plan.run(stream.value)
        plan.run(stream.value)
        plan.wait()
        assert (plan.records() == first).all() and (_raw_words(hip, ptr, nbytes) == raw).all()
        assert (first["status"] == MR_OK).all() and len(other.records()) == 7 and mp.records().shape == (3, 10, 4)
        ms, launches = plan.kernel_ms()
        assert launches >= 1 and ms >= 0.0 and plan.tour_ms() > 0.0
        assert plan.stats()["num_sources"] == plan.num_points
        # the other kinds' accessors on a tour plan
        buf = np.empty((4096, 8), dtype=np.uint32)
        res = (mr_result * 4)()
        n, p, nb = C.c_uint32(), C.c_void_p(), C.c_uint64()
        bad = MR_ERR_INVALID_ARG
        assert L.mr_matrix_records(plan.handle, buf.ctypes.data, 4096) == bad
        assert L.mr_matrix_device_records(plan.handle, C.byref(p), C.byref(nb)) == bad
        assert L.mr_matrix_record_pitch(plan.handle, C.byref(n)) == bad
        assert L.mr_matrix_source_rows(plan.handle, C.byref(n), 1) == bad
        assert L.mr_matrix_label(plan.handle, 0, 0, res, None, 0) == bad
        assert L.mr_nearest_records(plan.handle, buf.ctypes.data, 4096) == bad
        assert L.mr_nearest_label(plan.handle, 0, 0, res, None, 0) == bad
        assert L.mr_nearest_k(plan.handle, C.byref(n)) == bad
        assert L.mr_sssp_records(plan.handle, 0, buf.ctypes.data) == bad
        assert L.mr_sssp_record_pitch(plan.handle, C.byref(n)) == bad
        assert L.mr_plan_fetch(plan.handle, res, None, 0) == bad
        assert L.mr_plan_device_outputs(plan.handle, C.byref(p), C.byref(nb), C.byref(p), C.byref(nb)) == bad
        # the tour accessors on the other kinds
        npl = eng.NearestPlan(g, Params(), cells[:3], cells[:10])
        sp = eng.SSSPPlan(g, Params(), cells[:2])
        qp = eng.Plan(g, Params(), [(cells[0], cells[1])])
        rec = (mr_tour_record * 4)()
        for o in (mp, npl, sp, qp):
            o.run()
            assert L.mr_tour_records(o.handle, rec, 4) == bad
            assert L.mr_tour_device_records(o.handle, C.byref(p), C.byref(nb)) == bad
            assert L.mr_tour_leg_label(o.handle, 0, 0, res, None, 0) == bad
            assert L.mr_tour_num_points(o.handle, C.byref(n)) == bad
            assert L.mr_tour_kernel_ms(o.handle) == 0.0
        assert L.mr_tour_leg_label(plan.handle, len(tours), 0, res, None, 0) == bad
        assert L.mr_tour_records(plan.handle, rec, 4) == abi.MR_ERR_CAPACITY
        assert (plan.records() == first).all()  # the plan still answers
        assert first[-1]["n_legs"] == 3 and plan.orders()[-1] == [0, 1]  # a stop equal to the start comes first
    finally:
        hip.hipStreamSynchronize(stream)
        hip.hipStreamDestroy(stream)


# ---- 6. Fleetfoot 2, Time first: the SSSP kernel writes the matrix ------------------------------
@pytest.mark.parametrize("tmode", TOUR_MODES)
def test_fleetfoot_time_first_against_oracle(eng, oracle_lib, tmode):  # noqa: F811
    params = Params(fleetfoot=2, sort_by=(SORT_TIME, SORT_MONEY))
    m = SyntheticMap(21, campfires_per_homeland=4, seed=62)
    rng = random.Random(620)
    pool = rng.sample(m.all_indices(), 20)
    extra = 2 if tmode == abi.TOUR_TO_LAST else 1
    tours = [rng.sample(pool, n + extra) for n in (0, 2, 4, 5, 6, 7)]
    og = oracle_lib.OracleGrid(m.cells())
    pairs = [(a, b) for a in pool for b in pool]
    exp = dict(zip(pairs, og.find_path_batch(params, pairs, threads=0)))

    def metric(a, b):
        return (exp[a, b].legs, exp[a, b].money, exp[a, b].time_s)
    want = [expected_record(t, tmode, plan_order(params), metric, tr.brute_force) for t in tours]
    plan = eng.TourPlan(eng.MapGrid(m.cells()), params, tours, tmode)
    assert plan.stats()["solver"] not in ("hub", "hub_wide")
    plan.run()
    assert [record_tuple(r) for r in plan.records()] == want
    for t, r in ((3, 0), (5, 6)):
        seq = [tours[t][0]] + cell_sequence(tours[t], plan.orders()[t])
        assert as_expected(plan.leg(t, r)) == as_expected(exp[seq[r], seq[r + 1]])
    # FindPath.eval_tours: a plan, one pass, its records
    assert (eng.FindPath.with_params(eng.MapGrid(m.cells()), params).eval_tours(tours, tmode) == plan.records()).all()
