"""Nearest-source plans (mr_nearest_src_*): per destination and group of sources, the record of the
group's best (MR_SRC_BEST) or worst (MR_SRC_WORST) source and which source it was.

The rule (DESIGN.md section 3b'''''): the winner of group g for destination j is the source i with
group_of_src[i] == g and the least (BEST) or the greatest (WORST) (m[q0], m[q1], m[q2]), m the
metrics of FindPath::eval(sources[i], dests[j]) and (q0, q1, q2) the plan's metric order; ties on
all three go to the smallest i in both modes.  nearest_src_ref restates it in numpy; it is applied to
the oracle's labels (the three metrics and the position: the oracle has no via word) and to
MatrixPlan.records() of the same lists, whose four words, via included, the winner's record must
repeat.  Hub path, sources handed to the SSSP kernel, and the SSSP kernel alone feed the
matrix (the `mode` fixture).  Every comparison is exact."""
import ctypes as C
import random

import numpy as np
import pytest

import irregular_maps as im
import large_costs as lc
import nearest_src_ref as ns
from golden_util import as_expected
from marshrutka_amd import abi
from marshrutka_amd.abi import (MR_ERR_CAPACITY, MR_ERR_INVALID_ARG, MR_ERR_LIMIT, MR_NOT_FOUND, SORT_LEGS, SORT_MONEY,
                                SORT_TIME, CellIndex, Params, mr_nearest_src_record, mr_result)
from marshrutka_amd.mapgen import SyntheticMap
from test_gpu_nearest import matrix_records, plan_order
from test_gpu_sssp import PARAMS, _hip, _raw_words, eng, mode  # noqa: F401  (eng, mode: fixtures)

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
WHICH = [abi.SRC_BEST, abi.SRC_WORST]
SWITCHES = ("MR_ALGO", "MR_HUB_FALLBACK_ALL", "MR_DBG_FLAGS", "MR_MATRIX_GX", "MR_NSRC_SEG", "MR_NSRC_GX")


@pytest.fixture(autouse=True)
def _clear(monkeypatch):
    """No kernel switch set but the test's own (autouse: before `mode` sets its two)."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def device_words(plan):
    """The plan's device records as (n_groups, pitch, 8) words, pads included."""
    ptr, nbytes = plan.device_records()
    pitch = plan.record_pitch()
    assert pitch == (plan.n_dst + 3) // 4 * 4 and nbytes == plan.n_groups * pitch * 32
    return _raw_words(_hip(), ptr, nbytes).reshape(plan.n_groups, pitch, 8).copy()


def expected_words(want, pitch):
    """reduce_sources' (n_dst, n_groups, 5) as the device lays it out: [group][pitch] records of
    eight words, the reserved words and the pad records zeros."""
    n_dst, n_groups = want.shape[:2]
    out = np.zeros((n_groups, pitch, 8), dtype=np.uint32)
    out[:, :n_dst, :5] = want.transpose(1, 0, 2)
    return out


def equals_reduced_matrix(eng, g, params, sources, dests, groups, n_groups, which, mrec):  # noqa: F811
    """A plan of the lists against the reduced matrix records of the same lists: records() and the
    raw device words, pads included.  Returns (plan, records)."""
    plan = eng.NearestSourcePlan(g, params, sources, dests, groups, n_groups=n_groups, which=which)
    plan.run()
    rec = plan.records()
    want = ns.reduce_sources(mrec, groups, n_groups, plan_order(params), which == abi.SRC_WORST)
    assert rec.shape == want.shape == (len(dests), n_groups, 5)
    bad = np.argwhere((rec != want).any(axis=2))
    assert bad.size == 0, (f"{len(bad)} of {len(dests) * n_groups} records wrong", params, which, tuple(bad[0]),
                           rec[tuple(bad[0])], want[tuple(bad[0])])
    assert (device_words(plan) == expected_words(want, plan.record_pitch())).all()
    return plan, rec


# ---- (a) the oracle end to end --------------------------------------------------------------------
_oracle = {}


def oracle_case(oracle_lib, pi):
    """(map, 12 sources, their groups, 20 destinations, the oracle's labels [source][destination]),
    once per PARAMS entry."""
    if pi not in _oracle:
        m = SyntheticMap(33, campfires_per_homeland=4, seed=330 + pi)
        rng = random.Random(3300 + pi)
        cells = m.all_indices()
        sources = [CellIndex.center(), m.campfires()[0], CellIndex.border(1, 1)] + rng.sample(cells, 8)
        sources.append(sources[4])
        dests = [m.campfires()[1], sources[3], sources[4]] + [rng.choice(cells) for _ in range(17)]
        groups = [i % 3 for i in range(12)]
        rng.shuffle(groups)
        og = oracle_lib.OracleGrid(m.cells())
        exp = og.find_path_batch(PARAMS[pi], [(s, d) for s in sources for d in dests], threads=0)
        n = len(dests)
        _oracle[pi] = (m, sources, groups, dests, [exp[i * n:(i + 1) * n] for i in range(len(sources))])
    return _oracle[pi]


@pytest.mark.parametrize("pi", range(len(PARAMS)))
def test_winners_and_labels_match_oracle(eng, oracle_lib, mode, pi):  # noqa: F811
    m, sources, groups, dests, exp = oracle_case(oracle_lib, pi)
    assert len(sources) == 12 and len(dests) == 20
    g = eng.MapGrid(m.cells())
    met = np.zeros((12, 20, 4), dtype=np.int64)
    met[:, :, :3] = [[(e.legs, e.money, e.time_s) for e in row] for row in exp]
    for which in WHICH:
        want = ns.reduce_sources(met, groups, 3, plan_order(PARAMS[pi]), which == abi.SRC_WORST)
        plan = eng.NearestSourcePlan(g, PARAMS[pi], sources, dests, groups, which=which)
        assert plan.n_groups == 3
        plan.run()
        rec = plan.records()
        assert rec.shape == (20, 3, 5)
        assert (rec[:, :, (0, 1, 2, 4)] == want[:, :, (0, 1, 2, 4)]).all(), (PARAMS[pi], which)
        for j in range(20):
            for gi in range(3):
                i = int(rec[j, gi, 4])
                assert as_expected(plan.label(j, gi)) == as_expected(exp[i][j]), (PARAMS[pi], which, j, gi)


# ---- (b) the reduced matrix at the chunk, pitch and segment edges -------------------------------------
GROUP_SIZES = (1, 4, 5, 9, 0)
_edges = {}


def edges_case(eng):  # noqa: F811
    """65 x 65: 19 sources in groups of 1, 4, 5, 9 and 0 in shuffled positions, 130 destinations and
    the matrix records of the lists per Params."""
    if not _edges:
        m = SyntheticMap(65, campfires_per_homeland=5, seed=65)
        rng = random.Random(650)
        cells = m.all_indices()
        sources = [CellIndex.center(), m.campfires()[3]] + rng.sample(cells, 16)
        sources.append(sources[6])
        groups = [gi for gi, n in enumerate(GROUP_SIZES) for _ in range(n)]
        rng.shuffle(groups)
        dests = [rng.choice(cells) for _ in range(128)] + [sources[2], m.campfires()[0]]
        _edges["case"] = (m, sources, groups, dests, {})
    return _edges["case"]


@pytest.mark.parametrize("n_dst", [1, 3, 4, 63, 64, 65, 130])
@pytest.mark.parametrize("params", [Params(), Params(sort_by=(SORT_TIME, SORT_MONEY)), Params(sort_by=(SORT_MONEY, SORT_LEGS))])
def test_reduced_matrix_at_edges(eng, monkeypatch, params, n_dst):  # noqa: F811
    """MR_NSRC_SEG=4 cuts the groups of 5 and 9 into 2 and 3 segments (the partials and the merge),
    leaves the groups of 1 and 4 whole, the group of 4 ending exactly on a segment edge, and the
    empty group a segment of no source; the default segmentation keeps these small groups whole;
    MR_NSRC_GX=1 has four waves walk every item.  All give the reduced matrix, pads included."""
    m, sources, groups, dests, cache = edges_case(eng)
    assert len(sources) == 19 and [groups.count(gi) for gi in range(5)] == list(GROUP_SIZES)
    g = eng.MapGrid(m.cells())
    if params.sort_by not in cache:
        cache[params.sort_by] = matrix_records(eng, g, params, sources, dests)
    mrec = cache[params.sort_by][:, :n_dst]
    seen = {"whole": 0, "split": 0, "on_edge": 0}
    for env in ({"MR_NSRC_SEG": "4"}, {}, {"MR_NSRC_GX": "1"}, {"MR_NSRC_SEG": "4", "MR_NSRC_GX": "1"}):
        for k in ("MR_NSRC_SEG", "MR_NSRC_GX"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for which in WHICH:
            plan, rec = equals_reduced_matrix(eng, g, params, sources, dests[:n_dst], groups, 5, which, mrec)
            seg = plan.segmentation()
            if "MR_NSRC_SEG" in env:
                assert seg == {"seg_len": 4, "whole": 3, "split": 2, "on_edge": 1}, (env, seg)
            else:
                assert seg["seg_len"] >= 9 and seg["whole"] == 5 and seg["split"] == 0, (env, seg)
            for k in seen:
                seen[k] += seg[k]
            assert (rec[:, 4] == (0, 0, 0, 0, NONE)).all() and plan.label(0, 4) is None
    assert seen["whole"] and seen["split"] and seen["on_edge"]


def test_default_segmentation_splits_long_groups(eng):  # noqa: F811
    """256 + 136 sources x 5 destinations: one chunk x two groups leave nearly every wave slot empty,
    so the host cuts the groups at its floor of 128 sources: 2 segments ending on an edge, and 2."""
    m, _, _, dests, _ = edges_case(eng)
    rng = random.Random(651)
    cells = m.all_indices()
    pool = rng.sample(cells, 150)
    sources = [rng.choice(pool) for _ in range(392)]
    groups = [0] * 256 + [1] * 136
    rng.shuffle(groups)
    g = eng.MapGrid(m.cells())
    params = Params()
    mrec = matrix_records(eng, g, params, sources, dests[:5])
    for which in WHICH:
        plan, _ = equals_reduced_matrix(eng, g, params, sources, dests[:5], groups, 2, which, mrec)
        assert plan.segmentation() == {"seg_len": 128, "whole": 0, "split": 2, "on_edge": 1}


# ---- (c) ties ------------------------------------------------------------------------------------------
def test_ties_go_to_the_smallest_position(eng, mode, monkeypatch):  # noqa: F811
    """Group 0 lists one cell nine times (with MR_NSRC_SEG=4: within a segment and across three):
    every source ties for every destination, and position 0 wins under BEST and under WORST.  Group
    1 lists a cell at positions 3, 5 (one segment) and 13 (another) among others: where that cell
    wins, and it wins BEST where it is the destination, its record names position 3."""
    m = SyntheticMap(33, campfires_per_homeland=3, seed=7)
    rng = random.Random(77)
    cells = m.all_indices()
    b, c, *others = rng.sample(cells, 8)
    sources = [b, others[0], b, c, b, c, b, others[1], b, others[2], b, others[3], b, c, b, others[4], b, others[5]]
    groups = [i % 2 for i in range(len(sources))]
    dests = [c, b] + rng.sample(cells, 20)
    g = eng.MapGrid(m.cells())
    params = Params()
    mrec = matrix_records(eng, g, params, sources, dests)
    for seg in ("4", None):
        if seg:
            monkeypatch.setenv("MR_NSRC_SEG", seg)
        else:
            monkeypatch.delenv("MR_NSRC_SEG", raising=False)
        for which in WHICH:
            plan, rec = equals_reduced_matrix(eng, g, params, sources, dests, groups, 2, which, mrec)
            assert plan.segmentation()["split"] == (2 if seg else 0)
            assert (rec[:, 0, 4] == 0).all(), which
            if which == abi.SRC_BEST:
                assert tuple(rec[0, 1]) == (0, 0, 0, NONE, 3)
                assert tuple(rec[1, 0]) == (0, 0, 0, NONE, 0)
    # every source the same cell, one group, default segmentation
    for which in WHICH:
        plan = eng.NearestSourcePlan(g, params, [b] * 7, dests, which=which)
        plan.run()
        rec = plan.records()
        assert (rec[:, 0, 4] == 0).all() and (rec[:, 0, :4] == mrec[0]).all()


# ---- (d) further cases -----------------------------------------------------------------------------------
def test_destination_equal_to_a_source_and_specials(eng, mode):  # noqa: F811
    m = SyntheticMap(65, campfires_per_homeland=4, seed=12)
    rng = random.Random(120)
    cells = m.all_indices()
    specials = [CellIndex.center(), CellIndex.border(0, 2), CellIndex.border(3, 1)] + m.campfires()[:6]
    sources = rng.sample(cells, 9) + [specials[4]]
    sources.append(sources[2])                  # position 10 repeats position 2
    groups = [0, 0, 0, 0, 1, 1, 1, 2, 1, 0, 1]  # group 2: the source at position 7 alone
    dests = specials + [sources[2], sources[7], sources[5]] + rng.sample(cells, 10)
    g = eng.MapGrid(m.cells())
    for params in (Params(), Params(sort_by=(SORT_MONEY, SORT_TIME))):
        mrec = matrix_records(eng, g, params, sources, dests)
        best = equals_reduced_matrix(eng, g, params, sources, dests, groups, 3, abi.SRC_BEST, mrec)[1]
        worst = equals_reduced_matrix(eng, g, params, sources, dests, groups, 3, abi.SRC_WORST, mrec)[1]
        n = len(specials)
        # a destination that is a source wins BEST in its groups with the matrix record of a cell
        # to itself, at the cell's smallest position of the group
        assert tuple(best[n, 0]) == (0, 0, 0, NONE, 2) and tuple(best[n, 1]) == (0, 0, 0, NONE, 10)
        assert tuple(best[n + 2, 1]) == (0, 0, 0, NONE, 5) and tuple(best[4, 0]) == (0, 0, 0, NONE, 9)
        # it does not win WORST among others, and does where it is alone
        assert worst[n, 0, 4] != 2 and worst[n, 1, 4] != 10 and worst[n + 2, 1, 4] != 5 and worst[4, 0, 4] != 9
        assert tuple(worst[n + 1, 2]) == (0, 0, 0, NONE, 7) == tuple(best[n + 1, 2])


def test_transposed_layout_against_reduced_matrix(eng, mode):  # noqa: F811
    name, k, pi = "unequal9", 5, 1
    m = im.oriented(name, k)
    cells = m.all_indices()
    params = im.params_for(im.get_map(name))[pi]
    order = list(range(len(cells)))
    random.Random(96).shuffle(order)
    sources = im.transposed_sources(name) + [cells[j] for j in order[:20]]
    groups = [i % 3 for i in range(len(sources))]
    dests = [cells[j] for j in order] + [cells[order[0]]]
    g = eng.MapGrid(m.cells())
    mrec = matrix_records(eng, g, params, sources, dests)
    exp = im.py_ref_all(name, k, pi, im.transposed_sources(name))
    for i in range(len(exp)):  # the matrix is the reference's: (legs, money, time) per destination
        assert [tuple(int(x) for x in mrec[i, jj, :3]) for jj in range(len(order))] == [tuple(exp[i][j][:3]) for j in order]
    for which in WHICH:
        equals_reduced_matrix(eng, g, params, sources, dests, groups, 3, which, mrec)


# ---- (e) plan handling -----------------------------------------------------------------------------------
def test_reruns_streams_and_plan_kinds(eng, mode, monkeypatch):  # noqa: F811
    hip = _hip()
    L = eng.lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    try:
        m = SyntheticMap(33, campfires_per_homeland=3, seed=33)
        cells = m.all_indices()
        rng = random.Random(6)
        g = eng.MapGrid(m.cells())
        sources, dests = rng.sample(cells, 30), rng.sample(cells, 70)
        groups = [i % 2 for i in range(30)]
        monkeypatch.setenv("MR_NSRC_SEG", "4")
        plan = eng.NearestSourcePlan(g, Params(), sources, dests, groups, which=abi.SRC_WORST)
        monkeypatch.delenv("MR_NSRC_SEG")
        other = eng.NearestSourcePlan(g, Params(sort_by=(SORT_TIME, SORT_LEGS)), sources[:7], dests[:9])
        mp = eng.MatrixPlan(g, Params(), sources, dests)
        plan.run(stream.value)
        plan.wait()
        first = plan.records().copy()
        raw = device_words(plan)
        other.run()
        mp.run()
        plan.run(stream.value)
        plan.run(stream.value)
        plan.wait()
        assert (plan.records() == first).all() and (device_words(plan) == raw).all()
        assert (first == ns.reduce_sources(mp.records(), groups, 2, plan_order(Params()), True)).all()
        assert other.records().shape == (9, 1, 5)
        ms, launches = plan.kernel_ms()
        assert launches >= 1 and ms >= 0.0 and plan.reduce_ms() > 0.0
        assert plan.stats()["num_sources"] == 30
        # the other kinds' accessors on a nearest-source plan
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
        assert L.mr_tour_records(plan.handle, buf.ctypes.data, 4096) == bad
        assert L.mr_tour_num_points(plan.handle, C.byref(n)) == bad
        assert L.mr_tour_kernel_ms(plan.handle) == 0.0
        assert L.mr_sssp_records(plan.handle, 0, buf.ctypes.data) == bad
        assert L.mr_sssp_record_pitch(plan.handle, C.byref(n)) == bad
        assert L.mr_plan_fetch(plan.handle, res, None, 0) == bad
        assert L.mr_plan_device_outputs(plan.handle, C.byref(p), C.byref(nb), C.byref(p), C.byref(nb)) == bad
        # the nearest-source accessors on the other kinds
        npl = eng.NearestPlan(g, Params(), cells[:3], cells[:10])
        tp = eng.TourPlan(g, Params(), [cells[:4]])
        sp = eng.SSSPPlan(g, Params(), cells[:2])
        qp = eng.Plan(g, Params(), [(cells[0], cells[1])])
        rec = (mr_nearest_src_record * 4)()
        for o in (mp, npl, tp, sp, qp):
            o.run()
            assert L.mr_nearest_src_records(o.handle, rec, 4) == bad
            assert L.mr_nearest_src_device_records(o.handle, C.byref(p), C.byref(nb)) == bad
            assert L.mr_nearest_src_record_pitch(o.handle, C.byref(n)) == bad
            assert L.mr_nearest_src_label(o.handle, 0, 0, res, None, 0) == bad
            assert L.mr_nearest_src_segmentation(o.handle, C.byref(n), None, None, None) == bad
            assert L.mr_nearest_src_kernel_ms(o.handle) == 0.0
        assert L.mr_nearest_src_label(plan.handle, len(dests), 0, res, None, 0) == bad
        assert L.mr_nearest_src_label(plan.handle, 0, 2, res, None, 0) == bad
        assert L.mr_nearest_src_records(plan.handle, rec, 4) == MR_ERR_CAPACITY
        assert (plan.records() == first).all()  # the plan still answers
    finally:
        hip.hipStreamSynchronize(stream)
        hip.hipStreamDestroy(stream)


@pytest.mark.parametrize("which", WHICH)
def test_fleetfoot_time_first_against_oracle(eng, oracle_lib, which):  # noqa: F811
    """Fleetfoot 2, Time first: the SSSP kernel writes the matrix rows the reduction reads."""
    params = Params(fleetfoot=2, sort_by=(SORT_TIME, SORT_MONEY))
    m = SyntheticMap(33, campfires_per_homeland=4, seed=62)
    rng = random.Random(620)
    cells = m.all_indices()
    sources, dests = rng.sample(cells, 10), rng.sample(cells, 12)
    groups = [i % 2 for i in range(10)]
    og = oracle_lib.OracleGrid(m.cells())
    exp = og.find_path_batch(params, [(s, d) for s in sources for d in dests], threads=0)
    met = np.zeros((10, 12, 4), dtype=np.int64)
    met[:, :, :3] = np.array([(e.legs, e.money, e.time_s) for e in exp]).reshape(10, 12, 3)
    want = ns.reduce_sources(met, groups, 2, plan_order(params), which == abi.SRC_WORST)
    g = eng.MapGrid(m.cells())
    plan = eng.NearestSourcePlan(g, params, sources, dests, groups, which=which)
    assert plan.stats()["solver"] not in ("hub", "hub_wide")
    plan.run()
    rec = plan.records()
    assert (rec[:, :, (0, 1, 2, 4)] == want[:, :, (0, 1, 2, 4)]).all()
    for j, gi in ((0, 0), (5, 1), (11, 0)):
        assert as_expected(plan.label(j, gi)) == as_expected(exp[int(rec[j, gi, 4]) * 12 + j])
    # FindPath.eval_nearest_source: a plan, one pass, its records
    fp = eng.FindPath.with_params(g, params)
    assert (fp.eval_nearest_source(sources, dests, groups, worst=which == abi.SRC_WORST) == rec).all()


def test_scroll_prices_of_1e9_and_the_limit(eng, mode):  # noqa: F811
    """Scroll prices of 10^9 under (Legs, Money): money words near 2^30 compare and copy exactly.
    At a price of 2^32 - 1 a scroll plus anything passes 32 bits: the matrix pass flags it, and the
    accessors that wait report MR_ERR_LIMIT, never a wrapped record."""
    m, hq = lc.case_map("A2")
    params = lc.params_of(lc.cost_of("A2", "top"), (SORT_LEGS, SORT_MONEY), 0, hq)
    assert params.scroll_of_escape_cost == 1_000_000_000
    cells = m.all_indices()
    sources = cells
    groups = [i % 2 for i in range(len(sources))]
    g = eng.MapGrid(m.cells())
    mrec = matrix_records(eng, g, params, sources, cells)
    assert int(mrec[:, :, 1].max()) >= 999_999_990
    for which in WHICH:
        equals_reduced_matrix(eng, g, params, sources, cells, groups, 2, which, mrec)
    m, _ = lc.case_map("A1")
    params = lc.b_params(lc.B_PRICES[1], (SORT_LEGS, SORT_MONEY))
    plan = eng.NearestSourcePlan(eng.MapGrid(m.cells()), params, lc.sources_of("A1")[:8], m.all_indices(), [i % 4 for i in range(8)])
    plan.run()
    with pytest.raises(eng.EngineError) as ei:
        plan.records()
    assert ei.value.status == MR_ERR_LIMIT
    plan.run()
    with pytest.raises(eng.EngineError) as ei:
        plan.label(0, 0)
    assert ei.value.status == MR_ERR_LIMIT


# ---- (f) eval_rally --------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", [Params(), Params(sort_by=(SORT_TIME, SORT_MONEY))])
def test_eval_rally(eng, params):  # noqa: F811
    m = SyntheticMap(33, campfires_per_homeland=3, seed=91)
    rng = random.Random(910)
    cells = m.all_indices()
    members, candidates = rng.sample(cells, 9), m.campfires()[:5] + rng.sample(cells, 12)
    g = eng.MapGrid(m.cells())
    mrec = matrix_records(eng, g, params, members, candidates)
    j, rec = eng.FindPath.with_params(g, params).eval_rally(members, candidates)
    wj, wrec = ns.rally(mrec, plan_order(params))
    assert j == wj and (rec == wrec).all()
    assert (mrec[int(rec[4]), j] == rec[:4]).all()
