"""Cost matrix plans (mr_matrix_*): the records of n_src sources x n_dst listed destinations
against the oracle's FindPath::eval, against the all-destinations plans' records word for
word, at the chunk and pitch edges, across the Center's detour, over reruns and streams, at
the 32-bit money limit, and their device footprint.  Hub path (the matrix kernel), sources
handed to the SSSP kernel, and the SSSP kernel alone (the `mode` fixture)."""
import ctypes as C
import random

import numpy as np
import pytest

import large_costs as lc
from crafted_records import RESULT_DT
from golden_util import as_expected
from marshrutka_amd.abi import (MR_ERR_INVALID_ARG, MR_ERR_INVALID_INDEX, MR_ERR_LIMIT, SORT_LEGS, SORT_MONEY, CellIndex,
                                Params, mr_result)
from marshrutka_amd.mapgen import SyntheticMap, geo_to_index
from test_gpu_sssp import FILL_PARAMS, PARAMS, _hip, _raw_words, eng, mode  # noqa: F401  (eng, mode: fixtures)

pytestmark = pytest.mark.gpu


def metrics(labels):
    return np.array([(e.legs, e.money, e.time_s) for e in labels], dtype=np.int64)


def clean_env(monkeypatch):
    for k in ("MR_ALGO", "MR_HUB_FALLBACK_ALL", "MR_DBG_FLAGS", "MR_MATRIX_GX", "MR_FILL_GX", "MR_FILL_OVERLAP"):
        monkeypatch.delenv(k, raising=False)


# ---- 1. parity against the oracle ---------------------------------------------------------
_parity = {}


def parity_case(oracle_lib, size, k, clustered, pi):
    """(map, sources, destinations, the oracle's labels [source][destination]), once per case."""
    key = (size, pi)
    if key not in _parity:
        m = SyntheticMap(size, campfires_per_homeland=k, seed=size + pi, clustered=clustered)
        rng = random.Random(size * 10 + pi)
        cells = m.all_indices()
        three = rng.sample(cells, 3)
        sources = [CellIndex.center(), m.campfires()[0], CellIndex.border(1, 1)] + three + [three[1]]
        if size <= 21:
            dests = list(cells)
        else:
            H = size // 2
            specials = [CellIndex.center()] + [CellIndex.border(b, 1) for b in range(4)] + m.campfires()
            axes = [geo_to_index(x, 0) for x in range(-H, H + 1)] + [geo_to_index(0, y) for y in range(-H, H + 1)]
            dests = specials + sources + axes + rng.sample(cells, 150)
            dests += [dests[3], dests[40], dests[40]]
        og = oracle_lib.OracleGrid(m.cells())
        exp = og.find_path_batch(PARAMS[pi], [(s, d) for s in sources for d in dests], threads=0)
        n = len(dests)
        _parity[key] = (m, sources, dests, [exp[i * n:(i + 1) * n] for i in range(len(sources))])
    return _parity[key]


@pytest.mark.parametrize("size,k,clustered", [(9, 2, False), (21, 5, True), (33, 4, False)])
@pytest.mark.parametrize("pi", range(len(PARAMS)))
def test_records_and_labels_match_oracle(eng, oracle_lib, mode, size, k, clustered, pi):  # noqa: F811
    m, sources, dests, exp = parity_case(oracle_lib, size, k, clustered, pi)
    g = eng.MapGrid(m.cells())
    plan = eng.MatrixPlan(g, PARAMS[pi], sources, dests)
    plan.run()
    rec = plan.records()
    assert rec.shape == (len(sources), len(dests), 4)
    for i in range(len(sources)):
        want = metrics(exp[i])
        bad = np.nonzero((rec[i, :, :3].astype(np.int64) != want).any(axis=1))[0]
        assert bad.size == 0, (PARAMS[pi], sources[i], dests[bad[0]], rec[i, bad[0]], want[bad[0]])
        for j, d in enumerate(dests):
            if d == sources[i]:
                assert tuple(rec[i, j]) == (0, 0, 0, 0xFFFFFFFF)
    assert (rec[6] == rec[4]).all()  # the repeated source
    pairs = [(i, j) for i in range(len(sources)) for j in range(len(dests))]
    if size > 9:
        pairs = random.Random(pi).sample(pairs, 200)
    for i, j in pairs:
        assert as_expected(plan.label(i, j)) == as_expected(exp[i][j]), (PARAMS[pi], sources[i], dests[j])


# ---- 2. matrix against all-destinations, every cell ------------------------------------------
_sssp_all = {}


# gx "1": MR_MATRIX_GX=1, one workgroup.  Its four waves share every source in turn (G = 4), so a
# wave walks 65 (129^2) or 102 (161^2) chunks of each of the five sources: the chunk loop's
# prefetch of the next chunk's destinations and the stores between two loads, checked cell by cell.
@pytest.mark.parametrize("flags,gx", [("", None), ("2", None), ("", "1"), ("2", "1")])
@pytest.mark.parametrize("size,k,clustered,pi", [(129, 4, False, 0), (129, 9, True, 1), (161, 6, False, 2),
                                                  (129, 5, True, 3), (129, 8, False, 4), (161, 7, True, 5)])
def test_every_cell_equals_all_destinations_records(eng, oracle_lib, monkeypatch, flags, gx, size, k, clustered, pi):  # noqa: F811
    clean_env(monkeypatch)
    if flags:
        monkeypatch.setenv("MR_DBG_FLAGS", flags)
    if gx:
        monkeypatch.setenv("MR_MATRIX_GX", gx)
    params = FILL_PARAMS[pi]
    m = SyntheticMap(size, campfires_per_homeland=k, seed=size * 7 + pi, clustered=clustered)
    rng = random.Random(size + pi)
    cells = m.all_indices()
    sources = [m.campfires()[1], CellIndex.center()] + rng.sample(cells, 3)
    g = eng.MapGrid(m.cells())
    plan = eng.MatrixPlan(g, params, sources, cells)
    plan.run()
    assert plan.stats()["solver"] == "hub" and plan.stats()["fill_launch"] == "serial"
    rec = plan.records()
    monkeypatch.delenv("MR_DBG_FLAGS", raising=False)
    ref = eng.SSSPPlan(g, params, sources)
    ref.run()
    for i in range(len(sources)):
        want = ref.records(i)
        bad = np.nonzero((rec[i] != want).any(axis=1))[0]
        assert bad.size == 0, (params, sources[i], len(bad), cells[bad[0]], rec[i, bad[0]], want[bad[0]])
    if pi not in _sssp_all:  # one source per parameter set against the oracle's full search
        og = oracle_lib.OracleGrid(m.cells())
        _sssp_all[pi] = metrics(og.sssp_all(params, sources[2]))
    assert (rec[2, :, :3].astype(np.int64) == _sssp_all[pi]).all()


# ---- 3. chunk and pitch edges -------------------------------------------------------------------
_edges = {}


def edge_case(eng):  # noqa: F811
    """The 21^2 map, 300 sources (with repeats), 129 destinations, and a pair plan's metrics
    [source][destination] for all of them, once."""
    if not _edges:
        m = SyntheticMap(21, campfires_per_homeland=3, seed=21)
        cells = m.all_indices()
        rng = random.Random(300)
        sources = [rng.choice(cells) for _ in range(300)]
        dests = [CellIndex.center(), m.campfires()[0], sources[5]] + rng.sample(cells, 126)
        g = eng.MapGrid(m.cells())
        pairs = eng.Plan(g, Params(), [(s, d) for s in sources for d in dests])
        pairs.run()
        r = np.frombuffer(pairs.fetch_raw()[0], dtype=RESULT_DT, count=300 * 129)
        assert (r["status"] == 0).all()
        want = np.stack([r["legs"].astype(np.int64), r["money"].astype(np.int64), r["time_s"].astype(np.int64)], axis=1)
        _edges["case"] = (m, g, sources, dests, want.reshape(300, 129, 3))
    return _edges["case"]


@pytest.mark.parametrize("gx", [None, "1"])
@pytest.mark.parametrize("n_src", [1, 300])
@pytest.mark.parametrize("n_dst", [1, 7, 8, 9, 63, 64, 65, 129])
def test_chunk_and_pitch_edges(eng, monkeypatch, n_dst, n_src, gx):  # noqa: F811
    clean_env(monkeypatch)
    m, g, sources, dests, want = edge_case(eng)
    if gx:
        # one workgroup: its waves walk every source, at most one chunk of each (129 destinations
        # are 3 chunks for 4 waves; many chunks a wave: test_every_cell_equals_all_destinations_records)
        monkeypatch.setenv("MR_MATRIX_GX", gx)
    src = sources[:n_src]
    plan = eng.MatrixPlan(g, Params(), src, dests[:n_dst])
    plan.run()
    rec = plan.records()
    assert (rec[:, :, :3].astype(np.int64) == want[:n_src, :n_dst]).all()
    pitch = plan.record_pitch()
    assert pitch == (n_dst + 7) // 8 * 8
    ptr, nbytes = plan.device_records()
    distinct = sorted(set(src), key=m.cell_of)
    assert plan.num_sources == len(distinct) and nbytes == len(distinct) * pitch * 16
    rows = plan.source_rows()
    assert rows == [distinct.index(s) for s in src]  # plan sources: distinct, row-major cell order
    raw = _raw_words(_hip(), ptr, nbytes).reshape(len(distinct), pitch, 4)
    assert (raw[rows, :n_dst] == rec).all()


# ---- 4. the detour round the Center -----------------------------------------------------------------
@pytest.mark.parametrize("flags", ["", "2"])
def test_axis_detour(eng, oracle_lib, mode, monkeypatch, flags):  # noqa: F811
    monkeypatch.setenv("MR_DBG_FLAGS", flags or "0")
    m = SyntheticMap(15, campfires_per_homeland=2, seed=15)
    params = Params(use_soe=False, use_caravans=False)
    axis = [geo_to_index(x, 0) for x in range(-7, 8)] + [geo_to_index(0, y) for y in range(-7, 8) if y]
    assert CellIndex.center() in axis
    g = eng.MapGrid(m.cells())
    og = oracle_lib.OracleGrid(m.cells())
    plan = eng.MatrixPlan(g, params, axis, axis)
    plan.run()
    rec = plan.records()
    exp = og.find_path_batch(params, [(s, d) for s in axis for d in axis], threads=0)
    want = metrics(exp).reshape(len(axis), len(axis), 3)
    assert (rec[:, :, :3].astype(np.int64) == want).all()
    # full labels of pairs on opposite sides of the Center and with the Center itself
    i, j = axis.index(geo_to_index(-3, 0)), axis.index(geo_to_index(4, 0))
    for i, j in [(i, j), (j, i), (axis.index(CellIndex.center()), j), (i, axis.index(CellIndex.center()))]:
        assert as_expected(plan.label(i, j)) == as_expected(exp[i * len(axis) + j])


# ---- 5. reruns and streams -----------------------------------------------------------------------------
def test_reruns_and_streams(eng, mode):  # noqa: F811
    hip = _hip()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    try:
        m = SyntheticMap(33, campfires_per_homeland=3, seed=33)
        cells = m.all_indices()
        rng = random.Random(5)
        s = rng.choice(cells)
        g = eng.MapGrid(m.cells())
        plan = eng.MatrixPlan(g, Params(), [s, s, m.campfires()[1], CellIndex.center()], rng.sample(cells, 100))
        assert plan.num_sources == 3 and plan.stats()["num_sources"] == 3
        plan.run()
        first = plan.records().copy()
        plan.run(stream.value)
        plan.wait()
        assert (plan.records() == first).all()
        plan.run()
        assert (plan.records() == first).all()
        assert (first[0] == first[1]).all()
    finally:
        hip.hipStreamSynchronize(stream)
        hip.hipStreamDestroy(stream)


# ---- 6. the wrong kind of plan ---------------------------------------------------------------------------
def test_wrong_plan_kind(eng, monkeypatch):  # noqa: F811
    clean_env(monkeypatch)
    L = eng.lib()
    m = SyntheticMap(9, campfires_per_homeland=2, seed=9)
    cells = m.all_indices()
    g = eng.MapGrid(m.cells())
    mp = eng.MatrixPlan(g, Params(), cells[:3], cells[:10])
    sp = eng.SSSPPlan(g, Params(), cells[:3])
    qp = eng.Plan(g, Params(), [(cells[0], cells[1])])
    for p in (mp, sp, qp):
        p.run()
    buf = np.empty((81, 4), dtype=np.uint32)
    res = (mr_result * 4)()
    assert L.mr_sssp_records(mp.handle, 0, buf.ctypes.data) == MR_ERR_INVALID_ARG
    assert L.mr_plan_fetch(mp.handle, res, None, 0) == MR_ERR_INVALID_ARG
    assert L.mr_matrix_records(qp.handle, buf.ctypes.data, 81) == MR_ERR_INVALID_ARG
    assert L.mr_matrix_records(sp.handle, buf.ctypes.data, 81) == MR_ERR_INVALID_ARG
    n = C.c_uint32()
    assert L.mr_matrix_record_pitch(sp.handle, C.byref(n)) == MR_ERR_INVALID_ARG
    assert L.mr_sssp_record_pitch(mp.handle, C.byref(n)) == MR_ERR_INVALID_ARG
    with pytest.raises(eng.EngineError) as ei:
        eng.MatrixPlan(g, Params(), cells[:3], cells[:4] + [CellIndex.homeland(0, 9, 9)])
    assert ei.value.status == MR_ERR_INVALID_INDEX and "destination 4" in str(ei.value)
    with pytest.raises(eng.EngineError) as ei:
        eng.MatrixPlan(g, Params(), [cells[0], CellIndex.border(2, 7)], cells[:4])
    assert ei.value.status == MR_ERR_INVALID_INDEX and "source 1" in str(ei.value)
    assert mp.records().shape == (3, 10, 4)  # the plans still answer


# ---- 7. large money --------------------------------------------------------------------------------------
def test_large_money_is_exact(eng, oracle_lib, mode):  # noqa: F811
    """Scroll prices of 2^31 - 1000 under (Money, Legs): candidates with bit 31 set, nothing
    wraps (large_costs.oracle_answers asserts it), records exact against the oracle."""
    lc.oracle_answers(oracle_lib, "A1", "top")
    m, hq = lc.case_map("A1")
    params = lc.params_of(lc.cost_of("A1", "top"), (SORT_MONEY, SORT_LEGS), 0, hq)
    assert params.scroll_of_escape_cost == (1 << 31) - 1000
    sources, cells = lc.sources_of("A1")[:8], m.all_indices()
    og = oracle_lib.OracleGrid(m.cells())
    exp = og.find_path_batch(params, [(s, d) for s in sources for d in cells], threads=0)
    plan = eng.MatrixPlan(eng.MapGrid(m.cells()), params, sources, cells)
    plan.run()
    rec = plan.records()
    assert (rec[:, :, :3].astype(np.int64) == metrics(exp).reshape(len(sources), len(cells), 3)).all()
    for i, j in [(0, 5), (3, 40), (7, 80)]:
        assert as_expected(plan.label(i, j)) == as_expected(exp[i * len(cells) + j])


def test_money_past_32_bits_is_a_limit_error(eng, mode):  # noqa: F811
    """(Legs, Money) at a price of 2^32 - 1: a scroll plus anything passes 32 bits, so the
    plan reports MR_ERR_LIMIT and never hands out a wrapped record."""
    m, _ = lc.case_map("A1")
    params = lc.b_params(lc.B_PRICES[1], (SORT_LEGS, SORT_MONEY))
    plan = eng.MatrixPlan(eng.MapGrid(m.cells()), params, lc.sources_of("A1")[:8], m.all_indices())
    plan.run()
    with pytest.raises(eng.EngineError) as ei:
        plan.records()
    assert ei.value.status == MR_ERR_LIMIT


# ---- 8. footprint --------------------------------------------------------------------------------------------
def test_footprint_below_all_destinations_plan(eng, monkeypatch):  # noqa: F811
    clean_env(monkeypatch)
    L = eng.lib()
    m = SyntheticMap(129, campfires_per_homeland=4, seed=129)
    cells = m.all_indices()
    rng = random.Random(64)
    sources, dests = rng.sample(cells, 64), rng.sample(cells, 64)
    g = eng.MapGrid(m.cells())

    def live_with(make):
        L.mr_cache_trim()
        before = C.c_uint64()
        L.mr_cache_live(None, C.byref(before))
        plan = make()
        plan.run()
        plan.wait()
        now = C.c_uint64()
        L.mr_cache_live(None, C.byref(now))
        del plan
        return now.value - before.value

    matrix = live_with(lambda: eng.MatrixPlan(g, Params(), sources, dests))
    sssp = live_with(lambda: eng.SSSPPlan(g, Params(), sources))
    assert 0 < matrix < sssp, (matrix, sssp)
