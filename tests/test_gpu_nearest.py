"""Nearest-of-set plans (mr_nearest_*): per source and destination group, the record of the
group's best destination and which destination it was.

The rule (DESIGN.md section 3b''): the winner of group g from source i is the position j of the
caller's list with group_of_dst[j] == g and the least (m[q0], m[q1], m[q2], j), m the metrics of
FindPath::eval(sources[i], dests[j]) and (q0, q1, q2) the plan's metric order.  It is restated
here twice in numpy: over the oracle's (or py_ref's) labels, and over MatrixPlan.records() of
the same lists, whose four words the winner's record must repeat.  Hub path (nearest_kernel),
sources handed to the SSSP kernel (write_nearest), and the SSSP kernel alone (the `mode`
fixture)."""
import ctypes as C
import random

import numpy as np
import pytest

import irregular_maps as im
import large_costs as lc
from golden_util import as_expected
from marshrutka_amd.abi import (MR_ERR_INVALID_ARG, MR_ERR_INVALID_INDEX, MR_ERR_LIMIT, SORT_LEGS, SORT_MONEY, SORT_TIME,
                                CellIndex, Params, mr_result)
from marshrutka_amd.mapgen import SyntheticMap, geo_to_index
from test_gpu_sssp import FILL_PARAMS, PARAMS, _hip, _raw_words, eng, mode  # noqa: F401  (eng, mode: fixtures)

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
SWITCHES = ("MR_ALGO", "MR_HUB_FALLBACK_ALL", "MR_DBG_FLAGS", "MR_MATRIX_GX", "MR_NEAREST_GX", "MR_FILL_GX",
            "MR_FILL_OVERLAP")


@pytest.fixture(autouse=True)
def _clear(monkeypatch):
    """No kernel switch set but the test's own (autouse: before `mode` sets its two)."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def plan_order(params):
    """The plan's metric order as columns of (legs, money, time): sort_by completed to all
    three metrics the way the comparator does."""
    s1, s2 = params.sort_by
    if s1 == s2:
        s2 = SORT_TIME if s1 == SORT_LEGS else SORT_LEGS
    col = {SORT_LEGS: 0, SORT_MONEY: 1, SORT_TIME: 2}
    return [col[s1], col[s2], col[3 - s1 - s2]]


def winners(metrics, groups, n_groups, order):
    """metrics: (n_src, n_dst, >= 3) integers.  The winning position per (source, group), -1 for
    an empty group: the least (metrics in `order`, position)."""
    groups = np.asarray(groups)
    out = np.full((metrics.shape[0], n_groups), -1, dtype=np.int64)
    for g in range(n_groups):
        J = np.nonzero(groups == g)[0]
        if J.size:
            m = metrics[:, J].astype(np.int64)
            keys = (np.broadcast_to(J, m.shape[:2]), m[:, :, order[2]], m[:, :, order[1]], m[:, :, order[0]])
            out[:, g] = J[np.lexsort(keys, axis=-1)[:, 0]]
    return out


def reduce_matrix(rec, groups, n_groups, order):
    """The (n_src, n_groups, 5) records a nearest plan must give, from MatrixPlan.records()."""
    win = winners(rec, groups, n_groups, order)
    out = np.zeros((rec.shape[0], n_groups, 5), dtype=np.uint32)
    out[:, :, 4] = NONE
    for g in range(n_groups):
        if (win[:, g] >= 0).all():
            out[:, g, :4] = rec[np.arange(rec.shape[0]), win[:, g]]
            out[:, g, 4] = win[:, g]
    return out


def matrix_records(eng, g, params, sources, dests):  # noqa: F811
    plan = eng.MatrixPlan(g, params, sources, dests)
    plan.run()
    return plan.records()


def nearest_equals_reduced_matrix(eng, g, params, sources, dests, groups, n_groups, mrec=None):  # noqa: F811
    """A nearest plan of the lists against the reduced matrix of the same lists, all five words;
    empty groups read NONE and zeros and have no label.  Returns (plan, records)."""
    if mrec is None:
        mrec = matrix_records(eng, g, params, sources, dests)
    plan = eng.NearestPlan(g, params, sources, dests, groups, n_groups=n_groups)
    plan.run()
    rec = plan.records()
    want = reduce_matrix(mrec, [0] * len(dests) if groups is None else groups, n_groups, plan_order(params))
    assert rec.shape == want.shape
    bad = np.argwhere((rec != want).any(axis=2))
    assert bad.size == 0, (f"{len(bad)} of {want.shape[0] * n_groups} records wrong", params, sources[bad[0][0]],
                           "group %d" % bad[0][1], rec[tuple(bad[0])], want[tuple(bad[0])])
    for gi in range(n_groups):
        if groups is not None and gi not in groups:
            assert (rec[:, gi] == (0, 0, 0, 0, NONE)).all()
            assert plan.label(0, gi) is None
    return plan, rec


# ---- 1. parity against the oracle ---------------------------------------------------------
_parity = {}


def parity_case(oracle_lib, size, k, clustered, pi):
    """(map, sources, destinations, groups, the oracle's labels [source][destination] in
    as_expected's form), once per case."""
    key = (size, pi)
    if key not in _parity:
        m = SyntheticMap(size, campfires_per_homeland=k, seed=size + pi, clustered=clustered)
        rng = random.Random(size * 10 + pi)
        cells = m.all_indices()
        sources = [CellIndex.center(), m.campfires()[0], CellIndex.border(1, 1)] + rng.sample(cells, 36)
        sources.append(sources[5])
        dests = [rng.choice(cells) for _ in range(40)]
        groups = [j % 3 for j in range(40)]
        rng.shuffle(groups)
        og = oracle_lib.OracleGrid(m.cells())
        exp = og.find_path_batch(PARAMS[pi], [(s, d) for s in sources for d in dests], threads=0)
        n = len(dests)
        _parity[key] = (m, sources, dests, groups, [[as_expected(e) for e in exp[i * n:(i + 1) * n]]
                                                    for i in range(len(sources))])
    return _parity[key]


@pytest.mark.parametrize("size,k,clustered", [(9, 2, False), (21, 5, True), (33, 4, False)])
@pytest.mark.parametrize("pi", range(len(PARAMS)))
def test_winners_and_labels_match_oracle(eng, oracle_lib, mode, size, k, clustered, pi):  # noqa: F811
    m, sources, dests, groups, exp = parity_case(oracle_lib, size, k, clustered, pi)
    g = eng.MapGrid(m.cells())
    plan = eng.NearestPlan(g, PARAMS[pi], sources, dests, groups)
    assert plan.n_groups == 3
    plan.run()
    rec = plan.records()
    assert rec.shape == (len(sources), 3, 5)
    met = np.array([[e[:3] for e in row] for row in exp], dtype=np.int64)
    win = winners(met, groups, 3, plan_order(PARAMS[pi]))
    for i in range(len(sources)):
        for gi in range(3):
            j = win[i, gi]
            got = rec[i, gi]
            assert int(got[4]) == j and tuple(int(x) for x in got[:3]) == tuple(met[i, j]), (
                PARAMS[pi], sources[i], gi, got, j, met[i, j])
            if dests[j] == sources[i]:
                assert tuple(got) == (0, 0, 0, NONE, j)
            assert as_expected(plan.label(i, gi)) == exp[i][j], (PARAMS[pi], sources[i], dests[j])
    assert (rec[-1] == rec[5]).all()  # the repeated source


# ---- 2. equals the reduced matrix, every cell a destination ----------------------------------
@pytest.mark.parametrize("flags,gx", [("", None), ("2", None), ("", "1"), ("2", "1")])
@pytest.mark.parametrize("size,k,clustered,pi", [(129, 4, False, 0), (129, 9, True, 1), (161, 6, False, 2),
                                                  (129, 5, True, 3), (129, 8, False, 4), (161, 7, True, 5)])
def test_every_cell_in_seven_groups_equals_reduced_matrix(eng, monkeypatch, flags, gx, size, k, clustered, pi):  # noqa: F811
    """The maps and sources of test_gpu_matrix.py::test_every_cell_equals_all_destinations_records;
    group = row-major cell mod 7, so a group has 2 378 (129^2) or 3 703 (161^2) destinations in
    38 or 58 chunks.  MR_NEAREST_GX=1: the four waves of one workgroup share each source in turn
    and split its seven groups 1 / 2 / 2 / 2."""
    if flags:
        monkeypatch.setenv("MR_DBG_FLAGS", flags)
    if gx:
        monkeypatch.setenv("MR_NEAREST_GX", gx)
    params = FILL_PARAMS[pi]
    m = SyntheticMap(size, campfires_per_homeland=k, seed=size * 7 + pi, clustered=clustered)
    rng = random.Random(size + pi)
    cells = m.all_indices()
    sources = [m.campfires()[1], CellIndex.center()] + rng.sample(cells, 3)
    g = eng.MapGrid(m.cells())
    groups = [j % 7 for j in range(len(cells))]
    plan, rec = nearest_equals_reduced_matrix(eng, g, params, sources, cells, groups, 7)
    assert plan.stats()["solver"] == "hub" and plan.stats()["fill_launch"] == "serial"
    for i, s in enumerate(sources):  # the source's own cell wins its group
        j = cells.index(s)
        assert tuple(rec[i, j % 7]) == (0, 0, 0, NONE, j)


# ---- 3. chunk and group edges ---------------------------------------------------------------
_edges = {}


def edge_case(eng):  # noqa: F811
    """The 21^2 map, 300 sources (with repeats) and 130 destinations, once."""
    if not _edges:
        m = SyntheticMap(21, campfires_per_homeland=3, seed=21)
        cells = m.all_indices()
        rng = random.Random(300)
        sources = [rng.choice(cells) for _ in range(300)]
        dests = [CellIndex.center(), m.campfires()[0], sources[5]] + rng.sample(cells, 127)
        _edges["case"] = (m, eng.MapGrid(m.cells()), sources, dests)
    return _edges["case"]


def group_layouts(n_dst):
    """(name, groups or None, n_groups) for a list of n_dst destinations."""
    out = [("one", None, 1), ("singles", list(range(n_dst)), n_dst)]
    if n_dst >= 2:
        out.append(("singles reversed", list(range(n_dst - 1, -1, -1)), n_dst))
    for ng in (3, 4, 5):  # the pitch edge: 4, 4 and 8 records a row
        if n_dst >= ng:
            out.append((f"round robin {ng}", [j % ng for j in range(n_dst)], ng))
    if n_dst >= 5:
        # an empty group in the middle and an empty group last
        out.append(("empty 1 and 3", [0 if j % 3 else 2 for j in range(n_dst)], 4))
        out.append(("empty 0, 2 and 4", [1 if j % 2 else 3 for j in range(n_dst)], 5))
    if n_dst >= 130:
        # groups of 1, 64 and 65 destinations: one chunk, a full chunk, a chunk and one more;
        # interleaved in the caller's list, so the stable sort does the gathering
        sizes = {0: 1, 1: 64, 2: 65}
        groups = [2] * n_dst
        groups[0] = 0
        for j in range(64):
            groups[2 * j + 1] = 1
        assert all(groups.count(g) >= n for g, n in sizes.items()) and groups.count(0) == 1 and groups.count(1) == 64
        out.append(("sizes 1, 64, 65+", groups, 3))
        exact = [0] + [1] * 64 + [2] * 65
        out.append(("sizes 1, 64, 65 in order", exact + [2] * (n_dst - 130), 3))
    return out


@pytest.mark.parametrize("gx", [None, "1"])
@pytest.mark.parametrize("n_src", [1, 300])
@pytest.mark.parametrize("n_dst", [1, 63, 64, 65, 129, 130])
def test_chunk_and_group_edges(eng, monkeypatch, n_dst, n_src, gx):  # noqa: F811
    m, g, sources, dests = edge_case(eng)
    if gx:
        monkeypatch.setenv("MR_NEAREST_GX", gx)
    src, dst = sources[:n_src], dests[:n_dst]
    mrec = matrix_records(eng, g, Params(), src, dst)
    distinct = sorted(set(src), key=m.cell_of)
    for name, groups, ng in group_layouts(n_dst):
        plan, rec = nearest_equals_reduced_matrix(eng, g, Params(), src, dst, groups, ng, mrec)
        if name == "singles":  # n_dst groups of one: the matrix row
            assert (rec[:, :, :4] == mrec).all() and (rec[:, :, 4] == np.arange(n_dst)).all()
        pitch = plan.record_pitch()
        assert pitch == (ng + 3) // 4 * 4, name
        ptr, nbytes = plan.device_records()
        assert plan.num_sources == len(distinct) and nbytes == len(distinct) * pitch * 32, name
        rows = plan.source_rows()
        assert rows == [distinct.index(s) for s in src]  # plan sources: distinct, row-major cell order
        raw = _raw_words(_hip(), ptr, nbytes).reshape(len(distinct), pitch, 8)
        assert (raw[rows, :ng, :5] == rec).all(), name
        assert (raw[:, :, 5:] == 0).all() and (raw[:, ng:] == 0).all(), name  # reserved words, pad records


# ---- 4. ties go to the smallest position ------------------------------------------------------
TIE_SRC, TIE_A, TIE_B = geo_to_index(0, 2), geo_to_index(-1, 2), geo_to_index(1, 2)


def tie_lists(far):
    """On the 9^2 map with caravans and the Scroll off, the source (0, 2) lies on an axis; A =
    (-1, 2) and B = (1, 2) are mirror images about it, one step away.  `far`: the cells at least
    two legs away, the fillers (Legs first: strictly worse)."""
    src, A, B = TIE_SRC, TIE_A, TIE_B
    fill = (far * 2)[:100]

    def put(n, at):
        lst = fill[:n]
        for j, c in at.items():
            lst[j] = c
        return lst

    return src, A, B, [
        ("one chunk", put(40, {3: A, 10: B}), 3),
        ("one chunk, reversed", put(40, {3: A, 10: B})[::-1], 29),  # B first now
        ("64 apart", put(80, {5: A, 69: B}), 5),
        ("64 apart, reversed", put(80, {5: A, 69: B})[::-1], 10),
        ("listed twice, 70 apart", put(80, {3: A, 73: A}), 3),
        ("listed twice, reversed", put(80, {3: A, 73: A})[::-1], 6),
        ("second chunk only", put(80, {70: B, 75: A}), 70),
    ]


@pytest.mark.parametrize("algo", [None, "sssp"])
def test_ties_go_to_the_smallest_position(eng, monkeypatch, algo):  # noqa: F811
    if algo:
        monkeypatch.setenv("MR_ALGO", algo)
    m = SyntheticMap(9, campfires_per_homeland=2, seed=9)
    params = Params(use_soe=False, use_caravans=False)
    g = eng.MapGrid(m.cells())
    cells = m.all_indices()
    legs = matrix_records(eng, g, params, [TIE_SRC], cells)[0, :, 0]
    far = [c for c, k in zip(cells, legs) if k >= 2]
    assert len(far) >= 50 and TIE_A not in far and TIE_B not in far
    src, A, B, cases = tie_lists(far)
    for name, dests, want_j in cases:
        mrec = matrix_records(eng, g, params, [src], dests)
        tied = [j for j, d in enumerate(dests) if d in (A, B)]
        assert len(tied) == 2 and want_j == tied[0], name
        # the premise: the two are equal in all three metrics and better than every other
        assert (mrec[0, tied[0], :3] == mrec[0, tied[1], :3]).all() and tuple(mrec[0, tied[0], :3]) == (1, 0, 180), name
        others = np.delete(mrec[0], tied, axis=0)
        assert (others[:, 0] >= 2).all(), name
        plan, rec = nearest_equals_reduced_matrix(eng, g, params, [src], dests, None, 1, mrec)
        assert (plan.stats()["solver"] == "hub") == (algo is None), plan.stats()
        assert int(rec[0, 0, 4]) == want_j and plan.dests[want_j] == dests[want_j], name
        lab = plan.label(0, 0)
        assert (lab.legs, lab.money, lab.time_s) == (1, 0, 180) and lab.commands[-1].to == dests[want_j], name
        # the same with the fillers in a second group: the tie is its own group's business
        groups = [0 if j in tied else 1 for j in range(len(dests))]
        _, rec2 = nearest_equals_reduced_matrix(eng, g, params, [src], dests, groups, 2, mrec)
        assert int(rec2[0, 0, 4]) == want_j, name


# ---- 5. the source among its destinations -------------------------------------------------------
def test_source_among_destinations_wins(eng, mode):  # noqa: F811
    m = SyntheticMap(33, campfires_per_homeland=3, seed=33)
    cells = m.all_indices()
    rng = random.Random(33)
    sources = [CellIndex.center(), m.campfires()[2], CellIndex.border(2, 1)] + rng.sample(cells, 5)
    dests = rng.sample(cells, 90)
    at = [4, 70, 89, 0, 64, 63, 65, 17]
    for i, j in enumerate(at):
        dests[j] = sources[i]
    groups = [j % 2 for j in range(90)]
    g = eng.MapGrid(m.cells())
    plan, rec = nearest_equals_reduced_matrix(eng, g, Params(), sources, dests, groups, 2)
    for i, j in enumerate(at):
        assert tuple(rec[i, j % 2]) == (0, 0, 0, NONE, j), (sources[i], rec[i])
        lab = plan.label(i, j % 2)
        assert (lab.legs, lab.money, lab.time_s) == (0, 0, 0)


# ---- 6. specials as destinations ----------------------------------------------------------------
def test_specials_as_destinations(eng, oracle_lib, mode):  # noqa: F811
    """Groups of specials only: the Center, the border-1 cells, the campfires, the HQ.  The
    Center's record names its own table entry (via = 0x80000000 | t)."""
    m = SyntheticMap(21, campfires_per_homeland=3, seed=2121)
    cells = m.all_indices()
    rng = random.Random(6)
    hq = m.campfires()[4]
    params = Params(hq_position=hq, use_sfm=True)
    border1 = [CellIndex.border(b, 1) for b in range(4)]
    dests = [CellIndex.center()] + border1 + m.campfires() + [hq]
    groups = [0] + [1] * 4 + [2] * len(m.campfires()) + [3]
    order = list(range(len(dests)))
    rng.shuffle(order)
    dests, groups = [dests[j] for j in order], [groups[j] for j in order]
    sources = rng.sample([c for c in cells if c not in dests], 12)
    g = eng.MapGrid(m.cells())
    plan, rec = nearest_equals_reduced_matrix(eng, g, params, sources, dests, groups, 4)
    assert (rec[:, 0, 3] & 0x80000000).all() and (rec[:, :, 3] != NONE).all()
    og = oracle_lib.OracleGrid(m.cells())
    exp = og.find_path_batch(params, [(s, d) for s in sources for d in dests], threads=0)
    met = np.array([(e.legs, e.money, e.time_s) for e in exp], dtype=np.int64).reshape(len(sources), len(dests), 3)
    win = winners(met, groups, 4, plan_order(params))
    assert (rec[:, :, 4] == win).all() and (rec[:, :, :3] == met[np.arange(len(sources))[:, None], win]).all()
    for i in range(len(sources)):
        for gi in range(4):
            assert as_expected(plan.label(i, gi)) == as_expected(exp[i * len(dests) + win[i, gi]])


# ---- 7. a transposed layout against py_ref --------------------------------------------------------
def test_transposed_layout_against_py_ref(eng, mode):  # noqa: F811
    name, k, pi = "unequal9", 5, 1
    m = im.oriented(name, k)
    cells = m.all_indices()
    sources = im.transposed_sources(name)
    params = im.params_for(im.get_map(name))[pi]
    exp = im.py_ref_all(name, k, pi, sources)
    order = list(range(len(cells)))
    random.Random(95).shuffle(order)
    dests = [cells[j] for j in order] + [cells[order[0]]]
    groups = [j % 3 for j in range(len(dests))]
    met = np.array([[exp[i][j][:3] for j in order + [order[0]]] for i in range(len(sources))], dtype=np.int64)
    win = winners(met, groups, 3, plan_order(params))
    g = eng.MapGrid(m.cells())
    plan, rec = nearest_equals_reduced_matrix(eng, g, params, sources, dests, groups, 3)
    assert (rec[:, :, 4] == win).all() and (rec[:, :, :3] == met[np.arange(len(sources))[:, None], win]).all()
    for i, s in enumerate(sources):
        own = dests.index(s)
        assert tuple(rec[i, own % 3]) == (0, 0, 0, NONE, own)
        for gi in range(3):
            assert as_expected(plan.label(i, gi)) == exp[i][(order + [order[0]])[win[i, gi]]]


# ---- 8. reruns and streams -------------------------------------------------------------------------
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
        plan = eng.NearestPlan(g, Params(), [s, s, m.campfires()[1], CellIndex.center()], rng.sample(cells, 100),
                               [j % 6 for j in range(100)])
        assert plan.num_sources == 3 and plan.stats()["num_sources"] == 3
        plan.run()
        first = plan.records().copy()
        ptr, nbytes = plan.device_records()
        raw = _raw_words(hip, ptr, nbytes).copy()
        plan.run(stream.value)
        plan.wait()
        assert (plan.records() == first).all()
        plan.run()
        plan.run()
        assert (plan.records() == first).all()
        assert (_raw_words(hip, ptr, nbytes) == raw).all()
        assert (first[0] == first[1]).all() and (first[:, :, 4] != NONE).all()
        ms, launches = plan.kernel_ms()
        assert launches >= 1 and ms >= 0.0
    finally:
        hip.hipStreamSynchronize(stream)
        hip.hipStreamDestroy(stream)


# ---- 9. the wrong kind of plan ----------------------------------------------------------------------
def test_wrong_plan_kind(eng):  # noqa: F811
    L = eng.lib()
    m = SyntheticMap(9, campfires_per_homeland=2, seed=9)
    cells = m.all_indices()
    g = eng.MapGrid(m.cells())
    npl = eng.NearestPlan(g, Params(), cells[:3], cells[:10], [j % 2 for j in range(10)])
    mp = eng.MatrixPlan(g, Params(), cells[:3], cells[:10])
    sp = eng.SSSPPlan(g, Params(), cells[:3])
    qp = eng.Plan(g, Params(), [(cells[0], cells[1])])
    for p in (npl, mp, sp, qp):
        p.run()
    buf = np.empty((81, 8), dtype=np.uint32)
    res = (mr_result * 4)()
    n, ptr, nb = C.c_uint32(), C.c_void_p(), C.c_uint64()
    bad = MR_ERR_INVALID_ARG
    # the other kinds' accessors on a nearest plan
    assert L.mr_matrix_records(npl.handle, buf.ctypes.data, 162) == bad
    assert L.mr_matrix_device_records(npl.handle, C.byref(ptr), C.byref(nb)) == bad
    assert L.mr_matrix_record_pitch(npl.handle, C.byref(n)) == bad
    assert L.mr_matrix_source_rows(npl.handle, C.byref(n), 1) == bad
    assert L.mr_matrix_label(npl.handle, 0, 0, res, None, 0) == bad
    assert L.mr_sssp_records(npl.handle, 0, buf.ctypes.data) == bad
    assert L.mr_sssp_record_pitch(npl.handle, C.byref(n)) == bad
    assert L.mr_sssp_device_records(npl.handle, C.byref(ptr), C.byref(nb)) == bad
    assert L.mr_plan_fetch(npl.handle, res, None, 0) == bad
    assert L.mr_plan_device_outputs(npl.handle, C.byref(ptr), C.byref(nb), C.byref(ptr), C.byref(nb)) == bad
    # the nearest accessors on the other kinds
    for other in (mp, sp, qp):
        assert L.mr_nearest_records(other.handle, buf.ctypes.data, 81) == bad
        assert L.mr_nearest_device_records(other.handle, C.byref(ptr), C.byref(nb)) == bad
        assert L.mr_nearest_record_pitch(other.handle, C.byref(n)) == bad
        assert L.mr_nearest_source_rows(other.handle, C.byref(n), 1) == bad
        assert L.mr_nearest_label(other.handle, 0, 0, res, None, 0) == bad
    # indices
    assert L.mr_nearest_label(npl.handle, 3, 0, res, None, 0) == bad
    assert L.mr_nearest_label(npl.handle, 0, 2, res, None, 0) == bad
    with pytest.raises(eng.EngineError) as ei:
        eng.NearestPlan(g, Params(), cells[:3], cells[:4] + [CellIndex.homeland(0, 9, 9)])
    assert ei.value.status == MR_ERR_INVALID_INDEX and "destination 4" in str(ei.value)
    with pytest.raises(eng.EngineError) as ei:
        eng.NearestPlan(g, Params(), [cells[0], CellIndex.border(2, 7)], cells[:4])
    assert ei.value.status == MR_ERR_INVALID_INDEX and "source 1" in str(ei.value)
    with pytest.raises(eng.EngineError) as ei:
        eng.NearestPlan(g, Params(), cells[:3], cells[:4], [0, 1, 4, 1], n_groups=4)
    assert ei.value.status == MR_ERR_INVALID_ARG and "destination 2" in str(ei.value)
    assert npl.records().shape == (3, 2, 5) and mp.records().shape == (3, 10, 4)  # the plans still answer
    st = L.mr_nearest_label(npl.handle, 0, 0, res, None, 0)  # no room for commands: the count comes back
    assert st in (0, -4) and (st == 0) == (res[0].n_commands == 0)


def test_poi_groups(eng, oracle_lib):  # noqa: F811
    """FindPath.eval_nearest_poi: the nearest fountain and the nearest forum, a group a kind."""
    m = SyntheticMap(21, campfires_per_homeland=3, seed=77, fountains=5, forums=4)
    g = eng.MapGrid(m.cells())
    cells = m.all_indices()
    sources = random.Random(77).sample(cells, 20)
    fp = eng.FindPath(g)
    rec, dests = fp.eval_nearest_poi(sources)
    kinds = dict(m.cells())
    assert [kinds[d] for d in dests] == [2] * 5 + [3] * 4 and rec.shape == (20, 2, 5)
    og = oracle_lib.OracleGrid(m.cells())
    exp = og.find_path_batch(fp.params(), [(s, d) for s in sources for d in dests], threads=0)
    met = np.array([(e.legs, e.money, e.time_s) for e in exp], dtype=np.int64).reshape(20, 9, 3)
    win = winners(met, [0] * 5 + [1] * 4, 2, plan_order(fp.params()))
    assert (rec[:, :, 4] == win).all() and (rec[:, :, :3] == met[np.arange(20)[:, None], win]).all()
    # a kind the map lacks is an empty group, also with fewer cells than kinds, and with none
    bare = SyntheticMap(9, campfires_per_homeland=1, seed=3, fountains=1, forums=0)
    fb = eng.FindPath(eng.MapGrid(bare.cells()))
    rec, dests = fb.eval_nearest_poi([CellIndex.center(), bare.campfires()[0]])
    assert len(dests) == 1 and rec.shape == (2, 2, 5)
    assert (rec[:, 1] == (0, 0, 0, 0, NONE)).all() and (rec[:, 0, 4] == 0).all() and (rec[:, 0, 0] > 0).all()
    rec, dests = fb.eval_nearest_poi([CellIndex.center()], pois=(3, 2, 3))
    assert len(dests) == 1 and (rec[0, (0, 2)] == (0, 0, 0, 0, NONE)).all() and rec[0, 1, 4] == 0
    rec, dests = fb.eval_nearest_poi([CellIndex.center()], pois=(3,))
    assert dests == [] and tuple(rec[0, 0]) == (0, 0, 0, 0, NONE)


# ---- 10. large money ---------------------------------------------------------------------------------
def test_large_money_is_exact(eng, oracle_lib, mode):  # noqa: F811
    """test_gpu_matrix.py's case: scroll prices of 2^31 - 1000 under (Money, Legs), candidates
    with bit 31 set; the winners and their records exact against the oracle."""
    lc.oracle_answers(oracle_lib, "A1", "top")
    m, hq = lc.case_map("A1")
    params = lc.params_of(lc.cost_of("A1", "top"), (SORT_MONEY, SORT_LEGS), 0, hq)
    assert params.scroll_of_escape_cost == (1 << 31) - 1000
    sources, cells = lc.sources_of("A1")[:8], m.all_indices()
    groups = [j % 5 for j in range(len(cells))]
    og = oracle_lib.OracleGrid(m.cells())
    exp = og.find_path_batch(params, [(s, d) for s in sources for d in cells], threads=0)
    met = np.array([(e.legs, e.money, e.time_s) for e in exp], dtype=np.int64).reshape(len(sources), len(cells), 3)
    win = winners(met, groups, 5, plan_order(params))
    g = eng.MapGrid(m.cells())
    plan, rec = nearest_equals_reduced_matrix(eng, g, params, sources, cells, groups, 5)
    assert (rec[:, :, 4] == win).all() and (rec[:, :, :3] == met[np.arange(len(sources))[:, None], win]).all()
    # six destinations, each a group of its own: the records and labels of the pairs
    far = [5, 40, 80, 3, 17, 60]
    plan = eng.NearestPlan(g, params, sources, [cells[j] for j in far], list(range(6)))
    plan.run()
    rec = plan.records()
    assert (rec[:, :, :3] == met[:, far]).all()
    for i, gi in [(0, 5), (3, 2), (7, 0)]:
        assert as_expected(plan.label(i, gi)) == as_expected(exp[i * len(cells) + far[gi]])


def test_money_past_32_bits_is_a_limit_error(eng, mode):  # noqa: F811
    """(Legs, Money) at a price of 2^32 - 1: a scroll plus anything passes 32 bits, so the
    plan reports MR_ERR_LIMIT and never hands out a wrapped record."""
    m, _ = lc.case_map("A1")
    params = lc.b_params(lc.B_PRICES[1], (SORT_LEGS, SORT_MONEY))
    cells = m.all_indices()
    plan = eng.NearestPlan(eng.MapGrid(m.cells()), params, lc.sources_of("A1")[:8], cells, [j % 4 for j in range(len(cells))])
    plan.run()
    with pytest.raises(eng.EngineError) as ei:
        plan.records()
    assert ei.value.status == MR_ERR_LIMIT


# ---- 11. footprint ---------------------------------------------------------------------------------------
def test_footprint_below_matrix_plan(eng):  # noqa: F811
    """300 sources x 4 096 destinations in one group: the nearest plan holds 300 rows of 4
    records of 32 B where the matrix plan holds 300 rows of 4 096 records of 16 B, and nothing
    else of that size: its live device bytes (mr_cache_live: the blocks' size classes) are lower
    by at least the difference of the two."""
    L = eng.lib()
    m = SyntheticMap(129, campfires_per_homeland=4, seed=129)
    cells = m.all_indices()
    rng = random.Random(64)
    sources, dests = rng.sample(cells, 300), rng.sample(cells, 4096)
    g = eng.MapGrid(m.cells())
    warm = eng.MatrixPlan(g, Params(), sources[:2], dests[:2])  # the grid's own tables: live before both
    warm.run()
    warm.wait()

    def live_with(make):
        L.mr_cache_trim()
        before = C.c_uint64()
        L.mr_cache_live(None, C.byref(before))
        plan = make()
        plan.run()
        plan.wait()
        now = C.c_uint64()
        L.mr_cache_live(None, C.byref(now))
        sizes = (plan.num_sources, plan.record_pitch(), plan.device_records()[1])
        del plan
        return now.value - before.value, sizes

    nearest, (ns, npitch, nbytes) = live_with(lambda: eng.NearestPlan(g, Params(), sources, dests))
    matrix, (ms, mpitch, mbytes) = live_with(lambda: eng.MatrixPlan(g, Params(), sources, dests))
    assert ns == ms == 300 and npitch == 4 and mpitch == 4096
    assert nbytes == 300 * 4 * 32 and mbytes == 300 * 4096 * 16
    assert 0 < nearest <= matrix - (mbytes - nbytes), (nearest, matrix, mbytes - nbytes)
