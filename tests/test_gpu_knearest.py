"""k-nearest plans (mr_nearest_plan_create_ex): per source and destination group, the records of
the k best listed destinations in order.

The rule (DESIGN.md section 3b'''): rank r of group g from source i is the r-th least position j
of the caller's list with group_of_dst[j] == g under (m[q0], m[q1], m[q2], j), m the metrics of
FindPath::eval(sources[i], dests[j]) and (q0, q1, q2) the plan's metric order; a rank at or past
the group's size is the empty record.  The host reference is the first k of np.lexsort over
(j, m[q2], m[q1], m[q0]) per group (test_gpu_nearest.py's `winners`, extended), applied to
MatrixPlan.records() of the same lists or to the oracle's (or py_ref's) labels.  Hub path
(knearest_kernel), sources handed to the SSSP kernel (write_knearest), and the SSSP kernel alone
(the `mode` fixture)."""
import ctypes as C
import random

import numpy as np
import pytest

import irregular_maps as im
import large_costs as lc
from golden_util import as_expected
from marshrutka_amd.abi import MR_ERR_INVALID_ARG, MR_ERR_LIMIT, SORT_LEGS, SORT_MONEY, CellIndex, Params, mr_result
from marshrutka_amd.mapgen import SyntheticMap
from test_gpu_nearest import (TIE_A, TIE_B, TIE_SRC, edge_case, group_layouts, matrix_records, parity_case, plan_order,
                              tie_lists)
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


def topk(metrics, groups, n_groups, order, k):
    """metrics: (n_src, n_dst, >= 3) integers.  The positions of ranks 0..k-1 per (source, group),
    (n_src, n_groups, k), -1 for a rank at or past the group's size: the first k of the group's
    positions sorted by (metrics in `order`, position)."""
    groups = np.asarray(groups)
    out = np.full((metrics.shape[0], n_groups, k), -1, dtype=np.int64)
    for g in range(n_groups):
        J = np.nonzero(groups == g)[0]
        if J.size:
            m = metrics[:, J].astype(np.int64)
            keys = (np.broadcast_to(J, m.shape[:2]), m[:, :, order[2]], m[:, :, order[1]], m[:, :, order[0]])
            first = np.lexsort(keys, axis=-1)[:, :k]
            out[:, g, :first.shape[1]] = J[first]
    return out


def topk_records(rec, groups, n_groups, order, k):
    """The (n_src, n_groups, k, 5) records a k plan must give, from MatrixPlan.records()."""
    win = topk(rec, groups, n_groups, order, k)
    out = np.zeros((rec.shape[0], n_groups, k, 5), dtype=np.uint32)
    out[..., 4] = NONE
    rows = np.arange(rec.shape[0])
    for g in range(n_groups):
        for r in range(k):
            if win[0, g, r] >= 0:  # (a rank is empty for every source or for none)
                out[:, g, r, :4] = rec[rows, win[:, g, r]]
                out[:, g, r, 4] = win[:, g, r]
    return out


def knearest_equals_topk(eng, g, params, sources, dests, groups, n_groups, k, mrec=None):  # noqa: F811
    """A k plan of the lists against the host top-k of the matrix records of the same lists, all
    five words.  Returns (plan, records)."""
    if mrec is None:
        mrec = matrix_records(eng, g, params, sources, dests)
    plan = eng.NearestPlan(g, params, sources, dests, groups, n_groups=n_groups, k=k)
    assert plan.k == k
    plan.run()
    rec = plan.records()
    want = topk_records(mrec, [0] * len(dests) if groups is None else groups, n_groups, plan_order(params), k)
    assert rec.shape == want.shape == (len(sources), n_groups, k, 5)
    bad = np.argwhere((rec != want).any(axis=3))
    assert bad.size == 0, (f"{len(bad)} of {want.shape[0] * n_groups * k} records wrong", params, "k = %d" % k,
                           sources[bad[0][0]], "group %d rank %d" % (bad[0][1], bad[0][2]), rec[tuple(bad[0])],
                           want[tuple(bad[0])])
    return plan, rec


# ---- 1. parity against the oracle ---------------------------------------------------------
@pytest.mark.parametrize("k", [3, 16])
@pytest.mark.parametrize("size,cf,clustered", [(9, 2, False), (21, 5, True), (33, 4, False)])
@pytest.mark.parametrize("pi", range(len(PARAMS)))
def test_ranks_and_labels_match_oracle(eng, oracle_lib, mode, size, cf, clustered, pi, k):  # noqa: F811
    """40 destinations in 3 groups of 13 or 14: k = 3 fills every rank, k = 16 leaves the ranks
    past the group's size empty."""
    m, sources, dests, groups, exp = parity_case(oracle_lib, size, cf, clustered, pi)
    g = eng.MapGrid(m.cells())
    plan = eng.NearestPlan(g, PARAMS[pi], sources, dests, groups, k=k)
    assert plan.n_groups == 3 and plan.k == k
    plan.run()
    rec = plan.records()
    assert rec.shape == (len(sources), 3, k, 5)
    met = np.array([[e[:3] for e in row] for row in exp], dtype=np.int64)
    win = topk(met, groups, 3, plan_order(PARAMS[pi]), k)
    for gi in range(3):
        size_g = groups.count(gi)
        assert size_g in (13, 14) and (win[:, gi, :min(k, size_g)] >= 0).all() and (win[:, gi, size_g:] < 0).all()
    for i in range(len(sources)):
        for gi in range(3):
            for r in range(k):
                j = win[i, gi, r]
                got = rec[i, gi, r]
                if j < 0:
                    assert tuple(got) == (0, 0, 0, 0, NONE), (PARAMS[pi], sources[i], gi, r, got)
                    assert plan.label(i, gi, r) is None
                    continue
                assert int(got[4]) == j and tuple(int(x) for x in got[:3]) == tuple(met[i, j]), (
                    PARAMS[pi], sources[i], gi, r, got, j, met[i, j])
                if dests[j] == sources[i]:
                    assert tuple(got) == (0, 0, 0, NONE, j)
                assert as_expected(plan.label(i, gi, r)) == exp[i][j], (PARAMS[pi], sources[i], dests[j], r)
    assert (rec[-1] == rec[5]).all()  # the repeated source


# ---- 2. equals the top 5 of the matrix, every cell a destination ----------------------------
@pytest.mark.parametrize("flags,gx", [("", None), ("2", None), ("", "1"), ("2", "1")])
@pytest.mark.parametrize("size,cf,clustered,pi", [(129, 4, False, 0), (129, 9, True, 1), (161, 6, False, 2),
                                                   (129, 5, True, 3), (129, 8, False, 4), (161, 7, True, 5)])
def test_every_cell_in_seven_groups_equals_top5_of_matrix(eng, monkeypatch, flags, gx, size, cf, clustered, pi):  # noqa: F811
    """The maps and sources of test_gpu_nearest.py's test of this name; group = row-major cell
    mod 7, so a group has 38 or 58 chunks.  MR_DBG_FLAGS=2: the full compare.  MR_NEAREST_GX=1:
    the four waves of one workgroup share each source in turn and split its seven groups."""
    if flags:
        monkeypatch.setenv("MR_DBG_FLAGS", flags)
    if gx:
        monkeypatch.setenv("MR_NEAREST_GX", gx)
    params = FILL_PARAMS[pi]
    m = SyntheticMap(size, campfires_per_homeland=cf, seed=size * 7 + pi, clustered=clustered)
    rng = random.Random(size + pi)
    cells = m.all_indices()
    sources = [m.campfires()[1], CellIndex.center()] + rng.sample(cells, 3)
    g = eng.MapGrid(m.cells())
    groups = [j % 7 for j in range(len(cells))]
    plan, rec = knearest_equals_topk(eng, g, params, sources, cells, groups, 7, 5)
    assert plan.stats()["solver"] == "hub" and plan.stats()["fill_launch"] == "serial"
    for i, s in enumerate(sources):  # the source's own cell is rank 0 of its group
        j = cells.index(s)
        assert tuple(rec[i, j % 7, 0]) == (0, 0, 0, NONE, j)


# ---- 3. chunk, group and k edges ---------------------------------------------------------------
@pytest.mark.parametrize("gx", [None, "1"])
@pytest.mark.parametrize("k", [1, 2, 3, 63, 64])
@pytest.mark.parametrize("n_src", [1, 300])
@pytest.mark.parametrize("n_dst", [1, 63, 64, 65, 129, 130])
def test_chunk_group_and_k_edges(eng, monkeypatch, n_dst, n_src, k, gx):  # noqa: F811
    m, g, sources, dests = edge_case(eng)
    if gx:
        monkeypatch.setenv("MR_NEAREST_GX", gx)
    src, dst = sources[:n_src], dests[:n_dst]
    mrec = matrix_records(eng, g, Params(), src, dst)
    distinct = sorted(set(src), key=m.cell_of)
    for name, groups, ng in group_layouts(n_dst):
        plan, rec = knearest_equals_topk(eng, g, Params(), src, dst, groups, ng, k, mrec)
        pitch = plan.record_pitch()
        assert pitch == (ng * k + 3) // 4 * 4, name
        ptr, nbytes = plan.device_records()
        assert plan.num_sources == len(distinct) and nbytes == len(distinct) * pitch * 32, name
        rows = plan.source_rows()
        assert rows == [distinct.index(s) for s in src]  # plan sources: distinct, row-major cell order
        raw = _raw_words(_hip(), ptr, nbytes).reshape(len(distinct), pitch, 8)
        assert (raw[rows, :ng * k, :5] == rec.reshape(n_src, ng * k, 5)).all(), name
        assert (raw[:, :, 5:] == 0).all() and (raw[:, ng * k:] == 0).all(), name  # reserved words, pad records
        if k == 1:  # today's plan to the byte
            old = eng.NearestPlan(g, Params(), src, dst, groups, n_groups=ng)
            old.run()
            assert old.k == 1 and (old.records() == rec[:, :, 0]).all(), name
            optr, onbytes = old.device_records()
            assert onbytes == nbytes and (_raw_words(_hip(), optr, onbytes).reshape(raw.shape) == raw).all(), name


# ---- 4. the order of arrival --------------------------------------------------------------------
@pytest.mark.parametrize("n_dst", [130, 1000])
def test_order_of_arrival(eng, mode, n_dst):  # noqa: F811
    """One source, one group, k = 8.  The list sorted by that source's key ascending (the first
    chunk fills the list, nothing after it beats the threshold), descending (every chunk inserts
    k) and shuffled: the same eight cells in the same order.  The nine least keys of the list are
    distinct in their metrics, so no tie is settled by position among the eight or at their edge."""
    k = 8
    m = SyntheticMap(33, campfires_per_homeland=4, seed=33)
    cells = m.all_indices()
    rng = random.Random(n_dst)
    src = rng.choice(cells)
    params = Params()
    order = plan_order(params)
    g = eng.MapGrid(m.cells())
    all_rec = matrix_records(eng, g, params, [src], cells)[0]

    def key(j):
        return tuple(int(all_rec[j, q]) for q in order)

    by_key = sorted(range(len(cells)), key=lambda j: (key(j), j))
    least, seen = [], set()
    for j in by_key:  # the nine least distinct keys, a cell each
        if key(j) not in seen:
            seen.add(key(j))
            least.append(j)
        if len(least) == k + 1:
            break
    rest = [j for j in by_key if key(j) > key(least[-1])]
    assert len(least) == k + 1 and len(rest) >= 100
    picked = least + [rng.choice(rest) for _ in range(n_dst - len(least))]  # (cells may repeat past the ninth)
    asc = sorted(picked, key=lambda j: (key(j), j))
    shuffled = list(picked)
    rng.shuffle(shuffled)
    got = {}
    for name, lst in (("ascending", asc), ("descending", asc[::-1]), ("shuffled", shuffled)):
        dests = [cells[j] for j in lst]
        plan, rec = knearest_equals_topk(eng, g, params, [src], dests, None, 1, k)
        got[name] = [(dests[int(r[4])], tuple(int(x) for x in r[:4])) for r in rec[0, 0]]
        assert [c for c, _ in got[name]] == [cells[j] for j in least[:k]], name
    assert got["ascending"] == got["descending"] == got["shuffled"]


# ---- 5. ties go to the smaller position -----------------------------------------------------------
@pytest.mark.parametrize("algo", [None, "sssp"])
def test_ties_take_ranks_in_listing_order(eng, monkeypatch, algo):  # noqa: F811
    if algo:
        monkeypatch.setenv("MR_ALGO", algo)
    m = SyntheticMap(9, campfires_per_homeland=2, seed=9)
    params = Params(use_soe=False, use_caravans=False)
    g = eng.MapGrid(m.cells())
    cells = m.all_indices()
    legs = matrix_records(eng, g, params, [TIE_SRC], cells)[0, :, 0]
    far = [c for c, n in zip(cells, legs) if n >= 2]
    assert len(far) >= 50 and TIE_A not in far and TIE_B not in far
    src, A, B, cases = tie_lists(far)
    by_name = {name: dests for name, dests, _ in cases}

    def with_cells(name, at):
        lst = list(by_name[name])
        for j, c in at.items():
            lst[j] = c
        return lst

    # (name, list, k, the positions of ranks 0..k-1)
    checks = []
    for name, dests, want_j in cases:  # the mirror pair, or one cell listed twice: both, the earlier first
        tied = [j for j, d in enumerate(dests) if d in (A, B)]
        assert len(tied) == 2 and tied[0] == want_j
        checks.append((name, dests, 2, tied))
    # a cell listed three times gives its first two positions (one chunk; 70 apart)
    checks.append(("thrice, one chunk", with_cells("one chunk", {3: A, 10: A, 30: A}), 2, [3, 10]))
    checks.append(("thrice, two chunks", with_cells("listed twice, 70 apart", {3: A, 40: A, 73: A}), 2, [3, 40]))
    checks.append(("thrice, across", with_cells("listed twice, 70 apart", {3: A, 73: A, 75: A}), 2, [3, 73]))
    # a later destination whose metrics equal the current k-th does not displace it
    checks.append(("equal to the k-th, same chunk", with_cells("one chunk", {3: A, 10: B, 30: B}), 2, [3, 10]))
    checks.append(("equal to the k-th, next chunk", with_cells("64 apart", {5: A, 69: B, 75: A}), 2, [5, 69]))
    checks.append(("equal to the k-th, k = 3", with_cells("64 apart", {5: A, 6: B, 69: B, 75: A}), 3, [5, 6, 69]))
    for name, dests, k, want in checks:
        mrec = matrix_records(eng, g, params, [src], dests)
        tied = [j for j, d in enumerate(dests) if d in (A, B)]
        # the premise: the tied are equal in all three metrics and better than every other
        assert all(tuple(mrec[0, j, :3]) == (1, 0, 180) for j in tied), name
        assert (np.delete(mrec[0], tied, axis=0)[:, 0] >= 2).all(), name
        plan, rec = knearest_equals_topk(eng, g, params, [src], dests, None, 1, k, mrec)
        assert (plan.stats()["solver"] == "hub") == (algo is None), plan.stats()
        assert [int(x) for x in rec[0, 0, :, 4]] == want, name
        for r, j in enumerate(want):
            lab = plan.label(0, 0, r)
            assert (lab.legs, lab.money, lab.time_s) == (1, 0, 180) and lab.commands[-1].to == dests[j], (name, r)
        # the same with the fillers in a second group: the tie is its own group's business
        groups = [0 if j in tied else 1 for j in range(len(dests))]
        _, rec2 = knearest_equals_topk(eng, g, params, [src], dests, groups, 2, k, mrec)
        assert [int(x) for x in rec2[0, 0, :, 4]] == (tied + [NONE] * k)[:k], name


# ---- 6. the source among its destinations ---------------------------------------------------------
def test_source_among_destinations_takes_rank_0(eng, mode):  # noqa: F811
    m = SyntheticMap(33, campfires_per_homeland=3, seed=33)
    cells = m.all_indices()
    rng = random.Random(33)
    sources = [CellIndex.center(), m.campfires()[2], CellIndex.border(2, 1)] + rng.sample(cells, 5)
    dests = rng.sample([c for c in cells if c not in sources], 90)
    at = [4, 70, 89, 0, 64, 63, 65, 17]
    for i, j in enumerate(at):
        dests[j] = sources[i]
    twice = {0: 44, 1: 2, 4: 88}  # source i listed again, in the same group (same parity)
    for i, j in twice.items():
        assert j % 2 == at[i] % 2 and j not in at
        dests[j] = sources[i]
    groups = [j % 2 for j in range(90)]
    g = eng.MapGrid(m.cells())
    plan, rec = knearest_equals_topk(eng, g, Params(), sources, dests, groups, 2, 3)
    for i, j in enumerate(at):
        both = sorted([j, twice[i]]) if i in twice else [j]
        for r, jj in enumerate(both):
            assert tuple(rec[i, j % 2, r]) == (0, 0, 0, NONE, jj), (sources[i], rec[i, j % 2])
            lab = plan.label(i, j % 2, r)
            assert (lab.legs, lab.money, lab.time_s) == (0, 0, 0)
        nxt = rec[i, j % 2, len(both)]  # the next rank is another cell's label
        assert nxt[3] != NONE and dests[int(nxt[4])] != sources[i]


# ---- 7. specials as destinations ------------------------------------------------------------------
def test_specials_as_destinations(eng, oracle_lib, mode):  # noqa: F811
    """Groups of specials only: the Center, the border-1 cells, the campfires, the HQ; k = 3
    passes the size of the first and the last."""
    k = 3
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
    plan, rec = knearest_equals_topk(eng, g, params, sources, dests, groups, 4, k)
    assert (rec[:, 0, 0, 3] & 0x80000000).all() and (rec[:, :, 0, 3] != NONE).all()
    og = oracle_lib.OracleGrid(m.cells())
    exp = og.find_path_batch(params, [(s, d) for s in sources for d in dests], threads=0)
    met = np.array([(e.legs, e.money, e.time_s) for e in exp], dtype=np.int64).reshape(len(sources), len(dests), 3)
    win = topk(met, groups, 4, plan_order(params), k)
    assert (rec[..., 4] == np.where(win < 0, NONE, win)).all()
    assert (win[:, 0, 1:] < 0).all() and (win[:, 3, 1:] < 0).all() and (win[:, 1:3] >= 0).all()
    for i in range(len(sources)):
        for gi in range(4):
            for r in range(k):
                if win[i, gi, r] < 0:
                    assert plan.label(i, gi, r) is None
                    continue
                e = exp[i * len(dests) + win[i, gi, r]]
                assert tuple(int(x) for x in rec[i, gi, r, :3]) == (e.legs, e.money, e.time_s)
                assert as_expected(plan.label(i, gi, r)) == as_expected(e)


# ---- 8. a transposed layout against py_ref ----------------------------------------------------------
def test_transposed_layout_against_py_ref(eng, mode):  # noqa: F811
    name, cf, pi, k = "unequal9", 5, 1, 4
    m = im.oriented(name, cf)
    cells = m.all_indices()
    sources = im.transposed_sources(name)
    params = im.params_for(im.get_map(name))[pi]
    exp = im.py_ref_all(name, cf, pi, sources)
    order = list(range(len(cells)))
    random.Random(95).shuffle(order)
    listed = order + [order[0]]
    dests = [cells[j] for j in listed]
    groups = [j % 3 for j in range(len(dests))]
    met = np.array([[exp[i][j][:3] for j in listed] for i in range(len(sources))], dtype=np.int64)
    win = topk(met, groups, 3, plan_order(params), k)
    g = eng.MapGrid(m.cells())
    plan, rec = knearest_equals_topk(eng, g, params, sources, dests, groups, 3, k)
    assert (win >= 0).all() and (rec[..., 4] == win).all()
    assert (rec[..., :3] == met[np.arange(len(sources))[:, None, None], win]).all()
    for i, s in enumerate(sources):
        own = dests.index(s)
        assert tuple(rec[i, own % 3, 0]) == (0, 0, 0, NONE, own)
        for gi in range(3):
            for r in range(k):
                assert as_expected(plan.label(i, gi, r)) == exp[i][listed[win[i, gi, r]]]


# ---- 9. reruns and streams ------------------------------------------------------------------------------
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
                               [j % 6 for j in range(100)], k=4)
        assert plan.num_sources == 3 and plan.stats()["num_sources"] == 3
        plan.run()
        first = plan.records().copy()
        ptr, nbytes = plan.device_records()
        raw = _raw_words(hip, ptr, nbytes).copy()
        for _ in range(3):
            plan.run()
            assert (plan.records() == first).all()
        plan.run(stream.value)
        plan.wait()
        assert (plan.records() == first).all()
        assert (_raw_words(hip, ptr, nbytes) == raw).all()
        assert first.shape == (4, 6, 4, 5) and (first[0] == first[1]).all() and (first[..., 4] != NONE).all()
        ms, launches = plan.kernel_ms()
        assert launches >= 1 and ms >= 0.0
    finally:
        hip.hipStreamSynchronize(stream)
        hip.hipStreamDestroy(stream)


# ---- 10. the wrong kind of plan ----------------------------------------------------------------------------
def test_wrong_plan_kind(eng):  # noqa: F811
    L = eng.lib()
    m = SyntheticMap(9, campfires_per_homeland=2, seed=9)
    cells = m.all_indices()
    g = eng.MapGrid(m.cells())
    kpl = eng.NearestPlan(g, Params(), cells[:3], cells[:10], [j % 2 for j in range(10)], k=3)
    npl = eng.NearestPlan(g, Params(), cells[:3], cells[:10], [j % 2 for j in range(10)])
    mp = eng.MatrixPlan(g, Params(), cells[:3], cells[:10])
    sp = eng.SSSPPlan(g, Params(), cells[:3])
    qp = eng.Plan(g, Params(), [(cells[0], cells[1])])
    for p in (kpl, npl, mp, sp, qp):
        p.run()
    buf = np.empty((81, 8), dtype=np.uint32)
    res = (mr_result * 4)()
    n, ptr, nb = C.c_uint32(), C.c_void_p(), C.c_uint64()
    bad = MR_ERR_INVALID_ARG
    # the other kinds' accessors on a k plan
    assert L.mr_matrix_records(kpl.handle, buf.ctypes.data, 162) == bad
    assert L.mr_matrix_device_records(kpl.handle, C.byref(ptr), C.byref(nb)) == bad
    assert L.mr_matrix_record_pitch(kpl.handle, C.byref(n)) == bad
    assert L.mr_matrix_source_rows(kpl.handle, C.byref(n), 1) == bad
    assert L.mr_matrix_label(kpl.handle, 0, 0, res, None, 0) == bad
    assert L.mr_sssp_records(kpl.handle, 0, buf.ctypes.data) == bad
    assert L.mr_sssp_record_pitch(kpl.handle, C.byref(n)) == bad
    assert L.mr_sssp_device_records(kpl.handle, C.byref(ptr), C.byref(nb)) == bad
    assert L.mr_plan_fetch(kpl.handle, res, None, 0) == bad
    assert L.mr_plan_device_outputs(kpl.handle, C.byref(ptr), C.byref(nb), C.byref(ptr), C.byref(nb)) == bad
    # the new accessors on the other kinds
    for other in (mp, sp, qp):
        assert L.mr_nearest_k(other.handle, C.byref(n)) == bad
        assert L.mr_nearest_label_ex(other.handle, 0, 0, 0, res, None, 0) == bad
    # a nearest plan is a k plan with k = 1
    assert L.mr_nearest_k(npl.handle, C.byref(n)) == 0 and n.value == 1 and npl.k == 1
    assert L.mr_nearest_k(npl.handle, None) == bad
    assert L.mr_nearest_label_ex(npl.handle, 0, 0, 1, res, None, 0) == bad
    assert as_expected(npl.label(0, 1)) == as_expected(kpl.label(0, 1, 0))
    # indices, ranks and capacity
    assert L.mr_nearest_k(kpl.handle, C.byref(n)) == 0 and n.value == 3
    assert L.mr_nearest_label_ex(kpl.handle, 3, 0, 0, res, None, 0) == bad
    assert L.mr_nearest_label_ex(kpl.handle, 0, 2, 0, res, None, 0) == bad
    assert L.mr_nearest_label_ex(kpl.handle, 0, 0, 3, res, None, 0) == bad
    assert L.mr_nearest_records(kpl.handle, buf.ctypes.data, 17) == -4  # MR_ERR_CAPACITY below 3 x 2 x 3
    assert L.mr_nearest_records(kpl.handle, buf.ctypes.data, 18) == 0
    assert kpl.records().shape == (3, 2, 3, 5) and npl.records().shape == (3, 2, 5)
    assert (kpl.records()[:, :, 0] == npl.records()).all()
    st = L.mr_nearest_label_ex(kpl.handle, 0, 0, 2, res, None, 0)  # no room for commands: the count comes back
    assert st in (0, -4) and (st == 0) == (res[0].n_commands == 0)


# ---- 11. the 32-bit money limit ---------------------------------------------------------------------------
def test_money_past_32_bits_is_a_limit_error(eng, mode):  # noqa: F811
    """(Legs, Money) at a price of 2^32 - 1: a scroll plus anything passes 32 bits, so the plan
    reports MR_ERR_LIMIT and never hands out a wrapped record."""
    m, _ = lc.case_map("A1")
    params = lc.b_params(lc.B_PRICES[1], (SORT_LEGS, SORT_MONEY))
    cells = m.all_indices()
    plan = eng.NearestPlan(eng.MapGrid(m.cells()), params, lc.sources_of("A1")[:8], cells,
                           [j % 4 for j in range(len(cells))], k=2)
    plan.run()
    with pytest.raises(eng.EngineError) as ei:
        plan.records()
    assert ei.value.status == MR_ERR_LIMIT


# ---- 12. points of interest ---------------------------------------------------------------------------------
def test_poi_groups_top_2(eng, oracle_lib):  # noqa: F811
    """FindPath.eval_nearest_poi(k=2): the two nearest fountains and the two nearest forums."""
    m = SyntheticMap(21, campfires_per_homeland=3, seed=77, fountains=5, forums=4)
    g = eng.MapGrid(m.cells())
    cells = m.all_indices()
    sources = random.Random(77).sample(cells, 20)
    fp = eng.FindPath(g)
    rec, dests = fp.eval_nearest_poi(sources, k=2)
    kinds = dict(m.cells())
    assert [kinds[d] for d in dests] == [2] * 5 + [3] * 4 and rec.shape == (20, 2, 2, 5)
    og = oracle_lib.OracleGrid(m.cells())
    exp = og.find_path_batch(fp.params(), [(s, d) for s in sources for d in dests], threads=0)
    met = np.array([(e.legs, e.money, e.time_s) for e in exp], dtype=np.int64).reshape(20, 9, 3)
    win = topk(met, [0] * 5 + [1] * 4, 2, plan_order(fp.params()), 2)
    assert (win >= 0).all() and (rec[..., 4] == win).all()
    assert (rec[..., :3] == met[np.arange(20)[:, None, None], win]).all()
    rec1 = fp.eval_nearest(sources, dests, [0] * 5 + [1] * 4, k=2)
    assert (rec1 == rec).all()
    # a kind with one cell has an empty rank 1; a kind the map lacks is an empty group
    bare = SyntheticMap(9, campfires_per_homeland=1, seed=3, fountains=1, forums=0)
    fb = eng.FindPath(eng.MapGrid(bare.cells()))
    rec, dests = fb.eval_nearest_poi([CellIndex.center(), bare.campfires()[0]], k=2)
    assert len(dests) == 1 and rec.shape == (2, 2, 2, 5)
    assert (rec[:, 1] == (0, 0, 0, 0, NONE)).all() and (rec[:, 0, 1] == (0, 0, 0, 0, NONE)).all()
    assert (rec[:, 0, 0, 4] == 0).all() and (rec[:, 0, 0, 0] > 0).all()
