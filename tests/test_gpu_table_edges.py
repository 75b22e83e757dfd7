"""All-destinations, matrix, nearest and k-nearest plans at the edges of the special table
(table_edge_maps.py): T = NS + 1 = 32 and 33 (hub_kernel's two sources a wave / one), 63, 64 with a
campfire in the last entry, 64 with the HQ in the last entry (the table fills the wave: lane 63
holds an entry and boundary rank 63 is used), and 65 (too wide for the narrow hub: every
all-destinations kind runs on the SSSP kernel, whose writers and the host's label rebuild then
walk a table of more than 64 entries).

The fill, matrix, nearest and k-nearest kernels each keep their own copy of the table load and the
boundary ranking, so each kind is checked on its own: every cell's record and label of an SSSPPlan
against the C++ oracle bit for bit; MatrixPlan.records() over every cell against those records in
all four words; NearestPlan and NearestPlan(k) against the host reduction of the matrix records;
the nearest plans' labels against the oracle's.  test_table_edge_maps.py pins on the CPU that the
sources and parameter sets used here start labels from table entries all over the table, the last
one included, and that every source meets cells a tie between two boundaries decides.

Layouts: the standard one and one mirrored layout (both flips).  Transposed layouts are left out:
their specification is py_ref, which takes seconds a source at this table size.
"""
import dataclasses
import random

import numpy as np
import pytest

import irregular_maps as im
import table_edge_maps as tm
from golden_util import as_expected
from marshrutka_amd.abi import BLUE, RED, CellIndex
from marshrutka_amd.mapgen import random_queries
from test_gpu_irregular_maps import KERNEL_ENV
from test_gpu_knearest import knearest_equals_topk
from test_gpu_nearest import group_layouts, nearest_equals_reduced_matrix
from test_gpu_oriented_all_destinations import SOURCE_RECORD
from test_gpu_sssp import FILL_PARAMS, PARAMS, eng, mode  # noqa: F401  (eng, mode: fixtures)

pytestmark = pytest.mark.gpu

SWITCHES = KERNEL_ENV + ("MR_DBG_FLAGS", "MR_FILL_GX", "MR_MATRIX_GX", "MR_NEAREST_GX", "MR_FILL_OVERLAP", "MR_FILL_FUSED",
                         "MR_FILL_SLOTS", "MR_HUB_BLOCKS", "MR_CERT", "MR_CERT_SLOTS")
HUB = ("hub", "hub_wide")


@pytest.fixture(autouse=True)
def _clear(monkeypatch):
    """No kernel switch set but the test's own (autouse: before `mode` sets its two)."""
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)


def test_parameter_sets_are_fill_params():
    """table_edge_maps restates FILL_PARAMS without its HQ (the map supplies one)."""
    assert [dataclasses.replace(p, hq_position=None) for p in FILL_PARAMS] == tm.FILL_PARAMS


def check_stats(plan, ns, want_hub):
    st = plan.stats()
    assert st["num_specials"] == ns, st
    assert (st["solver"] in HUB) == want_hub and st["solver"] != "hub_wide", st
    return st


def four_kinds(eng, g, cells, params, sources, met, label_of, ns, want_hub, ks, rank_sample, label_at=None):  # noqa: F811
    """The four plan kinds on grid g from `sources` to every cell of `cells` against the
    reference: met[i] the (V, 3) metrics from source i, label_of(i, j) its label of cell number j
    in as_expected's form.

    SSSPPlan: every cell's metrics, the source's own record, the labels at the cell numbers
      label_at (None: every cell);
    MatrixPlan over every cell: the all-destinations records in all four words;
    NearestPlan, groups = cell number mod 7: the host reduction of the matrix records, and every
      winner's label;
    NearestPlan(k) for k in ks: the host top-k of the matrix records, rank 0 the nearest plan's
      record, and the labels of ranks rank_sample (those below k).
    Every plan reports ns specials and a hub solver exactly if want_hub.  Returns the matrix
    records."""
    plan = eng.SSSPPlan(g, params, sources)
    plan.run()
    check_stats(plan, ns, want_hub)
    recs = [plan.records(i) for i in range(len(sources))]
    at = range(len(cells)) if label_at is None else label_at
    for i, s in enumerate(sources):
        bad = np.nonzero((recs[i][:, :3].astype(np.int64) != met[i]).any(axis=1))[0]
        assert bad.size == 0, (f"{bad.size} of {len(cells)} records' metrics wrong", params, s, cells[bad[0]],
                               recs[i][bad[0]], met[i][bad[0]])
        assert tuple(recs[i][cells.index(s)]) == SOURCE_RECORD, (params, s)
        wrong = [cells[j] for j in at if as_expected(plan.label(i, cells[j])) != label_of(i, j)]
        assert not wrong, (f"{len(wrong)} of {len(at)} labels wrong", params, s, wrong[:4])
    mx = eng.MatrixPlan(g, params, sources, cells)
    mx.run()
    check_stats(mx, ns, want_hub)
    mrec = mx.records()
    for i, s in enumerate(sources):
        bad = np.nonzero((mrec[i] != recs[i]).any(axis=1))[0]
        assert bad.size == 0, (f"{bad.size} of {len(cells)} matrix records are not the all-destinations plan's", params, s,
                               cells[bad[0]], mrec[i, bad[0]], recs[i][bad[0]])
    groups = tm.groups_mod7(len(cells))
    near, nrec = nearest_equals_reduced_matrix(eng, g, params, sources, cells, groups, 7, mrec)
    check_stats(near, ns, want_hub)
    # (a source's own cell need not win its group: a free scroll reaches its campfire with the
    # same (0, 0, 0), and the smaller position wins)
    for i, s in enumerate(sources):
        for gi in range(7):
            j = int(nrec[i, gi, 4])
            assert as_expected(near.label(i, gi)) == label_of(i, j), (params, s, "group %d" % gi, cells[j])
    for k in ks:
        kn, krec = knearest_equals_topk(eng, g, params, sources, cells, groups, 7, k, mrec)
        check_stats(kn, ns, want_hub)
        assert (krec[:, :, 0] == nrec).all(), (params, k)
        for i, s in enumerate(sources):
            for gi in range(7):
                for r in [r for r in rank_sample if r < k]:
                    j = int(krec[i, gi, r, 4])
                    assert as_expected(kn.label(i, gi, r)) == label_of(i, j), (params, s, "k = %d" % k,
                                                                               "group %d rank %d" % (gi, r), cells[j])
    return mrec


def four_kinds_listed(eng, g, cells, params, sources, exp, ns, want_hub, ks, rank_sample):  # noqa: F811
    """four_kinds against whole lists of labels exp[source][cell]."""
    return four_kinds(eng, g, cells, params, sources, [tm.as_metrics(e) for e in exp], lambda i, j: exp[i][j], ns, want_hub,
                      ks, rank_sample)


# ---- a. the 21 x 21 maps, every table size, all three modes ----------------------------------
@pytest.mark.parametrize("pi", range(len(tm.EDGE_PARAMS)))
@pytest.mark.parametrize("hq", [False, True], ids=["nohq", "hq"])
@pytest.mark.parametrize("name", tm.SMALL)
def test_four_kinds_on_21(eng, oracle_lib, mode, name, hq, pi):  # noqa: F811
    """T = 32 / 33 (t32), 63 / 64 with the HQ last (t63), 64 with a campfire last / 65 (t64) and
    the same with 55 regions (t64_blue), under FILL_PARAMS' six orders and the two sets
    table_edge_maps adds; k = 5 and k = 64 (441 cells in 7 groups of 63: k = 64 leaves rank 63
    empty).  Without a switch a table of up to 64 entries runs on the hub solver and one of 65
    on the SSSP kernel."""
    m = tm.get_map(name)
    ns = tm.NUM_SPECIALS[name][hq]
    want_hub = mode != "sssp" and ns <= 63
    exp = tm.oracle_labels(oracle_lib, name, hq, pi)
    g = eng.MapGrid(m.cells())
    four_kinds_listed(eng, g, m.all_indices(), tm.params_for(name, hq, pi), tm.sources_for(name, hq), exp, ns, want_hub,
                      ks=(5, 64), rank_sample=(0, 1, 2, 3, 4, 31, 62))


# ---- b. the 129 x 129 map: fill tiles and packed keys with a full table ------------------------
_129 = {}


def case_129(oracle_lib, hq, pi, n_src):
    """(cells, cell array, sources, metrics [source] (V, 3), labels [source] {cell number: label},
    the cell numbers the labels are kept at, the oracle grid), once per case.  The oracle's search
    run to completion (sssp_all) gives every cell's label; full labels are kept on both axes
    through the Center, on the last column and at 300 sampled cells."""
    key = (hq, pi, n_src)
    if key not in _129:
        name, S, H = "t64_129", 129, 64
        m = tm.get_map(name)
        cells = m.all_indices()
        arr = m.cells_array()
        fires = m.campfires()
        rng = random.Random(129 + pi)
        sources = ([CellIndex.center(), fires[-1]] + [tm.sources_for(name, hq)[2]] + rng.sample(cells, 2))[:n_src]
        at = sorted(set(range(H * S, H * S + S)) | set(range(H, S * S, S)) | set(range(S - 1, S * S, S)) |
                    set(random.Random(pi).sample(range(S * S), 300)))
        og = oracle_lib.OracleGrid.from_array(arr)
        params = tm.params_for(name, hq, pi)
        met, labels = [], []
        for s in sources:
            full = og.sssp_all(params, s)
            met.append(np.array([(e.legs, e.money, e.time_s) for e in full], dtype=np.int64))
            labels.append({j: as_expected(full[j]) for j in at})
        _129[key] = (cells, arr, sources, met, labels, at, og)
    return _129[key]


def four_kinds_129(eng, oracle_lib, hq, pi, n_src, want_hub, ks):  # noqa: F811
    name = "t64_129"
    cells, arr, sources, met, labels, at, og = case_129(oracle_lib, hq, pi, n_src)
    params = tm.params_for(name, hq, pi)

    def label_of(i, j):  # a nearest plan's winner outside the kept labels: one oracle query, kept
        if j not in labels[i]:
            labels[i][j] = as_expected(og.find_path_batch(params, [(sources[i], cells[j])], threads=0)[0])
        return labels[i][j]

    four_kinds(eng, eng.MapGrid.from_array(arr), cells, params, sources, met, label_of, tm.NUM_SPECIALS[name][hq], want_hub,
               ks, rank_sample=(0, max(ks) - 1), label_at=at)


@pytest.mark.parametrize("flags,gx", [("", None), ("2", None), ("", "1")])
@pytest.mark.parametrize("pi", [0, 3, 6])
def test_four_kinds_on_129_hub(eng, oracle_lib, monkeypatch, flags, gx, pi):  # noqa: F811
    """T = 64 on a map wide enough for 64 x 16 fill tiles and the packed keys: five sources, the
    packed and (MR_DBG_FLAGS=2) the full compare, and one workgroup for the fill, the matrix and
    the nearest kernels (each wave walks many tiles, chunks and groups of every source)."""
    if flags:
        monkeypatch.setenv("MR_DBG_FLAGS", flags)
    if gx:
        for v in ("MR_FILL_GX", "MR_MATRIX_GX", "MR_NEAREST_GX"):
            monkeypatch.setenv(v, gx)
    four_kinds_129(eng, oracle_lib, False, pi, 5, True, ks=(5,))


def test_four_kinds_on_129_sssp_kernel(eng, oracle_lib):  # noqa: F811
    """T = 65 (the HQ on a plain cell): two sources, every kind on the SSSP kernel."""
    four_kinds_129(eng, oracle_lib, True, 0, 2, False, ks=(5,))


# ---- c. a mirrored layout ------------------------------------------------------------------------
@pytest.mark.parametrize("pi", [0, 5, 6])
def test_mirrored_layout(eng, oracle_lib, mode, pi):  # noqa: F811
    """t64 without the HQ flipped both ways (layout 3): the boundaries' order comes from the
    layout's rank table.  All four kinds against the oracle on the same cells, and nearest plans
    under test_gpu_nearest.py's group layouts (one group, 441 groups of one, empty groups)."""
    name, k = "t64", 3
    m = im.Oriented(tm.get_map(name), k)
    cells = m.all_indices()
    params = tm.params_for(name, False, pi)
    sources = tm.sources_for(name, False)
    exp = tm.oracle_labels(oracle_lib, name, False, pi, k)
    g = eng.MapGrid(m.cells())
    mrec = four_kinds_listed(eng, g, cells, params, sources, exp, 63, mode != "sssp", ks=(5,), rank_sample=(0, 4))
    for lname, groups, ng in group_layouts(len(cells)):
        nearest_equals_reduced_matrix(eng, g, params, sources, cells, groups, ng, mrec)
        if ng <= 5:
            knearest_equals_topk(eng, g, params, sources, cells, groups, ng, 5, mrec)


# ---- d. the two-sources-a-wave edge through a query plan ------------------------------------------
@pytest.mark.parametrize("spw_env", [None, "1"], ids=["hub2", "hub1"])
@pytest.mark.parametrize("hq", [False, True], ids=["nohq", "hq"])
def test_query_plan_on_hub_kernel_at_32_and_33(eng, oracle_lib, monkeypatch, hq, spw_env):  # noqa: F811
    """t32: 300 random queries and one plain source with 40 destinations on hub_kernel (no lane
    or group kernel, as test_gpu_parity.py's hub1 / hub2).  T = 32 runs two sources a wave and
    T = 33 one (MR_HUB_SPW=1: one either way), eight or four sources a workgroup, with the same
    labels: the oracle's."""
    monkeypatch.setenv("MR_HUB_LANE", "0")
    monkeypatch.setenv("MR_HUB_GROUP", "0")
    if spw_env:
        monkeypatch.setenv("MR_HUB_SPW", spw_env)
    name = "t32"
    m = tm.get_map(name)
    cells = m.all_indices()
    ns = tm.NUM_SPECIALS[name][hq]
    plain = tm.sources_for(name, hq)[3]
    qs = random_queries(m, 300, 32) + [(plain, d) for d in random.Random(33).choices(cells, k=40)]
    g = eng.MapGrid(m.cells())
    og = oracle_lib.OracleGrid(m.cells())
    spw = 2 if ns + 1 <= 32 and not spw_env else 1
    for p in PARAMS:
        params = dataclasses.replace(p, hq_position=tm.hq_cell(name) if hq else None)
        plan = eng.Plan(g, params, qs)
        plan.run()
        st = check_stats(plan, ns, True)
        assert st["lane_sources"] == 0 and st["lanes_per_source"] == 0, st
        assert st["hub_workgroups"] == (st["num_sources"] + 4 * spw - 1) // (4 * spw), (spw, st)
        exp = og.find_path_batch(params, qs, threads=0)
        bad = [(q, as_expected(e), as_expected(r)) for q, e, r in zip(qs, exp, plan.fetch())
               if as_expected(e) != as_expected(r)]
        assert not bad, (f"{len(bad)} of {len(qs)} labels wrong", params, bad[0])


# ---- e. many regions with a full table -------------------------------------------------------------
@pytest.mark.parametrize("homeland,nreg", [(BLUE, 55), (RED, 1)])
def test_many_regions_with_a_full_table(eng, oracle_lib, homeland, nreg):  # noqa: F811
    """t64_blue without the HQ, NS = 63: 55 Scroll-of-Escape regions under homeland Blue and one
    under Red.  hub_kernel's LDS tables grow with T x regions (64 x 55 region rows of 8 B are
    28 KB of hub_lds_bytes(63, 55, 1) = 42 560 B, far below the 160 KB bound, and no table the
    narrow hub takes has more than 58 regions), so plan creation must succeed for a query plan
    and the four all-destinations kinds, on the hub solver, with the oracle's labels."""
    name = "t64_blue"
    m = tm.get_map(name)
    cells = m.all_indices()
    sources = tm.sources_for(name, False)
    g = eng.MapGrid(m.cells())
    og = oracle_lib.OracleGrid(m.cells())
    qs = random_queries(m, 300, 64) + [(sources[3], d) for d in random.Random(65).choices(cells, k=40)]
    for pi in (0, 6):
        params = dataclasses.replace(tm.EDGE_PARAMS[pi], homeland=homeland)
        plan = eng.Plan(g, params, qs)
        plan.run()
        st = check_stats(plan, 63, True)
        assert st["num_regions"] == nreg, st
        exp = og.find_path_batch(params, qs, threads=0)
        bad = [(q, as_expected(e), as_expected(r)) for q, e, r in zip(qs, exp, plan.fetch())
               if as_expected(e) != as_expected(r)]
        assert not bad, (f"{len(bad)} of {len(qs)} labels wrong", params, bad[0])
        n = len(cells)
        all_exp = og.find_path_batch(params, [(s, d) for s in sources for d in cells], threads=0)
        labels = [[as_expected(e) for e in all_exp[i * n:(i + 1) * n]] for i in range(len(sources))]
        four_kinds_listed(eng, g, cells, params, sources, labels, 63, True, ks=(5,), rank_sample=(0, 4))
        assert eng.SSSPPlan(g, params, sources).stats()["num_regions"] == nreg
