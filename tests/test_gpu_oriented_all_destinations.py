"""All-destinations plans (SSSPPlan) and cost matrix plans (MatrixPlan) on irregular maps and
on all eight layouts (irregular_maps.py).

The rest of the suite builds both plan kinds on SyntheticMap maps in the standard layout, bar
test_gpu_irregular_maps.py::test_all_destinations (SSSPPlan, four irregular maps, standard
layout).  Off the standard layout the hub kernel's boundary order (out_lex), the SSSP kernel's
cell names, the host's expansion of a record into commands and the matrix plan's destination
table all go through the grid's rank table instead of the closed form, and the matrix kernel
had never met a campfire on a border cell or on the Center, a region of specials only, a
31-entry table or a table whose shape changes with params.homeland.

The bar is the parity suite's: bit-exact legs, money, time and every command.  The reference is
the C++ oracle on layouts 0..3 and py_ref on the transposed layouts 4..7 (DESIGN.md section 1,
"Grid orientation").  A record's `via` word is checked through the label rebuilt from it, and
directly at a source's own cell, which must read (0, 0, 0, 0xFFFFFFFF).  test_irregular_maps.py
pins on the CPU that the transposed tests tell py_ref from the oracle and that the sources
used here reach cells whose label a tie between two boundaries decides.

Sources are irregular_maps.sssp_sources (the Center, a border campfire or border-1 cell, a
homeland campfire, a plain cell); a matrix plan gets the last of them twice.

py_ref is the slow side of the transposed tests.  Measured where these tests were written,
every cell from one source under parameter sets 0 / 1: 0.14 / 0.19 s on unequal9 (81 cells),
1.0 / 1.4 s on unequal and 1.3 / 2.3 s on wide15 (225 cells).  One (map, layout, parameter
set) stays under about 5 s with all four sources on unequal9 (0.6 / 0.8 s), three on unequal
(2.8 / 4.2 s) and two on wide15 (2.6 / 4.2 s): irregular_maps.TRANSPOSED_SOURCES, the Center
and the plain cell first.  The labels are computed once and shared by the three plan modes.
"""
import random

import numpy as np
import pytest

import irregular_maps as im
from golden_util import as_expected
from marshrutka_amd.abi import CellIndex, Params
from marshrutka_amd.mapgen import SyntheticMap
from test_gpu_irregular_maps import KERNEL_ENV, N_PY_REF_65
from test_gpu_sssp import FILL_PARAMS, all_labels_match, eng, mode  # noqa: F401  (eng, mode: fixtures)

pytestmark = pytest.mark.gpu

SWITCHES = KERNEL_ENV + ("MR_DBG_FLAGS", "MR_FILL_GX", "MR_MATRIX_GX", "MR_FILL_OVERLAP", "MR_FILL_FUSED",
                         "MR_FILL_SLOTS")
SOURCE_RECORD = (0, 0, 0, 0xFFFFFFFF)


@pytest.fixture(autouse=True)
def _clear(monkeypatch):
    """No kernel switch set but the test's own (autouse: before `mode` sets its two)."""
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)


_oracle = {}


def oracle_all(oracle_lib, key, m, params, sources):
    """The oracle's labels of every cell of m from each source, [source][cell] in
    as_expected's form, once per key."""
    if key not in _oracle:
        og = oracle_lib.OracleGrid(m.cells())
        cells = m.all_indices()
        exp = og.find_path_batch(params, [(s, d) for s in sources for d in cells], threads=0)
        n = len(cells)
        _oracle[key] = [[as_expected(e) for e in exp[i * n:(i + 1) * n]] for i in range(len(sources))]
    return _oracle[key]


def metrics(labels):
    return np.array([e[:3] for e in labels], dtype=np.int64)


def sssp_matches(eng, g, cells, params, sources, exp, label_at=None):  # noqa: F811
    """An SSSPPlan on g: every cell's three metrics equal exp[source][cell], the source's own
    cell reads SOURCE_RECORD, and the label rebuilt from the record equals the reference's at
    every cell (at the cell numbers label_at, if given).  Returns (plan, records by source)."""
    plan = eng.SSSPPlan(g, params, sources)
    plan.run()
    recs = [plan.records(i) for i in range(len(sources))]
    for i, s in enumerate(sources):
        want = metrics(exp[i])
        bad = np.nonzero((recs[i][:, :3].astype(np.int64) != want).any(axis=1))[0]
        assert bad.size == 0, (f"{bad.size} of {len(cells)} records' metrics wrong", s, cells[bad[0]], recs[i][bad[0]],
                               want[bad[0]], params)
        assert tuple(recs[i][cells.index(s)]) == SOURCE_RECORD, (params, s)
        at = range(len(cells)) if label_at is None else label_at
        wrong = [cells[j] for j in at if as_expected(plan.label(i, cells[j])) != exp[i][j]]
        assert not wrong, (f"{len(wrong)} of {len(at)} labels wrong", s, wrong[:4], params)
    return plan, recs


def matrix_matches(eng, g, cells, params, sources, dests, exp, recs, n_labels, seed):  # noqa: F811
    """A MatrixPlan of sources x dests on g: the three metrics equal exp[source][cell], all four
    words equal the all-destinations records recs[source][cell], a source listed as a
    destination reads SOURCE_RECORD, and n_labels sampled label(i, j) (None: all) equal the
    reference's.  sources[-1] repeats sources[-2]: its row must too."""
    plan = eng.MatrixPlan(g, params, sources, dests)
    plan.run()
    rec = plan.records()
    assert rec.shape == (len(sources), len(dests), 4)
    pos = {c: j for j, c in enumerate(cells)}
    dj = np.array([pos[d] for d in dests])
    for i, s in enumerate(sources):
        want = metrics(exp[i])[dj]
        bad = np.nonzero((rec[i, :, :3].astype(np.int64) != want).any(axis=1))[0]
        assert bad.size == 0, (f"{bad.size} of {len(dests)} matrix records' metrics wrong", s, dests[bad[0]],
                               rec[i, bad[0]], want[bad[0]], params)
        bad = np.nonzero((rec[i] != recs[i][dj]).any(axis=1))[0]
        assert bad.size == 0, (f"{bad.size} of {len(dests)} matrix records are not the all-destinations plan's", s,
                               dests[bad[0]], rec[i, bad[0]], recs[i][dj[bad[0]]], params)
        own = [j for j, d in enumerate(dests) if d == s]
        assert own and all(tuple(rec[i, j]) == SOURCE_RECORD for j in own), (params, s)
    assert sources[-1] == sources[-2] and (rec[-1] == rec[-2]).all()
    pairs = [(i, j) for i in range(len(sources)) for j in range(len(dests))]
    if n_labels is not None:
        pairs = random.Random(seed).sample(pairs, n_labels)
    wrong = [(sources[i], dests[j]) for i, j in pairs if as_expected(plan.label(i, j)) != exp[i][dj[j]]]
    assert not wrong, (f"{len(wrong)} of {len(pairs)} matrix labels wrong", wrong[:4], params)
    return rec


# ---- 1. matrix plans on the catalogue, standard layout -------------------------------------
MATRIX_MAPS = ["unequal", "border1", "border_far", "center_fire", "corners", "ties", "s3", "s5_full"]


@pytest.mark.parametrize("name", MATRIX_MAPS)
def test_matrix_on_the_catalogue(eng, oracle_lib, mode, name):  # noqa: F811
    """Every cell and three repeats (a campfire, a source, a plain or border cell) from the
    four sources and a repeated one: campfires on border cells and on the Center, regions of
    specials only (s3), table shapes that change with the homeland (unequal, ties, s5_full)."""
    m = im.get_map(name)
    cells = m.all_indices()
    src4 = im.sssp_sources(m)
    sources = im.matrix_sources(m)
    dests = cells + [m.campfires()[-1], src4[3], cells[1]]
    g = eng.MapGrid(m.cells())
    prm = im.params_for(m)
    for pi in range(6 if m.size <= 5 else 3):
        exp = oracle_all(oracle_lib, (name, 0, pi), m, prm[pi], src4)
        ref = eng.SSSPPlan(g, prm[pi], src4)
        ref.run()
        recs = [ref.records(i) for i in range(4)]
        matrix_matches(eng, g, cells, prm[pi], sources, dests, exp + [exp[3]], recs + [recs[3]],
                       None if m.size <= 5 else 200, pi)


# ---- 2. mirrored layouts against the oracle ------------------------------------------------
@pytest.mark.parametrize("k", im.MIRRORED)
@pytest.mark.parametrize("name", im.ORIENTED)
def test_mirrored_layouts(eng, oracle_lib, mode, name, k):  # noqa: F811
    """k = 1, 2, 3: every cell's label and record against the oracle on the same cells, a
    matrix plan over all cells, and the metrics of the standard layout's plan at the cell with
    the same CellIndex (a mirror image changes no label)."""
    base, m = im.get_map(name), im.oriented(name, k)
    cells = m.all_indices()
    src4 = im.sssp_sources(base)
    g, g0 = eng.MapGrid(m.cells()), eng.MapGrid(base.cells())
    pos0 = {c: j for j, c in enumerate(base.all_indices())}
    same = np.array([pos0[c] for c in cells])
    for pi in (0, 1, 2, 4):
        params = im.params_for(base)[pi]
        all_labels_match(eng, oracle_lib, m, params, src4)
        exp = oracle_all(oracle_lib, (name, k, pi), m, params, src4)
        plan = eng.SSSPPlan(g, params, src4)
        plan.run()
        recs = [plan.records(i) for i in range(4)]
        own = eng.SSSPPlan(g0, params, src4)
        own.run()
        for i, s in enumerate(src4):
            assert tuple(recs[i][cells.index(s)]) == SOURCE_RECORD, (pi, s)
            assert (recs[i][:, :3] == own.records(i)[same, :3]).all(), (pi, s)
        matrix_matches(eng, g, cells, params, src4 + [src4[3]], cells, exp + [exp[3]], recs + [recs[3]], 100, pi)


# ---- 3. transposed layouts against py_ref --------------------------------------------------
@pytest.mark.parametrize("k", im.TRANSPOSED)
@pytest.mark.parametrize("name", im.ORIENTED)
def test_transposed_layouts(eng, mode, name, k):  # noqa: F811
    """k = 4..7: every cell's label and record, and a matrix plan over all cells, against
    py_ref from irregular_maps.transposed_sources(name) (the module docstring has the cost)."""
    m = im.oriented(name, k)
    cells = m.all_indices()
    sources = im.transposed_sources(name)
    assert len(sources) >= 2 and sources[0] == CellIndex.center()
    g = eng.MapGrid(m.cells())
    for pi in (0, 1, 2, 4) if name == "unequal9" else (0, 1):
        params = im.params_for(im.get_map(name))[pi]
        exp = im.py_ref_all(name, k, pi, sources)
        _, recs = sssp_matches(eng, g, cells, params, sources, exp)
        matrix_matches(eng, g, cells, params, sources + [sources[-1]], cells, exp + [exp[-1]], recs + [recs[-1]],
                       100, pi)


# ---- 4. fill tiles and matrix chunks off the standard layout -------------------------------
# 129 x 129: wide enough for 64 x 16 fill tiles away from the axes through the Center, with the
# key packing switched off (MR_DBG_FLAGS=2) and a fill grid of three workgroup columns
# (MR_FILL_GX=3), as test_gpu_sssp.py::test_fill_tiles_every_cell has them on the standard layout.
FILL_SWITCHES = [("", None), ("2", None), ("", "3")]
FILL_SEEDS = {3: 3129, 6: 6129}
_fill = {}


def fill_case(k, pi):
    """(map in layout k, its cells, a grid-ready cell array, sources), once per case."""
    if (k, pi) not in _fill:
        m = im.Oriented(SyntheticMap(129, campfires_per_homeland=k, seed=FILL_SEEDS[k] + pi), k)
        cells = m.all_indices()
        sources = [m.campfires()[1], CellIndex.center(), random.Random(FILL_SEEDS[k] + pi).choice(cells)]
        _fill[(k, pi)] = (m, cells, m.cells_array(), sources)
    return _fill[(k, pi)]


def _fill_switches(monkeypatch, flags, gx):
    if flags:
        monkeypatch.setenv("MR_DBG_FLAGS", flags)
    if gx:
        monkeypatch.setenv("MR_FILL_GX", gx)


def _matrix_equals_fill(eng, monkeypatch, g, params, sources, cells, recs):  # noqa: F811
    """A matrix plan over all cells gives the all-destinations records in all four words, on
    its default grid and on one workgroup (each wave walks 65 chunks of every source)."""
    for gx in (None, "1"):
        if gx:
            monkeypatch.setenv("MR_MATRIX_GX", gx)
        plan = eng.MatrixPlan(g, params, sources, cells)
        plan.run()
        assert plan.stats()["solver"] == "hub"
        rec = plan.records()
        for i, s in enumerate(sources):
            bad = np.nonzero((rec[i] != recs[i]).any(axis=1))[0]
            assert bad.size == 0, (gx, params, s, len(bad), cells[bad[0]], rec[i, bad[0]], recs[i][bad[0]])
    monkeypatch.delenv("MR_MATRIX_GX")
    return rec


@pytest.mark.parametrize("flags,gx", FILL_SWITCHES)
@pytest.mark.parametrize("pi", [0, 2])
def test_fill_and_matrix_mirrored_129(eng, oracle_lib, monkeypatch, flags, gx, pi):  # noqa: F811
    """Layout 3 (flipped both ways) against the oracle's search run to completion: every
    cell's metrics; full labels on both axes through the Center, on the last column and at
    300 sampled cells; the matrix plan equal to the fill word for word."""
    k, S, H = 3, 129, 64
    _fill_switches(monkeypatch, flags, gx)
    params = FILL_PARAMS[pi]
    m, cells, arr, sources = fill_case(k, pi)
    if ("exp", k, pi) not in _fill:
        og = oracle_lib.OracleGrid.from_array(arr)
        _fill[("exp", k, pi)] = [[as_expected(e) for e in og.sssp_all(params, s)] for s in sources]
    exp = _fill[("exp", k, pi)]
    at = sorted(set(range(H * S, H * S + S)) | set(range(H, S * S, S)) | set(range(S - 1, S * S, S)) |
                set(random.Random(pi).sample(range(S * S), 300)))
    g = eng.MapGrid.from_array(arr)
    plan, recs = sssp_matches(eng, g, cells, params, sources, exp, label_at=at)
    assert plan.stats()["solver"] == "hub"
    _matrix_equals_fill(eng, monkeypatch, g, params, sources, cells, recs)


@pytest.mark.parametrize("flags,gx", FILL_SWITCHES)
@pytest.mark.parametrize("pi", [0, 2])
def test_fill_and_matrix_transposed_129(eng, monkeypatch, flags, gx, pi):  # noqa: F811
    """Layout 6 (transposed, y flipped).  py_ref is too slow to be the reference at this size
    (50 ms a label at S = 65), so this is a cross-check between independent solvers, not a
    comparison with the specification: the hub solve with the fill kernel, the matrix kernel
    and the SSSP kernel alone (MR_ALGO=sssp) must give every cell the same three metrics, and
    the matrix plan the fill's records word for word.  test_transposed_65_against_py_ref
    anchors a transposed map of this kind to py_ref."""
    k = 6
    _fill_switches(monkeypatch, flags, gx)
    params = FILL_PARAMS[pi]
    m, cells, arr, sources = fill_case(k, pi)
    g = eng.MapGrid.from_array(arr)
    plan = eng.SSSPPlan(g, params, sources)
    plan.run()
    assert plan.stats()["solver"] == "hub"
    recs = [plan.records(i) for i in range(len(sources))]
    _matrix_equals_fill(eng, monkeypatch, g, params, sources, cells, recs)
    monkeypatch.setenv("MR_ALGO", "sssp")
    alone = eng.SSSPPlan(g, params, sources)
    monkeypatch.delenv("MR_ALGO")
    alone.run()
    assert alone.stats()["solver"] in ("bucketed", "levels"), alone.stats()
    for i, s in enumerate(sources):
        other = alone.records(i)
        bad = np.nonzero((recs[i][:, :3] != other[:, :3]).any(axis=1))[0]
        assert bad.size == 0, (params, s, len(bad), cells[bad[0]], recs[i][bad[0]], other[bad[0]])
        assert tuple(recs[i][cells.index(s)]) == SOURCE_RECORD and tuple(other[cells.index(s)]) == SOURCE_RECORD


def test_transposed_65_against_py_ref(eng):  # noqa: F811
    """The anchor to the specification: test_c2_map_oriented's 65 x 65 map in layout 5,
    N_PY_REF_65 sampled cells of one source as full labels against py_ref, from an
    all-destinations plan and from a matrix plan that lists exactly those cells."""
    m = im.Oriented(SyntheticMap(65, campfires_per_homeland=4, seed=2024), 5)
    cells = m.all_indices()
    params = Params()
    rng = random.Random(65)
    s = rng.choice([c for c in cells if c not in im.specials(m)])
    at = sorted(rng.sample(range(len(cells)), N_PY_REF_65 - 1) + [cells.index(s)])
    dests = [cells[j] for j in at]
    exp = im.py_ref_some(m.base, 5, params, [(s, d) for d in dests])
    g = eng.MapGrid.from_array(m.cells_array())
    plan = eng.SSSPPlan(g, params, [s])
    plan.run()
    assert plan.stats()["solver"] == "hub"
    rec = plan.records(0)[at]
    assert (rec[:, :3].astype(np.int64) == metrics(exp)).all()
    assert [as_expected(plan.label(0, d)) for d in dests] == exp
    mx = eng.MatrixPlan(g, params, [s], dests)
    mx.run()
    assert (mx.records()[0] == rec).all()
    assert tuple(rec[dests.index(s)]) == SOURCE_RECORD
    assert [as_expected(mx.label(0, j)) for j in range(len(dests))] == exp


# ---- 5. the rank table on the standard layout ----------------------------------------------
@pytest.mark.parametrize("pi,algo", [(0, None), (4, None), (4, "sssp")])
def test_rank_table_on_the_standard_layout(eng, monkeypatch, pi, algo):  # noqa: F811
    """MR_RANK_TABLE=1 at grid creation makes the kernels look every rank up, as they do on the
    seven other layouts, where the closed form would do: the records of both plan kinds are
    byte-equal to those of a grid made without the switch.  FILL_PARAMS[0] and FILL_PARAMS[4]
    run the hub solve and the fill (Fleetfoot 7 is past the skill's table, so the run time
    stays linear); MR_ALGO=sssp puts FILL_PARAMS[4] on the SSSP kernel alone."""
    if algo:
        monkeypatch.setenv("MR_ALGO", algo)
    params = FILL_PARAMS[pi]
    m = SyntheticMap(129, campfires_per_homeland=4, seed=129 + pi)
    arr = m.cells_array()
    cells = m.all_indices()
    rng = random.Random(129 + pi)
    sources = [m.campfires()[1], CellIndex.center()] + rng.sample(cells, 2)
    dests = rng.sample(cells, 1000) + m.campfires() + sources
    out = []
    for table in (False, True):
        if table:
            monkeypatch.setenv("MR_RANK_TABLE", "1")
        g = eng.MapGrid.from_array(arr)
        monkeypatch.delenv("MR_RANK_TABLE", raising=False)
        plan = eng.SSSPPlan(g, params, sources)
        plan.run()
        assert (plan.stats()["solver"] == "hub") == (algo is None), plan.stats()
        mx = eng.MatrixPlan(g, params, sources, dests)
        mx.run()
        out.append(([plan.records(i) for i in range(len(sources))], mx.records()))
    (std_recs, std_mx), (tab_recs, tab_mx) = out
    for i in range(len(sources)):
        assert std_recs[i].tobytes() == tab_recs[i].tobytes(), (pi, sources[i])
    assert std_mx.tobytes() == tab_mx.tobytes()
