"""The premises of test_gpu_irregular_maps.py, on the CPU: the two restatements of the
reference (the C++ oracle, py_ref) agree on every irregular map and on the mirrored
orientations, so either is a sound reference there; on the transposed orientations the
reference's projection shortcut (restated by the oracle) departs from its own
nearest_campfire function (py_ref's direct argmin), which is why py_ref alone specifies
those ("Grid orientation"); and the shape facts the GPU tests' kernel-choice assertions
rest on."""
import pytest

import irregular_maps as im
from golden_util import as_expected
from marshrutka_amd.abi import BLUE, CELL_HOMELAND, POI_CAMPFIRE
from marshrutka_amd.mapgen import random_queries

PARAMS3 = (0, 1, 2)  # Blue, Red and Green parameter sets


def _oracle_labels(oracle_lib, name, k, pi, qs):
    og = oracle_lib.OracleGrid(im.oriented(name, k).cells())
    return [as_expected(e) for e in og.find_path_batch(im.params_for(im.get_map(name))[pi], qs, threads=0)]


def _differences(oracle_lib, name, k):
    qs = im.capped_queries(name)
    return sum(a != b for pi in PARAMS3
               for a, b in zip(_oracle_labels(oracle_lib, name, k, pi, qs), im.py_ref_labels(name, k, pi)))


@pytest.mark.parametrize("name", im.CATALOGUE)
def test_oracle_equals_py_ref_on_the_catalogue(oracle_lib, name):
    assert _differences(oracle_lib, name, 0) == 0


@pytest.mark.parametrize("k", (0,) + im.MIRRORED)
def test_oracle_equals_py_ref_on_mirrored_9(oracle_lib, k):
    assert _differences(oracle_lib, "unequal9", k) == 0


def test_oracle_equals_py_ref_on_wide15(oracle_lib):
    assert _differences(oracle_lib, "wide15", 0) == 0 and len(im.specials(im.get_map("wide15"))) == 30


@pytest.mark.parametrize("k", im.TRANSPOSED)
def test_oracle_differs_from_py_ref_on_transposed_9(oracle_lib, k):
    """The documented finding: on a transposed map the reference's shortcut is not its
    nearest_campfire function, and the labels follow."""
    og = oracle_lib.OracleGrid(im.oriented("unequal9", k).cells())
    pairs = sum(og.nearest_campfire(i, h) != og.nearest_campfire(i, h, direct=True)
                for i in range(81) for h in range(4))
    diff = _differences(oracle_lib, "unequal9", k)
    print(f"unequal9 k={k}: {pairs} (cell, homeland) pairs, {diff} of {3 * len(im.capped_queries('unequal9'))} labels")
    assert pairs >= 1 and diff >= 1


def _oracle_all(oracle_lib, name, k, pi, sources):
    """The oracle's labels of every cell of orientation k from each source, [source][cell]."""
    om = im.oriented(name, k)
    return [_oracle_labels(oracle_lib, name, k, pi, [(s, d) for d in om.all_indices()]) for s in sources]


@pytest.mark.parametrize("k", im.TRANSPOSED)
def test_transposed_all_destinations_tell_py_ref_from_the_oracle(oracle_lib, k):
    """A premise of test_gpu_oriented_all_destinations.py's transposed tests: from the sources
    they use, under parameter set 0 (Blue, nine regions), some cell's py_ref label is not the
    oracle's, so an engine that followed the reference's projection shortcut would fail them."""
    sources = im.transposed_sources("unequal9")
    ref = im.py_ref_all("unequal9", k, 0, sources)
    diff = [sum(a != b for a, b in zip(o, r)) for o, r in zip(_oracle_all(oracle_lib, "unequal9", k, 0, sources), ref)]
    print(f"unequal9 k={k} params 0: labels that differ, by source: {diff} of 81 each")
    assert sum(diff) >= 1, diff


@pytest.mark.parametrize("name", im.ORIENTED)
def test_all_destinations_sources_meet_ties(oracle_lib, name):
    """The other premise: on every map of the mirrored and the transposed tests, the chosen
    sources reach some plain cell by two boundaries with equal legs, money and time and
    different commands (irregular_maps.tie_cells, parameter set 0), so the boundaries' order,
    which the kernels take from the layout's rank table, decides a label the tests compare.
    Mirrored layouts from the oracle's labels; transposed ones from py_ref's, every layout of
    the 9 x 9 map and one of each 15 x 15 map (py_ref takes a second a source there)."""
    m = im.get_map(name)
    params = im.params_for(m)[0]
    for k in im.MIRRORED:
        sources = im.sssp_sources(m)
        labels = _oracle_all(oracle_lib, name, k, 0, sources)
        n = [len(im.tie_cells(im.oriented(name, k), params, s, lab)) for s, lab in zip(sources, labels)]
        assert sum(n) >= 1, f"{name} k={k}: {sum(n)} tie cells, by source {n}"
    for k in im.TRANSPOSED if m.size == 9 else (5,):
        sources = im.transposed_sources(name)
        labels = im.py_ref_all(name, k, 0, sources)
        n = [len(im.tie_cells(im.oriented(name, k), params, s, lab)) for s, lab in zip(sources, labels)]
        print(f"{name} k={k}: {sum(n)} tie cells, by source {n}")
        assert sum(n) >= 1, f"{name} k={k}: {sum(n)} tie cells, by source {n}"


def test_tie_cells_on_a_case_worked_by_hand():
    """tie_cells itself.  From the Center with scrolls and caravans off, a label is one
    CentralMove to a border-1 cell and a walk.  A homeland cell is as far from the border-1
    cell on either of its two axes (a tie); a border cell is nearer the one on its own axis."""
    from marshrutka_amd.abi import CellIndex, Params
    m = im.get_map("unequal9")
    params = Params(use_soe=False, use_caravans=False)
    f = im.py_ref.Finder(im.finder_for("unequal9", 0, 0).g, params.to_json())
    labels = im.finder_labels(f, [(CellIndex.center(), d) for d in m.all_indices()])
    want = [c for c in m.all_indices() if c.kind == CELL_HOMELAND and c not in im.specials(m)]
    assert want and im.tie_cells(m, params, CellIndex.center(), labels) == want


@pytest.mark.parametrize("name", im.CATALOGUE + ["unequal9", "wide15", "unequal21"])
def test_projection_equals_direct_argmin_on_the_given_orientation(oracle_lib, name):
    m = im.get_map(name)
    for k in (0,) + im.MIRRORED:
        og = oracle_lib.OracleGrid(im.oriented(name, k).cells())
        for i in range(m.size * m.size):
            for h in range(4):
                assert og.nearest_campfire(i, h) == og.nearest_campfire(i, h, direct=True), (k, i, h)


@pytest.mark.parametrize("name", ["unequal9", "unequal", "unequal21"])
def test_mirrored_labels_equal_the_standard_orientation(oracle_lib, name):
    """A mirror image changes no label: 1 500 queries on S = 9, 15 and 21."""
    m = im.get_map(name)
    qs = random_queries(m, 1500, 31 + m.size)
    for pi in PARAMS3:
        base = _oracle_labels(oracle_lib, name, 0, pi, qs)
        for k in im.MIRRORED:
            assert _oracle_labels(oracle_lib, name, k, pi, qs) == base, (pi, k)


def test_orient_keeps_cells_and_agrees_between_lists_and_arrays():
    m = im.get_map("unequal9")
    base = m.cells()
    seen = set()
    for k in range(8):
        cells = im.orient(base, k)
        arr = im.orient(m.cells_array(), k)
        assert sorted(cells) == sorted(base)
        assert [(c.kind, c.sub, c.x, c.y, p) for c, p in cells] == \
            [(int(r["kind"]), int(r["sub"]), int(r["x"]), int(r["y"]), int(r["poi"])) for r in arr]
        seen.add(tuple(c for c, _ in cells))
    assert len(seen) == 8 and im.orient(base, 0) == base
    S = m.size
    assert im.orient(base, 1)[0] == base[S - 1] and im.orient(base, 2)[0] == base[S * (S - 1)]
    assert im.orient(base, 4)[1] == base[S]


SHAPES = {"six": [6, 1, 1, 1], "seven": [7, 1, 1, 1], "unequal": [9, 1, 2, 1], "border1": [2, 2, 2, 2],
          "border_far": [2, 2, 2, 2], "center_fire": [2, 2, 2, 2], "corners": [4, 4, 4, 4], "ties": [6, 2, 2, 2],
          "s3": [1, 1, 1, 1], "s5_full": [4, 1, 1, 1], "unequal9": [9, 1, 2, 1], "unequal21": [9, 1, 2, 1],
          "wide15": [7, 6, 6, 6]}


def test_shape_facts():
    for name, want in SHAPES.items():
        assert im.counts(name) == want, name
    assert im.K_LANE_REGS == 6
    assert im.lane_layout_expected(im.get_map("six"), BLUE) and not im.lane_layout_expected(im.get_map("seven"), BLUE)
    assert not im.lane_layout_expected(im.get_map("unequal"), BLUE)
    assert not im.lane_layout_expected(im.get_map("border1"), BLUE)
    # the off-homeland campfires, and only those maps have any
    off = {n: [str(c) for c in im.off_homeland_campfires(im.get_map(n))] for n in SHAPES}
    assert {n: v for n, v in off.items() if v} == {"border1": ["BR 1", "GY 1"], "border_far": ["RG 4", "YB 7"],
                                                   "center_fire": ["0#0"], "unequal21": ["BR 1", "RG 6"]}
    assert im.get_map("border_far").h == 7  # YB 7 is on the map's edge
    # s3 and s5_full's Blue: no homeland cell that is not a campfire
    for name, homelands in (("s3", range(4)), ("s5_full", [BLUE])):
        assert not [c for c, p in im.get_map(name).cells()
                    if c.kind == CELL_HOMELAND and c.sub in homelands and p != POI_CAMPFIRE]
    # ties: Blue's six campfires all have x + y = 7
    assert {c.x + c.y for c in im.get_map("ties").campfires() if c.kind == CELL_HOMELAND and c.sub == BLUE} == {7}
    # every parameter set's HQ is a cell of its map, and the queries hold more than 32 from one source
    for name in im.CATALOGUE:
        m = im.get_map(name)
        cells = set(m.all_indices())
        assert all(p.hq_position is None or p.hq_position in cells for p in im.params_for(m))
        assert {p.homeland for p in im.params_for(m)} == {0, 1, 2, 3}
        qs = im.queries_for(name)
        assert all(a in cells and b in cells for a, b in qs)
        if name != "s3":
            by_src = {}
            for a, _ in qs:
                by_src[a] = by_src.get(a, 0) + 1
            assert max(v for a, v in by_src.items() if a not in im.specials(m)) >= 40
    assert len(im.queries_for("s3")) == 81
