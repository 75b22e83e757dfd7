"""The premises of test_gpu_table_edges.py, on the CPU and from the oracle alone: the maps have the
campfire counts (so the table sizes) they are named for, and the sources and parameter sets the
GPU tests use on the 21 x 21 maps make labels that start their closing walk from table entries
all over the table, the last ones included, so a kernel that mishandles high entries cannot give
the oracle's labels.

A label's boundary is the cell at which its last command that is no StandardMove arrives
(table_edge_maps.boundary_of); a source's own cell does not count.  Per (map, HQ or not, parameter
set), over the four sources:

  sets 0 and 3 (Legs first: a caravan and a scroll cost no legs): every special is a boundary,
      a campfire of each homeland and the HQ among them;
  set 6 (Time first, Route Guru 5: a caravan beats a walk): at least half of the specials, the HQ
      and a campfire of each homeland among them (but Green's one campfire on t64_blue with the
      HQ, which sits next to it: GREEN_MISSED);
  sets 1 and 4 (Time first below Route Guru 2) on t64_blue: at least half, the HQ among them.
      A caravan never pays there (240 s a cell against a walk's 180 s over the same cells or more),
      but 55 of the specials are the query homeland's campfires, which a scroll reaches;
  sets 1 and 4 on t32, t63 and t64: without caravans only the Center, the border-1 cells, the
      query homeland's campfires and the HQ can be boundaries, and 5 + 7 + 1 or 5 + 15 + 1 of them
      is less than half of 31 or of 62 (reach_bound, asserted), so no choice of sources reaches half.
      REACH pins what the oracle does reach; the HQ is among it;
  sets 2, 5 and 7 (Money first) on every map: a caravan costs money and a walk none, so the
      same bound holds with the set's homeland (Blue at a scroll price of 50, which a walk beats
      too: the Center and the border-1 cells only; Yellow and Red with free scrolls: 14 or 15
      campfires, one on t64_blue).  REACH pins what the oracle reaches; the HQ is among it under
      set 7, whose HQ scroll is free.

Ties: from every source of every map, under set 0, some plain cell is reached from two boundaries
with equal legs, money and time and different commands (irregular_maps.tie_cells), so the
boundaries' rank order decides a label the GPU tests compare."""
import pytest

import irregular_maps as im
import table_edge_maps as tm
from marshrutka_amd.abi import CELL_HOMELAND, GREEN, SORT_LEGS, SORT_MONEY

FULL_SETS, HALF_SETS = (0, 3), (6,)
# (map, set) -> specials that are boundaries (without, with the HQ), where half is out of reach
REACH = {("t32", 1): (9, 10), ("t32", 2): (5, 5), ("t32", 4): (9, 10), ("t32", 5): (10, 10), ("t32", 7): (11, 11),
         ("t63", 1): (15, 16), ("t63", 2): (5, 5), ("t63", 4): (15, 16), ("t63", 5): (17, 18), ("t63", 7): (13, 14),
         ("t64", 1): (15, 16), ("t64", 2): (5, 5), ("t64", 4): (15, 16), ("t64", 5): (17, 18), ("t64", 7): (14, 15),
         ("t64_blue", 2): (5, 5), ("t64_blue", 5): (6, 6), ("t64_blue", 7): (6, 7)}
GREEN_MISSED = ("t64_blue", True, 6)
HQ_SETS = (0, 1, 3, 4, 6, 7)  # the sets under which the HQ is a boundary


def reach_bound(name, hq, pi):
    """The most specials that can be boundaries where a caravan never pays: the Center, the
    border-1 cells, the query homeland's campfires (by the Scroll of Escape) and the HQ; under
    Money first a scroll only where it is free (a walk costs no money)."""
    p = tm.EDGE_PARAMS[pi]
    assert p.sort_by[0] != SORT_LEGS and (p.sort_by[0] == SORT_MONEY or p.route_guru < 2)
    money_first = p.sort_by[0] == SORT_MONEY
    soe = p.use_soe and (not money_first or p.scroll_of_escape_cost == 0)
    shq = hq and (not money_first or p.scroll_of_escape_hq_cost == 0)
    return 5 + (tm.SPEC[name][1][p.homeland] if soe else 0) + shq


def test_counts_and_table_sizes():
    for name, (S, n) in tm.SPEC.items():
        assert tm.counts(name) == (list(n), 0), name
        m = tm.get_map(name)
        assert m.size == S
        for hq in (False, True):
            sp = tm.specials(name, hq)
            assert len(set(sp)) == len(sp) == tm.NUM_SPECIALS[name][hq], (name, hq)
        # the HQ, the sources' plain cell and border cell are no specials; the sources are distinct
        assert tm.hq_cell(name) not in tm.specials(name, False)
        for hq in (False, True):
            src = tm.sources_for(name, hq)
            assert len(set(src)) == 4 and src[3] not in tm.specials(name, True)
            assert (src[2] == tm.hq_cell(name)) == hq and src[1] in m.campfires()
    assert sorted(t + 1 for n in tm.NUM_SPECIALS.values() for t in n) == [32, 33, 63, 64, 64, 64, 64, 65, 65, 65]
    # spread over the homeland, not packed in a corner: six or seven campfires lie in at least
    # three of the homeland's four quarters, fourteen or more in all four
    for name in tm.SPEC:
        H = tm.get_map(name).h
        for h in range(4):
            fires = [c for c in tm.get_map(name).campfires() if c.kind == CELL_HOMELAND and c.sub == h]
            quarters = {(c.x > H // 2, c.y > H // 2) for c in fires}
            assert len(fires) < 6 or len(quarters) >= 3, (name, h)
            assert len(fires) < 14 or len(quarters) == 4, (name, h)


def test_parameter_sets():
    orders = [p.sort_by for p in tm.FILL_PARAMS]
    assert len(set(orders)) == 6 and tm.EDGE_PARAMS[:6] == tm.FILL_PARAMS and len(tm.EDGE_PARAMS) == 8
    assert all(tm.EDGE_PARAMS[pi].sort_by[0] == SORT_LEGS for pi in FULL_SETS)
    assert sorted(FULL_SETS + HALF_SETS + tuple({pi for _, pi in REACH})) == list(range(8))
    assert {p.homeland for p in tm.EDGE_PARAMS} == {0, 1, 3}


@pytest.mark.parametrize("hq", [False, True], ids=["nohq", "hq"])
@pytest.mark.parametrize("name", tm.SMALL)
def test_boundaries_cover_the_table(oracle_lib, name, hq):
    sp = tm.specials(name, hq)
    sources = tm.sources_for(name, hq)
    hq_key = tm.key(tm.hq_cell(name))
    for pi in range(len(tm.EDGE_PARAMS)):
        labels = tm.oracle_labels(oracle_lib, name, hq, pi)
        seen = set()
        for s, labs in zip(sources, labels):
            seen |= tm.boundaries(labs) - {tm.key(s)}
        hit = [c for c in sp if tm.key(c) in seen]
        by_homeland = [sum(c.kind == CELL_HOMELAND and c.sub == h and tm.key(c) != hq_key for c in hit) for h in range(4)]
        print(f"{name} hq={hq} set {pi}: {len(hit)} of {len(sp)} specials are boundaries, campfires by homeland {by_homeland}")
        if pi in FULL_SETS:
            assert len(hit) == len(sp), (pi, len(hit))
        if (name, pi) not in REACH:
            assert 2 * len(hit) >= len(sp), (pi, len(hit))
        else:
            assert 2 * reach_bound(name, hq, pi) < len(sp), pi  # half is out of reach whatever the sources
            assert len(hit) == REACH[(name, pi)][hq], (pi, len(hit))
        if pi in FULL_SETS + HALF_SETS:
            missed = [h for h in range(4) if not by_homeland[h]]
            assert missed == ([GREEN] if (name, hq, pi) == GREEN_MISSED else []), (pi, by_homeland)
        if hq and pi in HQ_SETS:
            assert hq_key in seen, pi
        if pi in FULL_SETS + HALF_SETS:  # the table's last entry: the last campfire in row-major order, or the HQ
            assert tm.key(sp[-1]) in seen, pi


@pytest.mark.parametrize("hq", [False, True], ids=["nohq", "hq"])
@pytest.mark.parametrize("name", tm.SMALL)
def test_every_source_meets_ties(oracle_lib, name, hq):
    m = tm.get_map(name)
    params = tm.params_for(name, hq, 0)
    n = [len(im.tie_cells(m, params, s, labs))
         for s, labs in zip(tm.sources_for(name, hq), tm.oracle_labels(oracle_lib, name, hq, 0))]
    print(f"{name} hq={hq}: tie cells by source {n}")
    assert all(n), n
