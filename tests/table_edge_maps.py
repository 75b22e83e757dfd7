"""Maps whose special table sits at the edges of what one wave holds (test infrastructure for
test_table_edge_maps.py on the CPU and test_gpu_table_edges.py on the device; no engine import).

The hub's per-source label table has T = NS + 1 entries: the source, then the NS specials (the
Center, the four border-1 cells, every campfire, and the HQ where it is a plain cell).  The fill,
matrix, nearest and k-nearest kernels each load it one entry a lane, so T = 64 fills the wave,
T = 32 / 33 is where hub_kernel goes from two sources a wave to one, and T = 65 is the first
table the narrow hub cannot hold.  Counts are homeland campfires in Blue / Red / Green / Yellow
order; NS is without -> with an HQ on a plain cell:

  t32       S = 21,  7/7/6/6     NS 31 -> 32   T = 32 (two sources a wave) and T = 33 (one)
  t63       S = 21,  15/14/14/14 NS 62 -> 63   T = 63, and T = 64 with the HQ as entry 63
  t64       S = 21,  15/15/14/14 NS 63 -> 64   T = 64 with a campfire as entry 63; T = 65 with the HQ
  t64_blue  S = 21,  55/1/1/1    NS 63 -> 64   55 regions under homeland Blue, 1 under Red
  t64_129   S = 129, 15/15/14/14 NS 63 -> 64   wide enough for 64 x 16 fill tiles and packed keys

Nothing is drawn: campfire i of homeland h is cell (i * STEP + 13 * h) mod H^2 of the homeland's
H x H cells, numbered x - 1 + H (y - 1).  STEP is coprime to H^2 and near 3/8 of it, so
consecutive campfires land far apart and any prefix of the sequence is spread over the homeland
(test_table_edge_maps.py counts the quarters of each homeland they reach).

The HQ of the "with HQ" variants is a plain Green cell near the middle of the homeland; the
table puts it last, after every campfire (plan_create's order: query-homeland campfires first,
then the others in row-major order, then the HQ).
"""
import dataclasses

import numpy as np

from marshrutka_amd.abi import (BLUE, BR, CELL_HOMELAND, CMD_STANDARD, GREEN, POI_CAMPFIRE, RED, RG, SORT_LEGS, SORT_MONEY,
                                SORT_TIME, YELLOW, CellIndex, Params)
from marshrutka_amd.mapgen import SyntheticMap

STEP = {10: 37, 64: 1571}

# name -> (S, homeland campfires in Blue / Red / Green / Yellow order)
SPEC = {
    "t32": (21, (7, 7, 6, 6)),
    "t63": (21, (15, 14, 14, 14)),
    "t64": (21, (15, 15, 14, 14)),
    "t64_blue": (21, (55, 1, 1, 1)),
    "t64_129": (129, (15, 15, 14, 14)),
}
SMALL = ["t32", "t63", "t64", "t64_blue"]
# NS without and with the HQ
NUM_SPECIALS = {"t32": (31, 32), "t63": (62, 63), "t64": (63, 64), "t64_blue": (63, 64), "t64_129": (63, 64)}


def spread(H, n, h):
    """The (x, y) of homeland h's n campfires on a map with H x H homelands."""
    out = []
    for i in range(n):
        c = (i * STEP[H] + 13 * h) % (H * H)
        out.append((1 + c % H, 1 + c // H))
    assert len(set(out)) == n
    return out


_maps = {}


def get_map(name):
    if name not in _maps:
        S, n = SPEC[name]
        extra = [CellIndex.homeland(h, x, y) for h in (BLUE, RED, GREEN, YELLOW) for x, y in spread(S // 2, n[h], h)]
        _maps[name] = SyntheticMap(S, campfires_per_homeland=0, seed=1, extra_campfires=extra, fountains=0, forums=0)
    return _maps[name]


def counts(name):
    """Homeland campfires per homeland, from the map's cells; campfires elsewhere."""
    n, off = [0, 0, 0, 0], 0
    for c, p in get_map(name).cells():
        if p == POI_CAMPFIRE:
            if c.kind == CELL_HOMELAND:
                n[c.sub] += 1
            else:
                off += 1
    return n, off


def hq_cell(name):
    """The HQ of the map's "with HQ" variants: the first plain cell of Green's row y = H / 2 from
    x = H / 2 on."""
    m = get_map(name)
    H = m.h
    fires = set(m.campfires())
    return next(c for c in (CellIndex.homeland(GREEN, x, H // 2) for x in range(H // 2, H + 1)) if c not in fires)


def specials(name, hq):
    """The NS specials of a plan on the map, with the HQ if hq."""
    out = [CellIndex.center()] + [CellIndex.border(b, 1) for b in range(4)] + get_map(name).campfires()
    return out + ([hq_cell(name)] if hq else [])


# test_gpu_sssp.py's FILL_PARAMS (the six metric orders, with its scroll and Route Guru variety), the
# HQ left to the map.  Restated here so that the CPU tests import no GPU test module;
# test_gpu_table_edges.py asserts the two lists equal but for hq_position.
FILL_PARAMS = [Params(), Params(sort_by=(SORT_TIME, SORT_MONEY)),
               Params(sort_by=(SORT_MONEY, SORT_LEGS), use_sfm=True, route_guru=2),
               Params(sort_by=(SORT_LEGS, SORT_TIME), use_soe=False),
               Params(sort_by=(SORT_TIME, SORT_LEGS), fleetfoot=7),
               Params(sort_by=(SORT_MONEY, SORT_TIME), scroll_of_escape_cost=0, homeland=3)]
# Two more sets, for the boundaries the six cannot reach.  A caravan costs money and, below Route
# Guru 2, more time a cell than a walk, so under FILL_PARAMS' Time- and Money-first sets no campfire
# outside the query homeland is ever a boundary, and the HQ scroll (75) never under Money first.
# Set 6: Time first at Route Guru 5 (102 s a cell against a walk's 180).  Set 7: Money first with
# free scrolls, Red the homeland.  Under Money first a caravan still never pays: the reach there is
# the Center, the border-1 cells, the query homeland's campfires and the HQ, whatever the sources.
EDGE_PARAMS = FILL_PARAMS + [Params(sort_by=(SORT_TIME, SORT_MONEY), route_guru=5),
                             Params(sort_by=(SORT_MONEY, SORT_LEGS), scroll_of_escape_cost=0, scroll_of_escape_hq_cost=0,
                                    homeland=RED)]


def params_for(name, hq, pi):
    return dataclasses.replace(EDGE_PARAMS[pi], hq_position=hq_cell(name) if hq else None)


def sources_for(name, hq):
    """The Center, a campfire, the HQ (a border cell where the variant has none) and a plain cell.
    The campfire is Red's first in row-major order; the plain cell is the Yellow cell nearest the
    middle of its homeland that is no campfire.

    t64_blue has its own: under Time first only a scroll reaches a campfire, always the one nearest
    the cell it is read at, so sources in and at Blue's far corner (the campfire B 10#10, the
    border cell BR 10 and the plain cell B 6#8) are what makes the walks from them pass the regions
    of more than half of Blue's 55 campfires."""
    m = get_map(name)
    H = m.h
    fires = m.campfires()
    if name == "t64_blue":
        out = [CellIndex.center(), CellIndex.homeland(BLUE, 10, 10), hq_cell(name) if hq else CellIndex.border(BR, 10),
               CellIndex.homeland(BLUE, 6, 8)]
        assert out[1] in fires and out[3] not in fires
        return out
    red = [c for c in fires if c.kind == CELL_HOMELAND and c.sub == RED]
    plain = next(c for c in (CellIndex.homeland(YELLOW, x, H // 2 + 1) for x in range(H // 2 + 1, H + 1)) if c not in fires)
    return [CellIndex.center(), red[0], hq_cell(name) if hq else CellIndex.border(RG, H // 2), plain]


def boundary_of(label):
    """The cell at which the last command of a label that is no StandardMove arrives (the boundary
    the label's closing walk starts from), in as_expected's form; None for a label that only walks."""
    for c in reversed(label[3]):
        if c[0] != CMD_STANDARD:
            return tuple(c[6])
    return None


def boundaries(labels):
    """The set of boundary_of over labels (lists of as_expected forms)."""
    return {b for lab in labels if lab is not None for b in [boundary_of(lab)] if b is not None}


def key(c):
    return (c.kind, c.sub, c.x, c.y)


def groups_mod7(n):
    return [j % 7 for j in range(n)]


def as_metrics(labels):
    return np.array([e[:3] for e in labels], dtype=np.int64)


_labels = {}


def oracle_labels(oracle_lib, name, hq, pi, k=0):
    """The oracle's labels [source][cell] of sources_for(name, hq) to every cell of the map in
    layout k (0: as built; 1..3: mirrored, irregular_maps.orient) under params_for(name, hq, pi),
    in as_expected's form, once per case."""
    from golden_util import as_expected
    from irregular_maps import orient
    case = (name, hq, pi, k)
    if case not in _labels:
        laid = orient(get_map(name).cells(), k)
        og = oracle_lib.OracleGrid(laid)
        params = params_for(name, hq, pi)
        _labels[case] = [[as_expected(e) for e in og.find_path_batch(params, [(s, d) for d, _ in laid], threads=0)]
                        for s in sources_for(name, hq)]
    return _labels[case]
