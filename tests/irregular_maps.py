"""Maps the synthetic generator never draws, in every orientation (test infrastructure for
test_irregular_maps.py on the CPU, test_gpu_irregular_maps.py and
test_gpu_oriented_all_destinations.py on the device; no engine import).

SyntheticMap(size, campfires_per_homeland=k) gives every homeland the same number of
campfires, campfires on homeland cells only, and the one standard orientation.  A map
parsed from HTML promises neither of the first two, and the engine accepts any
orientation.  The catalogue below has fixed campfire positions (nothing is drawn at test
time); counts are in Blue / Red / Green / Yellow order:

  six          S = 15, 6/1/1/1: the most regions hub_lane_kernel holds (Blue the query homeland)
  seven        S = 15, 7/1/1/1: one past it
  unequal      S = 15, 9/1/2/1: the table's shape changes with params.homeland
  border1      S = 15, 2 each, campfires on BR 1 and GY 1: border-1 cells that are caravan hubs
  border_far   S = 15, 2 each, campfires on RG 4 and YB 7 (the second on the map's edge)
  center_fire  S = 11, 2 each, the Center's poi a campfire
  corners      S = 15, every homeland with campfires at (1,1), (7,7), (1,7), (7,1)
  ties         S = 15, 2 each but Blue: six campfires with x + y = 7, many equidistant cells
  s3           S = 3, every homeland cell a campfire: regions of specials only
  s5_full      S = 5, Blue's four cells all campfires, one in each other homeland

and, for the orientation tests, `unequal9` (S = 9, 9/1/2/1), `wide15` (S = 15, 7/6/6/6: a
table of 31 entries, the widest the lane and group kernels hold, four slots a lane in a
group of 8) and `unequal21` (S = 21, 9/1/2/1 with a campfire on BR 1 and one on RG 6).

A campfire off the homelands (a border cell, the Center) is a caravan hub and no Scroll of
Escape target (the reference's grid.poi[Campfire], src/grid.rs:134-151, src/pathfinder.rs:
142-147).

orient(cells, k), k in 0..7: bit 0 flips x, bit 1 flips y, bit 2 transposes; every cell
keeps its label and poi.  On the standard and the mirrored orientations (k = 0..3) the
specification is the C++ oracle; on the transposed ones (k = 4..7) the reference's own
projection shortcut is not its nearest_campfire function, and the specification is
py_ref (the search over nearest campfires from the direct argmin): DESIGN.md section 1, "Grid orientation".
"""
import random

import numpy as np

import py_ref
from large_costs import finder_labels
from marshrutka_amd.abi import (BLUE, BR, CELL_BORDER, CELL_HOMELAND, GREEN, GY, POI_CAMPFIRE, RED, RG, SORT_LEGS,
                                SORT_MONEY, SORT_TIME, YB, YELLOW, CellIndex, Params)
from marshrutka_amd.mapgen import SyntheticMap, random_queries

K_LANE_REGS = 6  # hub_lane_kernel's region slots (kLaneRegs, mr_hub_lane.hpp)

_TWO = {BLUE: [(2, 3), (5, 6)], RED: [(4, 1), (1, 5)], GREEN: [(3, 3), (6, 2)], YELLOW: [(2, 6), (7, 4)]}
_BLUE9 = [(1, 1), (2, 5), (4, 3), (6, 6), (7, 2), (3, 7), (5, 5), (1, 4), (7, 7)]
_ONE = {RED: [(3, 3)], GREEN: [(5, 2)], YELLOW: [(2, 6)]}

# name -> (S, homeland campfires {homeland: [(x, y)]}, campfires off the homelands)
_SPEC = {
    "six": (15, {BLUE: _BLUE9[:6], **_ONE}, []),
    "seven": (15, {BLUE: _BLUE9[:7], **_ONE}, []),
    "unequal": (15, {BLUE: _BLUE9, RED: [(3, 3)], GREEN: [(5, 2), (2, 6)], YELLOW: [(4, 4)]}, []),
    "border1": (15, _TWO, [CellIndex.border(BR, 1), CellIndex.border(GY, 1)]),
    "border_far": (15, _TWO, [CellIndex.border(RG, 4), CellIndex.border(YB, 7)]),
    "center_fire": (11, {BLUE: [(2, 3), (5, 4)], RED: [(4, 1), (1, 5)], GREEN: [(3, 3), (5, 2)],
                         YELLOW: [(2, 5), (4, 4)]}, [CellIndex.center()]),
    "corners": (15, {h: [(1, 1), (7, 7), (1, 7), (7, 1)] for h in range(4)}, []),
    "ties": (15, {**_TWO, BLUE: [(1, 6), (6, 1), (2, 5), (5, 2), (3, 4), (4, 3)]}, []),
    "s3": (3, {h: [(1, 1)] for h in range(4)}, []),
    "s5_full": (5, {BLUE: [(1, 1), (1, 2), (2, 1), (2, 2)], RED: [(2, 1)], GREEN: [(1, 2)], YELLOW: [(2, 2)]}, []),
    "unequal9": (9, {BLUE: [(1, 1), (1, 3), (2, 2), (2, 4), (3, 1), (3, 3), (4, 2), (4, 4), (1, 4)], RED: [(2, 3)],
                     GREEN: [(3, 2), (1, 4)], YELLOW: [(4, 1)]}, []),
    "wide15": (15, {BLUE: _BLUE9[:7], RED: [(1, 2), (3, 6), (5, 1), (6, 4), (2, 4), (7, 7)],
                    GREEN: [(2, 1), (4, 5), (6, 6), (1, 7), (7, 3), (3, 3)],
                    YELLOW: [(1, 1), (2, 6), (4, 2), (5, 7), (7, 5), (3, 4)]}, []),
    "unequal21": (21, {BLUE: [(1, 2), (3, 9), (5, 5), (8, 1), (10, 10), (2, 6), (9, 4), (6, 8), (4, 1)],
                       RED: [(7, 3)], GREEN: [(2, 9), (8, 8)], YELLOW: [(5, 6)]},
                  [CellIndex.border(BR, 1), CellIndex.border(RG, 6)]),
}
CATALOGUE = ["six", "seven", "unequal", "border1", "border_far", "center_fire", "corners", "ties", "s3", "s5_full"]
ORIENTED = ["unequal9", "unequal", "wide15"]  # the maps of the orientation tests
MIRRORED = (1, 2, 3)
TRANSPOSED = (4, 5, 6, 7)

_maps = {}


def get_map(name):
    if name not in _maps:
        S, home, off = _SPEC[name]
        extra = [CellIndex.homeland(h, x, y) for h in sorted(home) for x, y in home[h]] + list(off)
        _maps[name] = SyntheticMap(S, campfires_per_homeland=0, seed=1, extra_campfires=extra, fountains=0, forums=0)
    return _maps[name]


def counts(name):
    """Homeland campfires (the SoE regions) per homeland, from the map's cells."""
    n = [0, 0, 0, 0]
    for c, p in get_map(name).cells():
        if p == POI_CAMPFIRE and c.kind == CELL_HOMELAND:
            n[c.sub] += 1
    return n


def off_homeland_campfires(m):
    return [c for c in m.campfires() if c.kind != CELL_HOMELAND]


def orient(cells, k):
    """The same cells (labels and poi) laid out in orientation k: a cells() list gives a
    list, a cells_array() a contiguous array."""
    if isinstance(cells, np.ndarray):
        S = int(round(len(cells) ** 0.5))
        a = cells.reshape(S, S)
    else:
        S = int(round(len(cells) ** 0.5))
        a = np.arange(S * S).reshape(S, S)
    if k & 1:
        a = a[:, ::-1]
    if k & 2:
        a = a[::-1, :]
    if k & 4:
        a = a.T
    if isinstance(cells, np.ndarray):
        return np.ascontiguousarray(a).reshape(-1)
    return [cells[i] for i in a.reshape(-1)]


class Oriented:
    """A map in orientation k with the part of SyntheticMap's interface the test helpers use
    (cells, all_indices, cells_array, campfires, query_array, size)."""

    def __init__(self, m, k):
        self.base, self.k, self.size, self.h = m, k, m.size, m.h
        self._cells = orient(m.cells(), k)

    def cells(self):
        return self._cells

    def all_indices(self):
        return [c for c, _ in self._cells]

    def cells_array(self):
        return orient(self.base.cells_array(), self.k)

    def campfires(self):
        return self.base.campfires()

    def query_array(self, src, dst, cells=None):
        return self.base.query_array(src, dst, self.cells_array() if cells is None else cells)


def oriented(name, k):
    key = (name, k)
    if key not in _maps:
        _maps[key] = Oriented(get_map(name), k)
    return _maps[key]


def _hqs(m):
    """(a border campfire, or a border-1 cell where the map has none; a Blue campfire; the
    Center): params_for's three HQ cells."""
    off = [c for c in off_homeland_campfires(m) if c.kind == CELL_BORDER]
    blue = [c for c in m.campfires() if c.kind == CELL_HOMELAND and c.sub == BLUE]
    return (off[-1] if off else CellIndex.border(GY, 1)), blue[-1], CellIndex.center()


def params_for(m):
    """Six parameter sets: each homeland; orders led by Legs, Time and Money; Fleetfoot 0 and
    2; the Scroll of the Forum; an HQ on a border cell (a campfire where the map has one),
    on another homeland's campfire and on the Center.  Set 0 is Legs first with a linear
    run time, Blue, no HQ: the plan whose kernel choice the tests assert."""
    border, blue_cf, center = _hqs(m)
    return [Params(),
            Params(homeland=RED, sort_by=(SORT_TIME, SORT_MONEY), fleetfoot=2, hq_position=border),
            Params(homeland=GREEN, sort_by=(SORT_MONEY, SORT_LEGS), use_sfm=True, hq_position=blue_cf),
            Params(homeland=YELLOW, sort_by=(SORT_LEGS, SORT_TIME), route_guru=3, hq_position=center),
            Params(homeland=BLUE, sort_by=(SORT_MONEY, SORT_TIME), fleetfoot=2, use_sfm=True, hq_position=border,
                   scroll_of_escape_cost=7),
            Params(homeland=BLUE, sort_by=(SORT_TIME, SORT_LEGS), route_guru=2, hq_position=blue_cf)]


def specials(m):
    """The Center, the four border-1 cells, every campfire and params_for's HQ cells."""
    out = [CellIndex.center()] + [CellIndex.border(b, 1) for b in range(4)] + m.campfires() + list(_hqs(m))
    return list(dict.fromkeys(out))


_queries = {}


def queries_for(name):
    """Every special to every special, 150 random queries and one plain source with 40
    destinations (more than the lane kernel's 32 queries a source); on s3 all 81 pairs."""
    if name not in _queries:
        m = get_map(name)
        cells = m.all_indices()
        if m.size == 3:
            qs = [(a, b) for a in cells for b in cells]
        else:
            sp = specials(m)
            qs = [(a, b) for a in sp for b in sp] + random_queries(m, 150, 7 + m.size)
            plain = [c for c in cells if c not in sp]
            rng = random.Random(m.size)
            qs += [(plain[len(plain) // 3], d) for d in rng.choices(cells, k=40)]  # (s5_full has 25 cells)
        _queries[name] = qs
    return _queries[name]


def capped_queries(name, n=150):
    """n of queries_for(name), the same ones on every call (all of them if there are fewer)."""
    qs = queries_for(name)
    return qs if len(qs) <= n else random.Random(len(qs)).sample(qs, n)


def lane_layout_expected(m, homeland):
    """What lane_layout_ok (mr_host.cpp) must say of a plan on m: no border-1 cell a caravan
    hub and at most K_LANE_REGS campfires in the query homeland (the table puts them first,
    so every special's region campfire is then in entries 6..11)."""
    cf = m.campfires()
    if any(c.kind == CELL_BORDER and c.x == 1 for c in cf):
        return False
    return sum(c.kind == CELL_HOMELAND and c.sub == homeland for c in cf) <= K_LANE_REGS


_finders, _labels = {}, {}


def finder_for(name, k, pi):
    if (name, k, pi) not in _finders:
        cells = oriented(name, k).cells()
        if (name, k) not in _finders:
            _finders[(name, k)] = py_ref.Grid([((c.kind, c.sub, c.x, c.y), p) for c, p in cells])
        _finders[(name, k, pi)] = py_ref.Finder(_finders[(name, k)], params_for(get_map(name))[pi].to_json())
    return _finders[(name, k, pi)]


def py_ref_labels(name, k, pi, n=150):
    """py_ref's labels of capped_queries(name, n) on orientation k under params_for(..)[pi],
    in golden_util.as_expected's form; computed once per (map, orientation, params, n)."""
    key = (name, k, pi, n)
    if key not in _labels:
        _labels[key] = finder_labels(finder_for(name, k, pi), capped_queries(name, n))
    return _labels[key]


def sssp_sources(m):
    """The sources of the all-destinations and matrix tests: the Center, a border campfire (a
    border-1 cell where the map has none), a homeland campfire and a plain cell."""
    cells = m.all_indices()
    off = off_homeland_campfires(m)
    home = [c for c in m.campfires() if c not in off]
    plain = [c for c in cells if c not in specials(m)]
    out = [CellIndex.center(), off[-1] if off else CellIndex.border(1, 1), home[0]]
    return out + ([plain[len(plain) // 2]] if plain else [CellIndex.border(3, 1)])


def matrix_sources(m):
    """sssp_sources(m) and its last source once more: matrix plans keep one row for both."""
    s = sssp_sources(m)
    return s + [s[3]]


# How many of sssp_sources(m) the transposed all-destinations tests give py_ref, the Center
# and the plain cell first: one (map, layout, parameter set) must stay under about 5 s of
# py_ref (the measured seconds: test_gpu_oriented_all_destinations.py's docstring).
TRANSPOSED_SOURCE_ORDER = (0, 3, 2, 1)
TRANSPOSED_SOURCES = {"unequal9": 4, "unequal": 3, "wide15": 2}


def transposed_sources(name):
    s = sssp_sources(get_map(name))
    return [s[i] for i in TRANSPOSED_SOURCE_ORDER[:TRANSPOSED_SOURCES[name]]]


_all = {}


def py_ref_all(name, k, pi, sources):
    """py_ref's labels of every cell of orientation k (in its cells() order) from each of
    sources under params_for(..)[pi], [source][cell] in golden_util.as_expected's form; computed
    once per (map, orientation, params, source)."""
    cells = oriented(name, k).all_indices()
    out = []
    for s in sources:
        key = (name, k, pi, s)
        if key not in _all:
            _all[key] = finder_labels(finder_for(name, k, pi), [(s, d) for d in cells])
        out.append(_all[key])
    return out


def tie_cells(m, params, source, labels):
    """The plain cells of m (a map or an Oriented) whose label from `source` is decided by a
    tie: another boundary (the source or a special but the Center) reaches the cell by a walk
    with the same legs, money and time as the label and other commands.  `labels` are the
    reference's labels of m.all_indices() from `source` in as_expected's form; params must have
    Fleetfoot 0, so that a walk of k cells adds k legs and 180 k seconds to its boundary's
    label, whether or not it lengthens that label's last walk."""
    assert params.fleetfoot == 0
    STANDARD, NOMOVE = 2, 0
    S, H = m.size, m.size // 2
    cells = m.all_indices()
    pos = {c: (j % S - H, j // S - H) for j, c in enumerate(cells)}
    at = {c: j for j, c in enumerate(cells)}
    sp = [c for c in dict.fromkeys([source] + specials(m) + ([params.hq_position] if params.hq_position else []))
          if c != CellIndex.center()]
    out = []
    for d, lab in zip(cells, labels):
        if d in sp or d == CellIndex.center() or lab is None:
            continue
        to = [d.kind, d.sub, d.x, d.y]
        for b in sp:
            base = labels[at[b]]
            if base is None:
                continue
            (ax, ay), (bx, by) = pos[b], pos[d]
            k = abs(ax - bx) + abs(ay - by)
            if (ay == 0 and by == 0 and (ax < 0) != (bx < 0)) or (ax == 0 and bx == 0 and (ay < 0) != (by < 0)):
                k += 2  # the walk goes round the Center
            if [base[0] + k, base[1], base[2] + 180 * k] != lab[:3]:
                continue
            cmds = [list(c) for c in base[3]]
            last = cmds[-1]
            if last[0] == STANDARD:
                cmds[-1] = [STANDARD, last[1] + 180 * k, last[2] + k, 0, 0, last[5], to]
            elif last[0] == NOMOVE:
                cmds[-1] = [STANDARD, 180 * k, k, 0, 0, last[5], to]
            else:
                cmds.append([STANDARD, 180 * k, k, 0, 0, [b.kind, b.sub, b.x, b.y], to])
            if cmds != lab[3]:
                out.append(d)
                break
    return out


def py_ref_some(name_or_map, k, params, qs):
    """py_ref's labels of qs on a map outside the catalogue (not cached)."""
    m = get_map(name_or_map) if isinstance(name_or_map, str) else name_or_map
    grid = py_ref.Grid([((c.kind, c.sub, c.x, c.y), p) for c, p in orient(m.cells(), k)])
    return finder_labels(py_ref.Finder(grid, params.to_json()), qs)
