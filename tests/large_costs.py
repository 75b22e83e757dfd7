"""Inputs and references for the large scroll prices (test_large_costs.py on the CPU,
test_gpu_large_costs.py on the device).

Money is the one metric a caller can push to the top of 32 bits: the three scroll prices
are u32 fields of mr_params, while legs and time are bounded by the grid.  Two regimes:

  A  prices so large that label money has its upper bytes (and bit 31) set, yet no label
     and no candidate (a final label plus one edge) passes 2^32.  The C++ oracle wraps
     u32 sums like the reference's release build, so it is a reference exactly where
     nothing wraps: the precondition below, asserted on every case before anything is
     compared.
  B  prices whose sums pass 2^32.  The wrapping oracle prefers wrapped labels there (a
     wrap acts as a negative edge; at 2^32 - 1 its search does not end), so it is never
     called on these inputs.  The reference is py_ref.Finder(wrap=False): exact integers,
     non-negative weights, a search that terminates.

The gate cost G = (2^32 - 2) // (2 NS + 4) is the largest price the lane and group
kernels' documented bound admits (NS specials: the Center, four border-1 cells, the
campfires, and the HQ where it is none of those).  It only chooses inputs; no test
expects a value computed from it.
"""
import ctypes as C
import random

import numpy as np

import py_ref
from crafted_records import COMMAND_DT, RESULT_DT
from marshrutka_amd.abi import (MR_ERR_CAPACITY, MR_OK, SORT_LEGS, SORT_MONEY, SORT_TIME, CellIndex, Params,
                                mr_command, mr_result)
from marshrutka_amd.mapgen import SyntheticMap

# the six orders with distinct keys and (Time, Time), each at Fleetfoot 0 and 2
ORDERS = [(SORT_LEGS, SORT_MONEY), (SORT_LEGS, SORT_TIME), (SORT_MONEY, SORT_LEGS), (SORT_MONEY, SORT_TIME),
          (SORT_TIME, SORT_LEGS), (SORT_TIME, SORT_MONEY), (SORT_TIME, SORT_TIME)]
FLEETFOOT = [0, 2]

# case -> (map arguments, where the HQ is, the costs above G and G + 1)
CASES = {
    "A1": (dict(size=9, campfires_per_homeland=1, seed=10), "campfire", [(1 << 31) - 1000]),
    "A2": (dict(size=15, campfires_per_homeland=3, seed=18), "campfire", [1_000_000_000]),
    "A3": (dict(size=21, campfires_per_homeland=4, seed=25, clustered=True), "plain", [700_000_000]),
    "A4": (dict(size=25, campfires_per_homeland=6, seed=9, clustered=True), "campfire", []),
}
COSTS = ["G", "G+1", "top"]
CASE_COSTS = [(case, c) for case in CASES for c in COSTS if c != "top" or CASES[case][2]]

_maps = {}


def case_map(case):
    """(map, HQ cell) of a case."""
    if case not in _maps:
        args, hq, _ = CASES[case]
        m = SyntheticMap(**args)
        _maps[case] = (m, m.campfires()[-1] if hq == "campfire" else m.all_indices()[7])
    return _maps[case]


def num_specials(case):
    m, hq = case_map(case)
    specials = {CellIndex.center()} | {CellIndex.border(b, 1) for b in range(4)} | set(m.campfires())
    return len(specials | {hq})


def gate_cost(case):
    return ((1 << 32) - 2) // (2 * num_specials(case) + 4)


def cost_of(case, which):
    return {"G": gate_cost(case), "G+1": gate_cost(case) + 1}.get(which) or CASES[case][2][0]


def params_of(cost, sort_by, fleetfoot, hq):
    """Three distinct prices round `cost`, the Scroll of the Forum and Route Guru 3."""
    return Params(scroll_of_escape_cost=cost, scroll_of_escape_hq_cost=cost - 1, scroll_of_escape_forum_cost=cost - 2,
                  use_sfm=True, route_guru=3, hq_position=hq, fleetfoot=fleetfoot, sort_by=sort_by)


def sources_of(case):
    """24 sources: the Center, a border-1 cell, two campfires, the HQ and 19 more cells."""
    m, hq = case_map(case)
    fixed = [CellIndex.center(), CellIndex.border(1, 1), m.campfires()[0], m.campfires()[1], hq]
    assert len(set(fixed)) == 5
    rest = [c for c in m.all_indices() if c not in fixed]
    return fixed + random.Random(1).sample(rest, 19)


def queries_of(case):
    """Every cell from three of the sources (the Center, the HQ, a plain cell); 12 random
    destinations from each of the others, so that the lane kernel (at most 32 queries a
    source) takes those."""
    m, _ = case_map(case)
    cells = m.all_indices()
    rng = random.Random(2)
    qs = []
    for i, s in enumerate(sources_of(case)):
        qs += [(s, d) for d in (cells if i in (0, 4, 5) else rng.sample(cells, 12))]
    return qs


def money_sums(og, params, src):
    """The oracle's label of every cell from src (mro_sssp_all): (the labels' money, the
    sums of their commands' money) as int64 arrays, every cell found."""
    from oracle_lib import lib
    p = params.to_c()
    res = (mr_result * og.n)()
    cap = og.n * 24
    while True:
        pool = (mr_command * cap)()
        st = lib().mro_sssp_all(og.h, C.byref(p), src.to_c(), res, pool, cap)
        if st != MR_ERR_CAPACITY or cap > og.n * 4096:
            break
        cap *= 4
    assert st == MR_OK, st
    r = np.frombuffer(res, dtype=RESULT_DT, count=og.n)
    assert (r["status"] == MR_OK).all()
    acc = np.concatenate([[0], np.cumsum(np.frombuffer(pool, dtype=COMMAND_DT, count=cap)["money"].astype(np.int64))])
    off = r["command_offset"].astype(np.int64)
    return r["money"].astype(np.int64), acc[off + r["n_commands"]] - acc[off]


_oracle = {}


def oracle_answers(oracle_lib, case, which):
    """Regime A's reference for one (case, cost), computed once: {(sort_by, fleetfoot):
    the oracle's labels of queries_of(case)}, and under "max_money" the largest label
    money of any cell from any of the 24 sources.  The precondition is asserted first: from
    every source, every cell's label money equals the integer sum of its commands' money,
    and the largest of them plus the price stays below 2^32, so that neither a label nor a
    candidate wraps, in the oracle or in the engine."""
    from golden_util import as_expected
    if (case, which) not in _oracle:
        m, hq = case_map(case)
        og = oracle_lib.OracleGrid(m.cells())
        cost, qs, out, top = cost_of(case, which), queries_of(case), {}, 0
        for sort_by in ORDERS:
            for ff in FLEETFOOT:
                params = params_of(cost, sort_by, ff, hq)
                for s in sources_of(case):
                    money, sums = money_sums(og, params, s)
                    assert (money == sums).all(), f"{case} C={cost} {sort_by} ff={ff} {s}: a label's money wrapped"
                    top = max(top, int(sums.max()))
                assert top + cost < 1 << 32, f"{case} C={cost} {sort_by} ff={ff}: a candidate can pass 2^32 ({top})"
                out[(sort_by, ff)] = [as_expected(e) for e in og.find_path_batch(params, qs, threads=0)]
        out["max_money"] = top
        _oracle[(case, which)] = out
    return _oracle[(case, which)]


# ---- regime B ---------------------------------------------------------------------------
B_PRICES = [(3_000_000_000, 2_999_999_999, 2_999_999_998),
            (0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD)]  # a one-scroll label equals the kernels' "no label" mark
B_ORDERS = [(SORT_LEGS, SORT_MONEY), (SORT_MONEY, SORT_LEGS)]


def b_params(prices, sort_by):
    _, hq = case_map("A1")
    return Params(scroll_of_escape_cost=prices[0], scroll_of_escape_hq_cost=prices[1],
                  scroll_of_escape_forum_cost=prices[2], use_sfm=True, route_guru=3, hq_position=hq, sort_by=sort_by)


def b_queries():
    """40 queries from 8 sources on A1's map."""
    m, _ = case_map("A1")
    cells = m.all_indices()
    rng = random.Random(3)
    return [(s, d) for s in sources_of("A1")[:8] for d in rng.sample(cells, 5)]


def finder(case, params, wrap):
    m, _ = case_map(case)
    grid = py_ref.Grid([((c.kind, c.sub, c.x, c.y), p) for c, p in m.cells()])
    return py_ref.Finder(grid, params.to_json(), wrap=wrap)


def finder_labels(f, qs):
    """Finder.eval over qs in the form of golden_util.as_expected."""
    out = []
    for a, b in qs:
        j = py_ref.label_to_json(f.eval((a.kind, a.sub, a.x, a.y), (b.kind, b.sub, b.x, b.y)))
        out.append(None if j is None else
                   [j["legs"], j["money"], j["time_s"], [[c["kind"], c["time_s"], c["legs"], c["money"], c["fleetfoot"],
                                                          c["from"], c["to"]] for c in j["commands"]]])
    return out


_exact = {}


def exact_answers(prices, sort_by):
    """Regime B's reference, computed once per (prices, order): the exact labels of
    b_queries()."""
    if (prices, sort_by) not in _exact:
        _exact[(prices, sort_by)] = finder_labels(finder("A1", b_params(prices, sort_by), wrap=False), b_queries())
    return _exact[(prices, sort_by)]
