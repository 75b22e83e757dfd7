"""The references of the large-price tests (large_costs.py), checked on the CPU so that a
changed map generator or oracle fails here first, before any device comparison."""
import pytest

import large_costs as lc
from golden_util import as_expected
from marshrutka_amd.abi import SORT_LEGS, SORT_MONEY


@pytest.mark.parametrize("case,which", lc.CASE_COSTS, ids=[f"{c}-{w}" for c, w in lc.CASE_COSTS])
def test_regime_a_nothing_wraps(oracle_lib, case, which):
    """Regime A's precondition for every listed (case, cost): from each of the 24 sources,
    under every order and Fleetfoot level, each cell's label money is the integer sum of
    its commands' money, and the largest plus the price is below 2^32."""
    ans = lc.oracle_answers(oracle_lib, case, which)
    assert lc.cost_of(case, which) <= ans["max_money"] < 1 << 32
    assert len(lc.sources_of(case)) == len(set(lc.sources_of(case))) == 24
    per_source = {}
    for a, _ in lc.queries_of(case):
        per_source[a] = per_source.get(a, 0) + 1
    V = len(lc.case_map(case)[0].all_indices())
    assert sorted(per_source.values()) == [12] * 21 + [V] * 3
    if (case, which) == ("A2", "top"):  # the case that sets bit 31 of the money word
        hi = {k: sum(e[1] >= 1 << 31 for e in v) for k, v in ans.items() if k != "max_money"}
        # (the Time-first orders: three scrolls cost no time)
        assert sum(n >= 10 for n in hi.values()) >= 6 and ans["max_money"] >= 3_000_000_000, hi


def test_gate_cost_inputs():
    """The table sizes the cases were chosen for: A3's plain HQ makes 22 specials, A4's
    29 need the 32-entry lane table; G + 1 is the first price past the documented bound."""
    assert [lc.num_specials(c) for c in lc.CASES] == [9, 17, 22, 29]
    for c in lc.CASES:
        ns, g = lc.num_specials(c), lc.gate_cost(c)
        assert (2 * ns + 4) * g <= (1 << 32) - 2 < (2 * ns + 4) * (g + 1)


@pytest.mark.parametrize("case,which", [("A1", "G"), ("A1", "G+1"), ("A1", "top"), ("A2", "G")])
def test_exact_finder_equals_oracle_where_nothing_wraps(oracle_lib, case, which):
    """py_ref.Finder(wrap=False), regime B's reference, equals the C++ oracle on 60
    queries of regime A (where nothing wraps, so both are the reference's answer)."""
    m, hq = lc.case_map(case)
    og = oracle_lib.OracleGrid(m.cells())
    qs = lc.queries_of(case)
    qs = qs[::max(1, len(qs) // 20)][:20]
    n = 0
    for sort_by, ff in (((SORT_LEGS, SORT_MONEY), 0), ((SORT_MONEY, SORT_LEGS), 2), (lc.ORDERS[5], 2)):
        params = lc.params_of(lc.cost_of(case, which), sort_by, ff, hq)
        exp = [as_expected(e) for e in og.find_path_batch(params, qs, threads=0)]
        got = lc.finder_labels(lc.finder(case, params, wrap=False), qs)
        assert got == exp, (case, which, sort_by, ff)
        n += len(qs)
    assert n == 60


@pytest.mark.parametrize("prices", lc.B_PRICES, ids=["3e9", "2^32-1"])
def test_regime_b_reference(prices):
    """Regime B's exact labels: legs and money are the sums of the commands'; and the
    strict case exists: at price 2^32 - 1 some (Legs, Money) optimum has money >= 2^32 (a
    scroll and a caravan), where MR_ERR_LIMIT is the only correct answer.  (At 3e9 one
    scroll and the caravans stay below 2^32, and a second scroll saves no leg.)"""
    qs = lc.b_queries()
    assert len(qs) == 40 and len({a for a, _ in qs}) == 8
    for sort_by in lc.B_ORDERS:
        for e in lc.exact_answers(prices, sort_by):
            assert e[1] == sum(c[3] for c in e[3]) and e[0] == sum(c[2] for c in e[3])
    over = [e for e in lc.exact_answers(prices, (SORT_LEGS, SORT_MONEY)) if e[1] >= 1 << 32]
    if prices[0] == 0xFFFFFFFF:
        assert len(over) >= 1, "no queried optimum passes 2^32: the strict case is missing"
    print(f"prices {prices}: {len(over)} of 40 (Legs, Money) optima have money >= 2^32")
