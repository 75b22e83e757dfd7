"""The two host references of tour plans agree: tour_ref.held_karp (the device kernel's
algorithm in Python integers) against tour_ref.brute_force (every permutation under the rule's
exact key), for every number of stops up to 7, the three end rules and the six metric orders, on
matrices whose small entries make ties the common case."""
import itertools
import random

import numpy as np
import pytest

import tour_ref as tr

ORDERS = list(itertools.permutations(range(3)))
MODES = [tr.MODE_OPEN, tr.MODE_RETURN, tr.MODE_TO_LAST]


def random_matrix(rng, n, top):
    return np.array([[[rng.randint(0, top) for _ in range(3)] for _ in range(n + 2)] for _ in range(n + 2)], dtype=np.int64)


@pytest.mark.parametrize("n", range(8))
def test_held_karp_equals_brute_force(n):
    rng = random.Random(100 + n)
    tied = 0
    # (fewer matrices where a brute force costs 5 040 permutations)
    for top in [3] * (6 if n < 6 else 2) + [1] * (4 if n < 6 else 1):
        M = random_matrix(rng, n, top)
        for mode in MODES:
            for order in ORDERS:
                cost, pi, n_best = tr.brute_force(M, mode, order)
                assert tr.held_karp(M, mode, order) == (cost, pi), (n, top, mode, order, M.tolist())
                assert sorted(pi) == list(range(n)) and n_best >= 1
                tied += n_best > 1
    # three stops or more with entries in 0..1: more than one optimal order for any seed
    assert tied > 0 or n < 3, n


def test_all_equal_matrix_gives_the_identity_order():
    for n in range(8):
        M = np.full((n + 2, n + 2, 3), 2, dtype=np.int64)
        for mode in MODES:
            L = tr.n_legs(M, mode)
            for order in ORDERS:
                cost, pi, n_best = tr.brute_force(M, mode, order)
                assert pi == list(range(n)) and cost == (2 * L, 2 * L, 2 * L)
                assert n_best == max(1, len(list(itertools.permutations(range(n)))))
                assert tr.held_karp(M, mode, order) == (cost, pi)


def test_costs_come_back_in_natural_order():
    """Distinct metrics per column: the sums are (legs, money, time) whatever the order compares
    first, and the order decides the winner."""
    M = np.zeros((4, 4, 3), dtype=np.int64)
    M[0, 1], M[1, 2] = (1, 50, 7), (1, 50, 7)   # start -> stop 0 -> stop 1: 2 legs, money 100
    M[0, 2], M[2, 1] = (2, 10, 7), (2, 10, 7)   # start -> stop 1 -> stop 0: 4 legs, money 20
    assert tr.brute_force(M, tr.MODE_OPEN, (0, 1, 2))[:2] == ((2, 100, 14), [0, 1])
    assert tr.brute_force(M, tr.MODE_OPEN, (1, 0, 2))[:2] == ((4, 20, 14), [1, 0])
    assert tr.held_karp(M, tr.MODE_OPEN, (1, 2, 0)) == ((4, 20, 14), [1, 0])


def test_limit_gate():
    M = np.zeros((5, 5, 3), dtype=np.int64)
    M[1, 2, 1] = (1 << 32) // 3            # 3 legs fit, 4 do not
    assert tr.limit_gate(M, 3) and not tr.limit_gate(M, 4)
    M[:] = 0
    M[4, 0, 2] = 1 << 31                   # the end's row counts only under MODE_TO_LAST
    assert tr.limit_gate(M, 3, tr.MODE_OPEN) and tr.limit_gate(M, 3, tr.MODE_RETURN) and not tr.limit_gate(M, 3)
    assert tr.limit_gate(M, 1)
