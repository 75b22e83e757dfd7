"""The numpy reference of nearest-source plans (nearest_src_ref.reduce_sources) against a plain
Python double loop, on random matrices with entries in 0..2 so that ties on all three metrics are
common: all six metric orders, both modes, empty groups."""
import itertools
import random

import numpy as np
import pytest

import nearest_src_ref as ns

ORDERS = list(itertools.permutations(range(3)))


def random_case(seed, n_src, n_dst, n_groups, empty=()):
    rng = random.Random(seed)
    M = np.array([[[rng.randint(0, 2) for _ in range(3)] + [rng.randrange(1 << 32)] for _ in range(n_dst)]
                  for _ in range(n_src)], dtype=np.uint32)
    live = [g for g in range(n_groups) if g not in empty]
    groups = [rng.choice(live) for _ in range(n_src)]
    return M, groups


@pytest.mark.parametrize("worst", [False, True])
@pytest.mark.parametrize("order", ORDERS)
def test_reference_equals_the_double_loop(order, worst):
    assert len(ORDERS) == 6
    for seed, (n_src, n_dst, n_groups, empty) in enumerate([(1, 1, 1, ()), (7, 5, 1, ()), (40, 9, 3, ()), (40, 6, 5, (0, 3)),
                                                            (13, 4, 4, (3,))]):
        M, groups = random_case(100 * seed + ORDERS.index(order), n_src, n_dst, n_groups, empty)
        got = ns.reduce_sources(M, groups, n_groups, order, worst)
        want = ns.reduce_sources_loops(M, groups, n_groups, order, worst)
        assert got.shape == (n_dst, n_groups, 5) and got.dtype == np.uint32
        assert (got == want).all(), (seed, order, worst)
        for g in empty:
            assert (got[:, g] == (0, 0, 0, 0, ns.NONE)).all()
        if n_groups == 1:
            assert (ns.reduce_sources(M, None, 1, order, worst) == ns.reduce_sources(M, [0] * n_src, 1, order, worst)).all()


def test_ties_keep_the_smallest_position_in_both_modes():
    M = np.zeros((6, 3, 4), dtype=np.uint32)
    M[:, :, :3] = 1
    M[:, :, 3] = np.arange(6)[:, None]  # via tells the rows apart
    for worst in (False, True):
        rec = ns.reduce_sources(M, [1, 0, 1, 0, 0, 1], 2, (0, 1, 2), worst)
        assert (rec[:, 0, 4] == 1).all() and (rec[:, 1, 4] == 0).all()
        assert (rec[:, 0, 3] == 1).all() and (rec[:, 1, 3] == 0).all()
        assert (rec == ns.reduce_sources_loops(M, [1, 0, 1, 0, 0, 1], 2, (0, 1, 2), worst)).all()
    # the modes differ where the keys do; the large words compare as unsigned
    M[2, :, 1] = 0xFFFFFFF0
    assert (ns.reduce_sources(M, None, 1, (1, 0, 2), True)[:, 0, 4] == 2).all()
    assert (ns.reduce_sources(M, None, 1, (1, 0, 2), False)[:, 0, 4] == 0).all()


def test_rally_takes_the_least_worst_member():
    M = np.zeros((3, 4, 4), dtype=np.uint32)
    M[:, :, 0] = [[5, 2, 2, 9], [1, 2, 1, 9], [3, 1, 2, 0]]  # the worst per candidate: 5, 2, 2, 9
    j, rec = ns.rally(M, (0, 1, 2))
    assert j == 1 and rec[0] == 2 and rec[4] == 0  # candidates 1 and 2 tie: the smaller j; members 0 and 1 tie: member 0
