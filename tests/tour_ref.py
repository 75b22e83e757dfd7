"""Host references for tour plans (mr_tour_plan_create; DESIGN.md section 3b'''').

A tour's legs are given as M, an (n + 2, n + 2, 3) integer array: index 0 is the start, 1..n are
the stops (stop position k is index 1 + k), n + 1 is the fixed end of MODE_TO_LAST (ignored under
the other modes); M[i, j] = (legs, money, time) of the leg i -> j.  `order` is the plan's metric
order as columns of M (test_gpu_nearest.plan_order).

The rule: the cost of a visiting order pi is the component-wise sum of its legs; the answer is
the pi with the least (m[order[0]], m[order[1]], m[order[2]], pi[0], .., pi[n-1]).  Everything
here is in Python integers, so nothing wraps."""
import itertools

MODE_OPEN, MODE_RETURN, MODE_TO_LAST = 0, 1, 2
LIMIT = (1 << 32) - 1


def n_stops(M):
    return len(M) - 2


def n_legs(M, mode):
    return n_stops(M) + (0 if mode == MODE_OPEN else 1)


def _leg(M, i, j, order):
    return tuple(int(M[i][j][q]) for q in order)


def _add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def _last_leg(M, mode, cur, order):
    """The end rule from cell index `cur`: nothing, back to the start, or on to the end."""
    if mode == MODE_OPEN:
        return (0, 0, 0)
    return _leg(M, cur, 0 if mode == MODE_RETURN else len(M) - 1, order)


def _natural(key, order):
    """(legs, money, time) of a cost held in comparator order."""
    out = [0, 0, 0]
    for i, q in enumerate(order):
        out[q] = key[i]
    return tuple(out)


def brute_force(M, mode, order):
    """((legs, money, time), the winning order as a list of stop positions, the number of
    optimal orders) over every permutation, with the exact key of the rule."""
    n = n_stops(M)
    M = M.tolist() if hasattr(M, "tolist") else M
    best, n_best = None, 0
    for pi in itertools.permutations(range(n)):
        cost, cur = (0, 0, 0), 0
        for k in pi:
            cost = _add(cost, _leg(M, cur, 1 + k, order))
            cur = 1 + k
        cost = _add(cost, _last_leg(M, mode, cur, order))
        if best is None or cost < best[0]:
            n_best = 0
        if best is None or (cost, pi) < best:
            best = (cost, pi)
        n_best += cost == best[0]
    return _natural(best[0], order), list(best[1]), n_best


def held_karp(M, mode, order):
    """((legs, money, time), the winning order): the backward subset DP E[S][j] = least cost of
    finishing from stop j with the stops S still to visit, then the forward walk that takes the
    smallest position whose leg plus remainder is the least."""
    n = n_stops(M)
    M = M.tolist() if hasattr(M, "tolist") else M
    E = {}
    by_size = sorted(range(1 << n), key=lambda s: bin(s).count("1"))
    for S in by_size:
        for j in range(n):
            if S >> j & 1:
                continue
            if S == 0:
                E[S, j] = _last_leg(M, mode, 1 + j, order)
            else:
                E[S, j] = min(_add(_leg(M, 1 + j, 1 + k, order), E[S & ~(1 << k), k]) for k in range(n) if S >> k & 1)
    cur, S, total, pi = 0, (1 << n) - 1, (0, 0, 0), []
    while S:
        cands = [(_add(_leg(M, cur, 1 + k, order), E[S & ~(1 << k), k]), k) for k in range(n) if S >> k & 1]
        _, k = min(cands)
        total = _add(total, _leg(M, cur, 1 + k, order))
        pi.append(k)
        cur, S = 1 + k, S & ~(1 << k)
    total = _add(total, _last_leg(M, mode, cur, order))
    return _natural(total, order), pi


def limit_gate(M, L, mode=MODE_TO_LAST):
    """True if the tour is answered: for each metric, L x the largest value over all ordered
    pairs of the tour's listed cells fits 32 bits.  (The end index is a listed cell only under
    MODE_TO_LAST.)"""
    c = len(M) if mode == MODE_TO_LAST else len(M) - 1
    return all(L * max(int(M[i][j][q]) for i in range(c) for j in range(c)) <= LIMIT for q in range(3))
