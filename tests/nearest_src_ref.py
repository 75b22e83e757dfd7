"""A numpy reference of nearest-source plans (DESIGN.md section 3b'''''): the reduction of a cost
matrix over each destination's sources, by group.

M is an (n_src, n_dst, 4) array of matrix records (legs, money, time, via).  For destination j and
group g the winner is the source i of the group with the least (worst=False) or the greatest
(worst=True) (M[i, j, q0], M[i, j, q1], M[i, j, q2]), `order` = (q0, q1, q2); ties on all three go to
the smallest i in both modes.  The record is M[winner, j] and the winner's position; an empty group
reads (0, 0, 0, 0, NONE)."""
import numpy as np

NONE = 0xFFFFFFFF


def reduce_sources(M, groups, n_groups, order, worst=False):
    """(n_dst, n_groups, 5) uint32: legs, money, time, via, position of the winner."""
    M = np.asarray(M)
    n_src, n_dst = M.shape[:2]
    groups = np.zeros(n_src, dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    out = np.zeros((n_dst, n_groups, 5), dtype=np.uint32)
    out[:, :, 4] = NONE
    for g in range(n_groups):
        idx = np.nonzero(groups == g)[0]
        if not idx.size:
            continue
        m = M[idx].astype(np.int64)  # (n_g, n_dst, 4)
        sign = -1 if worst else 1
        # lexsort: the last key is the primary one; the position ascends in both modes
        keys = (np.broadcast_to(idx[:, None], m.shape[:2]), sign * m[:, :, order[2]], sign * m[:, :, order[1]],
                sign * m[:, :, order[0]])
        win = idx[np.lexsort(keys, axis=0)[0]]  # (n_dst,)
        out[:, g, :4] = M[win, np.arange(n_dst)]
        out[:, g, 4] = win
    return out


def reduce_sources_loops(M, groups, n_groups, order, worst=False):
    """The same by a plain double loop over Python integers: a strict compare in ascending source
    order, so the earliest of equals stays."""
    n_src, n_dst = len(M), len(M[0])
    out = [[(0, 0, 0, 0, NONE) for _ in range(n_groups)] for _ in range(n_dst)]
    for j in range(n_dst):
        for g in range(n_groups):
            best = None
            for i in range(n_src):
                if (0 if groups is None else int(groups[i])) != g:
                    continue
                r = [int(x) for x in M[i][j]]
                key = (r[order[0]], r[order[1]], r[order[2]])
                if best is None or (key > best[0] if worst else key < best[0]):
                    best = (key, tuple(r[:4]) + (i,))
            if best is not None:
                out[j][g] = best[1]
    return np.array(out, dtype=np.uint32).reshape(n_dst, n_groups, 5)


def rally(M, order):
    """(j, record): the candidate j with the least (m[q0], m[q1], m[q2], j) of its worst member."""
    rec = reduce_sources(M, None, 1, order, worst=True)[:, 0, :]
    j = min(range(rec.shape[0]), key=lambda c: (int(rec[c, order[0]]), int(rec[c, order[1]]), int(rec[c, order[2]]), c))
    return j, rec[j]
