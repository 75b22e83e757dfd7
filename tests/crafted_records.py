"""Crafted compact records: random command chains of every kind with exact metrics.

Real labels are a handful of commands long (runs of StandardMoves merge), so the record
decoders and the wire encoder never see a long label from a real pass.  This module makes
the records a pass could have written for labels of any length up to max_cmds and beyond
(the overflow pool), in every layout that carries them:

    compact records   res (n, 4) u32, slots (n, max_cmds, 4) u32, ovf (*, 4) u32
                      (mr_plan_device_outputs / mr_decode_records)
    wire rows         rows (n, 1 + 2 max_cmds) u32, wpool (*, 2) u32
                      (mr_plan_wire_records / mr_decode_wire; max_cmds <= 63 only)

and the labels they stand for, which are the reference: metrics summed in Python integers,
the Fleetfoot time of a StandardMove run as a Fraction's ceiling, nothing taken from the
library.  A chain keeps from[j] == to[j-1], kinds 1..6, ranks < V, and payloads small
enough that 4096 commands sum to less than 2^30 in legs and time.  Money is the one metric
a caller's prices can push to the top of 32 bits: with max_scrolls a record holds at most
that many scrolls, so prices above 2^30 give label money past 2^31 and still below 2^32.
"""
from fractions import Fraction

import numpy as np

from marshrutka_amd.abi import MR_ERR_INVALID_INDEX, MR_NOT_FOUND, MR_OK

# Fleetfoot ratios (levels past 3 have none) and seconds per caravan distance unit
# (ceil(240 * the RouteGuru ratio)), as tests/test_abi.py has always spelled them
FLEETFOOT = {0: Fraction(1), 1: Fraction(50, 53), 2: Fraction(100, 109), 3: Fraction(25, 28)}
CARAVAN_UNIT = {0: 240, 1: 190, 2: 168, 3: 146, 4: 124, 5: 102}
MAX_CENTRAL, MAX_STANDARD, MAX_CARAVAN = 20, 400, 600  # payload bounds

# prices that put a label's money past 2^31 with three scrolls (4.2e9, below 2^32 with 4096
# caravans of at most 3000 on top): craft(..., max_scrolls=LARGE_MONEY_SCROLLS)
LARGE_MONEY_PRICES = dict(scroll_of_escape_cost=1_400_000_000, scroll_of_escape_hq_cost=1_399_999_999,
                          scroll_of_escape_forum_cost=1_399_999_998)
LARGE_MONEY_SCROLLS = 3

ST_OK, ST_NOT_FOUND, ST_OVERFLOW = 16 << 16, 17 << 16, 80 << 16  # the records' status half-word
OVF_TAG = 0xFFFFFFFF
WIRE_RANK_BITS, WIRE_OVF, WIRE_STATUS = 25, 64, 65

CELL_DT = np.dtype([("kind", "u1"), ("sub", "u1"), ("x", "<u2"), ("y", "<u2"), ("reserved", "<u2")])
COMMAND_DT = np.dtype([("kind", "u1"), ("reserved", "u1", (3,)), ("legs", "<u4"), ("money", "<u4"), ("fleetfoot", "<u4"),
                       ("time_s", "<i8"), ("from_", CELL_DT), ("to", CELL_DT)])
RESULT_DT = np.dtype([("legs", "<u4"), ("money", "<u4"), ("time_s", "<i8"), ("n_commands", "<u4"),
                      ("command_offset", "<u4"), ("status", "<i4"), ("reserved", "<u4")])
assert COMMAND_DT.itemsize == 40 and RESULT_DT.itemsize == 32


def edge_lengths(max_cmds, overflow):
    """The command counts every case holds: exactly max_cmds, none, one, max_cmds - 1, the
    counts round the wire header's 7-bit code (63, 64, 65) once max_cmds reaches it, and,
    with an overflow pool, one command more than the slots take."""
    want = [max_cmds, 0, 1, max_cmds - 1] + ([63, 64, 65] if max_cmds >= 64 else []) + [max_cmds + 1]
    out = []
    for c in want:
        if c >= 0 and (overflow or c <= max_cmds) and c not in out:
            out.append(c)
    return out


def cells_by_rank(m):
    """(V, 4) array: the CellIndex (kind, sub, x, y) of each rank (the derived Ord,
    src/index.rs:41-46), which is how compact commands name cells."""
    cells = sorted(m.all_indices(), key=lambda c: (c.kind, c.sub, c.x, c.y))
    return np.array([(c.kind, c.sub, c.x, c.y) for c in cells], dtype=np.int64)


def decoded_labels(results, pool, n, cells):
    """What a decoder wrote (an mr_result array of n entries and its mr_command pool, ctypes
    or numpy) in the form of Crafted.labels(); an entry whose status is neither OK nor
    NOT_FOUND reads as that status."""
    r = np.frombuffer(results, dtype=RESULT_DT, count=n)
    used = int((r["command_offset"].astype(np.int64) + r["n_commands"])[r["status"] == MR_OK].max(initial=0))
    p = np.frombuffer(pool, dtype=COMMAND_DT, count=used)
    rank = {tuple(c): i for i, c in enumerate(cells.tolist())}
    cell = lambda a: [rank[t] for t in zip(a["kind"].tolist(), a["sub"].tolist(), a["x"].tolist(), a["y"].tolist())]  # noqa: E731
    cmds = list(zip(p["kind"].tolist(), cell(p["from_"]), cell(p["to"]), p["time_s"].tolist(), p["legs"].tolist(),
                    p["money"].tolist(), p["fleetfoot"].tolist()))
    out = []
    for k in range(n):
        st, a, nc = int(r["status"][k]), int(r["command_offset"][k]), int(r["n_commands"][k])
        if st == MR_OK:
            out.append((int(r["legs"][k]), int(r["money"][k]), int(r["time_s"][k]), cmds[a:a + nc]))
        else:
            out.append(None if st == MR_NOT_FOUND else st)
    return out


def assert_same_bytes(got_results, got_pool, want_results, want_pool, what):
    """The decoder's arrays against Crafted.pack()'s: every mr_result field, then the
    command pool up to the total byte for byte (the first difference is named)."""
    n, total = len(want_results), len(want_pool)
    r = np.frombuffer(got_results, dtype=RESULT_DT, count=n)
    for f in RESULT_DT.names:
        bad = np.flatnonzero(r[f] != want_results[f])
        assert bad.size == 0, f"{what}: result {bad[0]} {f} = {r[f][bad[0]]}, expected {want_results[f][bad[0]]}"
    p = np.frombuffer(got_pool, dtype=np.uint8, count=total * COMMAND_DT.itemsize).reshape(total, -1)
    bad = np.flatnonzero((p != want_pool.view(np.uint8).reshape(total, -1)).any(axis=1))
    assert bad.size == 0, f"{what}: command {bad[0]} of the pool differs ({bad.size} do)"


class Crafted:
    """n crafted records (see craft()).  Per record k: found[k], ncmd[k], start[k] (its
    first command in the flat per-command arrays kind / pay / frm / to and c_time / c_legs /
    c_money / c_ff, the fields of the mr_command each expands to)."""

    def labels(self):
        """The reference: per record None (NOT_FOUND) or (legs, money, time_s,
        [(kind, from rank, to rank, time_s, legs, money, fleetfoot), ...])."""
        cmds = list(zip(self.kind.tolist(), self.frm.tolist(), self.to.tolist(), self.c_time.tolist(),
                        self.c_legs.tolist(), self.c_money.tolist(), self.c_ff.tolist()))
        out = []
        for k in range(self.n):
            a, b = int(self.start[k]), int(self.start[k] + self.ncmd[k])
            out.append((self.legs[k], self.money[k], self.time_s[k], cmds[a:b]) if self.found[k] else None)
        return out

    def pack(self, cells, order=None):
        """The labels as the ABI lays them out when entry i holds record order[i] (-1: a
        query without a record, MR_ERR_INVALID_INDEX): the mr_result array, the mr_command
        pool (entry i's commands at the sum of the counts before it) and the status a
        decoder returns when the pool is long enough (the first error in entry order)."""
        order = np.arange(self.n) if order is None else np.asarray(order, dtype=np.int64)
        has = order >= 0
        rec = np.where(has, order, 0)
        nc = np.where(has, self.ncmd[rec], 0)
        res = np.zeros(len(order), dtype=RESULT_DT)
        res["legs"] = np.where(has, np.array(self.legs, dtype=np.int64)[rec], 0)
        res["money"] = np.where(has, np.array(self.money, dtype=np.int64)[rec], 0)
        res["time_s"] = np.where(has, np.array(self.time_s, dtype=np.int64)[rec], 0)
        res["n_commands"] = nc
        res["command_offset"] = np.where(has, np.cumsum(nc) - nc, 0)
        res["status"] = np.where(has, np.where(self.found[rec], MR_OK, MR_NOT_FOUND), MR_ERR_INVALID_INDEX)
        total = int(nc.sum())
        src = np.repeat(self.start[rec], nc) + (np.arange(total) - np.repeat(np.cumsum(nc) - nc, nc))
        pool = np.zeros(total, dtype=COMMAND_DT)
        pool["kind"] = self.kind[src]
        pool["legs"], pool["money"], pool["fleetfoot"] = self.c_legs[src], self.c_money[src], self.c_ff[src]
        pool["time_s"] = self.c_time[src]
        for name, rank in (("from_", self.frm[src]), ("to", self.to[src])):
            for j, f in enumerate(("kind", "sub", "x", "y")):
                pool[name][f] = cells[rank, j]
        return res, pool, (MR_OK if has.all() else MR_ERR_INVALID_INDEX)


def craft(n, max_cmds, lengths, V, params, seed, overflow=True, not_found=None, max_scrolls=None):
    """n records for a plan of max_cmds command slots over a grid of V cells.

    lengths: the command counts to draw from, uniformly.  Whatever it holds, the counts of
    edge_lengths() come first (as many as n has room for), at random records.  overflow:
    counts above max_cmds are kept and go to the overflow pool / wire pool; without it
    they are cut to max_cmds (a test that cannot write a plan's pool).  not_found: how many
    records are NOT_FOUND (default: n / 20, at least 3 where n has room).  max_scrolls: at
    most that many commands of kinds 4..6 (the scrolls, whose money is the caller's price)
    in a record; the scrolls past them are redrawn from kinds 1..3."""
    rng = np.random.default_rng(seed)
    edges = edge_lengths(max_cmds, overflow)[:n]
    if not_found is None:
        not_found = min(max(3, n // 20), n - len(edges))
    where = rng.permutation(n)
    ncmd = rng.choice(np.asarray(list(lengths), dtype=np.int64), size=n)
    if not overflow:
        ncmd = np.minimum(ncmd, max_cmds)
    ncmd[where[:len(edges)]] = edges
    found = np.ones(n, dtype=bool)
    found[where[len(edges):len(edges) + not_found]] = False
    ncmd[~found] = 0
    assert int(ncmd.sum()) <= 100_000, "keep a case under 1e5 crafted commands"
    start = np.cumsum(ncmd) - ncmd
    T = int(ncmd.sum())

    # the chains: a kind, its payload, the cell each command ends in
    kind = rng.integers(1, 7, T)
    if max_scrolls is not None:  # (a generator of its own: the other draws stay what they were)
        is_scroll = kind >= 4
        seen = np.cumsum(is_scroll)
        nth = seen - np.repeat((seen - is_scroll)[start[ncmd > 0]], ncmd[ncmd > 0])  # within its record
        extra = is_scroll & (nth > max_scrolls)
        kind[extra] = np.random.default_rng([seed, 1]).integers(1, 4, int(extra.sum()))
    d = rng.integers(1, MAX_CARAVAN + 1, T)
    five = rng.integers(0, 2, T)
    pay = np.select([kind == 1, kind == 2, kind == 3],
                    [rng.integers(1, MAX_CENTRAL + 1, T), rng.integers(1, MAX_STANDARD + 1, T), d << 1 | five], 0)
    to = rng.integers(0, V, T)
    first = rng.integers(0, V, n)
    frm = np.empty(T, dtype=np.int64)
    frm[1:] = to[:-1]
    frm[start[ncmd > 0]] = first[ncmd > 0]

    # what each command expands to (mr_command) and what it adds to the label's time: a
    # StandardMove run's Fleetfoot ceiling, by Fraction, tabulated per run length
    ratio = FLEETFOOT.get(params.fleetfoot, Fraction(1))
    run_time = np.array([-((-ratio * 180 * p).numerator // (ratio * 180 * p).denominator)
                         for p in range(MAX_STANDARD + 1)], dtype=np.int64)
    unit = CARAVAN_UNIT[params.route_guru]
    scroll = {4: params.scroll_of_escape_cost, 5: params.scroll_of_escape_hq_cost, 6: params.scroll_of_escape_forum_cost}
    c_time = np.select([kind == 1, kind == 2, kind == 3], [10 * pay, 180 * pay, unit * d], 0)
    l_time = np.where(kind == 2, run_time[np.where(kind == 2, pay, 0)], c_time)
    c_legs = np.where(kind == 2, pay, 0)
    c_money = np.select([kind == 3, kind == 4, kind == 5, kind == 6],
                        [d * np.where(five == 1, 5, 2), scroll[4], scroll[5], scroll[6]], 0)
    c_ff = np.where(kind == 2, params.fleetfoot, 0)

    c = Crafted()
    c.n, c.max_cmds, c.V = n, max_cmds, V
    c.found, c.ncmd, c.start = found, ncmd, start
    c.kind, c.pay, c.frm, c.to = kind, pay, frm, to
    c.c_time, c.c_legs, c.c_money, c.c_ff = c_time, c_legs, c_money, c_ff
    c.legs, c.money, c.time_s = [], [], []
    for k in range(n):  # the labels' metrics: Python integers
        a, b = int(start[k]), int(start[k] + ncmd[k])
        c.legs.append(sum(c_legs[a:b].tolist()))
        c.money.append(sum(c_money[a:b].tolist()))
        c.time_s.append(sum(l_time[a:b].tolist()))
    assert max(c.legs + c.time_s + [0]) < 1 << 30 and max(c.money + [0]) < 1 << 32

    # the layouts.  A compact command: {kind << 29 | payload, from, to, 0}
    kp = (kind << 29 | pay).astype(np.uint32)
    cmd4 = np.stack([kp, frm.astype(np.uint32), to.astype(np.uint32), np.zeros(T, dtype=np.uint32)], axis=1)
    cmd2 = cmd4[:, [0, 2]]
    res = np.zeros((n, 4), dtype=np.uint32)
    slots = np.zeros((n, max_cmds, 4), dtype=np.uint32)
    # (the wire header counts in-slot commands in a 7-bit code: no rows from max_cmds 64 up)
    wire = max_cmds < WIRE_OVF
    rows = np.zeros((n, 1 + 2 * max_cmds) if wire else (0, 0), dtype=np.uint32)
    ovf, wpool, novf = [], [], 0
    for k in range(n):
        a, nc = int(start[k]), int(ncmd[k])
        if not found[k]:
            res[k, 3] = ST_NOT_FOUND
            if wire:
                rows[k, 0] = (WIRE_STATUS + 32 + MR_NOT_FOUND) << WIRE_RANK_BITS
            continue
        res[k] = [c.legs[k], c.money[k], c.time_s[k], ST_OK | nc]
        if nc <= max_cmds:
            slots[k, :nc] = cmd4[a:a + nc]
            if wire:
                rows[k, 0] = (int(first[k]) if nc else 0) | nc << WIRE_RANK_BITS
                rows[k, 1:1 + 2 * nc] = cmd2[a:a + nc].reshape(-1)
        else:  # in the pools, at the same offset in both
            res[k, 3] = ST_OVERFLOW | nc
            slots[k, 0] = [OVF_TAG, novf, nc, 0]
            if wire:
                rows[k, 0] = int(first[k]) | WIRE_OVF << WIRE_RANK_BITS
                rows[k, 1:3] = [novf, nc]
            ovf.append(cmd4[a:a + nc])
            wpool.append(cmd2[a:a + nc])
            novf += nc
    c.res, c.slots, c.rows = res, slots, rows
    c.ovf = np.concatenate(ovf) if ovf else np.zeros((0, 4), dtype=np.uint32)
    c.wpool = np.concatenate(wpool) if wpool else np.zeros((0, 2), dtype=np.uint32)
    return c
