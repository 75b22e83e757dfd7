"""The premise of the lane memo's winner table (DESIGN.md section 3a'''), on the CPU oracle
alone: where the memo's gate holds, the best boundary walk into a plain cell depends on a
plain source only through its SoE region.  For every region r and every plain destination
w, the labels from all plain sources of r are each either the single direct walk, or end in
StandardMove(b -> w) with one and the same b, and agree in every command after the first
(the first starts at the source's own cell).  So one table entry per (r, w) names the
boundary, and a source adds only its own walk as a second candidate."""
import numpy as np
import pytest

from marshrutka_amd.abi import CMD_STANDARD, SORT_LEGS, SORT_TIME, Params
from marshrutka_amd.mapgen import SyntheticMap
from oracle_raw import labels_raw

MAPS = {"seed7_cf4": (21, 7, 4), "seed11_cf3": (21, 11, 3)}
ORDERS = {"default": None, "legs_time": (SORT_LEGS, SORT_TIME)}  # (both lead with Legs: the gate's orders)


@pytest.fixture(scope="module")
def worlds(oracle_lib):
    out = {}
    for name, (size, seed, cf) in MAPS.items():
        m = SyntheticMap(size, campfires_per_homeland=cf, seed=seed)
        arr = m.cells_array()
        og = oracle_lib.OracleGrid.from_array(arr)
        S, H = m.size, m.h
        center = H * S + H
        specials = {center, center - 1, center + 1, center - S, center + S} | {m.cell_of(c) for c in m.campfires()}
        out[name] = (m, arr, og, [v for v in range(S * S) if v not in specials])
    return out


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("world", sorted(MAPS))
def test_best_boundary_depends_on_the_region_only(oracle_lib, worlds, world, order):
    m, arr, og, plain = worlds[world]
    p = Params() if ORDERS[order] is None else Params(sort_by=ORDERS[order])
    regions = {}
    for s in plain:
        regions.setdefault(str(og.nearest_campfire(s, p.homeland)), []).append(s)
    assert len(regions) == MAPS[world][2] and "None" not in regions
    n = len(plain)
    to_bytes = m.query_array(plain, plain, arr)["to"].tobytes()  # (8 B a cell: kind, sub, x, y, 2 reserved)
    bad, walks, tails_seen = [], 0, 0
    for r, sources in sorted(regions.items()):
        src = np.repeat(np.array(sources), n)
        dst = np.tile(np.array(plain), len(sources))
        res, cmds = labels_raw(oracle_lib, og, p, m.query_array(src, dst, arr))
        keep = src != dst
        assert (res["status"][keep] == 0).all() and (res["n"][keep] >= 1).all()
        last = cmds[(res["off"] + res["n"] - 1)[keep]]
        # every label ends in a StandardMove into the destination
        assert (last[:, 0] == CMD_STANDARD).all()
        assert last[:, 32:40].tobytes() == b"".join(to_bytes[8 * j:8 * j + 8] for j in np.nonzero(keep)[0] % n)
        for j, w in enumerate(plain):
            tails = set()
            for i in range(len(sources)):
                k = i * n + j
                nc, off = int(res["n"][k]), int(res["off"][k])
                if sources[i] == w or nc == 1:  # the source itself; the source's own walk
                    walks += nc == 1
                    continue
                tails.add(cmds[off + 1:off + nc].tobytes())  # (the last of them: StandardMove(b -> w))
            tails_seen += len(tails)
            if len(tails) > 1:
                bad.append((r, w, len(tails)))
    assert not bad, f"{len(bad)} (region, destination) pairs with more than one boundary tail; first {bad[0]}"
    assert walks > 0 and tails_seen > 0  # (both kinds of label occur)
