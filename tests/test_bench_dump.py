"""bench.py --dump-outputs: the .npy files dump_outputs writes from a plan's fetched
labels (a stand-in plan with known labels; no device needed)."""
import numpy as np

import bench
from marshrutka_amd import pathfinder


class FakePlan:
    """n labels in fetch_raw's layout: label i has legs i, money 2i, time 3i, i % 5
    commands at ascending pool offsets; every 17th has no path."""

    def __init__(self, n):
        self.n = n
        self.res, self.pool = pathfinder.fetch_buffers(n, 4)
        off = 0
        for i in range(n):
            r = self.res[i]
            r.legs, r.money, r.time_s, r.n_commands, r.command_offset = i, 2 * i, 3 * i, i % 5, off
            r.status = 1 if i % 17 == 0 else 0
            for k in range(r.n_commands):
                c = self.pool[off + k]
                c.kind, c.legs, c.money, c.fleetfoot, c.time_s = k, i, k + 1, 7, -5
                c.from_.kind, c.from_.sub, c.from_.x, c.from_.y = 1, 2, i, k
                c.to.kind, c.to.sub, c.to.x, c.to.y = 2, 3, k, i
            off += r.n_commands

    def fetch_raw(self):
        return self.res, self.pool


class FakeAllPlan:
    n = 10

    def records(self, i):
        return (np.arange(1000 * 4, dtype=np.uint32) + 10000 * i).reshape(1000, 4)


def load(d, *names):
    out = [np.load(d / (n + ".npy")) for n in names]
    assert all(a.dtype == np.float64 for a in out)
    return out


def check_query_dump(q, r, c, n):
    i = q.astype(int)
    found = i % 17 != 0
    assert (r[:, 4] == np.where(found, 0, 1)).all()
    assert (r[:, :4] == np.where(found[:, None], np.stack([i, 2 * i, 3 * i, i % 5], axis=1), 0)).all()
    row = c[:, 0].astype(int)
    assert (np.diff(row) >= 0).all()
    k = np.concatenate([np.arange(m) for m in np.where(found, i % 5, 0)])[:len(c)]
    src = i[row]
    exp = np.stack([row, k, src, k + 1, 0 * k + 7, 0 * k - 5, 0 * k + 1, 0 * k + 2, src, k, 0 * k + 2, 0 * k + 3, k, src],
                   axis=1)
    assert (c == exp).all()
    return len(k)


def test_dump_whole_batch(tmp_path):
    n = 3000
    bench.dump_outputs(str(tmp_path), FakePlan(n), False, 0)
    q, r, c = load(tmp_path, "queries", "results", "commands")
    assert (q == np.arange(n)).all() and r.shape == (n, 5) and c.shape[1] == 14
    assert check_query_dump(q, r, c, n) == len(c) == sum(i % 5 for i in range(n) if i % 17)


def test_dump_sample_is_fixed(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_QUERIES", 50)
    monkeypatch.setattr(bench, "DUMP_COMMANDS", 60)
    plan = FakePlan(3000)
    bench.dump_outputs(str(tmp_path / "a"), plan, False, 0)
    bench.dump_outputs(str(tmp_path / "b"), plan, False, 0)
    q, r, c = load(tmp_path / "a", "queries", "results", "commands")
    assert len(q) == 50 and len(np.unique(q)) == 50 and (np.diff(q) > 0).all() and len(c) == 60
    check_query_dump(q, r, c, 3000)
    for x, y in zip((q, r, c), load(tmp_path / "b", "queries", "results", "commands")):
        assert np.array_equal(x, y)


def test_dump_all_destinations(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_CELLS", 100)
    plan = FakeAllPlan()
    bench.dump_outputs(str(tmp_path), plan, True, 1000)
    s, cell, rec = load(tmp_path, "sources", "cells", "records")
    assert len(s) == bench.DUMP_SOURCES and len(cell) == 100 and rec.shape == (len(s), 100, 4)
    for j, i in enumerate(s.astype(int)):
        assert (rec[j] == plan.records(i)[cell.astype(int)]).all()
