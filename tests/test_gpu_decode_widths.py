"""The record decoders and the wire encoder (csrc/mr_k_decode.hip) at wide max_cmds.

Real labels are a handful of commands long, so a pass never fills wide command slots and
oracle parity cannot see what these kernels do with a long label.  The compact outputs
live in caller-visible device memory and every fetch route reads them afresh, so the
tests here run a pass, overwrite its records with crafted ones (crafted_records.py:
chains of 0 .. max_cmds commands with exact metrics) and read the labels back through
every route: the host decoder, the device decoder (pageable and page-locked arrays), the
wire fetch and mr_plan_wire_records + mr_decode_wire.  Each must give the crafted labels,
and the host decoder's bytes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from crafted_records import (LARGE_MONEY_PRICES, LARGE_MONEY_SCROLLS, WIRE_RANK_BITS, WIRE_STATUS, assert_same_bytes,
                             cells_by_rank, craft, decoded_labels, edge_lengths)
from golden_util import as_expected
from marshrutka_amd.abi import (BLUE, MR_ERR_CAPACITY, MR_ERR_INVALID_ARG, MR_ERR_INVALID_INDEX, MR_NOT_FOUND, MR_OK,
                                SORT_LEGS, SORT_MONEY, SORT_TIME, CellIndex, Params, mr_command, mr_result)
from marshrutka_amd.mapgen import SyntheticMap, random_queries

pytestmark = pytest.mark.gpu

H2D, D2H = 1, 2  # hipMemcpyKind
WIRE_MAX_CMDS = 63  # the wire header's 7-bit code: in-slot counts 0 .. 63
PARAMS = [Params(),
          Params(fleetfoot=2, sort_by=(SORT_TIME, SORT_MONEY), route_guru=3, scroll_of_escape_cost=7,
                 scroll_of_escape_hq_cost=11, scroll_of_escape_forum_cost=13),
          # three scrolls a record at 1.4e9 each: label money up to 4.2e9, bit 31 set
          Params(fleetfoot=1, sort_by=(SORT_MONEY, SORT_LEGS), route_guru=2, **LARGE_MONEY_PRICES)]
# n: 65 is one past a 64-thread workgroup, 257 one past a 256-thread one, 600 a multiple
# of neither; 4096 slots with a few full-length labels only
CASES = [(mc, n) for mc in (31, 32, 63, 64, 128) for n in (1, 65, 257, 600)] + [(4096, 65)]
# the large-money set once per shape of the wire encoder and of the device decoder
MONEY_CASES = [(31, 257), (32, 600), (63, 65), (64, 257), (128, 65), (4096, 65)]
OUTSIDE = (CellIndex.center(), CellIndex.homeland(BLUE, 99, 99))  # names no cell of the grid


@pytest.fixture(scope="module")
def eng():
    from marshrutka_amd import build, pathfinder
    build.build()
    if not pathfinder.device_available():
        pytest.fail("no gfx950 device visible to the GPU tests")
    return pathfinder


@pytest.fixture(scope="module")
def hip():
    # device buffers from the HIP runtime the engine library runs on
    h = C.CDLL("libamdhip64.so.7")
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipFree.argtypes = [C.c_void_p]
    return h


class DeviceWords:
    """nw zeroed 32-bit words of device memory."""

    def __init__(self, hip, nw):
        self.hip, self.nw, self.ptr = hip, nw, C.c_void_p()
        assert hip.hipMalloc(C.byref(self.ptr), max(nw, 1) * 4) == 0
        self.zero()

    def zero(self):
        assert self.hip.hipMemset(self.ptr, 0, max(self.nw, 1) * 4) == 0

    def read(self):
        host = np.zeros(self.nw, dtype=np.uint32)
        assert self.hip.hipMemcpy(host.ctypes.data, self.ptr, self.nw * 4, D2H) == 0
        return host

    def free(self):
        self.hip.hipFree(self.ptr)


def _upload(hip, dst, arr):
    arr = np.ascontiguousarray(arr)
    if arr.nbytes:
        assert hip.hipMemcpy(C.c_void_p(dst), arr.ctypes.data, arr.nbytes, H2D) == 0


def _clear_env(monkeypatch):
    for v in ("MR_HOST_DECODE", "MR_FETCH_WIRE", "MR_DEV_GROUP", "MR_GRID_STATE", "MR_ALGO"):
        monkeypatch.delenv(v, raising=False)


@pytest.mark.parametrize("mc,n,params,max_scrolls",
                         [(mc, n, PARAMS[i % 2], None) for i, (mc, n) in enumerate(CASES)]
                         + [(mc, n, PARAMS[2], LARGE_MONEY_SCROLLS) for mc, n in MONEY_CASES],
                         ids=[f"mc{mc}-n{n}-{'ff2' if i % 2 else 'default'}" for i, (mc, n) in enumerate(CASES)]
                         + [f"mc{mc}-n{n}-money4.2e9" for mc, n in MONEY_CASES])
def test_fetch_routes_decode_crafted_records(eng, hip, monkeypatch, mc, n, params, max_scrolls):
    """n crafted records (and 3 queries outside the grid: rows past the records) at
    max_cmds mc, through every route.  launch_wire runs 256 threads a workgroup up to
    mc 31 (64 512 B of LDS at 31, its largest request) and 64 up to 63; above that the
    wire format has no in-slot code, so wire_records refuses the plan and the
    MR_FETCH_WIRE=1 fetch decodes on the device."""
    _clear_env(monkeypatch)
    m = SyntheticMap(15, campfires_per_homeland=3, seed=11)
    g = eng.MapGrid(m.cells())
    cells = cells_by_rank(m)
    qs = random_queries(m, n, 100 + mc + n)
    for at in (len(qs), len(qs) // 2, 0):  # last, middle, first
        qs.insert(at, OUTSIDE)
    nq, nrec = n + 3, n
    plan = eng.Plan(g, params, qs, max_cmds=mc)
    plan.run()
    plan.wait()
    q_of = plan.record_queries()
    assert sorted(q_of[:nrec]) == [i for i, q in enumerate(qs) if q is not OUTSIDE]
    assert all(q == 0xFFFFFFFF for q in q_of[nrec:])

    lengths = list(range(100)) + [mc] * 6 if mc == 4096 else range(mc + 1)
    c = craft(nrec, mc, lengths, len(cells), params, seed=7 * mc + n, overflow=False, max_scrolls=max_scrolls)
    labels = c.labels()
    if max_scrolls is not None:  # the set is there for money words with bit 31 set
        assert sum(w is not None and w[1] >= 1 << 31 for w in labels) >= nrec // 4
    lens = [len(w[3]) for w in labels if w is not None]
    assert set(edge_lengths(mc, False)[:nrec]) <= set(lens) and max(lens) <= mc
    if mc == 4096:
        assert 1 <= lens.count(mc) <= 12
    d_res, rb, d_cmd, cb = plan.device_outputs()
    assert rb == nq * 16 and cb == nq * mc * 16
    _upload(hip, d_res, c.res)
    _upload(hip, d_cmd, c.slots)

    order = np.full(nq, -1, dtype=np.int64)  # query i holds record order[i]
    order[np.array(q_of[:nrec])] = np.arange(nrec)
    want_res, want_pool, want_st = c.pack(cells, order)
    assert want_st == MR_ERR_INVALID_INDEX
    total, cap = len(want_pool), len(want_pool) + 8
    want_labels = [labels[k] if k >= 0 else MR_ERR_INVALID_INDEX for k in order.tolist()]

    def fetch(mode):
        monkeypatch.setenv("MR_FETCH_WIRE", "1" if mode == "wire" else "0")
        if mode == "host":
            monkeypatch.setenv("MR_HOST_DECODE", "1")
        else:
            monkeypatch.delenv("MR_HOST_DECODE", raising=False)
        res, pool = (mr_result * nq)(), (mr_command * cap)()
        if mode == "pinned":
            eng.pin_host(res)
            eng.pin_host(pool)
        try:
            st = eng.lib().mr_plan_fetch(plan.handle, res, pool, cap)
        finally:
            if mode == "pinned":
                eng.unpin_host(res)
                eng.unpin_host(pool)
        return st, res, pool

    problems = []

    def check(what, fn):
        try:
            fn()
        except (AssertionError, pytest.fail.Exception) as e:  # (every route is reported, not the first)
            problems.append(f"{what}: {e}")

    h_st, h_res, h_pool = fetch("host")

    def host_route():
        assert h_st == want_st
        assert decoded_labels(h_res, h_pool, nq, cells) == want_labels
        assert_same_bytes(h_res, h_pool, want_res, want_pool, "host")
    check("MR_HOST_DECODE=1", host_route)

    def fetch_route(mode):
        st, res, pool = fetch(mode)
        assert st == want_st, f"returned {st}"
        assert_same_bytes(res, pool, want_res, want_pool, mode)
        assert st == h_st and bytes(res) == bytes(h_res), "results differ from the host route's"
        assert bytes(pool)[:total * 40] == bytes(h_pool)[:total * 40], "commands differ from the host route's"
    check("device decoder", lambda: fetch_route("device"))
    if mc <= 63:
        check("device decoder, page-locked arrays", lambda: fetch_route("pinned"))
    check("MR_FETCH_WIRE=1", lambda: fetch_route("wire"))

    rw, pcap = eng.wire_row_words(mc), 8
    assert rw == 1 + 2 * mc
    wbuf = DeviceWords(hip, nq * rw + 2 * pcap)
    try:
        def wire_records():
            plan.wire_records(wbuf.ptr.value, wbuf.ptr.value + nq * rw * 4, pcap)
            plan.wait()
            return wbuf.read()

        def wire_route():
            host = wire_records()
            rows = host[:nq * rw].reshape(nq, rw)
            # the rows themselves: the crafted ones, then INVALID_INDEX past the records
            past = np.zeros((nq - nrec, rw), dtype=np.uint32)
            past[:, 0] = (WIRE_STATUS + 32 + MR_ERR_INVALID_INDEX) << WIRE_RANK_BITS
            bad = np.flatnonzero((rows != np.concatenate([c.rows, past])).any(axis=1))
            assert bad.size == 0, f"row {bad[0]} differs from the crafted row ({bad.size} rows do)"
            assert not host[nq * rw:].any(), "the wire pool was written though no label is in it"
            out, cmds = eng.decode_wire_raw(g, params, rows, nq, mc, host[nq * rw:])
            rec_order = np.concatenate([np.arange(nrec), np.full(nq - nrec, -1)])
            r_res, r_pool, _ = c.pack(cells, rec_order)
            # (mr_decode_wire, like mr_decode_records, leaves the running offset in a row
            # that carries a status; mr_plan_fetch zeroes a query without a record)
            r_res["command_offset"][nrec:] = len(r_pool)
            assert decoded_labels(out, cmds, nq, cells) == labels + [MR_ERR_INVALID_INDEX] * (nq - nrec)
            assert_same_bytes(out, cmds, r_res, r_pool, "wire_records")
            if mc == 31:  # the largest LDS request: a second call writes the same bytes
                wbuf.zero()
                assert (wire_records() == host).all(), "a second wire_records call wrote other bytes"

        def wire_refused():
            with pytest.raises(eng.EngineError) as ei:
                plan.wire_records(wbuf.ptr.value, wbuf.ptr.value + nq * rw * 4, pcap)
            plan.wait()
            assert ei.value.status == MR_ERR_INVALID_ARG and "max_cmds" in str(ei.value)
            assert not wbuf.read().any(), "a refused wire_records call wrote rows"
        check("wire_records", wire_route if mc <= WIRE_MAX_CMDS else wire_refused)
        del plan
    finally:
        wbuf.free()
    assert not problems, "\n".join(problems)


def test_fetch_routes_agree_past_the_parts_threshold(eng):
    """Past 65 536 queries every fetch route splits its host work into one part per pool
    thread and folds the parts' statuses (a short pool wins, else the first error in query
    order).  tests/fetch_parts_child.py compares the three routes there, for both groupings
    and for a full and a short pool, in a process of its own: the pool's thread count
    (MR_HOST_THREADS=4) is read once per process."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items()
           if k not in ("MR_HOST_DECODE", "MR_FETCH_WIRE", "MR_DEV_GROUP", "MR_GRID_STATE", "MR_ALGO")}
    env["MR_HOST_THREADS"] = "4"
    r = subprocess.run([sys.executable, os.path.join(here, "fetch_parts_child.py")], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "fetch parts ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_wire_pool_cut(eng, oracle_lib, hip, monkeypatch):
    """mr_plan_wire_records with a wire pool shorter than the pass's overflow pool: exactly
    the records whose commands end past the capacity read MR_ERR_CAPACITY, every other
    record still decodes to the oracle's label, and nothing is written past the capacity.
    A real pass at max_cmds 1 with the overflow pool bound, so the offsets are the
    record-order prefix sums (ovf_order_kernel) and the cut is the same on every run."""
    _clear_env(monkeypatch)
    m = SyntheticMap(25, campfires_per_homeland=6, seed=9, clustered=True)
    g = eng.MapGrid(m.cells())
    params, mc = Params(), 1
    qs = random_queries(m, 400, 41)
    exp = [as_expected(e) for e in oracle_lib.OracleGrid(m.cells()).find_path_batch(params, qs, threads=0)]
    assert sum(1 for e in exp if e and len(e[3]) > mc) >= 20
    n, ovf_cap = len(qs), 8 * len(qs)
    rw = eng.wire_row_words(mc)
    obuf = DeviceWords(hip, n * 4 + n * mc * 4 + ovf_cap * 4)
    wbuf = None
    try:
        plan = eng.Plan(g, params, qs, max_cmds=mc)
        p0 = obuf.ptr.value
        plan.bind_outputs(p0, p0 + n * 16, p0 + n * (1 + mc) * 16, ovf_cap)
        plan.run()
        plan.wait()
        q_of = plan.record_queries()
        words = obuf.read()
        res, slots = words[:n * 4].reshape(n, 4), words[n * 4:n * (1 + mc) * 4].reshape(n, mc, 4)
        # the cut comes from the record tags: {0xFFFFFFFF, offset, count} of the overflowing records
        ov = np.flatnonzero(res[:, 3] >> 16 == 80)
        off, cnt = slots[ov, 0, 1].astype(np.int64), (res[ov, 3] & 0xFFFF).astype(np.int64)
        assert len(ov) >= 20 and (slots[ov, 0, 0] == 0xFFFFFFFF).all() and (slots[ov, 0, 2] == cnt).all()
        assert (off == np.cumsum(cnt) - cnt).all(), "overflow offsets not in record order"
        T = int(cnt.sum())
        wbuf = DeviceWords(hip, n * rw + 2 * T)
        for cap in (T, T - 1, int(off[len(ov) // 2])):
            cut = set(ov[off + cnt > cap].tolist())
            if cap == T:
                assert not cut
            elif cap == T - 1:
                assert cut == {int(ov[-1])}
            else:
                assert len(cut) >= 5 and len(ov) - len(cut) >= 5
            wbuf.zero()
            plan.wire_records(wbuf.ptr.value, wbuf.ptr.value + n * rw * 4, cap)
            plan.wait()
            host = wbuf.read()
            assert not host[n * rw + 2 * cap:].any(), f"cap {cap}: the wire pool was written past its capacity"
            out, cmds = (mr_result * n)(), (mr_command * (n * mc + T + 1))()
            prm = params.to_c()
            # (the library directly: decode_wire_raw raises nothing here, but it drops the status)
            st = eng.lib().mr_decode_wire(g.handle, C.byref(prm), host.ctypes.data, n, mc,
                                          host[n * rw:].ctypes.data if cap else None, cap, out, cmds, len(cmds))
            assert st == (MR_ERR_CAPACITY if cut else MR_OK), (cap, st, eng.last_error())
            assert {k for k in range(n) if out[k].status == MR_ERR_CAPACITY} == cut, cap
            for k in range(n):
                if k in cut:
                    continue
                assert out[k].status in (MR_OK, MR_NOT_FOUND), (cap, k, out[k].status)
                assert as_expected(eng.result_from_c(out[k], cmds)) == exp[q_of[k]], (cap, k)
        del plan
    finally:
        obuf.free()
        if wbuf is not None:
            wbuf.free()
