"""The lane memo's staged record stores (DESIGN.md section 3a''', read_off_staged): with the
winner table and at most 4 command slots a record, hub_lane_memo_kernel assembles each
record's command row in LDS and the wave stores whole rows.  MR_LANE_STAGE=require makes plan
creation fail where that kernel is not used, so a plan created under it stored through the
stage; MR_LANE_STAGE=0 runs the direct stores; MR_LANE_MEMO=0 runs hub_lane_kernel.  All give
the same labels, and the oracle's.  Every case sets MR_HUB_LANE=1 so that small plans take the
lane path.

Device buffers come from the HIP runtime the engine library runs on (as in
tests/test_gpu_parity.py: torch's wheel carries a runtime of its own, which cannot start in a
process where this one holds the device)."""
import ctypes as C

import numpy as np
import pytest

from marshrutka_amd.abi import MR_ERR_CAPACITY, MR_ERR_INVALID_ARG, MR_NOT_FOUND, MR_OK, SORT_LEGS, SORT_MONEY, SORT_TIME, Params
from marshrutka_amd.mapgen import random_query_cells
from oracle_raw import RESULT, command_rows, differing, labels_raw
from test_gpu_lane_winner import World, _oracle, _same

pytestmark = pytest.mark.gpu

# mode -> (MR_LANE_MEMO, MR_LANE_WIN, MR_LANE_STAGE)
MODES = {"stage": ("require", "require", "require"), "direct": ("require", "require", "0"), "lane": ("0", None, None),
         "default": (None, None, None)}
STAGE_MAX_CMDS = 4  # the widest plan the staged kernel takes
LANE_MAX_QUERIES = 32  # a source with more queries runs on hub_kernel
ORDERS = [(SORT_LEGS, SORT_MONEY), (SORT_LEGS, SORT_TIME)]
D2H = 2  # hipMemcpyKind


@pytest.fixture(scope="module")
def eng():
    from marshrutka_amd import build, pathfinder
    build.build()
    if not pathfinder.device_available():
        pytest.fail("no gfx950 device visible to the GPU tests")
    return pathfinder


@pytest.fixture(scope="module")
def hip():
    h = C.CDLL("libamdhip64.so.7")
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipFree.argtypes = [C.c_void_p]
    return h


@pytest.fixture(scope="module")
def w21(eng, oracle_lib):
    return World(eng, oracle_lib, 21, 7)


@pytest.fixture(scope="module")
def w65(eng, oracle_lib):
    return World(eng, oracle_lib, 65, 2024)


class DeviceBytes:
    """nbytes of device memory filled with `fill`, starting on a 256-byte boundary."""

    def __init__(self, hip, nbytes, fill=0):
        self.hip, self.nbytes, self.raw = hip, nbytes, C.c_void_p()
        assert hip.hipMalloc(C.byref(self.raw), nbytes + 256) == 0
        self.ptr = (self.raw.value + 255) & ~255
        assert hip.hipMemset(C.c_void_p(self.ptr), fill, nbytes) == 0

    def read(self):
        host = np.zeros(self.nbytes, dtype=np.uint8)
        assert self.hip.hipMemcpy(host.ctypes.data, C.c_void_p(self.ptr), self.nbytes, D2H) == 0
        return host

    def free(self):
        self.hip.hipFree(self.raw)


def _plan(eng, monkeypatch, w, params, src, dst, mode, max_cmds=4):
    monkeypatch.setenv("MR_HUB_LANE", "1")
    for k in ("MR_DEV_GROUP", "MR_LANE_WIN_BUDGET", "MR_LANE_LDS_PAD"):
        monkeypatch.delenv(k, raising=False)
    for k, v in zip(("MR_LANE_MEMO", "MR_LANE_WIN", "MR_LANE_STAGE"), MODES[mode]):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    q = w.m.query_array(src, dst, w.arr)
    return eng.Plan(w.g, params, None, max_cmds=max_cmds, query_array=q)


def _fetch(plan, n):
    res, pool = plan.fetch_raw()
    r = np.frombuffer(res, dtype=np.uint8, count=n * 32).copy()
    ncmd = int(r.view(RESULT)["n"].astype(np.int64).sum())
    return r, np.frombuffer(pool, dtype=np.uint8, count=ncmd * 40).copy()


def _run(eng, monkeypatch, w, params, src, dst, mode, max_cmds=4):
    plan = _plan(eng, monkeypatch, w, params, src, dst, mode, max_cmds)
    plan.run()
    r, p = _fetch(plan, len(src))
    out = {"res": r, "pool": p, "order": plan.record_queries(), "fallback": [str(c) for c in plan.fallback_sources()],
           "stats": plan.stats()}
    plan.__del__()
    return out


def _three_ways(eng, oracle_lib, monkeypatch, w, params, src, dst, max_cmds=4):
    a = _run(eng, monkeypatch, w, params, src, dst, "stage", max_cmds)
    assert a["stats"]["lanes_per_source"] == 1 and a["stats"]["lane_sources"] > 0
    _same(a, _run(eng, monkeypatch, w, params, src, dst, "direct", max_cmds))
    _same(a, _run(eng, monkeypatch, w, params, src, dst, "lane", max_cmds))
    _oracle(oracle_lib, w, params, a, src, dst)
    return a


def _with_specials(w, src, dst):
    sp = np.array(w.specials)
    return (np.concatenate([src, src[:len(sp)], sp, sp, sp]), np.concatenate([dst, sp, dst[:len(sp)], sp[::-1], sp]))


@pytest.mark.parametrize("sort_by", ORDERS)
@pytest.mark.parametrize("size", [21, 65])
def test_same_bytes_three_ways(eng, oracle_lib, monkeypatch, w21, w65, size, sort_by):
    """Random queries plus every special as a source, as a destination and as both: the
    staged stores, the direct stores and hub_lane_kernel give equal fetch_raw bytes, record
    order, fallback list and stats, and every label is the oracle's."""
    w = w21 if size == 21 else w65
    src, dst = random_query_cells(w.m, 2000 if size == 21 else 3000, 31 + size)
    src, dst = _with_specials(w, src, dst)
    _three_ways(eng, oracle_lib, monkeypatch, w, Params(sort_by=sort_by), src, dst)


def _wave_batch(w, n_lane, seed):
    """n_lane lane sources with 32, 31, .. 1, 32, .. queries each (the engine orders them by
    count: 64 of them put every count into one wave, twice; 65 and 130 put class boundaries
    inside waves and leave a partial last wave), the specials among them, and two sources of
    33 queries, which leave the lane path.  A source's first destination is itself, its second
    a special, the rest random cells."""
    rng = np.random.default_rng(seed)
    cells = list(w.specials[:min(len(w.specials), max(1, n_lane // 3))])
    plain = [int(v) for v in rng.permutation(w.V) if int(v) not in set(w.specials)]
    cells += plain[:n_lane - len(cells)]
    cells = cells[:n_lane]
    counts = [LANE_MAX_QUERIES - (i % LANE_MAX_QUERIES) for i in range(n_lane)]
    busy = plain[n_lane:n_lane + 2]
    src, dst = [], []
    for i, (s, c) in enumerate(list(zip(cells, counts)) + [(b, LANE_MAX_QUERIES + 1) for b in busy]):
        d = rng.integers(0, w.V, size=c)
        d[0] = s
        if c > 1:
            d[1] = w.specials[i % len(w.specials)]
        src += [s] * c
        dst += d.tolist()
    order = rng.permutation(len(src))  # (the plan groups the queries by source itself)
    return np.asarray(src, dtype=np.int64)[order], np.asarray(dst, dtype=np.int64)[order]


@pytest.mark.parametrize("n_lane", [1, 63, 64, 65, 130])
def test_wave_shapes(eng, oracle_lib, monkeypatch, w21, n_lane):
    """Waves whose lanes have different query counts, class boundaries inside a wave, a
    partial last wave, and sources that leave the lane path (their records follow the lane
    records)."""
    src, dst = _wave_batch(w21, n_lane, 100 + n_lane)
    assert len(src) <= 2500
    for sort_by in ORDERS:
        a = _three_ways(eng, oracle_lib, monkeypatch, w21, Params(sort_by=sort_by), src, dst)
        assert a["stats"]["lane_sources"] == n_lane and a["stats"]["num_sources"] == n_lane + 2


@pytest.mark.parametrize("mc", [1, 2, 3, 4, 5, 8, 16])
def test_max_cmds(eng, oracle_lib, monkeypatch, w65, mc):
    """Every width inside the gate under `require` (at 1 and 2 most labels keep a tag in slot
    0 and their commands in the overflow pool); outside it `require` fails and the default
    run equals MR_LANE_STAGE=0."""
    w, p = w65, Params()
    src, dst = _with_specials(w, *random_query_cells(w.m, 2500, 40 + mc))
    b = _run(eng, monkeypatch, w, p, src, dst, "direct", mc)
    if mc <= STAGE_MAX_CMDS:
        a = _run(eng, monkeypatch, w, p, src, dst, "stage", mc)
    else:
        with pytest.raises(eng.EngineError) as ei:
            _run(eng, monkeypatch, w, p, src, dst, "stage", mc)
        assert ei.value.status == MR_ERR_INVALID_ARG and "MR_LANE_STAGE=require" in str(ei.value)
        a = _run(eng, monkeypatch, w, p, src, dst, "default", mc)
    assert a["stats"]["lanes_per_source"] == 1 and a["stats"]["lane_sources"] > 0
    _same(a, b)
    _oracle(oracle_lib, w, p, a, src, dst)
    long = a["res"].view(RESULT)["n"] > mc
    if mc <= 2:
        assert long.mean() > 0.5


def _bound(hip, plan, n, mc, ovf_cap, offset=0, fill=0):
    """The plan's outputs bound to one poisoned device block: 4 KB guard, results, guard,
    command slots, guard, overflow pool; results and slots start `offset` bytes past a
    256-byte boundary.  Returns (block, byte ranges of results / slots / pool)."""
    up = lambda x: (x + 255) & ~255
    r0 = 4096 + offset
    c0 = up(r0 + n * 16 + 4096) + offset
    o0 = up(c0 + n * mc * 16 + 4096)
    blk = DeviceBytes(hip, o0 + ovf_cap * 16, fill)
    plan.bind_outputs(blk.ptr + r0, blk.ptr + c0, blk.ptr + o0, ovf_cap)
    return blk, (r0, r0 + n * 16), (c0, c0 + n * mc * 16), (o0, o0 + ovf_cap * 16)


def _decoded(eng, w, params, host, rr, cr, orr, n, mc):
    """decode_records_raw of a bound block's bytes: (RESULT array in record order, command rows)."""
    from marshrutka_amd.abi import mr_command, mr_result
    res, cmd, ovf = (np.ascontiguousarray(host[a:b]).view(np.uint32) for a, b in (rr, cr, orr))
    out, cap = (mr_result * n)(), n * mc + len(ovf) // 4 + 1
    pool, prm = (mr_command * cap)(), params.to_c()
    # (the library directly: decode_records_raw raises on the status of a record that did not fit)
    st = eng.lib().mr_decode_records(w.g.handle, C.byref(prm), res.ctypes.data, cmd.ctypes.data, n, mc,
                                     ovf.ctypes.data if len(ovf) else None, len(ovf) // 4, out, pool, cap)
    assert st in (MR_OK, MR_ERR_CAPACITY), (st, eng.last_error())
    return np.frombuffer(out, dtype=RESULT)[:n].copy(), command_rows(pool)


def test_overflow_capacity(eng, oracle_lib, hip, monkeypatch, w65):
    """max_cmds 2 with a bound overflow pool too small for the batch.  The pool offset is an
    atomic counter, so which records fit depends on the order the long labels arrive in; to
    fix it, all long labels belong to one source (one lane reads its 32 queries off in
    order) and every other source asks only for itself (one command).  Then record j of
    that source fits exactly when the command counts up to and including it do.  The records
    that do not fit read MR_ERR_CAPACITY, the others are the oracle's, and both store paths
    agree record by record."""
    w, p, mc = w65, Params(), 2
    rng = np.random.default_rng(5)
    plain = [int(v) for v in rng.permutation(w.V) if int(v) not in set(w.specials)]
    far = plain[0]
    others = np.array(plain[1:200] + w.specials)
    src = np.concatenate([np.full(LANE_MAX_QUERIES, far), others])
    dst = np.concatenate([np.array(plain[200:200 + LANE_MAX_QUERIES]), others])
    n = len(src)
    ores, ocmds = labels_raw(oracle_lib, w.og, p, w.m.query_array(src, dst, w.arr))
    assert (ores["n"][LANE_MAX_QUERIES:] <= mc).all()
    got = {}
    for mode in ("stage", "direct"):
        plan = _plan(eng, monkeypatch, w, p, src, dst, mode, mc)
        q_of = np.array(plan.record_queries())
        lens = ores["n"][q_of].astype(np.int64)
        longs = np.flatnonzero(lens > mc)
        assert len(longs) >= 12 and (src[q_of[longs]] == far).all()
        half = len(longs) // 2
        cap = int(lens[longs][:half].sum())
        fits = np.ones(n, dtype=bool)
        fits[longs] = np.cumsum(lens[longs]) <= cap
        assert fits[longs].sum() == half
        blk, rr, cr, orr = _bound(hip, plan, n, mc, cap)
        try:
            plan.run()
            plan.wait()
            res, cmds = _decoded(eng, w, p, blk.read(), rr, cr, orr, n, mc)
        finally:
            plan.__del__()
            blk.free()
        assert ((res["status"] == MR_ERR_CAPACITY) == ~fits).all(), mode
        ok = np.flatnonzero(fits)
        assert np.isin(res["status"][ok], (MR_OK, MR_NOT_FOUND)).all()
        assert len(differing(res[ok], cmds, ores[q_of[ok]], ocmds)) == 0, mode
        got[mode] = (q_of, res, cmds)
    (qa, ra, ca), (qb, rb, cb) = got["stage"], got["direct"]
    assert (qa == qb).all() and (ra["status"] == rb["status"]).all()
    ok = np.flatnonzero(ra["status"] != MR_ERR_CAPACITY)
    assert len(differing(ra[ok], ca, rb[ok], cb)) == 0


@pytest.mark.parametrize("offset", [0, 16, 48])
def test_bound_buffers_poisoned(eng, oracle_lib, hip, monkeypatch, w21, offset):
    """Caller buffers filled with 0xA5 whose record bases lie `offset` bytes past a 256-byte
    boundary: nothing outside the records is written, the buffers decode to the plan's own
    fetch and to the oracle's labels, every slot from n_commands on of a row the staged
    kernel wrote is zero and every written pad word is zero, the records of the sources that
    left the lane path (33 queries: hub_kernel writes them) are right too, and a second pass
    leaves the same bytes."""
    w, p, mc = w21, Params(), 4
    src, dst = _wave_batch(w, 65, 7)
    n, ovf_cap = len(src), 8 * len(src)
    ores, ocmds = labels_raw(oracle_lib, w.og, p, w.m.query_array(src, dst, w.arr))
    plan = _plan(eng, monkeypatch, w, p, src, dst, "stage", mc)
    blk, rr, cr, orr = _bound(hip, plan, n, mc, ovf_cap, offset, 0xA5)
    try:
        snaps = []
        for _ in range(2):
            plan.run()
            plan.wait()
            snaps.append(blk.read())
        host = snaps[0]
        assert (snaps[1] == host).all(), "a second pass wrote other bytes"
        outside = np.ones(len(host), dtype=bool)
        for a, b in (rr, cr, orr):
            outside[a:b] = False
        assert (host[outside] == 0xA5).all(), "bytes outside the records were written"
        q_of = np.array(plan.record_queries())
        res, cmds = _decoded(eng, w, p, host, rr, cr, orr, n, mc)
        fr, fp = _fetch(plan, n)
        fr = fr.view(RESULT)
        assert (res["status"] == fr["status"][q_of]).all()
        assert len(differing(res, cmds, fr[q_of], command_rows(fp.tobytes()))) == 0
        assert len(differing(res, cmds, ores[q_of], ocmds)) == 0
        stats = plan.stats()
    finally:
        plan.__del__()
        blk.free()
    assert stats["lane_sources"] == 65 and stats["num_sources"] == 67
    counts = np.bincount(src, minlength=w.V)
    lane = counts[src[q_of]] <= LANE_MAX_QUERIES  # the records the lane kernel wrote
    assert 0 < (~lane).sum() == 2 * (LANE_MAX_QUERIES + 1)
    slots = host[cr[0]:cr[1]].view(np.uint32).reshape(n, mc, 4)
    ncmd = host[rr[0]:rr[1]].view(np.uint32).reshape(n, 4)[:, 3] & 0xFFFF
    used = np.where(ncmd > mc, 1, ncmd)  # (a longer label keeps its tag in slot 0)
    past = np.arange(mc)[None, :] >= used[:, None]
    assert not slots[lane][past[lane]].any(), "a staged row has non-zero bytes past n_commands"
    assert not slots[:, :, 3][~past].any() and not slots[lane][:, :, 3].any(), "a pad word is not zero"


def test_wire_records(eng, hip, monkeypatch, w65):
    """mr_plan_wire_records (max_cmds 4) after a staged pass and after a direct one: equal
    rows and pool.  (The overflow pool is bound, so that the long labels' offsets are the
    record-order prefix sums in both.)"""
    w, p, mc = w65, Params(), 4
    src, dst = _with_specials(w, *random_query_cells(w.m, 2500, 77))
    n, ovf_cap = len(src), 8 * len(src)
    rw = eng.wire_row_words(mc)
    wire = {}
    for mode in ("stage", "direct"):
        plan = _plan(eng, monkeypatch, w, p, src, dst, mode, mc)
        blk, _, _, _ = _bound(hip, plan, n, mc, ovf_cap)
        wbuf = DeviceBytes(hip, n * rw * 4 + ovf_cap * 8)
        try:
            plan.run()
            plan.wire_records(wbuf.ptr, wbuf.ptr + n * rw * 4, ovf_cap)
            plan.wait()
            wire[mode] = wbuf.read()
            assert plan.stats()["lane_sources"] > 0
        finally:
            plan.__del__()
            blk.free()
            wbuf.free()
    assert wire["stage"][:n * rw * 4].any()
    assert (wire["stage"] == wire["direct"]).all()
