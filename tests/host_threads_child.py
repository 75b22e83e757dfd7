"""Child process of test_gpu_long_lived_grid.py::test_host_threads: 8 host threads on one
grid (the header's promise: "concurrent queries on one grid from several host threads are
safe").  The parent fixes the environment (MR_HUB_LANE set or not); nothing here touches it
once a thread runs, since setenv beside another thread's getenv is itself a race.

16 jobs on the 21^2 map of seed 11 (3 campfires per homeland): parameter sets drawn from the
(homeland, HQ) keys of hq_keys() (nine of them, one more than a grid keeps tables for), both
Legs-first orders, Money first, Fleetfoot 2 and three scroll prices, at max_cmds 2 or 8, 300
to 1 500 queries, fetched by one of three routes: fetch_raw, fetch_raw into page-locked
arrays, wire_records + decode_wire_raw through a caller device buffer.  Every job's expected
bytes come first, single-threaded, from a second grid of the same cells, and its labels are
checked against the oracle there.  The shared grid exists but is unused until a barrier
releases the threads, so the first uses of its rank and special tables, region tables, memos
and winner tables happen concurrently.  Each thread then runs 6 rounds (a barrier starts
each): it takes a job by a fixed schedule (in every round two threads hold the same key and
two hold different keys of one homeland), creates the plan, runs two passes, fetches,
compares with the job's bytes and destroys the plan.  Thread 0 calls mr_cache_trim between
its rounds.  Thread 1 makes a creation that must fail in every round and checks that
mr_last_error names it; every other thread checks that its own last error never changes.
At the end every plan is gone and mr_cache_live reports what it did before the threads.

Workers are daemon threads: the main thread joins them against a deadline and leaves with
os._exit when one is stuck in a native call, saying which job and call it was in."""
import ctypes as C
import os
import sys
import threading
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), HERE]

from marshrutka_amd.abi import (MR_ERR_INVALID_ARG, SORT_LEGS, SORT_MONEY, SORT_TIME, Params, mr_query)  # noqa: E402
from marshrutka_amd.mapgen import random_query_cells  # noqa: E402

THREADS, ROUNDS = 8, 6
DEADLINE_S = 80.0  # for all rounds of all threads; the parent's limit is 120 s
OFFSETS = (0, 0, 1, 2, 4, 6, 10, 13)  # thread t takes job (OFFSETS[t] + 3 * round) % 16
ROUTES = ("raw", "pinned", "wire")
D2H = 2  # hipMemcpyKind


def hq_keys(w):
    """The 12 (homeland, HQ) keys of a World: the 4 homelands x {no HQ, HQ on campfires[2], HQ
    on the first plain cell}, as (homeland, HQ CellIndex or None)."""
    plain = next(v for v in range(w.V) if v not in set(w.specials))
    return [(h, hq) for h in range(4) for hq in (None, w.m.index_at(w.campfires[2]), w.m.index_at(plain))]


def jobs(w):
    k = hq_keys(w)
    none, camp, plain = 0, 1, 2
    key = lambda h, which, **kw: Params(homeland=h, hq_position=k[3 * h + which][1], **kw)  # noqa: E731
    ps = [key(0, none), key(0, none), key(0, camp), key(0, plain), key(1, none), key(1, camp), key(2, plain), key(3, none),
          key(2, none, sort_by=(SORT_LEGS, SORT_TIME)), key(3, camp), key(0, none, sort_by=(SORT_LEGS, SORT_TIME)),
          key(0, none, sort_by=(SORT_MONEY, SORT_LEGS)), key(0, none, fleetfoot=2), key(0, none, scroll_of_escape_cost=0),
          key(0, none, scroll_of_escape_cost=7), key(0, camp, scroll_of_escape_cost=120)]
    out = []
    for j, p in enumerate(ps):
        n = (1500, 700, 300, 1000)[j % 4]
        src, dst = random_query_cells(w.m, n, 400 + j)
        hq = [w.m.cell_of(p.hq_position)] if p.hq_position is not None else []
        sp = np.array(hq + w.specials, dtype=np.int64)
        src, dst = np.concatenate([src, sp]), np.concatenate([dst, sp[::-1]])
        out.append({"id": j, "params": p, "src": src, "dst": dst, "q": w.m.query_array(src, dst, w.arr),
                    "mc": 2 if j in (1, 5, 10, 15) else 8, "route": ROUTES[j % 3], "key": (p.homeland, p.hq_position)})
    return out


def check_schedule(js):
    for r in range(ROUNDS):
        keys = [js[(o + 3 * r) % len(js)]["key"] for o in OFFSETS]
        assert len(set(keys)) < len(keys), f"round {r}: no two threads hold the same key"
        assert any(a != b and a[0] == b[0] for a in keys for b in keys), f"round {r}: no two keys of one homeland"
    assert len({j["key"] for j in js}) > 8


def make_hip():
    h = C.CDLL("libamdhip64.so.7")
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipFree.argtypes = [C.c_void_p]
    h.hipStreamSynchronize.argtypes = [C.c_void_p]
    return h


def run_job(eng, hip, grid, job, note=lambda call: None):
    """Creates the job's plan on `grid`, runs two passes, fetches by the job's route and
    destroys the plan: (result bytes, command bytes, query of each entry)."""
    from oracle_raw import RESULT
    q, n, mc = job["q"], len(job["q"]), job["mc"]
    note("plan_create")
    plan = eng.Plan(grid, job["params"], None, max_cmds=mc, query_array=q)
    try:
        for _ in range(2):
            note("plan_run")
            plan.run()
        if job["route"] == "wire":
            rw, pcap = eng.wire_row_words(mc), 8 * n
            nw = n * rw + 2 * pcap
            dbuf = C.c_void_p()
            assert hip.hipMalloc(C.byref(dbuf), nw * 4) == 0
            try:
                # (the clear goes through the null stream, which the plan's stream does not wait
                # for: it has to be done before the rows are written)
                assert hip.hipMemset(dbuf, 0, nw * 4) == 0 and hip.hipStreamSynchronize(None) == 0
                note("plan_wire_records")
                plan.wire_records(dbuf.value, dbuf.value + n * rw * 4, pcap)
                note("plan_wait")
                plan.wait()
                host = np.zeros(nw, dtype=np.uint32)
                assert hip.hipMemcpy(host.ctypes.data, dbuf, nw * 4, D2H) == 0
            finally:
                hip.hipFree(dbuf)
            note("decode_wire")
            res, pool = eng.decode_wire_raw(grid, job["params"], host[:n * rw], n, mc, host[n * rw:])
            note("record_queries")
            order = np.array(plan.record_queries(), dtype=np.int64)  # (row k is record k)
        else:
            out = plan.fetch_buffers()
            if job["route"] == "pinned":
                note("host_register")
                for b in out:
                    eng.pin_host(b)
            try:
                note("plan_fetch")
                res, pool = plan.fetch_raw(out=out)
            finally:
                if job["route"] == "pinned":
                    note("host_unregister")
                    for b in out:
                        eng.unpin_host(b)
            order = np.arange(n)
        r = np.frombuffer(res, dtype=np.uint8, count=n * 32).copy()
        ncmd = int(r.view(RESULT)["n"].astype(np.int64).sum())
        return r, np.frombuffer(pool, dtype=np.uint8, count=ncmd * 40).copy(), order
    finally:
        note("plan_destroy")
        plan.__del__()


def live(eng):
    L = eng.lib()
    L.mr_cache_trim()
    blocks, nbytes = C.c_uint64(), C.c_uint64()
    L.mr_cache_live(C.byref(blocks), C.byref(nbytes))
    return blocks.value, nbytes.value


def main():
    import oracle_lib
    from marshrutka_amd import pathfinder as eng
    from oracle_raw import RESULT, command_rows, differing, labels_raw
    from test_gpu_lane_winner import World
    oracle_lib.build()
    if not eng.device_available():
        sys.exit("no gfx950 device")
    hip = make_hip()
    w = World(eng, oracle_lib, 21, 11, cf=3)  # (w.g: the second grid, the expected bytes' one)
    js = jobs(w)
    check_schedule(js)
    for job in js:
        res, pool, order = run_job(eng, hip, w.g, job)
        ores, ocmds = labels_raw(oracle_lib, w.og, job["params"], job["q"])
        bad = differing(res.view(RESULT), command_rows(pool.tobytes()), ores[order], ocmds)
        assert len(bad) == 0, f"job {job['id']}: {len(bad)} labels differ from the oracle, first entry {bad[0]}"
        job["res"], job["pool"] = res, pool
    shared = eng.MapGrid.from_array(w.arr)
    before = live(eng)

    barrier = threading.Barrier(THREADS)
    where = [("start", None, None)] * THREADS  # (round, job, call) of each thread
    errors, done = [], [False] * THREADS
    L = eng.lib()
    bad_q = (mr_query * 1)()

    def worker(t):
        def sync():
            try:
                barrier.wait(timeout=DEADLINE_S)
            except threading.BrokenBarrierError:
                pass  # (a thread stopped on a mismatch: the others go on unaligned)

        try:
            err0 = eng.last_error()
            sync()
            for r in range(ROUNDS):
                job = js[(OFFSETS[t] + 3 * r) % len(js)]

                def note(call):
                    where[t] = (r, job["id"], call)

                res, pool, _ = run_job(eng, hip, shared, job, note)
                for what, got, exp in (("results", res, job["res"]), ("commands", pool, job["pool"])):
                    if got.shape != exp.shape or not np.array_equal(got, exp):
                        size = 32 if what == "results" else 40
                        m = min(len(got), len(exp)) // size * size
                        d = np.flatnonzero((got[:m] != exp[:m]).reshape(-1, size).any(axis=1))
                        first = int(d[0]) if len(d) else m // size
                        raise AssertionError(f"{what} differ from the single-threaded run's: first differing entry "
                                             f"{first} ({len(got)} bytes against {len(exp)}): "
                                             f"{got[first * size:(first + 1) * size].tobytes().hex()} against "
                                             f"{exp[first * size:(first + 1) * size].tobytes().hex()}; {len(d)} entries differ")
                if t == 1:  # a creation that must fail, and this thread's own error text
                    note("plan_create (must fail)")
                    h = C.c_void_p()
                    prm = job["params"].to_c()
                    st = L.mr_plan_create_ex(shared.handle, C.byref(prm), bad_q, 1, 4097, C.byref(h))
                    msg = eng.last_error()
                    if st != MR_ERR_INVALID_ARG or "max_cmds" not in msg:
                        raise AssertionError(f"failed creation: status {st}, last error {msg!r}")
                elif eng.last_error() != err0:
                    raise AssertionError(f"last error changed on a thread whose calls succeeded: {eng.last_error()!r}")
                if t == 0:
                    note("cache_trim")
                    L.mr_cache_trim()
                where[t] = (r, job["id"], "between rounds")
                if r + 1 < ROUNDS:
                    sync()
            done[t] = True
        except BaseException as e:  # noqa: BLE001 (reported by the main thread)
            errors.append(f"thread {t}, round {where[t][0]}, job {where[t][1]} ({where[t][2]}): {type(e).__name__}: {e}")
            barrier.abort()

    t0 = time.monotonic()
    threads = [threading.Thread(target=worker, args=(t,), daemon=True) for t in range(THREADS)]
    for th in threads:
        th.start()
    for t, th in enumerate(threads):
        th.join(max(0.0, t0 + DEADLINE_S - time.monotonic()))
    stuck = [t for t, th in enumerate(threads) if th.is_alive()]
    if stuck:
        for t in stuck:
            print(f"thread {t} did not finish in {DEADLINE_S:.0f} s: round {where[t][0]}, job {where[t][1]}, in {where[t][2]}")
        for e in errors:
            print(e)
        sys.stdout.flush()
        os._exit(3)
    wall = time.monotonic() - t0
    if errors or not all(done):
        for e in errors:
            print(e)
        sys.exit(1)
    after = live(eng)
    assert after == before, f"live device blocks after the threads {after}, before them {before}"
    del shared
    print(f"threads took {wall:.2f} s: {THREADS} threads x {ROUNDS} rounds")
    print("ok")


if __name__ == "__main__":
    main()
