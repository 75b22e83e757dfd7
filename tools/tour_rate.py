"""Pass times of a tour plan against what a caller does without one: the matrix plan's pass, its
records to the host, and a subset DP there.

    python tools/tour_rate.py [--out profiles/tour/rate.json] [--shapes s5,s8,s10]

The map and parameters are bench.py's c2 (65^2, 4 campfires a homeland, seed 2024, the default
Params()).  The tours draw their cells from a pool of 64 cells, so the plan's internal matrix is
64 x 64; the end rule is MR_TOUR_RETURN.  Shapes: s5 = 10 000 tours x 5 stops (the wave path), s8 =
2 000 x 8 and s10 = 256 x 10 (the two workgroup classes).  Per shape: five runs of 20 passes after 5
warm-up passes, the tour plan and the matrix plan of the pool alternated run by run, every pass
timed with HIP events on one stream; of the tour plan also mr_plan_kernel_ms (the matrix read-off)
and mr_tour_kernel_ms (the tour launches) per run, and the creation time.  The host side, wall
clock: the matrix plan's pass plus records() to the host, then the DP over all tours vectorised
with numpy (numpy_dp below), and tests/tour_ref.held_karp in plain Python on the first 20 tours
(its time a tour, and scaled to the shape).  The tool checks the plan's records against numpy_dp
for every tour, and numpy_dp against held_karp on those 20, and fails otherwise.
"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tour_ref  # noqa: E402
from marshrutka_amd import abi, build, pathfinder  # noqa: E402
from marshrutka_amd.abi import Params  # noqa: E402
from marshrutka_amd.mapgen import SyntheticMap  # noqa: E402

RUNS, PASSES, WARMUP = 5, 20, 5
POOL = 64
SAMPLE = 20
SHAPES = {"s5": (10_000, 5), "s8": (2_000, 8), "s10": (256, 10)}
BITS = 21  # a metric's sum in the packed key of numpy_dp


def hip_lib():
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    return hip


def timed_passes(hip, stream, events, plan, n):
    """n passes on `stream`, an event between each: the passes' times in ms."""
    assert hip.hipEventRecord(events[0], stream) == 0
    for k in range(n):
        plan.run(stream.value)
        assert hip.hipEventRecord(events[k + 1], stream) == 0
    assert hip.hipEventSynchronize(events[n]) == 0
    out = []
    for k in range(n):
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), events[k], events[k + 1]) == 0
        out.append(ms.value)
    return out


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def numpy_dp(K, n):
    """The rule for T round trips of n stops at once.  K: (T, n + 1, n + 1) int64, the legs' metrics
    packed in comparator order (BITS a metric, so a packed sum compares as its three sums do).
    Returns (the packed totals (T,), the orders (T, n)): tour_ref.held_karp's DP and walk, argmin
    taking the first of equal candidates."""
    import numpy as np
    T = K.shape[0]
    rows = np.arange(T)
    E = np.zeros((T, 1 << n, n), dtype=np.int64)
    for S in sorted(range(1 << n), key=lambda s: bin(s).count("1")):
        for j in range(n):
            if S >> j & 1:
                continue
            if S == 0:
                E[:, 0, j] = K[:, 1 + j, 0]
            else:
                E[:, S, j] = np.min([K[:, 1 + j, 1 + k] + E[:, S & ~(1 << k), k] for k in range(n) if S >> k & 1], axis=0)
    cur = np.zeros(T, dtype=np.int64)
    S = np.full(T, (1 << n) - 1, dtype=np.int64)
    total = np.zeros(T, dtype=np.int64)
    order = np.zeros((T, n), dtype=np.int64)
    big = np.iinfo(np.int64).max
    for r in range(n):
        cand = np.stack([np.where(S >> k & 1, K[rows, cur, 1 + k] + E[rows, S & ~(1 << k), k], big) for k in range(n)], axis=1)
        k = cand.argmin(axis=1)
        total += K[rows, cur, 1 + k]
        order[:, r] = k
        cur, S = 1 + k, S & ~(1 << k)
    return total + K[rows, cur, 0], order


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tour", "rate.json"))
    ap.add_argument("--shapes", default=",".join(SHAPES))
    args = ap.parse_args()
    build.build()
    hip = hip_lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    events = [C.c_void_p() for _ in range(PASSES + 1)]
    for e in events:
        assert hip.hipEventCreate(C.byref(e)) == 0
    m = SyntheticMap(65, campfires_per_homeland=4, seed=2024)
    grid = pathfinder.MapGrid.from_array(m.cells_array())
    params = Params()
    order = [0, 1, 2]  # Params(): (Legs, Money), completed by Time
    pool = random.Random(64).sample(m.all_indices(), POOL)
    result = {"map": "65^2, 4 campfires a homeland, seed 2024", "pool": POOL, "mode": "MR_TOUR_RETURN", "runs": RUNS,
              "passes": PASSES, "warmup": WARMUP, "shapes": {}}
    for name in args.shapes.split(","):
        n_tours, n = SHAPES[name]
        rng = random.Random(100 + n)
        idx = np.array([[rng.randrange(POOL) for _ in range(n + 1)] for _ in range(n_tours)])
        tours = [[pool[i] for i in row] for row in idx]
        plans, create_ms = {}, {}

        def timed_create(kind, make):
            make()  # made once and dropped: the grid's tables and the block cache are warm for both kinds
            t0 = time.perf_counter()
            plans[kind] = make()
            create_ms[kind] = (time.perf_counter() - t0) * 1e3

        timed_create("tour", lambda: pathfinder.TourPlan(grid, params, tours, abi.TOUR_RETURN))
        timed_create("matrix", lambda: pathfinder.MatrixPlan(grid, params, pool, pool))
        passes = {kind: [] for kind in plans}
        kernel = {kind: [] for kind in plans}
        tour_ms, fetch, dp_ms = [], [], []
        for kind, p in plans.items():
            timed_passes(hip, stream, events, p, WARMUP)
            p.kernel_ms()
        for _ in range(RUNS):
            for kind, p in plans.items():  # alternated
                passes[kind] += timed_passes(hip, stream, events, p, PASSES)
                kernel[kind].append(p.kernel_ms()[0])
            tour_ms.append(plans["tour"].tour_ms())
            # what a caller does today: the matrix plan's pass, its records on the host, the DP there
            t0 = time.perf_counter()
            plans["matrix"].run(stream.value)
            mrec = plans["matrix"].records()
            t1 = time.perf_counter()
            met = mrec[:, :, :3].astype(np.int64)
            met[np.arange(POOL), np.arange(POOL)] = 0  # a leg from a cell to itself
            assert int(met.max()) * (n + 1) < 1 << BITS
            packed = (met[:, :, order[0]] << 2 * BITS) | (met[:, :, order[1]] << BITS) | met[:, :, order[2]]
            total, pi = numpy_dp(packed[idx[:, :, None], idx[:, None, :]], n)
            t2 = time.perf_counter()
            fetch.append((t1 - t0) * 1e3)
            dp_ms.append((t2 - t1) * 1e3)
            plans["matrix"].kernel_ms()
        # plain Python on the first tours
        t0 = time.perf_counter()
        ref = []
        for row in idx[:SAMPLE]:
            M = np.zeros((n + 2, n + 2, 3), dtype=np.int64)
            M[:n + 1, :n + 1] = met[row[:, None], row[None, :]]
            ref.append(tour_ref.held_karp(M, tour_ref.MODE_RETURN, order))
        python_ms = (time.perf_counter() - t0) * 1e3 / SAMPLE
        mask = (1 << BITS) - 1
        host = np.stack([total >> 2 * BITS, (total >> BITS) & mask, total & mask], axis=1)
        rec = plans["tour"].records()
        got = np.stack([rec["legs"], rec["money"], rec["time_s"]], axis=1).astype(np.int64)
        equal = bool((got == host).all() and (rec["order"][:, :n] == pi).all() and (rec["status"] == 0).all() and
                     (rec["n_stops"] == n).all() and (rec["n_legs"] == n + 1).all())
        ref_equal = all(tuple(host[t]) == ref[t][0] and list(pi[t]) == ref[t][1] for t in range(SAMPLE))
        st = plans["tour"].stats()
        shape = {"n_tours": n_tours, "n_stops": n, "num_points": plans["tour"].num_points, "solver": st["solver"],
                 "tour": {"pass_ms": summary(passes["tour"]), "matrix_kernel_ms": summary(kernel["tour"]),
                          "tour_kernel_ms": summary(tour_ms), "create_ms": create_ms["tour"]},
                 "matrix": {"pass_ms": summary(passes["matrix"]), "kernel_ms": summary(kernel["matrix"]),
                            "create_ms": create_ms["matrix"]},
                 "host": {"matrix_pass_and_records_ms": summary(fetch), "numpy_dp_ms": summary(dp_ms),
                          "python_held_karp_ms_a_tour": python_ms, "python_held_karp_ms_scaled": python_ms * n_tours},
                 "records_equal_host": equal, "numpy_dp_equals_held_karp": ref_equal}
        today = statistics.median(fetch) + statistics.median(dp_ms)
        shape["host_numpy_over_tour_pass_median"] = today / shape["tour"]["pass_ms"]["median"]
        shape["host_python_over_tour_pass_median"] = (statistics.median(fetch) + python_ms * n_tours) / shape["tour"]["pass_ms"]["median"]
        result["shapes"][name] = shape
        print(json.dumps({name: shape}), flush=True)
        plans.clear()
        pathfinder.lib().mr_cache_trim()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    bad = [n for n, s in result["shapes"].items() if not (s["records_equal_host"] and s["numpy_dp_equals_held_karp"])]
    if bad:
        sys.exit("records differ from the host answer: " + ", ".join(bad))


if __name__ == "__main__":
    main()
