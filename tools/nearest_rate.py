"""Pass times of a nearest plan against the matrix plan of the same sources and destinations.

    python tools/nearest_rate.py [--out profiles/nearest/rate.json] [--shapes a,b,c]

The map and parameters are bench.py's c3 (1025^2, 4 campfires a homeland, seed 4096, the
default Params()).  Shapes: a = 1 024 sources x 1 024 destinations in one group, b = 65 536
sources x 64 destinations in 4 groups, c = 1 024 x 65 536 in one group (the documented bad
case: a group's destinations are reduced by one wave).  Per shape and plan kind: five runs of
20 passes after 5 warm-up passes, the kinds alternated run by run; every pass timed with HIP
events on one stream.  The comparison flatters the matrix plan: it leaves n_src x n_dst records
on the device and still owes the reduction the nearest plan has done.
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

from marshrutka_amd import build, pathfinder  # noqa: E402
from marshrutka_amd.abi import Params  # noqa: E402
from marshrutka_amd.mapgen import SyntheticMap  # noqa: E402

RUNS, PASSES, WARMUP = 5, 20, 5
CHECK_MAX = 8 << 20  # pairs up to which the winners are checked against the matrix plan's records


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest", "rate.json"))
    ap.add_argument("--shapes", default="a,b,c")
    args = ap.parse_args()
    build.build()
    hip = hip_lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    events = [C.c_void_p() for _ in range(PASSES + 1)]
    for e in events:
        assert hip.hipEventCreate(C.byref(e)) == 0
    m = SyntheticMap(1025, campfires_per_homeland=4, seed=4096)
    grid = pathfinder.MapGrid.from_array(m.cells_array())
    V = 1025 * 1025
    shapes = {"a": (1024, 1024, 1), "b": (65536, 64, 4), "c": (1024, 65536, 1)}
    result = {"map": "1025^2, 4 campfires a homeland, seed 4096", "runs": RUNS, "passes": PASSES, "warmup": WARMUP,
              "shapes": {}}
    params = Params()
    for name in args.shapes.split(","):
        n_src, n_dst, n_groups = shapes[name]
        rng = random.Random(1000 + n_dst)
        sources = [m.index_at(rng.randrange(V)) for _ in range(n_src)]
        dests = [m.index_at(rng.randrange(V)) for _ in range(n_dst)]
        groups = [j % n_groups for j in range(n_dst)]
        plans, create_ms = {}, {}

        def timed_create(kind, make):
            make()  # made once and dropped: the grid's tables and the block cache are warm for both kinds
            t0 = time.perf_counter()
            plans[kind] = make()
            create_ms[kind] = (time.perf_counter() - t0) * 1e3

        timed_create("nearest", lambda: pathfinder.NearestPlan(grid, params, sources, dests, groups, n_groups=n_groups))
        timed_create("matrix", lambda: pathfinder.MatrixPlan(grid, params, sources, dests))
        passes = {k: [] for k in plans}
        kernel = {k: [] for k in plans}
        for k, p in plans.items():
            timed_passes(hip, stream, events, p, WARMUP)
            p.kernel_ms()
        for _ in range(RUNS):
            for k, p in plans.items():  # alternated
                passes[k] += timed_passes(hip, stream, events, p, PASSES)
                kernel[k].append(p.kernel_ms()[0])
        shape = {"n_src": n_src, "n_dst": n_dst, "n_groups": n_groups, "sort_by": list(params.sort_by), "plans": {}}
        for k, p in plans.items():
            st = p.stats()
            shape["plans"][k] = {"pass_ms": summary(passes[k]), "kernel_ms": summary(kernel[k]), "create_ms": create_ms[k],
                                 "solver": st["solver"], "fallback_sources": st["fallback_sources"],
                                 "num_sources": st["num_sources"], "record_bytes": p.device_records()[1]}
        # the winners against the matrix plan's records, reduced on the host (all five words)
        # (shape c's matrix is 1 GB: no host copy of it is made)
        import numpy as np
        check = n_src * n_dst <= CHECK_MAX
        rec = plans["nearest"].records()
        mrec = plans["matrix"].records() if check else None
        same = True if check else None
        for g in range(n_groups if check else 0):
            J = np.arange(g, n_dst, n_groups)
            mm = mrec[:, J].astype(np.int64)
            keys = (np.broadcast_to(J, mm.shape[:2]), mm[:, :, 2], mm[:, :, 1], mm[:, :, 0])  # (Legs, Money, Time, j)
            w = J[np.lexsort(keys, axis=-1)[:, 0]]
            same = same and bool((rec[:, g, 4] == w).all() and (rec[:, g, :4] == mrec[np.arange(n_src), w]).all())
        shape["nearest_equals_reduced_matrix"] = same
        ns, mx = shape["plans"]["nearest"]["pass_ms"], shape["plans"]["matrix"]["pass_ms"]
        shape["nearest_over_matrix_median"] = ns["median"] / mx["median"]
        shape["nearest_slowest_below_matrix_fastest"] = ns["max"] < mx["min"]
        result["shapes"][name] = shape
        print(json.dumps({name: shape}), flush=True)
        plans.clear()
        del rec, mrec
        pathfinder.lib().mr_cache_trim()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
