"""Pass times of a k-nearest plan against its yardsticks: the nearest plan (k = 1) and the matrix
plan of the same sources and destinations.

    python tools/knearest_rate.py [--out profiles/knearest/rate.json] [--shapes a4,a16,...]

The map and parameters are bench.py's c3 (1025^2, 4 campfires a homeland, seed 4096, the
default Params()).  Shapes: a4 / a16 / a64 = 1 024 sources x 1 024 destinations in one group at
k = 4, 16 and 64; b4 = 65 536 x 64 in 4 groups at k = 4; c8 = 1 024 x 65 536 in one group at k = 8
(the documented bad case: a group's destinations are selected by one wave); d_far / d_shuf = the
first shape at k = 16 with the destinations listed farthest-first for source 0 (every chunk
inserts into that source's list) and shuffled.  Per shape and plan kind: five runs of 20 passes
after 5 warm-up passes, the kinds alternated run by run; every pass timed with HIP events on one
stream.  For the matrix plan also one pass plus records() to the host a run, wall clock: what a
caller pays today before selecting on the host.  Every shape's records are checked against the
host top-k of the matrix records (shape c8: of its first 32 sources, whose matrix rows come from
a plan of their own; the full matrix is 1 GB).
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
CHECK_MAX = 8 << 20  # pairs up to which the whole matrix is brought to the host for the check
CHECK_SOURCES = 32   # beyond it: the first sources only
NONE = 0xFFFFFFFF
# name: (n_src, n_dst, n_groups, k, listing)
SHAPES = {"a4": (1024, 1024, 1, 4, "random"), "a16": (1024, 1024, 1, 16, "random"), "a64": (1024, 1024, 1, 64, "random"),
          "b4": (65536, 64, 4, 4, "random"), "c8": (1024, 65536, 1, 8, "random"),
          "d_far": (1024, 1024, 1, 16, "farthest_first"), "d_shuf": (1024, 1024, 1, 16, "shuffled")}


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


def host_topk(mrec, groups, n_groups, k):
    """(n_src, n_groups, k, 5) from matrix records under (Legs, Money, Time, j): Params()'s order."""
    import numpy as np
    groups = np.asarray(groups)
    out = np.zeros((mrec.shape[0], n_groups, k, 5), dtype=np.uint32)
    out[..., 4] = NONE
    rows = np.arange(mrec.shape[0])[:, None]
    for g in range(n_groups):
        J = np.nonzero(groups == g)[0]
        if not J.size:
            continue
        mm = mrec[:, J].astype(np.int64)
        keys = (np.broadcast_to(J, mm.shape[:2]), mm[:, :, 2], mm[:, :, 1], mm[:, :, 0])
        w = J[np.lexsort(keys, axis=-1)[:, :k]]
        out[:, g, :w.shape[1], :4] = mrec[rows, w]
        out[:, g, :w.shape[1], 4] = w
    return out


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knearest", "rate.json"))
    ap.add_argument("--shapes", default=",".join(SHAPES))
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
    result = {"map": "1025^2, 4 campfires a homeland, seed 4096", "runs": RUNS, "passes": PASSES, "warmup": WARMUP,
              "shapes": {}}
    params = Params()
    for name in args.shapes.split(","):
        n_src, n_dst, n_groups, k, listing = SHAPES[name]
        rng = random.Random(1000 + n_dst)
        sources = [m.index_at(rng.randrange(V)) for _ in range(n_src)]
        dests = [m.index_at(rng.randrange(V)) for _ in range(n_dst)]
        if listing == "farthest_first":  # by source 0's key, descending
            one = pathfinder.MatrixPlan(grid, params, sources[:1], dests)
            one.run()
            r0 = one.records()[0].astype(np.int64)
            order = np.lexsort((np.arange(n_dst), r0[:, 2], r0[:, 1], r0[:, 0]))[::-1]
            dests = [dests[j] for j in order]
            del one
        elif listing == "shuffled":
            random.Random(7).shuffle(dests)
        groups = [j % n_groups for j in range(n_dst)]
        plans, create_ms = {}, {}

        def timed_create(kind, make):
            make()  # made once and dropped: the grid's tables and the block cache are warm for every kind
            t0 = time.perf_counter()
            plans[kind] = make()
            create_ms[kind] = (time.perf_counter() - t0) * 1e3

        timed_create("knearest", lambda: pathfinder.NearestPlan(grid, params, sources, dests, groups, n_groups=n_groups, k=k))
        timed_create("nearest", lambda: pathfinder.NearestPlan(grid, params, sources, dests, groups, n_groups=n_groups))
        timed_create("matrix", lambda: pathfinder.MatrixPlan(grid, params, sources, dests))
        passes = {kind: [] for kind in plans}
        kernel = {kind: [] for kind in plans}
        fetch = []
        for kind, p in plans.items():
            timed_passes(hip, stream, events, p, WARMUP)
            p.kernel_ms()
        for _ in range(RUNS):
            for kind, p in plans.items():  # alternated
                passes[kind] += timed_passes(hip, stream, events, p, PASSES)
                kernel[kind].append(p.kernel_ms()[0])
            t0 = time.perf_counter()  # the matrix plan's pass and its records on the host
            plans["matrix"].run(stream.value)
            mrec = plans["matrix"].records()
            fetch.append((time.perf_counter() - t0) * 1e3)
            plans["matrix"].kernel_ms()
            if n_src * n_dst > CHECK_MAX:
                del mrec
        shape = {"n_src": n_src, "n_dst": n_dst, "n_groups": n_groups, "k": k, "listing": listing,
                 "sort_by": list(params.sort_by), "plans": {}}
        for kind, p in plans.items():
            st = p.stats()
            shape["plans"][kind] = {"pass_ms": summary(passes[kind]), "kernel_ms": summary(kernel[kind]),
                                    "create_ms": create_ms[kind], "solver": st["solver"],
                                    "fallback_sources": st["fallback_sources"], "num_sources": st["num_sources"],
                                    "record_bytes": p.device_records()[1]}
        shape["plans"]["matrix"]["pass_and_records_to_host_ms"] = summary(fetch)
        # the records against the host top-k of the matrix records (all five words)
        rec = plans["knearest"].records()
        if n_src * n_dst <= CHECK_MAX:
            shape["checked_sources"] = n_src
        else:
            plans.pop("matrix")
            pathfinder.lib().mr_cache_trim()
            part = pathfinder.MatrixPlan(grid, params, sources[:CHECK_SOURCES], dests)
            part.run()
            mrec = part.records()
            rec = rec[:CHECK_SOURCES]
            shape["checked_sources"] = CHECK_SOURCES
            del part
        shape["knearest_equals_host_topk"] = bool((rec == host_topk(mrec, groups, n_groups, k)).all())
        kn = shape["plans"]["knearest"]["pass_ms"]["median"]
        shape["knearest_over_nearest_median"] = kn / shape["plans"]["nearest"]["pass_ms"]["median"]
        shape["knearest_over_matrix_median"] = kn / shape["plans"]["matrix"]["pass_ms"]["median"]
        shape["knearest_over_matrix_with_records_median"] = kn / shape["plans"]["matrix"]["pass_and_records_to_host_ms"]["median"]
        result["shapes"][name] = shape
        print(json.dumps({name: shape}), flush=True)
        plans.clear()
        del rec, mrec
        pathfinder.lib().mr_cache_trim()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    bad = [n for n, s in result["shapes"].items() if not s["knearest_equals_host_topk"]]
    if bad:
        sys.exit("records differ from the host top-k: " + ", ".join(bad))


if __name__ == "__main__":
    main()
