"""Pass times of a matrix plan against the two other routes to the same numbers: an
all-destinations plan of the same sources, and a pair plan of the n_src x n_dst pairs.

    python tools/matrix_rate.py [--out profiles/matrix/rate.json] [--shapes a,b,c]

The map and parameters are bench.py's c3 (1025^2, 4 campfires a homeland, seed 4096, the
default Params()).  Shapes: a = 1 024 sources x 1 024 destinations, b = 1 024 x 65 536,
c = a under (Time, Money).  Per shape and plan kind: five runs of 20 passes after 5 warm-up
passes, the kinds alternated run by run; every pass timed with HIP events on one stream.
The pair plan (max_cmds 1) is made only up to a chosen cut-off of 8 M pairs; shape b's 67 M
pairs (1 GB of queries, over 2 GB of records) were not tried.  Creation times are wall-clock
and comparable between the kinds: each kind's plan is first made once and dropped, which warms
the grid's tables and the block cache, and the second creation is the one timed.
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
from marshrutka_amd.abi import SORT_MONEY, SORT_TIME, Params  # noqa: E402
from marshrutka_amd.mapgen import SyntheticMap  # noqa: E402

RUNS, PASSES, WARMUP = 5, 20, 5
PAIR_MAX = 8 << 20


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix", "rate.json"))
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
    cells_arr = m.cells_array()
    grid = pathfinder.MapGrid.from_array(cells_arr)
    V = 1025 * 1025
    shapes = {"a": (1024, 1024, Params()), "b": (1024, 65536, Params()),
              "c": (1024, 1024, Params(sort_by=(SORT_TIME, SORT_MONEY)))}
    result = {"map": "1025^2, 4 campfires a homeland, seed 4096", "runs": RUNS, "passes": PASSES, "warmup": WARMUP,
              "shapes": {}}
    for name in args.shapes.split(","):
        n_src, n_dst, params = shapes[name]
        rng = random.Random(1000 + n_dst)
        src_i = [rng.randrange(V) for _ in range(n_src)]
        dst_i = [rng.randrange(V) for _ in range(n_dst)]
        sources, dests = [m.index_at(i) for i in src_i], [m.index_at(i) for i in dst_i]
        plans, create_ms = {}, {}

        def timed_create(kind, make):
            make()  # made once and dropped: the grid's tables and the block cache are warm for every kind
            t0 = time.perf_counter()
            plans[kind] = make()
            create_ms[kind] = (time.perf_counter() - t0) * 1e3

        timed_create("matrix", lambda: pathfinder.MatrixPlan(grid, params, sources, dests))
        timed_create("sssp", lambda: pathfinder.SSSPPlan(grid, params, sources))
        pairs_note = None
        if n_src * n_dst <= PAIR_MAX:
            qa = m.query_array([s for s in src_i for _ in range(n_dst)], dst_i * n_src, cells=cells_arr)
            timed_create("pairs", lambda: pathfinder.Plan(grid, params, None, max_cmds=1, query_array=qa))
        else:
            pairs_note = "not made: %d pairs are above this tool's cut-off of %d" % (n_src * n_dst, PAIR_MAX)
        passes = {k: [] for k in plans}
        kernel = {k: [] for k in plans}
        for k, p in plans.items():
            timed_passes(hip, stream, events, p, WARMUP)
            p.kernel_ms()
        for _ in range(RUNS):
            for k, p in plans.items():  # alternated
                passes[k] += timed_passes(hip, stream, events, p, PASSES)
                kernel[k].append(p.kernel_ms()[0])
        shape = {"n_src": n_src, "n_dst": n_dst, "sort_by": list(params.sort_by), "pairs_note": pairs_note, "plans": {}}
        for k, p in plans.items():
            st = p.stats()
            shape["plans"][k] = {"pass_ms": summary(passes[k]), "kernel_ms": summary(kernel[k]), "create_ms": create_ms[k],
                                 "solver": st["solver"], "fallback_sources": st["fallback_sources"],
                                 "num_sources": st["num_sources"]}
        if "matrix" in plans:
            ptr, nbytes = plans["matrix"].device_records()
            shape["plans"]["matrix"]["record_bytes"] = nbytes
            ptr, nbytes = plans["sssp"].device_records()
            shape["plans"]["sssp"]["record_bytes"] = nbytes
        shape["matrix_slowest_below_sssp_fastest"] = passes["matrix"] and max(passes["matrix"]) < min(passes["sssp"])
        result["shapes"][name] = shape
        print(json.dumps({name: shape}), flush=True)
        plans.clear()
        pathfinder.lib().mr_cache_trim()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
