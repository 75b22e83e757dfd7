"""Pass times of a nearest-source plan against what a caller does without one: the matrix plan's
pass, its records to the host, and the reduction over the sources there in numpy.

    python tools/nearest_src_rate.py [--out profiles/nearest_src/rate.json] [--shapes a,b,b1,c]

The map and parameters are bench.py's c3 (1025^2, 4 campfires a homeland, seed 4096, the default
Params()); sources and destinations are uniform random cells.  Shapes: a = 1 024 sources x 1 024
destinations in one group; b = 65 536 sources x 64 destinations in 4 groups (one chunk x 4 groups:
the shape segments exist for); b1 = b with MR_NSRC_SEG set to the group size, so that no group is
cut; c = 1 024 x 65 536 in one group; on request b32, b64 and b256 = b with MR_NSRC_SEG at 32, 64 and
256 sources (the default floor is 128).  MR_SRC_BEST.  Per shape: five runs of 20 passes after 5 warm-up
passes, the nearest-source plan and the matrix plan of the same lists alternated run by run, every
pass timed with HIP events on one stream; of the nearest-source plan also mr_plan_kernel_ms (the
matrix read-off) and mr_nearest_src_kernel_ms (the new launches alone) per run.  "today", wall
clock, once a run: the matrix plan's pass plus records() to the host plus the numpy reduction
(numpy_reduce below: a min per metric in turn over the sources still tied, then the first of them).
The tool checks every record of the plan against that reduction, and the reduction against
tests/nearest_src_ref.reduce_sources on the first 64 destinations, and fails otherwise.
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

import nearest_src_ref  # noqa: E402
from marshrutka_amd import abi, build, pathfinder  # noqa: E402
from marshrutka_amd.abi import Params  # noqa: E402
from marshrutka_amd.mapgen import SyntheticMap  # noqa: E402

RUNS, PASSES, WARMUP = 5, 20, 5
# n_src, n_dst, n_groups, MR_NSRC_SEG
SHAPES = {"a": (1024, 1024, 1, None), "b": (65536, 64, 4, None), "b1": (65536, 64, 4, "group"), "c": (1024, 65536, 1, None),
          "b32": (65536, 64, 4, 32), "b64": (65536, 64, 4, 64), "b256": (65536, 64, 4, 256)}
DEFAULT_SHAPES = "a,b,b1,c"


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


def numpy_reduce(mrec, groups, n_groups, order):
    """The rule under MR_SRC_BEST for (n_src, n_dst, 4) matrix records: (n_dst, n_groups, 5)."""
    import numpy as np
    n_dst = mrec.shape[1]
    out = np.zeros((n_dst, n_groups, 5), dtype=np.uint32)
    out[:, :, 4] = 0xFFFFFFFF
    groups = np.asarray(groups)
    for g in range(n_groups):
        idx = np.nonzero(groups == g)[0]
        if not idx.size:
            continue
        m = mrec if idx.size == mrec.shape[0] else mrec[idx]
        tied = np.ones(m.shape[:2], dtype=bool)
        for q in order:
            k = np.where(tied, m[:, :, q], np.uint32(0xFFFFFFFF))
            tied &= k == k.min(axis=0)
        win = tied.argmax(axis=0)  # the first of the sources still tied
        out[:, g, :4] = m[win, np.arange(n_dst)]
        out[:, g, 4] = idx[win]
    return out


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest_src", "rate.json"))
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
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
    params = Params()
    order = pathfinder.metric_order(params)
    result = {"map": "1025^2, 4 campfires a homeland, seed 4096", "which": "MR_SRC_BEST", "runs": RUNS, "passes": PASSES,
              "warmup": WARMUP, "shapes": {}}
    if os.path.exists(args.out):  # a run of some shapes keeps the others' results
        with open(args.out) as f:
            result["shapes"] = json.load(f).get("shapes", {})
    for name in args.shapes.split(","):
        n_src, n_dst, n_groups, seg = SHAPES[name]
        rng = random.Random(1000 + n_src + n_dst)
        sources = [m.index_at(rng.randrange(V)) for _ in range(n_src)]
        dests = [m.index_at(rng.randrange(V)) for _ in range(n_dst)]
        groups = [i % n_groups for i in range(n_src)]
        if seg is not None:
            os.environ["MR_NSRC_SEG"] = str(n_src // n_groups if seg == "group" else seg)
        else:
            os.environ.pop("MR_NSRC_SEG", None)
        plans, create_ms = {}, {}

        def timed_create(kind, make):
            make()  # made once and dropped: the grid's tables and the block cache are warm for both kinds
            t0 = time.perf_counter()
            plans[kind] = make()
            create_ms[kind] = (time.perf_counter() - t0) * 1e3

        timed_create("nearest_src", lambda: pathfinder.NearestSourcePlan(grid, params, sources, dests, groups, n_groups=n_groups))
        timed_create("matrix", lambda: pathfinder.MatrixPlan(grid, params, sources, dests))
        os.environ.pop("MR_NSRC_SEG", None)
        passes = {kind: [] for kind in plans}
        kernel = {kind: [] for kind in plans}
        reduce_ms, fetch, host_ms = [], [], []
        for kind, p in plans.items():
            timed_passes(hip, stream, events, p, WARMUP)
            p.kernel_ms()
        want = None
        for _ in range(RUNS):
            for kind, p in plans.items():  # alternated
                passes[kind] += timed_passes(hip, stream, events, p, PASSES)
                kernel[kind].append(p.kernel_ms()[0])
            reduce_ms.append(plans["nearest_src"].reduce_ms())
            # what a caller does today: the matrix plan's pass, its records on the host, the reduction there
            t0 = time.perf_counter()
            plans["matrix"].run(stream.value)
            mrec = plans["matrix"].records()
            t1 = time.perf_counter()
            want = numpy_reduce(mrec, groups, n_groups, order)
            t2 = time.perf_counter()
            fetch.append((t1 - t0) * 1e3)
            host_ms.append((t2 - t1) * 1e3)
            plans["matrix"].kernel_ms()
        rec = plans["nearest_src"].records()
        equal = bool((rec == want).all())
        ref_equal = bool((want[:64] == nearest_src_ref.reduce_sources(mrec[:, :64], groups, n_groups, order)).all())
        del mrec
        st = plans["nearest_src"].stats()
        distinct = plans["nearest_src"].stats()["num_sources"]
        pitch8 = (n_dst + 7) // 8 * 8
        shape = {"n_src": n_src, "n_dst": n_dst, "n_groups": n_groups, "distinct_sources": distinct, "solver": st["solver"],
                 "segmentation": plans["nearest_src"].segmentation(),
                 "bytes_read": n_src * pitch8 * 16,
                 "nearest_src": {"pass_ms": summary(passes["nearest_src"]), "matrix_kernel_ms": summary(kernel["nearest_src"]),
                                 "reduce_kernels_ms": summary(reduce_ms), "create_ms": create_ms["nearest_src"]},
                 "matrix": {"pass_ms": summary(passes["matrix"]), "kernel_ms": summary(kernel["matrix"]),
                            "create_ms": create_ms["matrix"]},
                 "today": {"matrix_pass_and_records_ms": summary(fetch), "numpy_reduce_ms": summary(host_ms),
                           "total_ms": summary([a + b for a, b in zip(fetch, host_ms)])},
                 "records_equal_host": equal, "numpy_reduce_equals_reference": ref_equal}
        red = shape["nearest_src"]["reduce_kernels_ms"]["median"]
        shape["reduce_read_GBps"] = shape["bytes_read"] / (red * 1e-3) / 1e9 if red > 0 else None
        shape["today_over_plan_pass_median"] = shape["today"]["total_ms"]["median"] / shape["nearest_src"]["pass_ms"]["median"]
        result["shapes"][name] = shape
        print(json.dumps({name: shape}), flush=True)
        plans.clear()
        pathfinder.lib().mr_cache_trim()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    bad = [n for n, s in result["shapes"].items() if not (s["records_equal_host"] and s["numpy_reduce_equals_reference"])]
    if bad:
        sys.exit("records differ from the host answer: " + ", ".join(bad))


if __name__ == "__main__":
    main()
