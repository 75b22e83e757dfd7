"""Child process of test_gpu_decode_widths.py::test_fetch_routes_agree_past_the_parts_threshold
(the host pool reads MR_HOST_THREADS once, when the process first uses it, so the test
starts this script with the variable set).

65 536 + 37 queries on the 7-square map at max_cmds 2, three of them naming no cell (the
first, the last, one in the middle): past the 65 536 queries from which mr_plan_fetch
splits its host work into one part per pool thread and folds the parts' statuses.  One
pass per grouping (MR_DEV_GROUP 0 and 1), fetched through the device decoder, the wire
route and the host decoder, into a pool that holds every command and into one of 1000
commands.  Every route must return the same status and the same mr_result bytes; the same
pool bytes too, up to the first label that does not fit when the pool is short."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from crafted_records import RESULT_DT  # noqa: E402
from marshrutka_amd import pathfinder as eng  # noqa: E402
from marshrutka_amd.abi import (BLUE, MR_ERR_CAPACITY, MR_ERR_INVALID_INDEX, MR_OK, CellIndex, Params,  # noqa: E402
                                mr_command, mr_result)
from marshrutka_amd.mapgen import SyntheticMap, random_queries  # noqa: E402

N, MC, SHORT = 65536 + 37, 2, 1000
OUTSIDE = (CellIndex.center(), CellIndex.homeland(BLUE, 99, 99))  # names no cell of the grid
ROUTES = {"device": {"MR_FETCH_WIRE": "0"}, "wire": {"MR_FETCH_WIRE": "1"}, "host": {"MR_HOST_DECODE": "1"}}


def fetch(plan, route, cap):
    for v in ("MR_FETCH_WIRE", "MR_HOST_DECODE"):
        os.environ.pop(v, None)
    os.environ.update(ROUTES[route])
    res, pool = (mr_result * N)(), (mr_command * cap)()
    st = eng.lib().mr_plan_fetch(plan.handle, res, pool, cap)
    return st, bytes(res), bytes(pool)


def main():
    assert os.environ.get("MR_HOST_THREADS") == "4"
    m = SyntheticMap(7, campfires_per_homeland=1, seed=4)
    g = eng.MapGrid(m.cells())
    qs = random_queries(m, N, 77)
    bad = (0, N // 2 + 5, N - 1)
    for i in bad:
        qs[i] = OUTSIDE
    for group in ("0", "1"):
        os.environ["MR_DEV_GROUP"] = group
        plan = eng.Plan(g, Params(), qs, max_cmds=MC)
        plan.run()
        plan.wait()
        full = N * MC + N * 8
        for cap, want_st in ((full, MR_ERR_INVALID_INDEX), (SHORT, MR_ERR_CAPACITY)):
            got = {route: fetch(plan, route, cap) for route in ROUTES}
            st, res, pool = got["host"]
            r = np.frombuffer(res, dtype=RESULT_DT)
            ok = r["status"] == MR_OK
            end = r["command_offset"].astype(np.int64) + r["n_commands"]
            assert st == want_st, (group, cap, st)
            assert [int(s) for s in r["status"][list(bad)]] == [MR_ERR_INVALID_INDEX] * 3, (group, cap)
            assert not res[32 * bad[1]:32 * bad[1] + 24].strip(b"\0"), "a query without a record is not zeroed"
            assert (r["n_commands"][ok] > MC).any(), "no label in the overflow pool"
            total = int(r["n_commands"][ok].sum())
            assert SHORT < total <= full
            # the commands every route must have written: all, or those before the first label past the pool
            past = np.flatnonzero(ok & (end > cap))
            keep = total if cap == full else int(r["command_offset"][past[0]])
            assert (cap == full and past.size == 0) or 0 < keep <= SHORT, (group, cap, keep)
            for route in ("device", "wire"):
                o_st, o_res, o_pool = got[route]
                assert o_st == st, (group, cap, route, o_st, st)
                assert o_res == res, (group, cap, route, "results differ from the host decoder's")
                assert o_pool[:40 * keep] == pool[:40 * keep], (group, cap, route, "commands differ from the host decoder's")
        del plan
    print("fetch parts ok:", int((r["n_commands"][ok] > MC).sum()), "labels in the overflow pool")


if __name__ == "__main__":
    main()
