"""The oracle's labels of a numpy query array as numpy arrays (no Python label objects: at
10^5 queries the object form costs several times the oracle's own time).  Results and
commands have the ABI's layout (mr_result 32 B, mr_command 40 B), the one the engine's
mr_plan_fetch fills, so both sides compare as arrays."""
import ctypes as C

import numpy as np

from marshrutka_amd.abi import mr_command, mr_query, mr_result

RESULT = np.dtype([("legs", "<u4"), ("money", "<u4"), ("time_s", "<i8"), ("n", "<u4"), ("off", "<u4"),
                   ("status", "<i4"), ("res", "<u4")])
assert C.sizeof(mr_result) == RESULT.itemsize and C.sizeof(mr_command) == 40 and C.sizeof(mr_query) == 16


def command_rows(pool, count=None):
    """A command pool (a ctypes array or bytes) as rows of 40 bytes with the reserved bytes
    cleared: kind + 3 reserved | legs, money, fleetfoot | time | from, to (6 + 2 reserved each)."""
    rows = np.frombuffer(pool, dtype=np.uint8)
    rows = rows[:(len(rows) // 40 if count is None else count) * 40].reshape(-1, 40).copy()
    rows[:, 1:4] = 0
    rows[:, 30:32] = 0
    rows[:, 38:40] = 0
    return rows


def labels_raw(oracle_lib, og, params, q, threads=16):
    """(results as a RESULT array, commands as command_rows) of the queries q
    (SyntheticMap.query_array's layout)."""
    n = len(q)
    q = np.ascontiguousarray(q)
    res = (mr_result * max(n, 1))()
    cap = max(1, n * 24)
    pool = (mr_command * cap)()
    st = oracle_lib.lib().mro_find_path_batch(og.h, C.byref(params.to_c()), (mr_query * n).from_buffer(q), n, res, pool,
                                              cap, threads)
    if st < 0:
        raise ValueError(f"oracle batch failed: {st}")
    return np.frombuffer(res, dtype=RESULT)[:n], command_rows(pool)


def differing(res_a, cmds_a, res_b, cmds_b):
    """Indices of the queries whose labels (metrics and commands) differ between two (results,
    commands) pairs."""
    bad = (res_a["legs"] != res_b["legs"]) | (res_a["money"] != res_b["money"]) | (res_a["time_s"] != res_b["time_s"]) | \
          (res_a["n"] != res_b["n"])
    ok = np.nonzero(~bad)[0]
    n = res_a["n"][ok].astype(np.int64)
    within = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    ia = np.repeat(res_a["off"][ok].astype(np.int64), n) + within
    ib = np.repeat(res_b["off"][ok].astype(np.int64), n) + within
    diff = (cmds_a[ia] != cmds_b[ib]).any(axis=1)
    bad[np.repeat(ok, n)[diff]] = True
    return np.nonzero(bad)[0]
