"""CPU-side checks of the k-nearest entry points (mr_nearest_plan_create_ex, mr_nearest_k,
mr_nearest_label_ex): they are exported, listed and declared for Rust under ABI version 7;
creation rejects k = 0, k > MR_NEAREST_MAX_K and every null, empty or ill-grouped argument of
the nearest plan before anything touches a device, and fails loudly without one."""
import ctypes as C
import os
import re

import pytest

from marshrutka_amd import abi
from marshrutka_amd.abi import CellIndex, Params
from marshrutka_amd.mapgen import SyntheticMap

KNEAREST_SYMBOLS = ["mr_nearest_plan_create_ex", "mr_nearest_k", "mr_nearest_label_ex"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    from marshrutka_amd import build, pathfinder
    build.build()
    return pathfinder


def test_knearest_symbols_are_exported_listed_and_declared(eng):
    L = C.CDLL(eng.LIB_PATH)
    ffi = open(os.path.join(ROOT, "integration", "rust", "src", "ffi.rs")).read()
    header = open(os.path.join(ROOT, "include", "marshrutka_pf.h")).read()
    for name in KNEAREST_SYMBOLS:
        assert hasattr(L, name), name
        assert name in eng.EXPORTED_SYMBOLS, name
        assert re.search(r"pub fn %s\s*\(" % name, ffi), name
        assert re.search(r"\bint %s\s*\(" % name, header), name
    assert abi.MR_NEAREST_MAX_K == 64
    assert re.search(r"pub const MR_NEAREST_MAX_K:\s*u32\s*=\s*64\s*;", ffi)
    assert re.search(r"#define\s+MR_NEAREST_MAX_K\s+64u", header)
    assert eng.lib().mr_abi_version() == 7


def _cells(cs):
    arr = (abi.mr_cell_index * len(cs))()
    for i, c in enumerate(cs):
        arr[i].kind, arr[i].sub, arr[i].x, arr[i].y = c.kind, c.sub, c.x, c.y
    return arr


def test_invalid_arguments_before_any_device(eng):
    """Every rejection below is an argument error, so it reads MR_ERR_INVALID_ARG whether or not
    a device is visible: were a device touched first, a machine without one would read
    MR_ERR_NO_DEVICE."""
    L = eng.lib()
    m = SyntheticMap(7, campfires_per_homeland=1, seed=4)
    g = eng.MapGrid(m.cells())
    p = Params().to_c()
    src, dst = _cells(m.all_indices()[:3]), _cells(m.all_indices()[3:8])
    grp = (C.c_uint32 * 5)(0, 1, 1, 0, 1)
    h = C.c_void_p()
    bad = abi.MR_ERR_INVALID_ARG
    create = L.mr_nearest_plan_create_ex
    for k in (0, 65, 0xFFFFFFFF):
        assert create(g.handle, C.byref(p), src, 3, dst, 5, grp, 2, k, C.byref(h)) == bad, k
        assert re.search(r"\bk\b", eng.last_error()), eng.last_error()
        assert create(g.handle, C.byref(p), src, 3, dst, 5, None, 1, k, C.byref(h)) == bad, k
        assert re.search(r"\bk\b", eng.last_error()), eng.last_error()
    # the nearest plan's null, empty and ill-grouped cases through _ex
    for k in (1, 3, 64):
        assert create(None, C.byref(p), src, 3, dst, 5, grp, 2, k, C.byref(h)) == bad
        assert create(g.handle, None, src, 3, dst, 5, grp, 2, k, C.byref(h)) == bad
        assert create(g.handle, C.byref(p), None, 3, dst, 5, grp, 2, k, C.byref(h)) == bad
        assert create(g.handle, C.byref(p), src, 3, None, 5, grp, 2, k, C.byref(h)) == bad
        assert create(g.handle, C.byref(p), src, 3, dst, 5, grp, 2, k, None) == bad
        assert create(g.handle, C.byref(p), src, 0, dst, 5, grp, 2, k, C.byref(h)) == bad
        assert create(g.handle, C.byref(p), src, 3, dst, 0, grp, 2, k, C.byref(h)) == bad
        assert create(g.handle, C.byref(p), src, 3, dst, 5, grp, 0, k, C.byref(h)) == bad
        assert create(g.handle, C.byref(p), src, 3, dst, 5, None, 0, k, C.byref(h)) == bad
        assert create(g.handle, C.byref(p), src, 3, dst, 5, grp, 6, k, C.byref(h)) == bad  # n_groups > n_dst
        assert create(g.handle, C.byref(p), src, 3, dst, 5, None, 6, k, C.byref(h)) == bad
    grp[3] = 2  # a group id >= n_groups: the message names the position
    assert create(g.handle, C.byref(p), src, 3, dst, 5, grp, 2, 3, C.byref(h)) == bad
    assert "destination 3" in eng.last_error()
    assert not h.value
    # through the Python class
    cells = m.all_indices()
    for k in (0, 65):
        with pytest.raises(eng.EngineError) as ei:
            eng.NearestPlan(g, Params(), cells[:2], cells[:5], k=k)
        assert ei.value.status == bad and re.search(r"\bk\b", str(ei.value))
    # the new accessors on no plan
    n = C.c_uint32()
    res = abi.mr_result()
    assert L.mr_nearest_k(None, C.byref(n)) == bad
    assert L.mr_nearest_label_ex(None, 0, 0, 0, C.byref(res), None, 0) == bad


def test_creation_without_a_device_fails_loudly(eng):
    m = SyntheticMap(7, campfires_per_homeland=1, seed=4)
    g = eng.MapGrid(m.cells())
    cells = m.all_indices()
    if eng.device_available():  # (the suite's CPU half on a GPU machine: creation works)
        plan = eng.NearestPlan(g, Params(), cells[:2], cells[:5], [0, 1, 2, 3, 4], k=3)
        assert plan.k == 3 and plan.record_pitch() == 16
        return
    with pytest.raises(eng.EngineError, match="NO_DEVICE"):
        eng.NearestPlan(g, Params(), cells[:2], cells[:5], k=3)
    with pytest.raises(eng.EngineError, match="NO_DEVICE"):
        eng.NearestPlan(g, Params(), cells[:2], cells[:5], [0, 1, 1, 0, 2], k=3)
    with pytest.raises(eng.EngineError, match="NO_DEVICE"):
        eng.FindPath(g).eval_nearest([CellIndex.center()], cells[:5], k=3)
    with pytest.raises(eng.EngineError, match="NO_DEVICE"):
        eng.FindPath(g).eval_nearest_poi([CellIndex.center()], k=3)
