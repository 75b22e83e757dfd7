"""CPU-side checks of the cost-matrix entry points (mr_matrix_*): they are exported and
declared, reject null and empty arguments before anything touches a device, and fail loudly
without one."""
import ctypes as C

import pytest

from marshrutka_amd import abi
from marshrutka_amd.abi import CellIndex, Params
from marshrutka_amd.mapgen import SyntheticMap

MATRIX_SYMBOLS = ["mr_matrix_plan_create", "mr_matrix_records", "mr_matrix_device_records", "mr_matrix_record_pitch",
                  "mr_matrix_source_rows", "mr_matrix_label"]


@pytest.fixture(scope="module")
def eng():
    from marshrutka_amd import build, pathfinder
    build.build()
    return pathfinder


def test_matrix_symbols_are_exported(eng):
    L = C.CDLL(eng.LIB_PATH)
    for name in MATRIX_SYMBOLS:
        assert hasattr(L, name), name
        assert name in eng.EXPORTED_SYMBOLS, name
    assert eng.lib().mr_abi_version() == 7


def _cells(cs):
    arr = (abi.mr_cell_index * len(cs))()
    for i, c in enumerate(cs):
        arr[i].kind, arr[i].sub, arr[i].x, arr[i].y = c.kind, c.sub, c.x, c.y
    return arr


def test_null_and_empty_arguments(eng):
    L = eng.lib()
    m = SyntheticMap(7, campfires_per_homeland=1, seed=4)
    g = eng.MapGrid(m.cells())
    p = Params().to_c()
    src, dst = _cells(m.all_indices()[:3]), _cells(m.all_indices()[3:8])
    h = C.c_void_p()
    bad = abi.MR_ERR_INVALID_ARG
    assert L.mr_matrix_plan_create(None, C.byref(p), src, 3, dst, 5, C.byref(h)) == bad
    assert L.mr_matrix_plan_create(g.handle, None, src, 3, dst, 5, C.byref(h)) == bad
    assert L.mr_matrix_plan_create(g.handle, C.byref(p), None, 3, dst, 5, C.byref(h)) == bad
    assert L.mr_matrix_plan_create(g.handle, C.byref(p), src, 3, None, 5, C.byref(h)) == bad
    assert L.mr_matrix_plan_create(g.handle, C.byref(p), src, 3, dst, 5, None) == bad
    assert L.mr_matrix_plan_create(g.handle, C.byref(p), src, 0, dst, 5, C.byref(h)) == bad
    assert L.mr_matrix_plan_create(g.handle, C.byref(p), src, 3, dst, 0, C.byref(h)) == bad
    assert not h.value
    # the accessors on no plan
    n, ptr, nb = C.c_uint32(), C.c_void_p(), C.c_uint64()
    res = abi.mr_result()
    assert L.mr_matrix_records(None, None, 0) == bad
    assert L.mr_matrix_device_records(None, C.byref(ptr), C.byref(nb)) == bad
    assert L.mr_matrix_record_pitch(None, C.byref(n)) == bad
    assert L.mr_matrix_source_rows(None, C.byref(n), 1) == bad
    assert L.mr_matrix_label(None, 0, 0, C.byref(res), None, 0) == bad


def test_creation_without_a_device_fails_loudly(eng):
    m = SyntheticMap(7, campfires_per_homeland=1, seed=4)
    g = eng.MapGrid(m.cells())
    cells = m.all_indices()
    if eng.device_available():  # (the suite's CPU half on a GPU machine: creation works)
        assert eng.MatrixPlan(g, Params(), cells[:2], cells[:5]).record_pitch() == 8
        return
    with pytest.raises(eng.EngineError, match="NO_DEVICE"):
        eng.MatrixPlan(g, Params(), cells[:2], cells[:5])
    with pytest.raises(eng.EngineError, match="NO_DEVICE"):
        eng.FindPath(g).eval_matrix([CellIndex.center()], cells[:5])
