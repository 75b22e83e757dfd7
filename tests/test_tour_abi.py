"""CPU-side checks of the tour entry points (mr_tour_plan_create and the mr_tour_* accessors): they
are exported, listed and declared for Rust under ABI version 7 with the record's 32 B layout and
the constants; creation rejects every ill-formed argument before anything touches a device, naming
the tour and the position, and fails loudly without a device."""
import ctypes as C
import os
import re

import pytest

from marshrutka_amd import abi
from marshrutka_amd.abi import CellIndex, Params
from marshrutka_amd.mapgen import SyntheticMap

TOUR_SYMBOLS = ["mr_tour_plan_create", "mr_tour_records", "mr_tour_device_records", "mr_tour_leg_label",
                "mr_tour_num_points", "mr_tour_kernel_ms"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    from marshrutka_amd import build, pathfinder
    build.build()
    return pathfinder


def test_tour_symbols_are_exported_listed_and_declared(eng):
    L = C.CDLL(eng.LIB_PATH)
    ffi = open(os.path.join(ROOT, "integration", "rust", "src", "ffi.rs")).read()
    header = open(os.path.join(ROOT, "include", "marshrutka_pf.h")).read()
    for name in TOUR_SYMBOLS:
        assert hasattr(L, name), name
        assert name in eng.EXPORTED_SYMBOLS, name
        assert re.search(r"pub fn %s\s*\(" % name, ffi), name
        assert re.search(r"\b(int|double) %s\s*\(" % name, header), name
    assert abi.TOUR_MAX_STOPS == 10 and (abi.TOUR_OPEN, abi.TOUR_RETURN, abi.TOUR_TO_LAST) == (0, 1, 2)
    assert re.search(r"#define\s+MR_TOUR_MAX_STOPS\s+10u", header)
    assert re.search(r"MR_TOUR_OPEN\s*=\s*0\s*,\s*MR_TOUR_RETURN\s*=\s*1\s*,\s*MR_TOUR_TO_LAST\s*=\s*2", header)
    assert re.search(r"pub const MR_TOUR_MAX_STOPS:\s*u32\s*=\s*10\s*;", ffi)
    for name, v in (("MR_TOUR_OPEN", 0), ("MR_TOUR_RETURN", 1), ("MR_TOUR_TO_LAST", 2)):
        assert re.search(r"pub const %s:\s*u32\s*=\s*%d\s*;" % (name, v), ffi), name
    assert re.search(r"pub struct mr_tour_record\b", ffi)
    assert eng.lib().mr_abi_version() == 7


def test_record_layout():
    r = abi.mr_tour_record
    assert C.sizeof(r) == 32
    assert [(f, getattr(r, f).offset) for f, _ in r._fields_] == [
        ("legs", 0), ("money", 4), ("time_s", 8), ("status", 12), ("n_stops", 16), ("n_legs", 17), ("order", 18),
        ("reserved", 28)]
    assert r.order.size == 10


def _cells(cs):
    arr = (abi.mr_cell_index * max(len(cs), 1))()
    for i, c in enumerate(cs):
        arr[i].kind, arr[i].sub, arr[i].x, arr[i].y = c.kind, c.sub, c.x, c.y
    return arr


def _u32(xs):
    return (C.c_uint32 * len(xs))(*xs)


def test_invalid_arguments_before_any_device(eng):
    """Every rejection below is an argument error, so it reads MR_ERR_INVALID_ARG whether or not
    a device is visible: were a device touched first, a machine without one would read
    MR_ERR_NO_DEVICE."""
    L = eng.lib()
    m = SyntheticMap(7, campfires_per_homeland=1, seed=4)
    g = eng.MapGrid(m.cells())
    p = Params().to_c()
    cells = m.all_indices()
    arr = _cells(cells[:30])
    begin = _u32([0, 3, 7])
    h = C.c_void_p()
    bad = abi.MR_ERR_INVALID_ARG
    create = L.mr_tour_plan_create
    for mode in (0, 1, 2):
        assert create(None, C.byref(p), arr, begin, 2, mode, C.byref(h)) == bad
        assert create(g.handle, None, arr, begin, 2, mode, C.byref(h)) == bad
        assert create(g.handle, C.byref(p), None, begin, 2, mode, C.byref(h)) == bad
        assert create(g.handle, C.byref(p), arr, None, 2, mode, C.byref(h)) == bad
        assert create(g.handle, C.byref(p), arr, begin, 2, mode, None) == bad
        assert create(g.handle, C.byref(p), arr, begin, 0, mode, C.byref(h)) == bad  # no tour
        assert create(g.handle, C.byref(p), arr, _u32([1, 3, 7]), 2, mode, C.byref(h)) == bad  # tour_begin[0] != 0
        assert "tour 0" in eng.last_error()
        assert create(g.handle, C.byref(p), arr, _u32([0, 5, 3]), 2, mode, C.byref(h)) == bad  # offsets decrease
        assert "tour 1" in eng.last_error() and "position 5" in eng.last_error()
        assert create(g.handle, C.byref(p), arr, _u32([0, 3, 3, 7]), 3, mode, C.byref(h)) == bad  # a tour with no cell
        assert "tour 1" in eng.last_error() and "position 3" in eng.last_error()
        # 11 stops: 12 cells (13 with a fixed end), in the second tour
        n11 = 13 if mode == abi.TOUR_TO_LAST else 12
        assert create(g.handle, C.byref(p), arr, _u32([0, 3, 3 + n11]), 2, mode, C.byref(h)) == bad
        assert "tour 1" in eng.last_error() and "11 stops" in eng.last_error() and "position 3" in eng.last_error()
    for mode in (3, 7, 0xFFFFFFFF):
        assert create(g.handle, C.byref(p), arr, begin, 2, mode, C.byref(h)) == bad
        assert "mode" in eng.last_error()
    # a short MR_TOUR_TO_LAST tour: one cell is a tour under the other modes, not with a fixed end
    assert create(g.handle, C.byref(p), arr, _u32([0, 3, 4, 7]), 3, abi.TOUR_TO_LAST, C.byref(h)) == bad
    assert "tour 1" in eng.last_error() and "position 3" in eng.last_error()
    assert not h.value
    # a cell that is not a grid cell: its tour and its position in the tour
    off = cells[:6] + [CellIndex.homeland(0, 9, 9)] + cells[6:8]
    assert create(g.handle, C.byref(p), _cells(off), _u32([0, 4, 9]), 2, 0, C.byref(h)) == abi.MR_ERR_INVALID_INDEX
    assert "tour 1" in eng.last_error() and "position 2" in eng.last_error()
    assert not h.value
    # through the Python class
    with pytest.raises(eng.EngineError) as ei:
        eng.TourPlan(g, Params(), [cells[:3], cells[:12]])
    assert ei.value.status == bad and "tour 1" in str(ei.value) and "11 stops" in str(ei.value)
    with pytest.raises(eng.EngineError) as ei:
        eng.TourPlan(g, Params(), [cells[:3], cells[3:4]], abi.TOUR_TO_LAST)
    assert ei.value.status == bad and "tour 1" in str(ei.value)
    with pytest.raises(eng.EngineError) as ei:
        eng.TourPlan(g, Params(), [])
    assert ei.value.status == bad
    with pytest.raises(eng.EngineError) as ei:
        eng.TourPlan(g, Params(), [cells[:3]], 3)
    assert ei.value.status == bad
    # the accessors on no plan
    n, ptr, nb = C.c_uint32(), C.c_void_p(), C.c_uint64()
    res = abi.mr_result()
    rec = abi.mr_tour_record()
    assert L.mr_tour_records(None, C.byref(rec), 1) == bad
    assert L.mr_tour_device_records(None, C.byref(ptr), C.byref(nb)) == bad
    assert L.mr_tour_leg_label(None, 0, 0, C.byref(res), None, 0) == bad
    assert L.mr_tour_num_points(None, C.byref(n)) == bad
    assert L.mr_tour_kernel_ms(None) == 0.0


def test_creation_without_a_device_fails_loudly(eng):
    m = SyntheticMap(7, campfires_per_homeland=1, seed=4)
    g = eng.MapGrid(m.cells())
    cells = m.all_indices()
    tours = [cells[:4], cells[2:3], cells[5:16]]
    if eng.device_available():  # (the suite's CPU half on a GPU machine: creation works)
        plan = eng.TourPlan(g, Params(), tours, abi.TOUR_RETURN)
        assert plan.num_points == 15
        return
    for mode in (abi.TOUR_OPEN, abi.TOUR_RETURN):
        with pytest.raises(eng.EngineError, match="NO_DEVICE"):
            eng.TourPlan(g, Params(), tours, mode)
    with pytest.raises(eng.EngineError, match="NO_DEVICE"):
        eng.TourPlan(g, Params(), [cells[:4], cells[5:17]], abi.TOUR_TO_LAST)
    with pytest.raises(eng.EngineError, match="NO_DEVICE"):
        eng.FindPath(g).eval_tours(tours)
