"""CPU-side checks of the nearest-source entry points (mr_nearest_src_plan_create and the
mr_nearest_src_* accessors): they are exported, listed and declared for Rust under ABI version 7
with the record's 32 B layout and the constants; creation rejects every ill-formed argument before
anything touches a device, naming the position, and fails loudly without a device."""
import ctypes as C
import os
import re

import pytest

from marshrutka_amd import abi
from marshrutka_amd.abi import CellIndex, Params
from marshrutka_amd.mapgen import SyntheticMap

SYMBOLS = ["mr_nearest_src_plan_create", "mr_nearest_src_records", "mr_nearest_src_device_records",
           "mr_nearest_src_record_pitch", "mr_nearest_src_label", "mr_nearest_src_segmentation", "mr_nearest_src_kernel_ms"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    from marshrutka_amd import build, pathfinder
    build.build()
    return pathfinder


def test_symbols_are_exported_listed_and_declared(eng):
    L = C.CDLL(eng.LIB_PATH)
    ffi = open(os.path.join(ROOT, "integration", "rust", "src", "ffi.rs")).read()
    header = open(os.path.join(ROOT, "include", "marshrutka_pf.h")).read()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in eng.EXPORTED_SYMBOLS, name
        assert re.search(r"pub fn %s\s*\(" % name, ffi), name
        assert re.search(r"\b(int|double) %s\s*\(" % name, header), name
    assert (abi.SRC_BEST, abi.SRC_WORST) == (0, 1) and abi.SRC_NONE == 0xFFFFFFFF
    assert re.search(r"MR_SRC_BEST\s*=\s*0\s*,\s*MR_SRC_WORST\s*=\s*1", header)
    for name, v in (("MR_SRC_BEST", 0), ("MR_SRC_WORST", 1)):
        assert re.search(r"pub const %s:\s*u32\s*=\s*%d\s*;" % (name, v), ffi), name
    assert re.search(r"pub struct mr_nearest_src_record\b", ffi)
    assert re.search(r"typedef struct mr_nearest_src_record\b", header)
    assert eng.lib().mr_abi_version() == 7


def test_record_layout():
    r = abi.mr_nearest_src_record
    assert C.sizeof(r) == 32
    assert [(f, getattr(r, f).offset) for f, _ in r._fields_] == [
        ("legs", 0), ("money", 4), ("time_s", 8), ("via", 12), ("src", 16), ("reserved", 20)]
    assert r.reserved.size == 12


def _cells(cs):
    arr = (abi.mr_cell_index * max(len(cs), 1))()
    for i, c in enumerate(cs):
        arr[i].kind, arr[i].sub, arr[i].x, arr[i].y = c.kind, c.sub, c.x, c.y
    return arr


def _u32(xs):
    return (C.c_uint32 * len(xs))(*xs)


def test_invalid_arguments_before_any_device(eng):
    """Every rejection below is an argument error, so it reads the same status whether or not a
    device is visible: were a device touched first, a machine without one would read
    MR_ERR_NO_DEVICE."""
    L = eng.lib()
    m = SyntheticMap(7, campfires_per_homeland=1, seed=4)
    g = eng.MapGrid(m.cells())
    p = Params().to_c()
    cells = m.all_indices()
    src, dst = _cells(cells[:6]), _cells(cells[10:14])
    grp = _u32([0, 1, 2, 0, 1, 2])
    h = C.c_void_p()
    bad = abi.MR_ERR_INVALID_ARG
    create = L.mr_nearest_src_plan_create
    for which in (abi.SRC_BEST, abi.SRC_WORST):
        assert create(None, C.byref(p), src, 6, grp, 3, dst, 4, which, C.byref(h)) == bad
        assert create(g.handle, None, src, 6, grp, 3, dst, 4, which, C.byref(h)) == bad
        assert create(g.handle, C.byref(p), None, 6, grp, 3, dst, 4, which, C.byref(h)) == bad
        assert create(g.handle, C.byref(p), src, 6, grp, 3, None, 4, which, C.byref(h)) == bad
        assert create(g.handle, C.byref(p), src, 6, grp, 3, dst, 4, which, None) == bad
        assert create(g.handle, C.byref(p), src, 0, grp, 3, dst, 4, which, C.byref(h)) == bad  # no source
        assert create(g.handle, C.byref(p), src, 6, grp, 3, dst, 0, which, C.byref(h)) == bad  # no destination
        assert create(g.handle, C.byref(p), src, 6, grp, 0, dst, 4, which, C.byref(h)) == bad  # no group
        assert create(g.handle, C.byref(p), src, 6, None, 0, dst, 4, which, C.byref(h)) == bad
        assert create(g.handle, C.byref(p), src, 6, grp, 7, dst, 4, which, C.byref(h)) == bad  # more groups than sources
        assert "n_groups 7" in eng.last_error()
        assert create(g.handle, C.byref(p), src, 6, None, 7, dst, 4, which, C.byref(h)) == bad
        assert create(g.handle, C.byref(p), src, 6, _u32([0, 1, 2, 0, 3, 2]), 3, dst, 4, which, C.byref(h)) == bad
        assert "source 4" in eng.last_error() and "group 3" in eng.last_error()
        assert create(g.handle, C.byref(p), src, 6, _u32([0, 1, 2, 0, 1, 0xFFFFFFFF]), 3, dst, 4, which, C.byref(h)) == bad
        assert "source 5" in eng.last_error()
    for which in (2, 7, 0xFFFFFFFF):
        assert create(g.handle, C.byref(p), src, 6, grp, 3, dst, 4, which, C.byref(h)) == bad
        assert "which" in eng.last_error()
    assert not h.value
    # a cell that is not a grid cell: the list and the position
    off = CellIndex.homeland(0, 9, 9)
    assert create(g.handle, C.byref(p), _cells(cells[:3] + [off] + cells[4:6]), 6, grp, 3, dst, 4, 0,
                  C.byref(h)) == abi.MR_ERR_INVALID_INDEX
    assert "source 3" in eng.last_error()
    assert create(g.handle, C.byref(p), src, 6, None, 1, _cells(cells[10:12] + [off]), 3, 1,
                  C.byref(h)) == abi.MR_ERR_INVALID_INDEX
    assert "destination 2" in eng.last_error()
    assert not h.value
    # through the Python class
    with pytest.raises(eng.EngineError) as ei:
        eng.NearestSourcePlan(g, Params(), cells[:6], cells[10:14], [0, 1, 2, 0, 5, 2], n_groups=3)
    assert ei.value.status == bad and "source 4" in str(ei.value)
    with pytest.raises(eng.EngineError) as ei:
        eng.NearestSourcePlan(g, Params(), cells[:6], cells[10:14], [0, 1])  # an id per source
    assert ei.value.status == bad
    with pytest.raises(eng.EngineError) as ei:
        eng.NearestSourcePlan(g, Params(), cells[:6], [], None)
    assert ei.value.status == bad
    with pytest.raises(eng.EngineError) as ei:
        eng.NearestSourcePlan(g, Params(), cells[:6], cells[10:14], which=2)
    assert ei.value.status == bad and "which" in str(ei.value)
    # the accessors on no plan
    n, ptr, nb = C.c_uint32(), C.c_void_p(), C.c_uint64()
    res = abi.mr_result()
    rec = abi.mr_nearest_src_record()
    assert L.mr_nearest_src_records(None, C.byref(rec), 1) == bad
    assert L.mr_nearest_src_device_records(None, C.byref(ptr), C.byref(nb)) == bad
    assert L.mr_nearest_src_record_pitch(None, C.byref(n)) == bad
    assert L.mr_nearest_src_label(None, 0, 0, C.byref(res), None, 0) == bad
    assert L.mr_nearest_src_segmentation(None, C.byref(n), None, None, None) == bad
    assert L.mr_nearest_src_kernel_ms(None) == 0.0


def test_limits_before_any_device(eng):
    """The matrix block and the records are sized from the arguments alone, against the block
    cache's 16 GiB: 32 776 distinct sources x 32 768 destinations are more than 2^30 records of
    16 B; one cell listed 16 385 times in as many groups is one matrix row, and 16 385 groups x
    32 768 records of 32 B are more than 2^29."""
    L = eng.lib()
    m = SyntheticMap(193, campfires_per_homeland=2, seed=4)
    g = eng.MapGrid(m.cells())
    p = Params().to_c()
    cells = m.all_indices()
    assert len(cells) >= 32776
    dst = _cells(cells[:32768])
    h = C.c_void_p()
    st = L.mr_nearest_src_plan_create(g.handle, C.byref(p), _cells(cells[:32776]), 32776, None, 1, dst, 32768, 0, C.byref(h))
    assert st == abi.MR_ERR_LIMIT and "32776 distinct sources" in eng.last_error() and not h.value
    st = L.mr_nearest_src_plan_create(g.handle, C.byref(p), _cells(cells[:1] * 16385), 16385, _u32(list(range(16385))), 16385,
                                      dst, 32768, 1, C.byref(h))
    assert st == abi.MR_ERR_LIMIT and "16385 groups" in eng.last_error() and not h.value


def test_creation_without_a_device_fails_loudly(eng):
    m = SyntheticMap(7, campfires_per_homeland=1, seed=4)
    g = eng.MapGrid(m.cells())
    cells = m.all_indices()
    if eng.device_available():  # (the suite's CPU half on a GPU machine: creation works)
        plan = eng.NearestSourcePlan(g, Params(), cells[:6], cells[10:14], [0, 1, 2, 0, 1, 2])
        assert plan.n_groups == 3 and plan.record_pitch() == 4
        return
    for which in (abi.SRC_BEST, abi.SRC_WORST):
        with pytest.raises(eng.EngineError, match="NO_DEVICE"):
            eng.NearestSourcePlan(g, Params(), cells[:6], cells[10:14], [0, 1, 2, 0, 1, 2], which=which)
    with pytest.raises(eng.EngineError, match="NO_DEVICE"):
        eng.FindPath(g).eval_nearest_source(cells[:6], cells[10:14])
    with pytest.raises(eng.EngineError, match="NO_DEVICE"):
        eng.FindPath(g).eval_rally(cells[:6], cells[10:14])
