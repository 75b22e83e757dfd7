"""CPU-side checks of the nearest-of-set entry points (mr_nearest_*, mr_grid_poi_cells): they
are exported, listed and declared for Rust; creation rejects null, empty and ill-grouped
arguments before anything touches a device and fails loudly without one; and the grid lists
its points of interest in row-major order."""
import ctypes as C
import os
import re

import pytest

from marshrutka_amd import abi
from marshrutka_amd.abi import POI_CAMPFIRE, POI_FORUM, POI_FOUNTAIN, POI_NONE, CellIndex, Params
from marshrutka_amd.mapgen import SyntheticMap

NEAREST_SYMBOLS = ["mr_nearest_plan_create", "mr_nearest_records", "mr_nearest_device_records",
                   "mr_nearest_record_pitch", "mr_nearest_source_rows", "mr_nearest_label", "mr_grid_poi_cells"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    from marshrutka_amd import build, pathfinder
    build.build()
    return pathfinder


def test_nearest_symbols_are_exported_listed_and_declared(eng):
    L = C.CDLL(eng.LIB_PATH)
    ffi = open(os.path.join(ROOT, "integration", "rust", "src", "ffi.rs")).read()
    for name in NEAREST_SYMBOLS:
        assert hasattr(L, name), name
        assert name in eng.EXPORTED_SYMBOLS, name
        assert re.search(r"pub fn %s\s*\(" % name, ffi), name
    assert "pub struct mr_nearest_record" in ffi
    assert C.sizeof(abi.mr_nearest_record) == 32 and abi.mr_nearest_record.dst.offset == 16
    assert eng.lib().mr_abi_version() == 7


def _cells(cs):
    arr = (abi.mr_cell_index * len(cs))()
    for i, c in enumerate(cs):
        arr[i].kind, arr[i].sub, arr[i].x, arr[i].y = c.kind, c.sub, c.x, c.y
    return arr


def test_invalid_arguments_before_any_device(eng):
    L = eng.lib()
    m = SyntheticMap(7, campfires_per_homeland=1, seed=4)
    g = eng.MapGrid(m.cells())
    p = Params().to_c()
    src, dst = _cells(m.all_indices()[:3]), _cells(m.all_indices()[3:8])
    grp = (C.c_uint32 * 5)(0, 1, 1, 0, 1)
    h = C.c_void_p()
    bad = abi.MR_ERR_INVALID_ARG
    create = L.mr_nearest_plan_create
    assert create(None, C.byref(p), src, 3, dst, 5, grp, 2, C.byref(h)) == bad
    assert create(g.handle, None, src, 3, dst, 5, grp, 2, C.byref(h)) == bad
    assert create(g.handle, C.byref(p), None, 3, dst, 5, grp, 2, C.byref(h)) == bad
    assert create(g.handle, C.byref(p), src, 3, None, 5, grp, 2, C.byref(h)) == bad
    assert create(g.handle, C.byref(p), src, 3, dst, 5, grp, 2, None) == bad
    assert create(g.handle, C.byref(p), src, 0, dst, 5, grp, 2, C.byref(h)) == bad
    assert create(g.handle, C.byref(p), src, 3, dst, 0, grp, 2, C.byref(h)) == bad
    assert create(g.handle, C.byref(p), src, 3, dst, 5, grp, 0, C.byref(h)) == bad
    assert create(g.handle, C.byref(p), src, 3, dst, 5, None, 0, C.byref(h)) == bad
    assert create(g.handle, C.byref(p), src, 3, dst, 5, grp, 6, C.byref(h)) == bad  # n_groups > n_dst
    assert create(g.handle, C.byref(p), src, 3, dst, 5, None, 6, C.byref(h)) == bad
    grp[3] = 2  # a group id >= n_groups: the message names the position
    assert create(g.handle, C.byref(p), src, 3, dst, 5, grp, 2, C.byref(h)) == bad
    assert "destination 3" in eng.last_error()
    assert not h.value
    # the accessors on no plan
    n, ptr, nb = C.c_uint32(), C.c_void_p(), C.c_uint64()
    res = abi.mr_result()
    assert L.mr_nearest_records(None, None, 0) == bad
    assert L.mr_nearest_device_records(None, C.byref(ptr), C.byref(nb)) == bad
    assert L.mr_nearest_record_pitch(None, C.byref(n)) == bad
    assert L.mr_nearest_source_rows(None, C.byref(n), 1) == bad
    assert L.mr_nearest_label(None, 0, 0, C.byref(res), None, 0) == bad


def test_creation_without_a_device_fails_loudly(eng):
    m = SyntheticMap(7, campfires_per_homeland=1, seed=4)
    g = eng.MapGrid(m.cells())
    cells = m.all_indices()
    if eng.device_available():  # (the suite's CPU half on a GPU machine: creation works)
        assert eng.NearestPlan(g, Params(), cells[:2], cells[:5], [0, 1, 2, 3, 4]).record_pitch() == 8
        return
    with pytest.raises(eng.EngineError, match="NO_DEVICE"):
        eng.NearestPlan(g, Params(), cells[:2], cells[:5])
    with pytest.raises(eng.EngineError, match="NO_DEVICE"):
        eng.NearestPlan(g, Params(), cells[:2], cells[:5], [0, 1, 1, 0, 2])
    with pytest.raises(eng.EngineError, match="NO_DEVICE"):
        eng.FindPath(g).eval_nearest([CellIndex.center()], cells[:5])
    with pytest.raises(eng.EngineError, match="NO_DEVICE"):
        eng.FindPath(g).eval_nearest_poi([CellIndex.center()])


def test_poi_cells_in_row_major_order(eng):
    L = eng.lib()
    m = SyntheticMap(7, campfires_per_homeland=2, seed=7, fountains=3, forums=2)
    cells = m.cells()
    g = eng.MapGrid(cells)
    counts = {}
    for poi in (POI_NONE, POI_CAMPFIRE, POI_FOUNTAIN, POI_FORUM):
        want = [ci for ci, p in cells if p == poi]  # cells(): row-major
        assert g.poi_cells(poi) == want, poi
        counts[poi] = len(want)
    assert counts[POI_CAMPFIRE] == 8 and counts[POI_FOUNTAIN] == 3 and counts[POI_FORUM] == 2
    assert sum(counts.values()) == 49
    # a cap that is too small: the count is still reported and the first `cap` cells written
    n = C.c_uint32()
    out = (abi.mr_cell_index * 8)()
    assert L.mr_grid_poi_cells(g.handle, POI_CAMPFIRE, out, 3, C.byref(n)) == abi.MR_ERR_CAPACITY
    assert n.value == 8
    fires = g.poi_cells(POI_CAMPFIRE)
    assert [CellIndex(c.kind, c.sub, c.x, c.y) for c in out[:3]] == fires[:3]
    assert out[3].kind == 0 and out[3].x == 0 and out[3].y == 0  # nothing past the cap
    assert L.mr_grid_poi_cells(g.handle, POI_CAMPFIRE, None, 0, C.byref(n)) == abi.MR_ERR_CAPACITY and n.value == 8
    assert L.mr_grid_poi_cells(g.handle, POI_CAMPFIRE, out, 8, C.byref(n)) == abi.MR_OK and n.value == 8
    assert sorted(fires) == m.campfires()
    # poi = 4 is no kind; null arguments
    bad = abi.MR_ERR_INVALID_ARG
    assert L.mr_grid_poi_cells(g.handle, 4, out, 8, C.byref(n)) == bad
    assert L.mr_grid_poi_cells(None, POI_FORUM, out, 8, C.byref(n)) == bad
    assert L.mr_grid_poi_cells(g.handle, POI_FORUM, out, 8, None) == bad
    assert L.mr_grid_poi_cells(g.handle, POI_FORUM, None, 8, C.byref(n)) == bad
    with pytest.raises(eng.EngineError):
        g.poi_cells(4)
