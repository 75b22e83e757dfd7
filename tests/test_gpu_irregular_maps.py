"""Parity on irregular maps and on every map orientation (irregular_maps.py).

The rest of the GPU suite draws its maps from SyntheticMap(size, campfires_per_homeland=k):
equal counts in the four homelands, campfires on homeland cells only, the one standard
orientation.  Here: unequal counts (the table's shape changes with params.homeland, and
more than hub_lane_kernel's six regions in one homeland), campfires on border cells and on
the Center (caravan hubs that are no SoE target), regions made of specials only, and the
seven other orientations, whose cells the kernels reach through the {sinfo, rank} table
and the layout's unit steps instead of the closed forms of the standard layout.

The bar is the parity suite's: bit-exact (legs, money, time, every command).  The
reference is the C++ oracle on the standard and the mirrored orientations and py_ref on
the transposed ones ("Grid orientation"); test_irregular_maps.py pins on the CPU that the
two agree where both are used, that they differ where only py_ref is, and the shape facts
the kernel-choice assertions below rest on."""
import random

import numpy as np
import pytest

import irregular_maps as im
from golden_util import as_expected
from marshrutka_amd.abi import BLUE, Params, result_from_c
from marshrutka_amd.mapgen import SyntheticMap, random_query_cells
from test_gpu_decode_widths import DeviceWords, hip  # noqa: F401  (hip: a fixture)
from test_gpu_dev_group import _run, _same
from test_gpu_parity import eng, grid_state  # noqa: F401  (fixtures: the 19 solver modes)
from test_gpu_region_table import _check as check_region_table
from test_gpu_sssp import all_labels_match, mode  # noqa: F401  (mode: a fixture, auto / fallback / sssp)

pytestmark = pytest.mark.gpu

KERNEL_ENV = ("MR_HUB_LANE", "MR_HUB_LANE_MIN", "MR_HUB_GROUP", "MR_HUB_GROUP_FORCE", "MR_HUB_FALLBACK_ALL", "MR_ALGO",
              "MR_HUB_WIDE", "MR_HUB_SPW", "MR_LANE_NONLIN", "MR_RANK_TABLE", "MR_GRID_STATE", "MR_DEV_GROUP",
              "MR_HOST_DECODE", "MR_FETCH_WIRE")

_oracle = {}


def oracle_labels(oracle_lib, name, k, pi, qs_key="all"):
    """The oracle's labels on orientation k of a named map, computed once: of
    queries_for(name), or of capped_queries(name, n) with qs_key = n."""
    key = (name, k, pi, qs_key)
    if key not in _oracle:
        qs = im.queries_for(name) if qs_key == "all" else im.capped_queries(name, qs_key)
        og = oracle_lib.OracleGrid(im.oriented(name, k).cells())
        _oracle[key] = [as_expected(e) for e in og.find_path_batch(im.params_for(im.get_map(name))[pi], qs, threads=0)]
    return _oracle[key]


def _bad(qs, exp, got):
    return [(q, e, as_expected(r)) for q, e, r in zip(qs, exp, got) if as_expected(r) != e]


def _clear(monkeypatch):
    for v in KERNEL_ENV:
        monkeypatch.delenv(v, raising=False)


def _plan_labels(eng, g, params, qs):
    plan = eng.Plan(g, params, qs)
    plan.run()
    got = plan.fetch()
    return got, plan.stats()


@pytest.mark.parametrize("name", im.CATALOGUE)
def test_parity_on_the_catalogue(eng, oracle_lib, grid_state, name):  # noqa: F811
    """Every solver path on every catalogue map, every parameter set."""
    m = im.get_map(name)
    g = eng.MapGrid(m.cells())
    qs = im.queries_for(name)
    for pi, params in enumerate(im.params_for(m)):
        got = eng.FindPath.with_params(g, params).eval_batch(qs)
        bad = _bad(qs, oracle_labels(oracle_lib, name, 0, pi), got)
        assert not bad, f"{name} {grid_state} params {pi} {params}: {len(bad)}/{len(qs)} mismatches; first: {bad[0]}"


LANE_CASES = ["six", "seven", "unequal", "border1", "border_far", "center_fire", "ties", "s5_full"]


@pytest.mark.parametrize("name", LANE_CASES)
def test_lane_kernel_layout_gate(eng, oracle_lib, monkeypatch, name):  # noqa: F811
    """MR_HUB_LANE=1 asks for hub_lane_kernel wherever it applies; lane_layout_ok must keep it
    off a plan whose border-1 cell is a caravan hub or whose query homeland has more than
    six campfires, and LaneHub::from_s trusts that.  Each parameter set's plan is on the
    lane kernel exactly when irregular_maps.lane_layout_expected says so (six / Blue: yes;
    seven / Blue, unequal / Blue, border1: no; unequal with Red, Green or Yellow: yes;
    center_fire: the Center is a hub in every plan and no border-1 cell is, so yes), and
    the labels are the oracle's either way.  The queries without the 40-destination
    source: every source then has at most 32."""
    _clear(monkeypatch)
    monkeypatch.setenv("MR_HUB_LANE", "1")
    m = im.get_map(name)
    g = eng.MapGrid(m.cells())
    qs = im.queries_for(name)[:-40]
    assert max(sum(a == s for a, _ in qs) for s in {a for a, _ in qs}) <= 32
    want = {"six": True, "seven": False, "unequal": False, "border1": False, "center_fire": True}
    assert name not in want or im.lane_layout_expected(m, BLUE) == want[name]
    for pi, params in enumerate(im.params_for(m)):
        got, st = _plan_labels(eng, g, params, qs)
        bad = _bad(qs, oracle_labels(oracle_lib, name, 0, pi)[:-40], got)
        assert not bad, f"{name} params {pi}: {len(bad)}/{len(qs)} mismatches; first: {bad[0]}; {st}"
        assert st["solver"] == "hub", (pi, st)
        if not im.lane_layout_expected(m, params.homeland):
            assert st["lane_sources"] == 0 and st["lanes_per_source"] != 1, (pi, st)
        elif params.fleetfoot == 0:
            assert st["lane_sources"] == st["num_sources"] and st["lanes_per_source"] == 1, (pi, st)
        else:
            print(f"{name} params {pi} (Fleetfoot {params.fleetfoot}): {st}")
    # the whole batch: the 40-destination source is the one the lane kernel leaves to hub_kernel
    params = im.params_for(m)[0]
    got, st = _plan_labels(eng, g, params, im.queries_for(name))
    assert not _bad(im.queries_for(name), oracle_labels(oracle_lib, name, 0, 0), got)
    if im.lane_layout_expected(m, BLUE):
        assert st["lane_sources"] == st["num_sources"] - 1 and st["lanes_per_source"] == 1, st


@pytest.mark.parametrize("name", im.CATALOGUE)
def test_default_plan_runs_the_group_kernel(eng, oracle_lib, monkeypatch, name):  # noqa: F811
    """With no switches a plan this small is not the lane kernel's (too few sources): the
    Legs-first linear plan runs on hub_group_kernel, whatever its table layout.  The plans
    the lane kernel's gate is tested on hand no source over; on the other maps a blocker
     may send one to the SSSP kernel, which is no error."""
    _clear(monkeypatch)
    m = im.get_map(name)
    qs = im.queries_for(name)
    got, st = _plan_labels(eng, eng.MapGrid(m.cells()), im.params_for(m)[0], qs)
    print(f"{name}: default plan {st}")
    assert st["solver"] == "hub" and st["lanes_per_source"] in (8, 16, 32) and st["lane_sources"] == 0, st
    assert st["fallback_sources"] == 0 or name not in ("six", "seven", "unequal", "border1", "center_fire"), st
    assert not _bad(qs, oracle_labels(oracle_lib, name, 0, 0), got)


@pytest.mark.parametrize("group", [8, 16, 32])
@pytest.mark.parametrize("name", ["unequal", "border1", "ties"])
def test_group_kernel_takes_any_layout(eng, oracle_lib, monkeypatch, name, group):  # noqa: F811
    """hub_group_kernel's claim (roles as run-time bits, any table layout) on the layouts the
    lane kernel refuses, at each group size: the linear plans report G lanes a source."""
    _clear(monkeypatch)
    monkeypatch.setenv("MR_HUB_GROUP_FORCE", "1")
    monkeypatch.setenv("MR_HUB_GROUP", str(group))
    m = im.get_map(name)
    g = eng.MapGrid(m.cells())
    qs = im.queries_for(name)
    for pi, params in enumerate(im.params_for(m)):
        got, st = _plan_labels(eng, g, params, qs)
        bad = _bad(qs, oracle_labels(oracle_lib, name, 0, pi), got)
        assert not bad, f"{name} G={group} params {pi}: {len(bad)}/{len(qs)} mismatches; first: {bad[0]}; {st}"
        if params.fleetfoot == 0:
            assert st["solver"] == "hub" and st["lanes_per_source"] == group, (pi, st)


def test_homeland_changes_the_table_shape(eng, monkeypatch):  # noqa: F811
    _clear(monkeypatch)
    m = im.get_map("unequal")
    g = eng.MapGrid(m.cells())
    qs = im.queries_for("unequal")[:50]
    shapes = []
    for h in range(4):
        st = eng.Plan(g, Params(homeland=h), qs).stats()
        shapes.append((st["num_regions"], st["num_specials"]))
    assert shapes == [(9, 18), (1, 18), (2, 18), (1, 18)], shapes


@pytest.mark.parametrize("name", ["unequal", "border1", "ties", "s3"])
def test_all_destinations(eng, oracle_lib, mode, name):  # noqa: F811
    """An all-destinations plan from the Center, a border campfire (a border-1 cell where the
    map has none), a homeland campfire and a plain cell: every cell's label and record."""
    m = im.get_map(name)
    prm = im.params_for(m)
    for params in (prm[0], prm[1], prm[2]) if m.size > 3 else prm:
        all_labels_match(eng, oracle_lib, m, params, im.sssp_sources(m))


@pytest.mark.parametrize("name", ["unequal", "ties", "corners", "s3", "s5_full"])
def test_region_table(eng, oracle_lib, name):  # noqa: F811
    check_region_table(eng, oracle_lib, im.get_map(name), range(4))


@pytest.mark.parametrize("k", range(1, 8))
def test_region_table_every_orientation(eng, oracle_lib, k):  # noqa: F811
    """The regions are the direct argmin over the cells as given (region_util.cell_regions
    works from positions), so one reference serves the mirrored and the transposed layouts."""
    check_region_table(eng, oracle_lib, im.oriented("ties", k), range(4))


@pytest.mark.parametrize("name", im.ORIENTED)
def test_mirrored_orientations(eng, oracle_lib, grid_state, name):  # noqa: F811
    """k = 1..3: the oracle's labels on the same cells, which are also the engine's own on
    the standard orientation."""
    m = im.get_map(name)
    qs = im.queries_for(name)
    grids = [eng.MapGrid(im.oriented(name, k).cells()) for k in range(4)]
    for pi, params in enumerate(im.params_for(m)):
        own = [as_expected(r) for r in eng.FindPath.with_params(grids[0], params).eval_batch(qs)]
        for k in im.MIRRORED:
            got = eng.FindPath.with_params(grids[k], params).eval_batch(qs)
            bad = _bad(qs, oracle_labels(oracle_lib, name, k, pi), got)
            assert not bad, f"{name} k={k} {grid_state} params {pi}: {len(bad)}/{len(qs)} mismatches; first: {bad[0]}"
            assert [as_expected(r) for r in got] == own, (name, k, pi)


N_TRANSPOSED = 200  # py_ref is the slow side: 2 ms a query at S = 9, 5 at S = 15, once per session


@pytest.mark.parametrize("k", im.TRANSPOSED)
@pytest.mark.parametrize("name", im.ORIENTED)
def test_transposed_orientations(eng, grid_state, name, k):  # noqa: F811
    """k = 4..7 against py_ref (the reference's search over the nearest campfires of its own
    nearest_campfire function): the Blue, Red and Green parameter sets, and set 4, the
    Fleetfoot plan that the group kernels take."""
    qs = im.capped_queries(name, N_TRANSPOSED)
    g = eng.MapGrid(im.oriented(name, k).cells())
    for pi in (0, 1, 2, 4):
        params = im.params_for(im.get_map(name))[pi]
        got = eng.FindPath.with_params(g, params).eval_batch(qs)
        bad = _bad(qs, im.py_ref_labels(name, k, pi, N_TRANSPOSED), got)
        assert not bad, f"{name} k={k} {grid_state} params {pi}: {len(bad)}/{len(qs)} mismatches; first: {bad[0]}"


N_PY_REF_65 = 60  # of the 400 sampled labels on the transposed 65 x 65 map (py_ref: 50 ms each there)


@pytest.mark.parametrize("k", [3, 5])
def test_c2_map_oriented(eng, oracle_lib, monkeypatch, k):  # noqa: F811
    """The 65 x 65 benchmark map flipped both ways (k = 3) and transposed with a flip (k = 5),
    10 000 queries: device grouping (cells looked up through the layout's unit steps) gives
    the host grouping's bytes, by default and on the lane kernel, which takes the whole
    plan; 400 sampled labels equal the orientation's reference (k = 3: the oracle; k = 5:
    py_ref, N_PY_REF_65 of the 400)."""
    _clear(monkeypatch)
    m = im.Oriented(SyntheticMap(65, campfires_per_homeland=4, seed=2024), k)
    arr = m.cells_array()
    g = eng.MapGrid.from_array(arr)
    src, dst = random_query_cells(m.base, 10_000, 77)
    q = m.query_array(src, dst, arr)
    params = Params()
    a = _run(eng, monkeypatch, True, g, params, q)
    b = _run(eng, monkeypatch, False, g, params, q)
    _same(a, b)
    la = _run(eng, monkeypatch, True, g, params, q, env=(("MR_HUB_LANE", "1"),))
    lb = _run(eng, monkeypatch, False, g, params, q, env=(("MR_HUB_LANE", "1"),))
    _same(la, lb)
    assert la["stats"]["lanes_per_source"] == 1 and la["stats"]["lane_sources"] > 0, la["stats"]
    _clear(monkeypatch)
    cells = m.all_indices()
    pick = random.Random(k).sample(range(len(q)), 400 if k == 3 else N_PY_REF_65)
    qs = [(cells[src[i]], cells[dst[i]]) for i in pick]
    if k == 3:
        exp = [as_expected(e) for e in oracle_lib.OracleGrid.from_array(arr).find_path_batch(params, qs, threads=0)]
    else:
        exp = im.py_ref_some(m.base, k, params, qs)
    for env in ((), (("MR_HUB_LANE", "1"),)):
        for var, v in env:
            monkeypatch.setenv(var, v)
        got = eng.FindPath.with_params(g, params).eval_batch(qs)
        bad = _bad(qs, exp, got)
        assert not bad, f"k={k} {env}: {len(bad)}/{len(qs)} mismatches; first: {bad[0]}"


def test_wire_round_trip_mirrored(eng, oracle_lib, hip, monkeypatch):  # noqa: F811
    """mr_plan_wire_records then mr_decode_wire on a map flipped both ways (the decoder names
    cells by rank through the grid's rank table): the plan's own fetch and the oracle."""
    _clear(monkeypatch)
    name, k, pi, mc = "unequal", 3, 1, 2
    m = im.get_map(name)
    g = eng.MapGrid(im.oriented(name, k).cells())
    params, qs = im.params_for(m)[pi], im.queries_for(name)
    n, rw, pcap = len(qs), eng.wire_row_words(mc), 8 * len(qs)
    wbuf = DeviceWords(hip, n * rw + 2 * pcap)
    try:
        plan = eng.Plan(g, params, qs, max_cmds=mc)
        plan.run()
        plan.wire_records(wbuf.ptr.value, wbuf.ptr.value + n * rw * 4, pcap)
        plan.wait()
        host = wbuf.read()
        out, cmds = eng.decode_wire_raw(g, params, host[:n * rw], n, mc, host[n * rw:])
        q_of = plan.record_queries()
        got = [None] * n
        for r in range(n):
            assert out[r].status == 0, (r, out[r].status)
            got[q_of[r]] = as_expected(result_from_c(out[r], cmds))
        assert got == [as_expected(r) for r in plan.fetch()]
        assert got == oracle_labels(oracle_lib, name, k, pi)
        assert any(len(e[3]) > mc for e in got)  # some labels went through the wire pool
        del plan
    finally:
        wbuf.free()
