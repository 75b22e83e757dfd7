"""CPU-side checks of the C-ABI library: it builds, loads, exports every
function include/marshrutka_pf.h declares, validates grids on the host, and
fails loudly (MR_ERR_NO_DEVICE) instead of falling back to the CPU."""
import ctypes as C
import os
import re

import pytest

from marshrutka_amd import abi
from crafted_records import LARGE_MONEY_PRICES, LARGE_MONEY_SCROLLS
from marshrutka_amd.abi import BLUE, CellIndex, Params
from marshrutka_amd.mapgen import SyntheticMap, to_html

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    from marshrutka_amd import build, pathfinder
    build.build()
    return pathfinder


def declared_functions():
    names = []
    for fn in os.listdir(os.path.join(ROOT, "include")):
        if fn.endswith(".h"):
            src = open(os.path.join(ROOT, "include", fn)).read()
            src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
            names += re.findall(r"^[A-Za-z_][\w \*]*?\b(mr_\w+)\s*\(", src, flags=re.M)
    return sorted(set(names))


def test_header_declares_api():
    names = declared_functions()
    assert "mr_find_path" in names and "mr_find_path_batch" in names and "mr_grid_create" in names
    assert len(names) >= 15


def test_library_exports_every_declared_symbol(eng):
    L = C.CDLL(eng.LIB_PATH)
    for name in declared_functions():
        assert hasattr(L, name), name
    assert sorted(declared_functions()) == sorted(eng.EXPORTED_SYMBOLS)


def test_abi_version_and_defaults(eng):
    L = eng.lib()
    assert L.mr_abi_version() == 7
    p = abi.mr_params()
    L.mr_params_default(C.byref(p))
    d = Params().to_c()
    for f, _ in abi.mr_params._fields_:
        if f in ("hq_position", "sort_by", "reserved"):
            continue
        assert getattr(p, f) == getattr(d, f), f
    assert list(p.sort_by) == [abi.SORT_LEGS, abi.SORT_MONEY]


def test_cache_live_without_a_device(eng):
    """mr_cache_live needs no device: with no plan made it reports no blocks (either
    output may be NULL)."""
    L = eng.lib()
    blocks, nbytes = C.c_uint64(99), C.c_uint64(99)
    L.mr_cache_live(C.byref(blocks), C.byref(nbytes))
    assert (blocks.value, nbytes.value) == (0, 0)
    L.mr_cache_live(None, None)
    L.mr_cache_trim()
    L.mr_cache_live(C.byref(blocks), None)
    assert blocks.value == 0


def test_grid_validation_on_host(eng):
    m = SyntheticMap(9, campfires_per_homeland=2, seed=1)
    g = eng.MapGrid(m.cells())
    assert g.square_size == 9 and g.homeland_size() == 4
    cells = m.cells()
    # not square
    with pytest.raises(eng.EngineError, match="INVALID_GRID"):
        eng.MapGrid(cells[:-1])
    # duplicate index
    bad = list(cells)
    bad[0] = bad[1]
    with pytest.raises(eng.EngineError, match="INVALID_GRID"):
        eng.MapGrid(bad)
    # labels that are not a consistent 4-grid (two homeland cells swapped)
    bad = list(cells)
    bad[0], bad[10] = bad[10], bad[0]
    with pytest.raises(eng.EngineError, match="INVALID_GRID"):
        eng.MapGrid(bad)
    # a homeland without campfires: the reference panics (src/grid.rs:209)
    m2 = SyntheticMap(7, campfires_per_homeland=0, seed=0,
                      extra_campfires=[CellIndex.homeland(h, 3, 3) for h in range(3)])
    with pytest.raises(eng.EngineError, match="INVALID_GRID"):
        eng.MapGrid(m2.cells())


def test_rotated_layout_is_accepted(eng):
    # any orientation whose labels are consistent with the index adjacency is a valid map
    # (grid creation only; all eight orientations are solved, device-grouped and given a region
    # table in tests/test_gpu_irregular_maps.py, with the references pinned by
    # tests/test_irregular_maps.py)
    m = SyntheticMap(7, campfires_per_homeland=1, seed=4)
    S = 7
    cells = m.cells()
    rot = [cells[(S - 1 - (i % S)) * S + (i // S)] for i in range(S * S)]  # transpose + flip
    eng.MapGrid(rot)


def test_no_cpu_fallback_without_device(eng):
    if eng.device_available():
        pytest.skip("a device is visible")
    m = SyntheticMap(7, campfires_per_homeland=1, seed=4)
    g = eng.MapGrid(m.cells())
    fp = eng.FindPath(g)
    with pytest.raises(eng.EngineError, match="NO_DEVICE"):
        fp.eval(CellIndex.homeland(BLUE, 1, 1), CellIndex.center())


def test_html_writer_schema():
    m = SyntheticMap(5, campfires_per_homeland=1, seed=2)
    html = to_html(m)
    assert html.count('class="map-cell"') == 25
    assert '<div class="top-right-text">0#0</div>' in html


def _ranks(m):
    """CellIndex -> rank (position in the derived Ord, src/index.rs:41-46)."""
    cells = sorted(m.all_indices(), key=lambda c: (c.kind, c.sub, c.x, c.y))
    return {c: i for i, c in enumerate(cells)}


def test_decode_records_on_host(eng):
    """mr_decode_records: compact records as another rank gathers them (result
    record, command slots, overflow pool) decode to full labels without a device."""
    import numpy as np
    from marshrutka_amd.abi import GREEN, Command, TotalCost
    m = SyntheticMap(7, campfires_per_homeland=1, seed=4)
    g = eng.MapGrid(m.cells())
    rk = _ranks(m)
    b33, c, g33 = CellIndex.homeland(BLUE, 3, 3), CellIndex.center(), CellIndex.homeland(GREEN, 3, 3)
    car = lambda d, five: (3 << 29) | (d << 1) | five  # noqa: E731  Caravan payload: d << 1 | coef==5
    # (0, 42, 2880, [Caravan{1440,12} B3#3->0#0, Caravan{1440,30} 0#0->G3#3])
    want = TotalCost(0, 42, 2880, [Command(3, 1440, 0, 12, 0, b33, c), Command(3, 1440, 0, 30, 0, c, g33)])
    cmds = [[car(6, 0), rk[b33], rk[c], 0], [car(6, 1), rk[c], rk[g33], 0]]
    p = Params(route_guru=0)
    # three records, max_cmds 2: the label in its slots, a NOT_FOUND record, the label
    # again but tagged into the overflow pool at offset 3
    res = np.array([[0, 42, 2880, (16 << 16) | 2], [0, 0, 0, 17 << 16], [0, 42, 2880, ((16 + 64) << 16) | 2]],
                   dtype=np.uint32)
    slots = np.zeros((3, 2, 4), dtype=np.uint32)
    slots[0] = cmds
    slots[2, 0] = [0xFFFFFFFF, 3, 2, 0]
    pool = np.zeros((5, 4), dtype=np.uint32)
    pool[3:5] = cmds
    out = eng.decode_records(g, p, res, slots, 3, 2, pool)
    assert out[0].as_tuple() == want.as_tuple()
    assert out[1] is None
    assert out[2].as_tuple() == want.as_tuple()
    # a tag that points past the pool, and a command naming no cell, are errors
    with pytest.raises(eng.EngineError, match="DEVICE"):
        eng.decode_records(g, p, res, slots, 3, 2, pool[:4])
    bad = slots.copy()
    bad[0, 1, 2] = 49
    with pytest.raises(eng.EngineError, match="DEVICE"):
        eng.decode_records(g, p, res, bad, 3, 2, pool)


def test_decode_wire_on_host(eng):
    """mr_decode_wire: wire rows (first `from` rank | count, then {kind|payload, `to`}) with
    the metrics left out decode to the same full labels as the compact records."""
    import numpy as np
    from marshrutka_amd.abi import GREEN, Command, TotalCost
    m = SyntheticMap(7, campfires_per_homeland=1, seed=4)
    g = eng.MapGrid(m.cells())
    rk = _ranks(m)
    b33, c, g33 = CellIndex.homeland(BLUE, 3, 3), CellIndex.center(), CellIndex.homeland(GREEN, 3, 3)
    car = lambda d, five: (3 << 29) | (d << 1) | five  # noqa: E731
    want = TotalCost(0, 42, 2880, [Command(3, 1440, 0, 12, 0, b33, c), Command(3, 1440, 0, 30, 0, c, g33)])
    p = Params(route_guru=0)
    # max_cmds 2: the label in its slots, NOT_FOUND, the label in the pool at offset 3,
    # a capacity row (what the encoder writes for a label past the pool)
    st = lambda s_: (65 + 32 + s_) << 25  # noqa: E731
    rows = np.array([[rk[b33] | 2 << 25, car(6, 0), rk[c], car(6, 1), rk[g33]],
                     [st(1), 0, 0, 0, 0],
                     [rk[b33] | 64 << 25, 3, 2, 0, 0],
                     [st(-4), 0, 0, 0, 0]], dtype=np.uint32)
    pool = np.zeros((5, 2), dtype=np.uint32)
    pool[3:5] = [[car(6, 0), rk[c]], [car(6, 1), rk[g33]]]
    out, cmds = eng.decode_wire_raw(g, p, rows, 4, 2, pool)
    lab = [eng.result_from_c(out[k], cmds) if out[k].status == 0 else out[k].status for k in range(4)]
    assert lab[0].as_tuple() == want.as_tuple() and lab[2].as_tuple() == want.as_tuple()
    assert lab[1] == 1 and lab[3] == -4
    assert eng.wire_row_words(4) == 9  # 36 B a query at max_cmds 4
    with pytest.raises(eng.EngineError, match="DEVICE"):  # a pool reference past the pool
        eng.decode_wire_raw(g, p, rows, 4, 2, pool[:4])


@pytest.mark.parametrize("ff,rg", [(0, 0), (1, 3), (2, 5), (3, 1), (7, 2)])
def test_decode_wire_matches_decode_records(eng, ff, rg):
    """Random command chains of every kind: the wire decoder's recomputed metrics
    (Fleetfoot ceil per StandardMove run, caravan time and coefficient, scroll prices)
    and commands equal mr_decode_records over the same labels with the metrics given."""
    from crafted_records import craft
    m = SyntheticMap(15, campfires_per_homeland=3, seed=ff + 11)
    g = eng.MapGrid(m.cells())
    V = len(m.all_indices())
    p = Params(fleetfoot=ff, route_guru=rg, scroll_of_escape_cost=7, scroll_of_escape_hq_cost=11,
               scroll_of_escape_forum_cost=13)
    n, mc = 300, 3
    c = craft(n, mc, range(0, 7), V, p, seed=ff * 31 + rg)
    a_out, a_pool = eng.decode_records_raw(g, p, c.res, c.slots, n, mc, c.ovf)
    b_out, b_pool = eng.decode_wire_raw(g, p, c.rows, n, mc, c.wpool)
    for k in range(n):
        fa = [getattr(a_out[k], f) for f, _ in a_out[k]._fields_]
        fb = [getattr(b_out[k], f) for f, _ in b_out[k]._fields_]
        assert fa == fb, k
    ncmd = sum(a_out[k].n_commands for k in range(n))
    assert bytes(memoryview(a_pool)[:ncmd]) == bytes(memoryview(b_pool)[:ncmd])


def _decode_raw(eng, which, g, p, a, b, n, mc, cap):
    """mr_decode_records (a, b: result records and command slots; c: overflow pool) or
    mr_decode_wire (a: rows; c: wire pool) straight through the C ABI with a command pool of
    `cap` entries: (returned status, mr_last_error text, the n results' fields, the pool)."""
    import numpy as np
    from marshrutka_amd.abi import mr_command, mr_result
    out, pool = (mr_result * max(n, 1))(), (mr_command * max(cap, 1))()
    prm = p.to_c()
    arr = [np.ascontiguousarray(x, dtype=np.uint32) for x in (a, *b)]
    ptr = [x.ctypes.data if x.size else None for x in arr]
    if which == "records":
        st = eng.lib().mr_decode_records(g.handle, C.byref(prm), ptr[0], ptr[1], n, mc, ptr[2], arr[2].size // 4, out,
                                         pool, cap)
    else:
        st = eng.lib().mr_decode_wire(g.handle, C.byref(prm), ptr[0], n, mc, ptr[1], arr[1].size // 2, out, pool, cap)
    res = [(r.legs, r.money, r.time_s, r.n_commands, r.command_offset, r.status) for r in out[:n]]
    return st, (eng.last_error() if st < 0 else ""), res, pool


@pytest.fixture(scope="module")
def kat7(eng):
    """The 7-square map, max_cmds 2 and SURVEY 8c KAT7's two caravans, as compact commands,
    as wire commands and as the mr_commands they expand to."""
    from marshrutka_amd.abi import GREEN
    m = SyntheticMap(7, campfires_per_homeland=1, seed=4)
    rk = _ranks(m)
    b33, c, g33 = CellIndex.homeland(BLUE, 3, 3), CellIndex.center(), CellIndex.homeland(GREEN, 3, 3)
    car = lambda d, five: (3 << 29) | (d << 1) | five  # noqa: E731
    cmd4 = [[car(6, 0), rk[b33], rk[c], 0], [car(6, 1), rk[c], rk[g33], 0]]
    full = [(3, 0, 12, 0, 1440, b33, c), (3, 0, 30, 0, 1440, c, g33)]
    return eng.MapGrid(m.cells()), Params(route_guru=0), rk[b33], cmd4, full


def _commands(pool, lo, hi):
    return [(c.kind, c.legs, c.money, c.fleetfoot, c.time_s, CellIndex.from_c(c.from_), CellIndex.from_c(c.to))
            for c in pool[lo:hi]]


def test_decoders_malformed_command_and_short_pool(eng, kat7):
    """A record whose second command names cell 49 of 49, after a well-formed record.  Both
    host decoders check a command only where they write it: with a pool of 3 commands the
    second record does not fit, nothing of it is read, and the status is MR_ERR_CAPACITY (-4),
    not MR_ERR_DEVICE; the wire decoder still sums the row's metrics.  With room for it the
    command is found: MR_ERR_DEVICE, "command names no cell", the commands before it written."""
    import numpy as np
    g, p, first, cmd4, full = kat7
    bad = [cmd4[0], [cmd4[1][0], cmd4[1][1], 49, 0]]
    res = np.array([[0, 42, 2880, (16 << 16) | 2], [0, 42, 2880, (16 << 16) | 2]], dtype=np.uint32)
    slots = np.array([cmd4, bad], dtype=np.uint32)
    rows = np.array([[first | 2 << 25, cmd4[0][0], cmd4[0][2], cmd4[1][0], cmd4[1][2]],
                     [first | 2 << 25, bad[0][0], bad[0][2], bad[1][0], bad[1][2]]], dtype=np.uint32)
    none = np.zeros(0, dtype=np.uint32)
    want = [(0, 42, 2880, 2, 0, 0), (0, 42, 2880, 2, 2, 0)]
    for which, a, b in (("records", res, (slots, none)), ("wire", rows, (none,))):
        st, msg, out, pool = _decode_raw(eng, which, g, p, a, b, 2, 2, 3)
        assert (st, out) == (abi.MR_ERR_CAPACITY, want), which
        assert _commands(pool, 0, 2) == full and bytes(pool[2]) == bytes(40), which
        st, msg, out, pool = _decode_raw(eng, which, g, p, a, b, 2, 2, 4)
        assert (st, msg) == (abi.MR_ERR_DEVICE, "command names no cell"), which
        assert _commands(pool, 0, 3) == full + full[:1], which


def test_decoders_overflow_tag_at_max_cmds_0(eng, kat7):
    """max_cmds 0 leaves no slot for an overflow tag: a record (or wire row) that claims its
    commands are in the pool is malformed, whatever the pool holds."""
    import numpy as np
    g, p, first, cmd4, _ = kat7
    res = np.array([[0, 42, 2880, ((16 + 64) << 16) | 2]], dtype=np.uint32)
    ovf = np.array(cmd4, dtype=np.uint32)
    st, msg, _, _ = _decode_raw(eng, "records", g, p, res, (np.zeros(0, dtype=np.uint32), ovf), 1, 0, 4)
    assert (st, msg) == (abi.MR_ERR_DEVICE, "overflow pool record")
    rows = np.array([[first | 64 << 25]], dtype=np.uint32)
    st, msg, _, _ = _decode_raw(eng, "wire", g, p, rows, (ovf[:, [0, 2]],), 1, 0, 4)
    assert (st, msg) == (abi.MR_ERR_DEVICE, "wire pool record")


def test_decoders_status_rows_among_labels(eng, kat7):
    """Status rows before, between and after labels: a status row's command_offset is the
    count of the commands before it (0 for the first row), a NOT_FOUND row is no error, a
    compact record of another status keeps its command count (a wire row carries none), and
    the status returned is the first error in row order."""
    import numpy as np
    g, p, first, cmd4, full = kat7
    res = np.array([[0, 0, 0, 17 << 16 | 9], [0, 42, 2880, (16 << 16) | 2], [7, 8, 9, (16 - 4) << 16 | 5],
                    [0, 42, 2880, (16 << 16) | 2], [0, 0, 0, (16 - 3) << 16]], dtype=np.uint32)
    slots = np.zeros((5, 2, 4), dtype=np.uint32)
    slots[1] = slots[3] = cmd4
    st_row = lambda s_: [(65 + 32 + s_) << 25, 0, 0, 0, 0]  # noqa: E731
    lab = [first | 2 << 25, cmd4[0][0], cmd4[0][2], cmd4[1][0], cmd4[1][2]]
    rows = np.array([st_row(1), lab, st_row(-4), lab, st_row(-3)], dtype=np.uint32)
    none = np.zeros(0, dtype=np.uint32)
    label = lambda off: (0, 42, 2880, 2, off, 0)  # noqa: E731
    want = {"records": [(0, 0, 0, 0, 0, 1), label(0), (7, 8, 9, 5, 2, -4), label(2), (0, 0, 0, 0, 4, -3)],
            "wire": [(0, 0, 0, 0, 0, 1), label(0), (0, 0, 0, 0, 2, -4), label(2), (0, 0, 0, 0, 4, -3)]}
    for which, a, b in (("records", res, (slots, none)), ("wire", rows, (none,))):
        st, _, out, pool = _decode_raw(eng, which, g, p, a, b, 5, 2, 4)
        assert (st, out) == (abi.MR_ERR_CAPACITY, want[which]), which
        assert _commands(pool, 0, 4) == full + full, which


WIDE_PARAMS = [Params(),
               Params(fleetfoot=2, sort_by=(abi.SORT_TIME, abi.SORT_MONEY), route_guru=3, scroll_of_escape_cost=7,
                      scroll_of_escape_hq_cost=11, scroll_of_escape_forum_cost=13),
               # three scrolls a record at 1.4e9 each: label money up to 4.2e9, bit 31 set
               Params(fleetfoot=1, sort_by=(abi.SORT_MONEY, abi.SORT_LEGS), route_guru=2, **LARGE_MONEY_PRICES)]
WIDE_MAX_SCROLLS = [None, None, LARGE_MONEY_SCROLLS]


@pytest.mark.parametrize("params,max_scrolls", list(zip(WIDE_PARAMS, WIDE_MAX_SCROLLS)),
                         ids=["default", "ff2-time-rg3", "money-4.2e9"])
@pytest.mark.parametrize("mc", [31, 32, 63])
def test_host_decoders_at_wide_max_cmds(eng, mc, params, max_scrolls):
    """mr_decode_records and mr_decode_wire at the widths where the wire encoder changes
    shape (31: the last 256-thread staged row, 32: the first 64-thread one, 63: the largest
    in-slot count the wire header's 7-bit code carries) over crafted records: labels of 0,
    1, mc - 1, mc and mc + 1 commands among random lengths up to mc + 8 (the longer ones
    in the pools), and NOT_FOUND records.  Both equal the crafted labels: every mr_result
    field, and the command pool byte for byte."""
    from crafted_records import assert_same_bytes, cells_by_rank, craft, decoded_labels, edge_lengths
    m = SyntheticMap(15, campfires_per_homeland=3, seed=11)
    g = eng.MapGrid(m.cells())
    cells = cells_by_rank(m)
    n = 300
    c = craft(n, mc, range(0, mc + 9), len(cells), params, seed=1000 + mc, max_scrolls=max_scrolls)
    want = c.labels()
    if max_scrolls is not None:  # the set is there for money words with bit 31 set
        assert sum(w is not None and w[1] >= 1 << 31 for w in want) >= n // 4
    lens = {len(w[3]) for w in want if w is not None}
    assert set(edge_lengths(mc, True)) <= lens and sum(w is None for w in want) >= 3
    assert len(c.ovf) > mc and (c.res[:, 3] >> 16 == 80).sum() >= 5
    want_res, want_pool, want_st = c.pack(cells)
    assert want_st == abi.MR_OK
    for what, (out, pool) in (("mr_decode_records", eng.decode_records_raw(g, params, c.res, c.slots, n, mc, c.ovf)),
                              ("mr_decode_wire", eng.decode_wire_raw(g, params, c.rows, n, mc, c.wpool))):
        assert decoded_labels(out, pool, n, cells) == want, what
        assert_same_bytes(out, pool, want_res, want_pool, what)


def test_labels_digest_follows_query_order(eng):
    """labels_digest (the N > 1 gather check): the same labels stored in another
    order hash alike once the order is given, and differently without it."""
    import numpy as np
    from marshrutka_amd.abi import mr_command, mr_result
    n, perm = 4, [2, 0, 3, 1]
    res, pool = (mr_result * n)(), (mr_command * (2 * n))()
    res2, pool2 = (mr_result * n)(), (mr_command * (2 * n))()
    for i in range(n):
        res[i].legs, res[i].n_commands, res[i].command_offset = i, 2, 2 * i
        for c in range(2):
            pool[2 * i + c].kind, pool[2 * i + c].money = c, 10 * i + c
    for k, i in enumerate(perm):  # record k holds query i
        res2[k].legs, res2[k].n_commands, res2[k].command_offset = i, 2, 2 * k
        for c in range(2):
            pool2[2 * k + c].kind, pool2[2 * k + c].money = c, 10 * i + c
    inv = np.empty(n, dtype=np.int64)
    inv[np.array(perm)] = np.arange(n)
    assert eng.labels_digest(res2, pool2, n, inv) == eng.labels_digest(res, pool, n)
    assert eng.labels_digest(res2, pool2, n) != eng.labels_digest(res, pool, n)
