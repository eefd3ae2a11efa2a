"""GPU tests of the ordered compaction at the edges of its pipelined kernels
(wx_project_compact_deep, and WX_CM_DEEP behind SELECT, the window broadcast
and the join probe), over tables built tile by tile (tests/compact_layouts.py).

A compaction launches min(tiles, resident workgroups) workgroups, so on a
table a test can afford every workgroup runs one or two tiles and the
pipeline's steady state -- iteration k >= 2 with three tiles in flight: t_{k-2}
written out of the stage buffer that t_k then overwrites -- is never reached.
WARPDB_COMPACT_GRID caps the grid (1: one workgroup runs every tile in order),
wx_compact_last_launch says what a call launched, and the layouts choose every
tile's passing count, hence the head / 16-byte body / tail split of its output
run, the look-back's path over empty tiles and who writes the count.

Every case compares values, row ids and counts with a CPU reference, bit for
bit: the rows with numpy (np.nonzero of the layout's keep mask), the plain
expressions with oracle_lib.project_filter, window and join outputs with the
numpy expectations of test_gpu_window / test_gpu_join.  Outputs are prefilled
with NaN / -1 / -7 sentinels and must be untouched at positions >= count and
in front of an offset pointer.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import pytest

import compact_layouts as cl
import oracle_lib as ora
from test_gpu_join import AB as JOIN_EXPRS, expected as join_expected
from test_gpu_parity import bits, dev_table, launch
from test_gpu_window import ITEM1, PLAIN1, expected as window_expected

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from warpdb_amd import _warpexec as wx  # noqa: E402

SENTINEL = np.float32(np.nan).view(np.uint32)  # torch.full's NaN
WHERE = "pp > 0.5"
# one fixed expression text per family: each (family, tile size) is one module
PLAIN = {"single": ["va * 2"], "select2": ["va", "va * 0.5 + 1"], "select4": ["va", "va * 2", "va + pp", "va * 0.5 - 3"]}
FAMILIES = ["single", "select2", "select4", "window", "join_direct", "join_hash", "join_left"]
NOUT = {"single": 1, "select2": 2, "select4": 4, "window": 2, "join_direct": 2, "join_hash": 2, "join_left": 2}


@functools.lru_cache(maxsize=None)
def layouts():
    return cl.all_layouts()


def host_cols(name, family):
    lay = layouts()[name]
    return lay.left_cols() if family == "join_left" else lay.inner_cols() if family.startswith("join") else lay.cols()


@functools.lru_cache(maxsize=None)
def device_table(name, kind):
    lay = layouts()[name]
    return dev_table({"base": lay.cols, "inner": lay.inner_cols, "left": lay.left_cols}[kind]())


@functools.lru_cache(maxsize=None)
def right_table():
    return dev_table(cl.right_columns())


@functools.lru_cache(maxsize=None)
def reference(name, family):
    """(values per output, row ids, matched right rows or None), computed once and left unchanged."""
    lay = layouts()[name]
    cols = host_cols(name, family)
    rrow = None
    if family in PLAIN:
        ht = ora.HostTable(cols)
        vals = []
        for e in PLAIN[family]:
            v, rows = ora.project_filter(ht, e, WHERE)
            assert np.array_equal(rows, lay.rows)
            vals.append(v)
    elif family == "window":
        vals, rows = window_expected(cols, PLAIN1, ITEM1)
    else:
        vals, rows, rrow = join_expected(cols, cl.right_columns(), JOIN_EXPRS,
                                         wx.JOIN_LEFT if family == "join_left" else wx.JOIN_INNER)
        if family != "join_left":
            rrow = None
        else:
            assert (rrow == -1).sum() == lay.left_miss.sum()
    assert np.array_equal(rows, lay.rows) and len(vals) == NOUT[family]   # the numpy restatement: np.nonzero(keep)
    for a in vals:
        a.setflags(write=False)
    return vals, lay.rows, rrow


def setup(monkeypatch, tile_rows, mode, family):
    """mode: "deep" (uncapped), "cap<n>" (WARPDB_COMPACT_GRID=n) or "ticket"."""
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", cl.DEFINES[tile_rows])
    monkeypatch.delenv("WARPDB_WINDOW_FORM", raising=False)
    for var, val in (("WARPDB_JOIN_FORM", "hash" if family in ("join_hash", "join_left") else None),
                     ("WARPDB_COMPACT_SCHED", "ticket" if mode == "ticket" else None),
                     ("WARPDB_COMPACT_GRID", mode[3:] if mode.startswith("cap") else None)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, val)


def run(family, name, offset=0, ids=8, null=False):
    """One call.  Value, id and right-row buffers come back whole, the offset slack included."""
    lay = layouts()[name]
    n, m = lay.n, NOUT[family]
    bufs = [torch.full((n + offset + 1,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(m)]
    idx = torch.full((n + offset + 1,), -1, dtype=torch.int64 if ids == 8 else torch.int32, device="cuda") if ids else None
    rr = torch.full((n + offset + 1,), -7, dtype=torch.int32, device="cuda") if family == "join_left" else None
    dc = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    ptrs = [0 if null else b[offset:].data_ptr() for b in bufs]
    d_idx = idx[offset:].data_ptr() if ids else 0
    L = launch()
    cond = ora.lower(WHERE)
    if family == "single":
        table, _ = device_table(name, "base")
        cnt = wx.project_filter(table, ora.lower(PLAIN[family][0]), cond, L, wx.MODE_COMPACT, ptrs[0], d_idx, ids or 8, 0,
                                dc.data_ptr(), want_count=True)
    elif family in PLAIN:
        table, _ = device_table(name, "base")
        cnt = wx.project_filter_multi(table, [ora.lower(e) for e in PLAIN[family]], cond, L, ptrs, d_idx, ids or 8, 0,
                                      dc.data_ptr(), want_count=True)
    elif family == "window":
        table, _ = device_table(name, "base")
        cnt = wx.window_select(table, PLAIN1, ITEM1, "kk[idx]", cond, L, ptrs, d_out_idx=d_idx, idx_bytes=ids or 8,
                               d_count=dc.data_ptr(), want_count=True)
    else:
        table, _ = device_table(name, "left" if family == "join_left" else "inner")
        cnt = wx.join_select(table, right_table()[0], "kk[idx]", "rk", JOIN_EXPRS, cond, L, ptrs,
                             join_type=wx.JOIN_LEFT if family == "join_left" else wx.JOIN_INNER, d_out_idx=d_idx,
                             idx_bytes=ids or 8, d_out_right_row=rr[offset:].data_ptr() if rr is not None else 0,
                             d_count=dc.data_ptr(), want_count=True)
    return SimpleNamespace(count=cnt, d_count=int(dc.item()), vals=[b.cpu().numpy() for b in bufs],
                           idx=None if idx is None else idx.cpu().numpy(), rr=None if rr is None else rr.cpu().numpy(),
                           geom=wx.compact_last_launch(L), offset=offset, null=null)


def check(r, family, name):
    ref_vals, ref_rows, ref_rr = reference(name, family)
    cnt, offset = len(ref_rows), r.offset
    assert r.count == cnt, "host count"
    assert r.d_count == cnt, "device count"
    for j, v in enumerate(r.vals):
        u = bits(v)
        if r.null:
            assert (u == SENTINEL).all(), f"output {j}: written through a null pointer's neighbour"
            continue
        assert np.array_equal(u[offset:offset + cnt], bits(ref_vals[j])), f"output {j}"
        assert (u[offset + cnt:] == SENTINEL).all(), f"output {j}: written at positions >= count"
        assert (u[:offset] == SENTINEL).all(), f"output {j}: written in front of the pointer"
    if r.idx is not None:
        assert np.array_equal(r.idx[offset:offset + cnt], ref_rows)
        assert (r.idx[offset + cnt:] == -1).all() and (r.idx[:offset] == -1).all()
    if r.rr is not None:
        assert np.array_equal(r.rr[offset:offset + cnt], ref_rr)
        assert (r.rr[offset + cnt:] == -7).all() and (r.rr[:offset] == -7).all()


def check_geom(g, name, mode):
    lay = layouts()[name]
    assert (g.tile_rows, g.n_tiles) == (lay.tile_rows, lay.n_tiles)
    if mode == "ticket":
        assert (g.grid, g.deep) == (lay.n_tiles, 0)
    else:
        assert g.deep == 1 and 1 <= g.grid <= lay.n_tiles
        if mode.startswith("cap"):
            assert g.grid == min(int(mode[3:]), lay.n_tiles)


# ------------------------------------------------------------- steady state
@pytest.mark.parametrize("tile_rows", [512, 1024])
@pytest.mark.parametrize("family", FAMILIES)
def test_steady_state(family, tile_rows, monkeypatch):
    """48 tiles through one, two and three workgroups: iteration k >= 2 with three tiles in flight, the stage
    buffer written out and overwritten, the s_tiles ring reused; with one workgroup in ticket order."""
    name = f"steady_{tile_rows}"
    for cap in (1, 2, 3):
        setup(monkeypatch, tile_rows, f"cap{cap}", family)
        r = run(family, name)
        check(r, family, name)
        g = r.geom
        assert (g.deep, g.n_tiles, g.tile_rows) == (1, 48, tile_rows)
        assert g.grid <= cap and g.n_tiles >= 16 * g.grid
        if cap == 1:
            assert g.grid == 1


# -------------------------------------------------------------- store shapes
@pytest.mark.parametrize("mode", ["cap1", "deep"])
@pytest.mark.parametrize("family", FAMILIES)
def test_store_shapes(family, mode, monkeypatch):
    """Every class of (excl % 32, head, body, tail), for ids of 4 and 8 bytes and output pointers at element
    offsets 0 and 1 (offset 1: 16-byte body stores to a pointer that is only 4-byte aligned)."""
    name = "store_shapes_512"
    setup(monkeypatch, 512, mode, family)
    for ids in (4, 8):
        for offset in (0, 1):
            r = run(family, name, offset=offset, ids=ids)
            check(r, family, name)
            check_geom(r.geom, name, mode)
    check(run(family, name, offset=1, ids=4, null=True), family, name)   # ids only
    check(run(family, name, ids=0), family, name)                        # no ids


# ------------------------------------------- empty runs, full tiles, last tile, positions
EDGE_LAYOUTS = ["empty_run_512", "full_tiles_512", "full_tiles_1024", "positions_1024"] + \
               [f"last_{v}_512" for v in cl.LAST_VARIANTS]


@pytest.mark.parametrize("name", EDGE_LAYOUTS)
@pytest.mark.parametrize("family", FAMILIES)
def test_edge_layouts(family, name, monkeypatch):
    lay = layouts()[name]
    for mode in ("deep", "cap2", "ticket"):
        setup(monkeypatch, lay.tile_rows, mode, family)
        r = run(family, name, ids=4 if mode == "cap2" else 8)
        check(r, family, name)            # the host count and the device count, each on its own
        check_geom(r.geom, name, mode)
    if name == "last_one_drop_512":
        assert r.count > 0 and lay.shapes[-1][1] == 0   # the tile that wrote the count had no row


# ------------------------------------------------------- the grid cap itself
def test_bad_grid_cap_is_refused_before_anything_is_enqueued(monkeypatch):
    name = "last_exact_512"
    setup(monkeypatch, 512, "deep", "single")
    check(run("single", name), "single", name)
    before = wx.compact_last_launch(launch())
    for bad in ("0", "-1", "x", "2x", "1.5"):
        monkeypatch.setenv("WARPDB_COMPACT_GRID", bad)
        for family in ("single", "select2"):
            with pytest.raises(wx.WarpExecError, match="WARPDB_COMPACT_GRID") as ei:
                run(family, name)
            assert ei.value.status == wx.WX_ERR_INVALID
        g = wx.compact_last_launch(launch())   # the failed calls launched nothing
        assert (g.tile_rows, g.n_tiles, g.grid, g.deep) == (before.tile_rows, before.n_tiles, before.grid, before.deep)
    wx.check(launch())
    # the ticket schedule ignores the variable
    monkeypatch.setenv("WARPDB_COMPACT_SCHED", "ticket")
    r = run("single", name)
    check(r, "single", name)
    check_geom(r.geom, name, "ticket")
    # a cap above the grid changes nothing; an empty table reports zeros
    setup(monkeypatch, 512, "cap100000", "single")
    r = run("single", name)
    check(r, "single", name)
    assert r.geom.grid == r.geom.n_tiles == 5
    table, _ = dev_table({k: v[:0] for k, v in layouts()[name].cols().items()})
    assert wx.project_filter(table, ora.lower("va * 2"), ora.lower(WHERE), launch(), wx.MODE_COMPACT, 0, 0, 8, 0,
                             want_count=True) == 0
    g = wx.compact_last_launch(launch())
    assert (g.tile_rows, g.n_tiles, g.grid, g.deep) == (0, 0, 0, 0)


# ------------------------------------------ one status array for every family
def test_families_share_status_words_epochs_and_ticket(monkeypatch):
    """70 calls in a row on one stream -- single-output, SELECT and join probe in turn, over tables of 1 to 149
    tiles, capped and not: the status array grows and is reused shorter, the epoch wraps (63 launches), and each
    launch finds the ticket its predecessor returned."""
    fams = ["single", "select2", "join_direct"]
    names = ["steady_512", "empty_run_512", "last_single_512", "full_tiles_512", "store_shapes_512"]
    modes = ["deep", "cap1", "deep", "cap2", "ticket", "cap3", "deep"]
    tiles = set()
    for i in range(70):
        family, name, mode = fams[i % 3], names[i % 5], modes[i % 7]
        setup(monkeypatch, 512, mode, family)
        r = run(family, name, offset=i % 2, ids=(4, 8)[i % 2])
        check(r, family, name)
        check_geom(r.geom, name, mode)
        tiles.add(r.geom.n_tiles)
    assert min(tiles) == 1 and max(tiles) == 149 and len(tiles) == 5
