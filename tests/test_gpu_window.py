"""GPU tests of the window aggregates (wx_window.hip) through wx_window_select,
WarpDB::query_sql_windowed and its Arrow export.

Expectations are computed here with numpy.  They are bit-exact: every value
of the columns lies on a 1/8 grid with |v| <= 1024 (the value expressions
built from them stay on it with |v| <= 2048) and a table has at most 2^20
rows, so a partition's double sum is exact whatever the order of the atomic
adds (2^20 * 2048 * 8 = 2^34 grid units, far below 2^53), and SUM / AVG / COUNT /
MIN / MAX columns, plain columns, row ids and counts are compared bit for
bit.  `check_bounds` asserts that on the inputs.  Outputs are prefilled with
a NaN / -1 sentinel and must be untouched at positions >= count and in front
of an offset pointer.

The clamp: the broadcast kernels look the partition of EVERY row of a tile
up, rows the WHERE drops and the zero-filled rows past n_rows included.  The
tables here give the dropped rows keys that belong to no partition --
INT32_MIN, INT32_MAX and the values just outside the key span on both sides
-- in valid queries whose answer is known; the results must not change.
"""
from __future__ import annotations

import ctypes
import functools
import os

import numpy as np
import pytest

from test_gpu_arrow import ArrowArray, ArrowSchema, _ptr
from test_gpu_parity import DISCOUNT_SRC, bits, dev_table, launch

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from warpdb_amd import _warpexec as wx  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEST_CSV = os.path.join(ROOT, "tests", "golden", "test.csv")
SENTINEL = np.float32(np.nan).view(np.uint32)  # torch.full's NaN
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
COND = "(pp[idx] > 0.5f)"
SUM, AVG, COUNT, MIN, MAX = wx.WIN_SUM, wx.WIN_AVG, wx.WIN_COUNT, wx.WIN_MIN, wx.WIN_MAX

# key sets: name -> (keys of the partitions, dense form expected)
KEYSETS = {
    "one": (np.array([7], np.int64), True),
    "dense2048": (np.arange(-1000, -1000 + 2048, dtype=np.int64), True),   # span exactly 2048, negative, not at 0
    "span2049": (np.concatenate([np.arange(5, 900), [5 + 2048]]).astype(np.int64), False),
    "wide5000": (np.unique(np.random.default_rng(11).integers(-(10 ** 9), 10 ** 9, 5000)).astype(np.int64), False),
}


def check_bounds(cols, n):
    assert n <= 1 << 20
    for name in ("va", "vb"):
        x = cols[name].astype(np.float64)
        assert np.all(np.abs(x) <= 1024) and np.all(x * 8 == np.round(x * 8))


@functools.lru_cache(maxsize=None)
def columns(n, keyset, pass_mode):
    """kk: the partition key, va / vb: values on the 1/8 grid, pp: 1 where the WHERE keeps the row.
    Dropped rows carry keys outside every partition (the clamp cases)."""
    rng = np.random.default_rng(1000 + n % 9973)
    keys, _ = KEYSETS[keyset]
    p = {"none": np.zeros(n), "all": np.ones(n), "most": (rng.random(n) < 0.6)}[pass_mode].astype(np.float32)
    k = keys[rng.integers(0, len(keys), n)]
    if n >= 2:  # both ends of the span are present whenever rows pass
        k[0], k[-1] = keys[0], keys[-1]
    lo, hi = int(keys[0]), int(keys[-1])
    poison = np.array([I32_MIN, I32_MAX, max(lo - 1, I32_MIN), min(hi + 1, I32_MAX), lo - 2048 if lo - 2048 > I32_MIN
                       else I32_MIN, hi + 2048], np.int64)
    if len(keys) > 1 and keyset != "dense2048":  # between two keys of a search table
        gaps = np.setdiff1d(np.arange(lo, min(hi, lo + 4096)), keys)
        if len(gaps):
            poison = np.concatenate([poison, gaps[:2]])
    drop = p < 0.5
    k = np.where(drop, poison[np.arange(n) % len(poison)], k)
    if pass_mode == "most" and n >= 2:
        p[0] = p[-1] = 1.0
        k[0], k[-1] = keys[0], keys[-1]
    cols = {
        "kk": k.astype(np.int32),
        "va": (rng.integers(-8192, 8193, n) / 8.0).astype(np.float32),
        "vb": (rng.integers(0, 8193, n) / 8.0).astype(np.float32),
        "pp": p,
    }
    check_bounds(cols, n)
    for c in cols.values():
        c.setflags(write=False)
    return cols


@functools.lru_cache(maxsize=None)
def device_table(n, keyset, pass_mode, offset=0):
    return dev_table(columns(n, keyset, pass_mode), offset)


# value expressions: lowered text -> numpy (float32 arithmetic as the kernel's)
VALUES = {
    "va[idx]": lambda c: c["va"],
    "vb[idx]": lambda c: c["vb"],
    "(va[idx] * 2.0f)": lambda c: c["va"] * np.float32(2),
    "(vb[idx] - va[idx])": lambda c: c["vb"] - c["va"],
    "(va[idx] + 1.0f)": lambda c: c["va"] + np.float32(1),
    "(vb[idx] * 0.5f)": lambda c: c["vb"] * np.float32(0.5),
    "kk[idx]": lambda c: c["kk"].astype(np.float32),
    "(va[idx] + vb[idx])": lambda c: c["va"] + c["vb"],
    "1.0f": lambda c: np.ones(len(c["va"]), np.float32),
}


def expected(cols, plain, items, one_partition=False):
    """(values per output, row ids): plain expressions first, then the window items."""
    keep = cols["pp"] > 0.5
    rows = np.nonzero(keep)[0].astype(np.int64)
    out = [np.asarray(VALUES[e](cols), np.float32)[keep] for e in plain]
    k = np.zeros(len(rows), np.int64) if one_partition else cols["kk"][keep].astype(np.int64)
    uniq, inv = np.unique(k, return_inverse=True)
    cnt = np.bincount(inv, minlength=len(uniq)).astype(np.int64)
    for e, agg in items:
        val = np.asarray(VALUES[e](cols), np.float32)[keep]
        if agg in (SUM, AVG):
            s = np.bincount(inv, weights=val.astype(np.float64), minlength=len(uniq))
            g = s.astype(np.float32) if agg == SUM else (s / cnt.astype(np.float64)).astype(np.float32)
        elif agg == COUNT:
            g = cnt.astype(np.float32)
        else:
            g = np.full(len(uniq), np.inf if agg == MIN else -np.inf, np.float32)
            (np.minimum if agg == MIN else np.maximum).at(g, inv, val)
        out.append(g[inv] if len(rows) else np.zeros(0, np.float32))
    return out, rows


def run(table, plain, items, part="kk[idx]", cond=COND, cap=8192, key_lo=0, offset=0, ids=8, row_base=0, null=(),
        d_count=False, L=None):
    """One call.  Returns (count, [full value buffers incl. the offset slack], full id buffer)."""
    n, m = table.n_rows, len(plain) + len(items)
    bufs = [torch.full((n + offset + 1,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(m)]
    idx = None
    if ids:
        idx = torch.full((n + offset + 1,), -1, dtype=torch.int64 if ids == 8 else torch.int32, device="cuda")
    dc = torch.full((1,), -5, dtype=torch.int64, device="cuda") if d_count else None
    ptrs = [0 if j in null else b[offset:].data_ptr() for j, b in enumerate(bufs)]
    cnt = wx.window_select(table, plain, items, part, cond, L or launch(), ptrs, key_window_lo=key_lo,
                           group_capacity=cap, d_out_idx=idx[offset:].data_ptr() if ids else 0, idx_bytes=ids or 8,
                           row_base=row_base, d_count=dc.data_ptr() if d_count else 0, want_count=True)
    if d_count:
        assert int(dc.item()) == cnt
    return cnt, [b.cpu().numpy() for b in bufs], None if idx is None else idx.cpu().numpy()


def check(got, want, offset=0, row_base=0, null=()):
    cnt, vals, idx = got
    ref_vals, ref_idx = want
    assert cnt == len(ref_idx)
    for j, v in enumerate(vals):
        if j in null:
            assert (bits(v) == SENTINEL).all(), f"output {j}: written through a null pointer's neighbour"
            continue
        assert np.array_equal(bits(v[offset:offset + cnt]), bits(ref_vals[j])), f"output {j}"
        assert (bits(v[offset + cnt:]) == SENTINEL).all(), f"output {j}: written at positions >= count"
        assert (bits(v[:offset]) == SENTINEL).all(), f"output {j}: written in front of the pointer"
    if idx is not None:
        assert np.array_equal(idx[offset:offset + cnt], ref_idx + row_base)
        assert (idx[offset + cnt:] == -1).all() and (idx[:offset] == -1).all()


PLAIN1, ITEM1 = ["va[idx]"], [("va[idx]", SUM)]  # the issue's query: SELECT va, SUM(va) OVER (PARTITION BY kk) WHERE ..


def sizes(search):
    t = wx.window_tile_rows(2, 1, search)
    assert t > 0
    return [0, 1, t - 1, t, t + 1, 3 * t + 5, 40 * t + 3]


@pytest.mark.parametrize("sched", ["deep", "ticket"])
@pytest.mark.parametrize("keyset", ["dense2048", "span2049"])
def test_sizes(keyset, sched, monkeypatch):
    monkeypatch.delenv("WARPDB_EXTRA_DEFINES", raising=False)
    if sched == "ticket":
        monkeypatch.setenv("WARPDB_COMPACT_SCHED", "ticket")
    else:
        monkeypatch.delenv("WARPDB_COMPACT_SCHED", raising=False)
    for n in sizes(not KEYSETS[keyset][1]):
        table, _ = device_table(n, keyset, "most")
        check(run(table, PLAIN1, ITEM1, d_count=True), expected(columns(n, keyset, "most"), PLAIN1, ITEM1))


@pytest.mark.parametrize("pass_mode", ["none", "all", "most"])
@pytest.mark.parametrize("keyset", list(KEYSETS))
def test_keysets_and_selectivity(keyset, pass_mode):
    n = sizes(not KEYSETS[keyset][1])[5] if keyset != "wide5000" else 60_001
    table, _ = device_table(n, keyset, pass_mode)
    cols = columns(n, keyset, pass_mode)
    got = run(table, PLAIN1, ITEM1)
    check(got, expected(cols, PLAIN1, ITEM1))
    if pass_mode == "none":
        assert got[0] == 0
    if pass_mode == "all":
        assert got[0] == n
    if keyset == "wide5000" and pass_mode != "none":
        assert len(np.unique(cols["kk"][cols["pp"] > 0.5])) > 4096  # the general-key table, sorted on the device


@pytest.mark.parametrize("keyset", ["dense2048", "span2049"])
def test_clamp_keys_are_present_and_harmless(keyset):
    """Dropped rows carry INT32_MIN, INT32_MAX and the keys next to the span; the last tile is partial."""
    search = not KEYSETS[keyset][1]
    n = sizes(search)[5]
    cols = columns(n, keyset, "most")
    keys = KEYSETS[keyset][0]
    dropped = cols["kk"][cols["pp"] < 0.5].astype(np.int64)
    for bad in (I32_MIN, I32_MAX, int(keys[0]) - 1, int(keys[-1]) + 1):
        assert bad in dropped
    assert not np.isin(dropped, keys).any()
    assert n % wx.window_tile_rows(2, 1, search) != 0  # the zero-filled rows past n_rows look key 0 up too
    table, _ = device_table(n, keyset, "most")
    want = expected(cols, PLAIN1, ITEM1)
    check(run(table, PLAIN1, ITEM1), want)
    # the group pass's own window placed on the keys gives the same answer
    check(run(table, PLAIN1, ITEM1, key_lo=int(keys[0])), want)


def test_forced_search_form_matches_dense(monkeypatch):
    n = sizes(False)[5]
    table, _ = device_table(n, "dense2048", "most")
    want = expected(columns(n, "dense2048", "most"), PLAIN1, ITEM1)
    dense = run(table, PLAIN1, ITEM1)
    monkeypatch.setenv("WARPDB_WINDOW_FORM", "search")
    search = run(table, PLAIN1, ITEM1)
    check(dense, want)
    check(search, want)


def test_over_empty_is_one_partition():
    n = sizes(False)[5]
    table, _ = device_table(n, "dense2048", "most")
    items = [("va[idx]", SUM), ("1.0f", COUNT)]
    check(run(table, ["vb[idx]"], items, part="0"), expected(columns(n, "dense2048", "most"), ["vb[idx]"], items, True))


ALL5 = [("va[idx]", a) for a in (SUM, AVG, COUNT, MIN, MAX)]
SHAPES = {
    "0+1": ([], [("vb[idx]", MAX)]),
    "1+3": (["va[idx]"], [("va[idx]", SUM), ("vb[idx]", AVG), ("(vb[idx] - va[idx])", MIN)]),
    "0+4": ([], [("va[idx]", SUM), ("(va[idx] * 2.0f)", SUM), ("vb[idx]", MAX), ("(vb[idx] - va[idx])", AVG)]),
    "5+4": (["va[idx]", "vb[idx]", "(va[idx] + vb[idx])", "kk[idx]", "(va[idx] + 1.0f)"],   # three launches, the first all plain
            [("va[idx]", SUM), ("va[idx]", MAX), ("vb[idx]", AVG), ("kk[idx]", COUNT)]),
    "0+5": ([], ALL5),                                                               # five aggregates of one value
    "2 values": (["vb[idx]"], [("va[idx]", MIN), ("(vb[idx] * 0.5f)", SUM)]),
}


# every shape in the dense form; the chunked and the widest ones in the search form too
@pytest.mark.parametrize("shape,keyset", [(s, "dense2048") for s in SHAPES] +
                         [(s, "span2049") for s in ("1+3", "5+4", "0+5")])
def test_shapes(shape, keyset):
    plain, items = SHAPES[shape]
    n = 3 * wx.window_tile_rows(min(4, len(plain) + len(items)), min(4, len(items)), False) + 5
    table, _ = device_table(n, keyset, "most")
    check(run(table, plain, items, d_count=True), expected(columns(n, keyset, "most"), plain, items))


def test_ticket_schedule_matches_default_over_chunks(monkeypatch):
    plain, items = SHAPES["5+4"]
    n = sizes(False)[5]
    table, _ = device_table(n, "dense2048", "most")
    want = expected(columns(n, "dense2048", "most"), plain, items)
    monkeypatch.delenv("WARPDB_COMPACT_SCHED", raising=False)
    deep = run(table, plain, items)
    monkeypatch.setenv("WARPDB_COMPACT_SCHED", "ticket")
    ticket = run(table, plain, items)
    check(deep, want)
    check(ticket, want)


@pytest.mark.parametrize("keyset", ["dense2048", "span2049"])
def test_tiny_tiles_pipeline_and_lookback_window(keyset, monkeypatch):
    # 512-row tiles: 541 (dense form) / 601 (search form) tiles, and the
    # look-back window moves past 64 predecessors.  That is fewer tiles than
    # an MI355X keeps workgroups resident, so the grid is n_tiles (measured:
    # 541 / 601): the workgroups that start first take two tiles at entry (a
    # further one only while later workgroups have not started), so about
    # ceil(n_tiles / grid) + 1 = 2 tiles at the most, and the rest find the
    # tickets gone.  The pipeline's steady state (three tiles in flight in one
    # workgroup, iteration after iteration) is not what this test reaches;
    # tests/test_gpu_compact_edges.py runs it.
    search = not KEYSETS[keyset][1]
    n = sizes(search)[6]
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_COMPACT_GROUPS=1,WX_COMPACT_DWAVES=2")
    assert wx.window_tile_rows(2, 1, search) == 512
    table, _ = device_table(n, keyset, "most")
    check(run(table, PLAIN1, ITEM1, ids=4), expected(columns(n, keyset, "most"), PLAIN1, ITEM1))
    g = wx.compact_last_launch(launch())
    assert (g.deep, g.tile_rows, g.n_tiles) == (1, 512, -(-n // 512)) and 64 < g.grid <= g.n_tiles


@pytest.mark.parametrize("ids,row_base", [(0, 0), (4, 1000), (8, 1 << 33)])
def test_row_ids_and_unaligned_columns(ids, row_base):
    plain, items = SHAPES["1+3"]
    n = 3 * wx.window_tile_rows(4, 3, False) + 5
    table, _ = device_table(n, "dense2048", "most", 1)  # every column pointer 4 bytes off a 16-byte boundary
    want = expected(columns(n, "dense2048", "most"), plain, items)
    check(run(table, plain, items, offset=1, ids=ids, row_base=row_base), want, offset=1, row_base=row_base)


def test_null_outputs_and_custom_function():
    n = sizes(False)[5]
    table, _ = device_table(n, "dense2048", "most")
    cols = columns(n, "dense2048", "most")
    plain, items = SHAPES["1+3"]
    check(run(table, plain, items, null=(0, 2)), expected(cols, plain, items), null=(0, 2))
    got = run(table, ["discount(va[idx], 0.5f)"], [("discount(vb[idx], 0.5f)", SUM)], L=launch(custom=DISCOUNT_SRC))
    want_vals, want_idx = expected(cols, ["va[idx]"], [("(vb[idx] * 0.5f)", SUM)])
    check(got, ([want_vals[0] * np.float32(0.5), want_vals[1]], want_idx))


def test_capacity_error_reports_the_found_count():
    n = sizes(False)[5]
    table, _ = device_table(n, "dense2048", "most")
    cols = columns(n, "dense2048", "most")
    found = len(np.unique(cols["kk"][cols["pp"] > 0.5]))
    assert found > 100
    with pytest.raises(wx.WarpExecError, match=f"{found} found, group_capacity is 100") as ei:
        run(table, PLAIN1, ITEM1, cap=100)
    assert ei.value.status == wx.WX_ERR_CAPACITY
    wx.check(launch())  # the error bit is cleared: the workspace is usable
    check(run(table, PLAIN1, ITEM1), expected(cols, PLAIN1, ITEM1))


# ------------------------------------------------------------------ facade
def write_csv(path, cols):
    with open(path, "w") as f:
        f.write(",".join(cols) + "\n")
        for row in zip(*cols.values()):
            f.write(",".join(repr(x.item()) for x in row) + "\n")


@pytest.fixture(scope="module")
def window_db(tmp_path_factory):
    from warpdb_amd import pywarpdb as pw

    n = 20_011
    cols = dict(columns(n, "dense2048", "most"))
    cols["kk"] = (cols["kk"].astype(np.int64) % 37).astype(np.int32)  # every row a real key: 37 partitions
    path = str(tmp_path_factory.mktemp("window") / "window.csv")
    write_csv(path, cols)
    D = pw.DataType
    return pw.WarpDB(path, [D.Int32, D.Float32, D.Float32, D.Float32], 0), cols


def test_query_sql_windowed_on_test_csv():
    from warpdb_amd import pywarpdb as pw

    db = pw.WarpDB(TEST_CSV)
    names, cols, rows = db.query_sql_windowed("SELECT price, SUM(price) OVER (PARTITION BY quantity) FROM t "
                                              "WHERE price > 15")
    assert names == ["price", "expr1"] and rows.tolist() == [1, 2, 3]
    assert cols[0].tolist() == [20.0, 15.25, 30.0] and cols[1].tolist() == [20.0, 15.25, 30.0]
    names, cols, rows = db.query_sql_windowed("SELECT COUNT(*) OVER (), price, MAX(price * quantity) OVER (), "
                                              "AVG(price) OVER () FROM t WHERE price > 15")
    assert names == ["expr0", "price", "expr2", "expr3"] and rows.tolist() == [1, 2, 3]
    assert cols[0].tolist() == [3.0] * 3 and cols[1].tolist() == [20.0, 15.25, 30.0]
    assert cols[2].tolist() == [150.0] * 3 and cols[3].tolist() == [21.75] * 3
    with pytest.raises(RuntimeError, match="two different expressions"):
        db.query_sql_windowed("SELECT SUM(price) OVER (PARTITION BY quantity), COUNT(*) OVER () FROM t")
    # the other entry points keep refusing window items, and this one what it cannot run
    with pytest.raises(RuntimeError, match="window functions are not supported by the execution engine"):
        db.query_sql_table("SELECT price, SUM(price) OVER (PARTITION BY quantity) FROM t")
    with pytest.raises(RuntimeError, match="window functions are not supported by query_sql_ordered"):
        db.query_sql_ordered("SELECT price, SUM(price) OVER (PARTITION BY quantity) FROM t ORDER BY price")
    with pytest.raises(RuntimeError, match="ORDER BY inside OVER"):
        db.query_sql_windowed("SELECT price, SUM(price) OVER (PARTITION BY quantity ORDER BY price) FROM t")
    with pytest.raises(RuntimeError, match="needs a window item"):
        db.query_sql_windowed("SELECT price, quantity FROM t")
    with pytest.raises(RuntimeError, match="SELECT clause: Unknown column: nope"):
        db.query_sql_windowed("SELECT price, SUM(price) OVER (PARTITION BY nope) FROM t")


def test_query_sql_windowed_vs_numpy_and_grouped(window_db):
    db, cols = window_db
    sql = ("SELECT va, SUM(va) OVER (PARTITION BY kk), vb, AVG(vb) OVER (PARTITION BY kk), "
           "COUNT(*) OVER (PARTITION BY kk), MIN(va + vb) OVER (PARTITION BY kk), kk FROM t WHERE pp > 0.5")
    names, out, rows = db.query_sql_windowed(sql)
    assert names == ["va", "expr1", "vb", "expr3", "expr4", "expr5", "kk"]
    want_vals, want_rows = expected(cols, ["va[idx]", "vb[idx]", "kk[idx]"],
                                    [("va[idx]", SUM), ("vb[idx]", AVG), ("1.0f", COUNT), ("(va[idx] + vb[idx])", MIN)])
    order = [0, 3, 1, 4, 5, 6, 2]  # select item -> (plain first, then items)
    assert np.array_equal(rows, want_rows)
    for j, o in enumerate(order):
        assert np.array_equal(bits(out[j]), bits(want_vals[o])), names[j]
    # every row's aggregates are what query_sql_grouped returns for the row's key
    gnames, g = db.query_sql_grouped("SELECT kk, SUM(va), AVG(vb), COUNT(va), MIN(va + vb) FROM t WHERE pp > 0.5 GROUP BY kk")
    by_key = {int(k): i for i, k in enumerate(g[0])}
    at = np.array([by_key[int(k)] for k in out[6]])
    for j, gj in ((1, 1), (3, 2), (4, 3), (5, 4)):
        assert np.array_equal(bits(out[j]), bits(g[gj][at])), names[j]
    # LIMIT / OFFSET cut the same result
    for tail, lo, hi in ((" LIMIT 100 OFFSET 7", 7, 107), (" LIMIT 5", 0, 5), (" OFFSET 12000", 12000, None),
                         (" LIMIT 0", 0, 0), (" OFFSET 999999", len(rows), None)):
        n2, o2, r2 = db.query_sql_windowed(sql + tail)
        assert n2 == names and np.array_equal(r2, rows[lo:hi])
        for a, b in zip(o2, out):
            assert np.array_equal(bits(a), bits(b[lo:hi]))


def test_alternating_calls_share_one_workspace(window_db):
    """Windowed, grouped and plain calls in turn: the shared accumulators return to idle after each."""
    db, _ = window_db
    w_sql = "SELECT va, SUM(va) OVER (PARTITION BY kk), MAX(vb) OVER (PARTITION BY kk) FROM t WHERE pp > 0.5"
    g_sql = "SELECT kk, SUM(va), MAX(vb), MIN(va) FROM t WHERE pp > 0.5 GROUP BY kk"
    first = None
    for _ in range(3):
        w = db.query_sql_windowed(w_sql)
        g = db.query_sql_grouped(g_sql)
        s = db.query_select(["va", "vb * 2"], "pp > 0.5")
        now = [bits(c).tobytes() for c in w[1]] + [bits(c).tobytes() for c in g[1]] + [bits(c).tobytes() for c in s[1]]
        now += [w[2].tobytes(), s[2].tobytes()]
        assert first is None or now == first
        first = now


def test_arrow_struct_export():
    from warpdb_amd import pywarpdb as pw

    db = pw.WarpDB(TEST_CSV)
    arr_cap, sch_cap = db.query_arrow_sql_windowed("SELECT price, SUM(price) OVER () FROM t WHERE price > 15")
    a = ArrowArray.from_address(_ptr(arr_cap, None))
    s = ArrowSchema.from_address(_ptr(sch_cap, None))
    assert s.format == b"+s" and s.n_children == 3 and a.n_children == 3 and a.length == 3
    want = [(b"price", np.float32, [20.0, 15.25, 30.0]), (b"expr1", np.float32, [65.25] * 3), (b"row", np.int64, [1, 2, 3])]
    for j, (name, dt, values) in enumerate(want):
        cs, ca = s.children[j].contents, a.children[j].contents
        assert cs.name == name and ca.length == 3
        got = np.ctypeslib.as_array(ctypes.cast(ca.buffers[1], ctypes.POINTER(np.ctypeslib.as_ctypes_type(dt))),
                                    shape=(3,))
        assert got.tolist() == values
    release_a = ctypes.CFUNCTYPE(None, ctypes.POINTER(ArrowArray))(a.release)
    release_s = ctypes.CFUNCTYPE(None, ctypes.POINTER(ArrowSchema))(s.release)
    release_a(ctypes.byref(a))
    release_s(ctypes.byref(s))
    assert not a.release and not s.release
    del arr_cap, sch_cap
