"""GPU tests of the fused multi-output ordered compaction (wx_select.hip)
through wx_project_filter_multi, WarpDB::query_select / query_sql_table and
the Arrow struct export.

The oracle for M outputs is oracle_lib.project_filter called once per
expression with the same condition.  Every comparison is bit-exact (values,
row ids, counts); outputs are prefilled with a NaN / -1 sentinel and must be
untouched at positions >= count and in front of an offset pointer.
"""
from __future__ import annotations

import ctypes
import functools
import os

import numpy as np
import pytest

import oracle_lib as ora
import synth
from test_gpu_arrow import ArrowArray, ArrowSchema, _ptr
from test_gpu_fuzz import gen_cond, gen_expr
from test_gpu_parity import DISCOUNT_SRC, bits, dev_table, launch

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from warpdb_amd import _warpexec as wx  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEST_CSV = os.path.join(ROOT, "tests", "golden", "test.csv")
SENTINEL = np.float32(np.nan).view(np.uint32)  # torch.full's NaN

EXPRS = ["price * quantity", "price", "quantity + 1", "price * 0.5 - quantity"]
CONDS = {"none": None, "never": "price < 0", "always": "price >= 0", "gt15": "price > 15"}
BIG = 1_000_003


def shapes(m):
    t = wx.select_tile_rows(m)
    assert t > 0
    return [0, 1, t - 1, t, t + 1, 3 * t + 5, BIG]


@functools.lru_cache(maxsize=None)
def columns(n):
    return synth.c2_table(n)  # shared by every test of this size: read, never written


@functools.lru_cache(maxsize=None)
def reference(n, cond_key):
    """(values per EXPRS entry, row ids) of the oracle, computed once per (n, condition)."""
    ht = ora.HostTable(columns(n))
    out, idx = [], None
    for e in EXPRS:
        v, i = ora.project_filter(ht, e, CONDS[cond_key])
        assert idx is None or np.array_equal(idx, i)
        idx = i
        v.setflags(write=False)
        out.append(v)
    idx.setflags(write=False)
    return out, idx


@functools.lru_cache(maxsize=None)
def device_table(n, offset):
    return dev_table(columns(n), offset)


def run(table, exprs_c, cond_c, offset=0, ids=8, row_base=0, null=(), d_count=False, L=None):
    """One fused call.  Returns (count, [full value buffers incl. the offset slack], full id buffer)."""
    n = table.n_rows
    bufs = [torch.full((n + offset + 1,), float("nan"), dtype=torch.float32, device="cuda") for _ in exprs_c]
    idx = None
    if ids:
        idx = torch.full((n + offset + 1,), -1, dtype=torch.int64 if ids == 8 else torch.int32, device="cuda")
    dc = torch.full((1,), -5, dtype=torch.int64, device="cuda") if d_count else None
    ptrs = [0 if j in null else b[offset:].data_ptr() for j, b in enumerate(bufs)]
    cnt = wx.project_filter_multi(table, exprs_c, cond_c, L or launch(), ptrs,
                                  idx[offset:].data_ptr() if ids else 0, ids or 8, row_base,
                                  dc.data_ptr() if d_count else 0, want_count=True)
    if d_count:
        assert int(dc.item()) == cnt
    return cnt, [b.cpu().numpy() for b in bufs], None if idx is None else idx.cpu().numpy()


def check(cnt, vals, idx, ref_vals, ref_idx, offset=0, row_base=0, null=()):
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


def lowered(exprs):
    return [ora.lower(e) for e in exprs]


def lower_cond(c):
    return ora.lower(c) if c else None


@pytest.mark.parametrize("cond_key", list(CONDS))
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_shapes_vs_oracle(m, offset, cond_key):
    for n in shapes(m):
        table, _ = device_table(n, offset)
        ref_vals, ref_idx = reference(n, cond_key)
        cnt, vals, idx = run(table, lowered(EXPRS[:m]), lower_cond(CONDS[cond_key]), offset=offset, d_count=True)
        check(cnt, vals, idx, ref_vals, ref_idx, offset=offset)


@pytest.mark.parametrize("ids,row_base", [(0, 0), (4, 0), (8, 0), (4, 1000), (8, 1 << 33)])
@pytest.mark.parametrize("m", [2, 3, 4])
def test_row_ids(m, ids, row_base):
    for n in (shapes(m)[5], BIG):
        table, _ = device_table(n, 0)
        ref_vals, ref_idx = reference(n, "gt15")
        cnt, vals, idx = run(table, lowered(EXPRS[:m]), lower_cond(CONDS["gt15"]), ids=ids, row_base=row_base)
        check(cnt, vals, idx, ref_vals, ref_idx, row_base=row_base)


@pytest.mark.parametrize("m,null", [(2, (0,)), (2, (0, 1)), (3, (1,)), (4, (0, 2, 3))])
def test_null_outputs(m, null):
    n = shapes(m)[5]
    table, _ = device_table(n, 0)
    ref_vals, ref_idx = reference(n, "gt15")
    cnt, vals, idx = run(table, lowered(EXPRS[:m]), lower_cond(CONDS["gt15"]), ids=4, null=null)
    check(cnt, vals, idx, ref_vals, ref_idx, null=null)


@pytest.mark.parametrize("m", [2, 4])
def test_tiny_tiles_pipeline_and_lookback_window(m, monkeypatch):
    # 512-row tiles: 1954 tiles, and the look-back window moves past 64
    # predecessors.  The grid is min(tiles, resident workgroups) -- measured
    # on the 256 CUs of an MI355X: 1536 workgroups for m = 2, 1280 for m = 4
    # -- so grid * 3 > n_tiles: the workgroups that start first take two
    # tiles at entry (a further one only while later workgroups have not
    # started), so about ceil(n_tiles / grid) + 1 = 3 tiles at the most, and
    # the late ones find the tickets gone.  The pipeline's steady state
    # (three tiles in flight in one workgroup, iteration after iteration) is
    # not what this test reaches; tests/test_gpu_compact_edges.py runs it.
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_COMPACT_GROUPS=1,WX_COMPACT_DWAVES=2")
    assert wx.select_tile_rows(m) == 512
    table, _ = device_table(BIG, 0)
    ref_vals, ref_idx = reference(BIG, "gt15")
    cnt, vals, idx = run(table, lowered(EXPRS[:m]), lower_cond(CONDS["gt15"]), ids=4)
    check(cnt, vals, idx, ref_vals, ref_idx)
    g = wx.compact_last_launch(launch())
    assert (g.deep, g.tile_rows, g.n_tiles) == (1, 512, -(-BIG // 512)) and 64 < g.grid <= g.n_tiles


def test_ticket_schedule_matches_default(monkeypatch):
    m = 3
    for n in (shapes(m)[5], BIG):
        table, _ = device_table(n, 0)
        ref_vals, ref_idx = reference(n, "gt15")
        monkeypatch.delenv("WARPDB_COMPACT_SCHED", raising=False)
        deep = run(table, lowered(EXPRS[:m]), lower_cond(CONDS["gt15"]))
        monkeypatch.setenv("WARPDB_COMPACT_SCHED", "ticket")
        ticket = run(table, lowered(EXPRS[:m]), lower_cond(CONDS["gt15"]))
        check(*ticket, ref_vals, ref_idx)
        assert ticket[0] == deep[0]
        for a, b in zip(deep[1], ticket[1]):
            assert np.array_equal(bits(a), bits(b))
        assert np.array_equal(deep[2], ticket[2])


def test_mixed_type_table_and_custom_function():
    n = 50_000
    rng = np.random.default_rng(7)
    cols = {
        "a": rng.integers(-1000, 1000, n).astype(np.int32),
        "d": rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64),
        "c": rng.uniform(-5, 5, n).astype(np.float64),
        "price": rng.uniform(0, 40, n).astype(np.float32),
    }
    table, _ = dev_table(cols)
    exprs = ["c * a + 1", "d / 3", "discount(price, 0.9)", "a"]
    cond = "c < 2.5"
    ht = ora.HostTable(cols)
    refs = [ora.project_filter(ht, e, cond) for e in exprs]
    cnt, vals, idx = run(table, lowered(exprs), ora.lower(cond), L=launch(custom=DISCOUNT_SRC))
    check(cnt, vals, idx, [r[0] for r in refs], refs[0][1])


@pytest.mark.parametrize("m", [2, 3, 4])
def test_fused_equals_separate_calls(m):
    n = shapes(m)[5]
    table, _ = device_table(n, 0)
    exprs_c, cond_c = lowered(EXPRS[:m]), lower_cond(CONDS["gt15"])
    cnt, vals, idx = run(table, exprs_c, cond_c)
    for j, e in enumerate(exprs_c):
        v = torch.full((n + 1,), float("nan"), dtype=torch.float32, device="cuda")
        i = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        c = wx.project_filter(table, e, cond_c, launch(), wx.MODE_COMPACT, v.data_ptr(), i.data_ptr(), 8, 0,
                              want_count=True)
        assert c == cnt
        assert np.array_equal(bits(v.cpu().numpy()), bits(vals[j]))
        assert np.array_equal(i.cpu().numpy(), idx)


def test_single_expression_forwards_to_every_mode():
    n = 4099
    table, _ = device_table(n, 0)
    out = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    wx.project_filter_multi(table, ["(price[idx] * quantity[idx])"], "(price[idx] > 15.0f)", launch(),
                            [out.data_ptr()], mode=wx.MODE_DENSE_FILL)
    ref = ora.dense(ora.HostTable(columns(n)), "price * quantity", "price > 15", np.zeros(n, np.float32))
    assert np.array_equal(bits(out.cpu().numpy()), bits(ref))


# ------------------------------------------------------------ query_select
def write_csv(path, cols):
    with open(path, "w") as f:
        f.write(",".join(cols) + "\n")
        for row in zip(*cols.values()):
            f.write(",".join(repr(x.item()) for x in row) + "\n")


@pytest.fixture(scope="module")
def fuzz_db(tmp_path_factory):
    from warpdb_amd import pywarpdb as pw

    n = 50_000
    rng = np.random.default_rng(2025)
    cols = {
        "price": rng.uniform(0, 40, n).astype(np.float32),
        "quantity": rng.integers(1, 101, n).astype(np.float32),
        "qi": rng.integers(-50, 51, n).astype(np.int32),
        "w": (rng.integers(-8000, 8001, n) / 8.0).astype(np.float64),
    }
    path = str(tmp_path_factory.mktemp("select") / "fuzz.csv")
    write_csv(path, cols)
    D = pw.DataType
    return pw.WarpDB(path, [D.Float32, D.Float32, D.Int32, D.Float64], 0), ora.HostTable(cols)


@pytest.mark.parametrize("case", range(20))
def test_random_select_lists_vs_oracle(fuzz_db, case):
    db, ht = fuzz_db
    rng = np.random.default_rng(5000 + case)
    m = 1 + case % 6  # 1..6 expressions: 5 and 6 run as two fused passes
    exprs = [gen_expr(rng, 3) for _ in range(m)]
    cond = gen_cond(rng) if case % 5 else ""
    names, cols, rows = db.query_select(exprs, cond)
    assert len(names) == len(cols) == m
    for j, e in enumerate(exprs):
        rv, ri = ora.project_filter(ht, e, cond or None)
        assert np.array_equal(rows, ri), (e, cond)
        assert np.array_equal(bits(cols[j]), bits(rv)), (e, cond)
    assert rows.dtype == np.int64 and all(c.dtype == np.float32 for c in cols)


def test_query_select_limits(fuzz_db):
    db, _ = fuzz_db
    with pytest.raises(RuntimeError, match="at most 16"):
        db.query_select(["price"] * 17)
    with pytest.raises(RuntimeError, match="Empty SELECT list"):
        db.query_select([])
    with pytest.raises(RuntimeError, match="Unknown column"):
        db.query_select(["price", "nope + 1"])
    names, cols, rows = db.query_select(["price"] * 16, "price > 39.9")
    assert len(cols) == 16 and all(np.array_equal(bits(c), bits(cols[0])) for c in cols)
    assert len(rows) == len(cols[0]) > 0


# ------------------------------------------------- pywarpdb on test.csv
def test_sql_table_plain():
    from warpdb_amd import pywarpdb as pw

    db = pw.WarpDB(TEST_CSV)
    names, cols, rows = db.query_sql_table("SELECT price, quantity, price * quantity FROM t WHERE price > 10")
    assert names == ["price", "quantity", "expr2"]
    assert cols[0].tolist() == [10.5, 20.0, 15.25, 30.0] and cols[1].tolist() == [3.0, 4.0, 2.0, 5.0]
    assert cols[2].tolist() == [31.5, 80.0, 30.5, 150.0]
    assert rows.tolist() == [0, 1, 2, 3]
    names, cols, rows = db.query_sql_table("SELECT price, price * quantity FROM t WHERE price > 15 LIMIT 2 OFFSET 1")
    assert cols[0].tolist() == [15.25, 30.0] and cols[1].tolist() == [30.5, 150.0] and rows.tolist() == [2, 3]
    names, cols, rows = db.query_sql_table("SELECT price, quantity FROM t WHERE price > 100")
    assert [c.tolist() for c in cols] == [[], []] and rows.tolist() == []
    # one item: the same values as query_sql
    names, cols, rows = db.query_sql_table("SELECT price * quantity FROM t WHERE price > 15")
    assert cols[0].tolist() == db.query_sql("SELECT price * quantity FROM t WHERE price > 15") and rows.tolist() == [1, 2, 3]
    names, cols, rows = db.query_sql_table("SELECT price FROM t ORDER BY price DESC LIMIT 2")
    assert cols[0].tolist() == [30.0, 20.0] and len(rows) == 0


def test_sql_table_grouped():
    from warpdb_amd import pywarpdb as pw

    db = pw.WarpDB(TEST_CSV)
    sql = "SELECT quantity, SUM(price), COUNT(price), AVG(price) FROM t GROUP BY quantity"
    names, cols, rows = db.query_sql_table(sql)
    assert names == ["quantity", "sum_1", "count_2", "avg_3"]
    assert cols[0].tolist() == [2.0, 3.0, 4.0, 5.0]
    assert cols[1].tolist() == [15.25, 10.5, 20.0, 30.0]
    assert cols[2].tolist() == [1.0] * 4 and cols[3].tolist() == [15.25, 10.5, 20.0, 30.0]
    assert len(rows) == 0
    names, cols, rows = db.query_sql_table(sql + " HAVING SUM(price) > 15 ORDER BY SUM(price) DESC LIMIT 2")
    assert cols[0].tolist() == [5.0, 4.0] and cols[1].tolist() == [30.0, 20.0]
    assert cols[2].tolist() == [1.0, 1.0] and cols[3].tolist() == [30.0, 20.0]
    names, cols, rows = db.query_sql_table("SELECT MAX(price), quantity, MIN(price) FROM t GROUP BY quantity")
    assert cols[0].tolist() == [15.25, 10.5, 20.0, 30.0] == cols[2].tolist() and cols[1].tolist() == [2.0, 3.0, 4.0, 5.0]
    # query_sql's own results are what they were
    assert db.query_sql("SELECT SUM(price) FROM t GROUP BY quantity HAVING SUM(price) > 15 ORDER BY SUM(price) DESC "
                        "LIMIT 2") == [30.0, 20.0]


def test_sql_table_refusals():
    from warpdb_amd import pywarpdb as pw

    db = pw.WarpDB(TEST_CSV)
    with pytest.raises(RuntimeError, match="not supported"):
        db.query_sql_table("SELECT price, quantity FROM t ORDER BY price")
    with pytest.raises(RuntimeError, match="not supported"):
        db.query_sql_table("SELECT DISTINCT price, quantity FROM t")
    with pytest.raises(RuntimeError, match="two different expressions"):
        db.query_sql_table("SELECT quantity, SUM(price), AVG(price * 2) FROM t GROUP BY quantity")
    with pytest.raises(RuntimeError, match="GROUP BY key or an aggregate"):
        db.query_sql_table("SELECT price, SUM(price) FROM t GROUP BY quantity")
    with pytest.raises(RuntimeError, match="Unknown column"):
        db.query_sql_table("SELECT price, nope FROM t")


# ------------------------------------------------------------- Arrow export
def test_arrow_struct_export():
    from warpdb_amd import pywarpdb as pw

    db = pw.WarpDB(TEST_CSV)
    arr_cap, sch_cap = db.query_arrow_select(["price", "price * quantity", "quantity"], "price > 15")
    a = ArrowArray.from_address(_ptr(arr_cap, None))
    s = ArrowSchema.from_address(_ptr(sch_cap, None))
    assert s.format == b"+s" and s.n_children == 4 and a.n_children == 4 and a.length == 3 and a.n_buffers == 1
    want = [(b"price", b"f", np.float32, [20.0, 15.25, 30.0]), (b"expr1", b"f", np.float32, [80.0, 30.5, 150.0]),
            (b"quantity", b"f", np.float32, [4.0, 2.0, 5.0]), (b"row", b"l", np.int64, [1, 2, 3])]
    for j, (name, fmt, dt, values) in enumerate(want):
        cs, ca = s.children[j].contents, a.children[j].contents
        assert cs.name == name and cs.format == fmt and cs.n_children == 0
        assert ca.length == 3 and ca.n_buffers == 2 and not ca.buffers[0] and ca.null_count == 0
        got = np.ctypeslib.as_array(ctypes.cast(ca.buffers[1], ctypes.POINTER(np.ctypeslib.as_ctypes_type(dt))),
                                    shape=(3,))
        assert got.tolist() == values
    # release: the callbacks clear themselves (children first) and a second release is a no-op
    assert a.release and s.release
    release_a = ctypes.CFUNCTYPE(None, ctypes.POINTER(ArrowArray))(a.release)
    release_s = ctypes.CFUNCTYPE(None, ctypes.POINTER(ArrowSchema))(s.release)
    release_a(ctypes.byref(a))
    release_s(ctypes.byref(s))
    assert not a.release and not s.release
    del arr_cap, sch_cap  # the capsules' destructors see released structs


def test_arrow_struct_export_pyarrow():
    pa = pytest.importorskip("pyarrow")
    from warpdb_amd import pywarpdb as pw

    db = pw.WarpDB(TEST_CSV)
    arr_cap, sch_cap = db.query_arrow_select(["price", "price * quantity"], "price > 15")
    a = pa.Array._import_from_c(_ptr(arr_cap, None), _ptr(sch_cap, None))
    assert a.to_pylist() == [{"price": 20.0, "expr1": 80.0, "row": 1}, {"price": 15.25, "expr1": 30.5, "row": 2},
                             {"price": 30.0, "expr1": 150.0, "row": 3}]
