"""GPU tests of the ordered multi-column SELECT: the multi-output row gather
(wx_gather.hip) through wx_gather_multi, wx_select_ordered with its two
routes (top-K scan / key compaction + pair sort), and the host layer
(query_select_ordered, query_rows, query_sql_ordered, the Arrow export).

The oracle is oracle_lib.project_filter, called per expression and for the
ORDER BY key, then numpy's stable argsort (key ascending, -key descending:
NaN last in both directions, -0.0 == +0.0, ties by ascending row) -- the
oracle of every sort test here.  Every comparison is bit-exact; outputs are
prefilled with a NaN / -1 sentinel that must be intact at positions >= count
and in front of an offset pointer.
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
from test_gpu_parity import DISCOUNT_SRC, bits, dev_table, launch, read_csv
from test_gpu_select_multi import write_csv

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from warpdb_amd import _warpexec as wx  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEST_CSV = os.path.join(ROOT, "tests", "golden", "test.csv")
SENTINEL = np.float32(np.nan).view(np.uint32)  # torch.full's NaN

EXPRS = ["price * quantity", "price", "quantity + 1", "price * 0.5 - quantity"] + \
        [f"price * {k} + quantity" for k in range(2, 14)]
CONDS = {"none": None, "never": "price < 0", "always": "price >= 0", "gt15": "price > 15"}
BIG = 1_000_003
LIMITS = [0, 1, 5, 32, 33, 1000, -1]


# ------------------------------------------------------------------ tables
@functools.lru_cache(maxsize=None)
def columns(key):
    """Host columns by key: an int is a synth.c2_table of that many rows; "nan"
    is the heavy-ties table of test_topk_heavy_ties_nan_signed_zero (six
    distinct keys, 1 % NaN, 29 % -0.0) at BIG rows."""
    if key == "nan":
        n = BIG
        u = synth.uniform_f32(n, 9, 0.0, 1.0)
        p = np.floor(synth.uniform_f32(n, 1, -3.0, 3.0)).astype(np.float32)
        p[u < 0.01] = np.nan
        p[(u >= 0.01) & (u < 0.3)] = np.float32(-0.0)
        cols = {"price": p, "quantity": synth.uniform_int(n, 2, 1, 100).astype(np.float32)}
    else:
        cols = synth.c2_table(key)
    for v in cols.values():
        v.setflags(write=False)
    return cols


@functools.lru_cache(maxsize=None)
def device_table(key):
    return dev_table(columns(key))


@functools.lru_cache(maxsize=None)
def ref_expr(key, expr, cond_key):
    """(values, row ids) of one expression over the rows the condition keeps: computed once, read-only."""
    v, i = ora.project_filter(ora.HostTable(columns(key)), expr, CONDS[cond_key])
    v.setflags(write=False)
    i.setflags(write=False)
    return v, i


@functools.lru_cache(maxsize=None)
def ref_order(key, order, cond_key, desc):
    k, _ = ref_expr(key, order, cond_key)
    o = np.argsort(-k if desc else k, kind="stable")
    o.setflags(write=False)
    return o


def lowered(exprs):
    return [ora.lower(e) for e in exprs]


def lower_cond(c):
    return ora.lower(c) if c else None


# ----------------------------------------------------------- wx_gather_multi
def run_gather(table, exprs_c, ids, idx_bytes, row_base=0, out_row_base=0, offset=0, null=(), d_count=None,
               want_rows=True, L=None):
    """One gather call over `ids` (numpy, already including row_base).  Returns
    ([value buffers incl. slack], row buffer), each count + offset + 9 long."""
    count = len(ids)
    size = count + offset + 9
    dt = torch.int64 if idx_bytes == 8 else torch.int32
    d_ids = torch.from_numpy(np.ascontiguousarray(ids).astype(np.int64 if idx_bytes == 8 else np.int32)).cuda() \
        if count else torch.empty(1, dtype=dt, device="cuda")
    bufs = [torch.full((size,), float("nan"), dtype=torch.float32, device="cuda") for _ in exprs_c]
    rows = torch.full((size + 1,), -1, dtype=torch.int64, device="cuda")
    dc = torch.tensor([d_count], dtype=torch.int64, device="cuda") if d_count is not None else None
    ptrs = [0 if j in null else b[offset:].data_ptr() for j, b in enumerate(bufs)]
    wx.gather_multi(table, exprs_c, d_ids.data_ptr(), idx_bytes, count, L or launch(), ptrs,
                    rows[offset:].data_ptr() if want_rows else 0, row_base, out_row_base,
                    dc.data_ptr() if dc is not None else 0)
    return [b.cpu().numpy() for b in bufs], rows.cpu().numpy()


def check_gather(vals, rows, ref_vals, ref_rows, count, offset=0, null=(), want_rows=True):
    for j, v in enumerate(vals):
        if j in null:
            assert (bits(v) == SENTINEL).all(), f"output {j}: written through a null pointer's neighbour"
            continue
        assert np.array_equal(bits(v[offset:offset + count]), bits(ref_vals[j][:count])), f"output {j}"
        assert (bits(v[offset + count:]) == SENTINEL).all(), f"output {j}: written at positions >= count"
        assert (bits(v[:offset]) == SENTINEL).all(), f"output {j}: written in front of the pointer"
    if want_rows:
        assert np.array_equal(rows[offset:offset + count], ref_rows[:count])
        assert (rows[offset + count:] == -1).all() and (rows[:offset] == -1).all()
    else:
        assert (rows == -1).all()


GATHER_N = 100_003


def make_ids(pattern, count, seed):
    rng = np.random.default_rng(seed)
    if pattern == "random":
        return rng.integers(0, GATHER_N, count)
    if pattern == "ascending":
        return np.sort(rng.choice(GATHER_N, count, replace=False)) if count else np.zeros(0, np.int64)
    return np.full(count, GATHER_N - 1, np.int64)  # all equal: the table's last row


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("idx_bytes", [4, 8])
@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_gather_shapes_vs_oracle(m, idx_bytes, offset):
    t = wx.gather_tile_rows(m)
    assert t > 0
    table, _ = device_table(GATHER_N)
    full = [ref_expr(GATHER_N, e, "none")[0] for e in EXPRS[:m]]
    for count in (0, 1, 3, 4, 5, t - 1, t, t + 1, 3 * t + 5):
        for pattern in ("random", "ascending", "equal"):
            ids = make_ids(pattern, count, 100 * m + count % 97)
            vals, rows = run_gather(table, lowered(EXPRS[:m]), ids, idx_bytes, offset=offset)
            check_gather(vals, rows, [f[ids] for f in full], ids, count, offset=offset)


@pytest.mark.parametrize("idx_bytes,row_base,out_row_base", [(4, 1000, 0), (8, 1 << 33, 1 << 35), (4, 0, 1 << 40),
                                                             (8, -7, 5)])
def test_gather_row_bases(idx_bytes, row_base, out_row_base):
    m = 3
    count = 2 * wx.gather_tile_rows(m) + 3
    table, _ = device_table(GATHER_N)
    ids = make_ids("random", count, 5)
    full = [ref_expr(GATHER_N, e, "none")[0] for e in EXPRS[:m]]
    vals, rows = run_gather(table, lowered(EXPRS[:m]), ids + row_base, idx_bytes, row_base=row_base,
                            out_row_base=out_row_base)
    check_gather(vals, rows, [f[ids] for f in full], ids + out_row_base, count)


@pytest.mark.parametrize("m,null", [(4, (1,)), (4, (0, 2, 3)), (2, (0, 1)), (3, (2,))])
@pytest.mark.parametrize("want_rows", [True, False])
def test_gather_null_outputs(m, null, want_rows):
    count = wx.gather_tile_rows(m) + 7
    table, _ = device_table(GATHER_N)
    ids = make_ids("random", count, 6)
    full = [ref_expr(GATHER_N, e, "none")[0] for e in EXPRS[:m]]
    vals, rows = run_gather(table, lowered(EXPRS[:m]), ids, 8, null=null, want_rows=want_rows)
    check_gather(vals, rows, [f[ids] for f in full], ids, count, null=null, want_rows=want_rows)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("d_count", [0, 1, 6, 2049, 10**9])
def test_gather_device_count_bounds_the_host_count(d_count, offset):
    # the top-K route's shape: the host passes the limit, the device the rows found
    m = 4
    count = 2 * wx.gather_tile_rows(m) + 2
    table, _ = device_table(GATHER_N)
    ids = make_ids("random", count, 8)
    full = [ref_expr(GATHER_N, e, "none")[0] for e in EXPRS[:m]]
    vals, rows = run_gather(table, lowered(EXPRS[:m]), ids, 4, offset=offset, d_count=d_count)
    check_gather(vals, rows, [f[ids] for f in full], ids, min(count, d_count), offset=offset)


def test_gather_mixed_type_table_and_custom_function():
    n = 50_000
    rng = np.random.default_rng(7)
    cols = {
        "a": rng.integers(-1000, 1000, n).astype(np.int32),
        "d": rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64),
        "c": rng.uniform(-5, 5, n).astype(np.float64),
        "price": rng.uniform(0, 40, n).astype(np.float32),
    }
    table, _ = dev_table(cols, 1)  # columns 4 / 8 bytes past a 16-byte boundary
    exprs = ["c * a + 1", "d / 3", "discount(price, 0.9)", "a"]
    ht = ora.HostTable(cols)
    full = [ora.project_filter(ht, e, None)[0] for e in exprs]
    ids = rng.integers(0, n, 4099)
    vals, rows = run_gather(table, lowered(exprs), ids, 8, L=launch(custom=DISCOUNT_SRC))
    check_gather(vals, rows, [f[ids] for f in full], ids, len(ids))


def test_gather_of_compaction_row_ids_equals_compaction_values():
    # late materialisation: the row ids of one compaction feed the gather on the device
    m = 4
    table, _ = device_table(GATHER_N)
    exprs_c, cond_c = lowered(EXPRS[:m]), lower_cond(CONDS["gt15"])
    idx = torch.full((GATHER_N,), -1, dtype=torch.int32, device="cuda")
    dc = torch.zeros(1, dtype=torch.int64, device="cuda")
    cnt = wx.project_filter(table, exprs_c[0], cond_c, launch(), wx.MODE_COMPACT, 0, idx.data_ptr(), 4, 0,
                            dc.data_ptr(), want_count=True)
    bufs = [torch.full((GATHER_N,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(m)]
    wx.gather_multi(table, exprs_c, idx.data_ptr(), 4, GATHER_N, launch(), [b.data_ptr() for b in bufs],
                    d_count=dc.data_ptr())
    for j in range(m):
        rv, ri = ref_expr(GATHER_N, EXPRS[j], "gt15")
        assert cnt == len(ri)
        out = bufs[j].cpu().numpy()
        assert np.array_equal(bits(out[:cnt]), bits(rv)) and (bits(out[cnt:]) == SENTINEL).all()


# --------------------------------------------------------- wx_select_ordered
def run_ordered(table, exprs_c, cond_c, order_c, desc, limit, capacity, null_vals=(), keys=True, rows=True,
                d_count=True, L=None):
    """One call.  Returns (count, [value buffers], key buffer, row buffer), each capacity + 1 long."""
    size = capacity + 1
    bufs = [torch.full((size,), float("nan"), dtype=torch.float32, device="cuda") for _ in exprs_c]
    kb = torch.full((size,), float("nan"), dtype=torch.float32, device="cuda")
    rb = torch.full((size,), -1, dtype=torch.int64, device="cuda")
    dc = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    ptrs = [0 if j in null_vals else b.data_ptr() for j, b in enumerate(bufs)]
    cnt = wx.select_ordered(table, exprs_c, cond_c, order_c, desc, limit, L or launch(), ptrs,
                            kb.data_ptr() if keys else 0, rb.data_ptr() if rows else 0, capacity,
                            d_count=dc.data_ptr() if d_count else 0)
    if d_count:
        assert int(dc.item()) == cnt
    return cnt, [b.cpu().numpy() for b in bufs], kb.cpu().numpy(), rb.cpu().numpy()


def check_ordered(res, key, exprs, order, cond_key, desc, limit, row_base=0, null_vals=(), keys=True, rows=True):
    cnt, vals, kb, rb = res
    o = ref_order(key, order, cond_key, desc)
    want = len(o) if limit < 0 else min(limit, len(o))
    assert cnt == want
    o = o[:want]
    rk, ri = ref_expr(key, order, cond_key)
    if keys:
        assert np.array_equal(bits(kb[:cnt]), bits(rk[o]))
        assert (bits(kb[cnt:]) == SENTINEL).all()
    else:
        assert (bits(kb) == SENTINEL).all()
    if rows:
        assert np.array_equal(rb[:cnt], ri[o] + row_base)
        assert (rb[cnt:] == -1).all()
    else:
        assert (rb == -1).all()
    for j, v in enumerate(vals):
        if j in null_vals:
            assert (bits(v) == SENTINEL).all()
            continue
        assert np.array_equal(bits(v[:cnt]), bits(ref_expr(key, exprs[j], cond_key)[0][o])), f"output {j}"
        assert (bits(v[cnt:]) == SENTINEL).all(), f"output {j}: written at positions >= count"


def capacity_for(key, order, cond_key, limit):
    passing = len(ref_expr(key, order, cond_key)[0])
    return passing if limit < 0 else min(limit, passing)


def table_sizes():
    return [0, 1, wx.gather_tile_rows(4) + 1, BIG]


@pytest.mark.parametrize("cond_key", list(CONDS))
@pytest.mark.parametrize("size", range(4))
def test_ordered_tables_conditions_limits(size, cond_key):
    n = table_sizes()[size]
    table, _ = device_table(n)
    m = 4
    for desc in (True, False):
        for limit in LIMITS:
            cap = capacity_for(n, "price", cond_key, limit) if limit < 0 else limit
            res = run_ordered(table, lowered(EXPRS[:m]), lower_cond(CONDS[cond_key]), ora.lower("price"), desc,
                              limit, cap)
            check_ordered(res, n, EXPRS[:m], "price", cond_key, desc, limit)


@pytest.mark.parametrize("desc", [True, False])
@pytest.mark.parametrize("key,order", [(BIG, "price"), (BIG, "quantity"), ("nan", "price")])
def test_ordered_key_data(key, order, desc):
    # nearly unique keys; 100 distinct keys (the ties-by-row rule decides almost
    # every position); six distinct keys with NaN and +-0.0
    table, _ = device_table(key)
    m = 4
    for limit in LIMITS:
        cap = capacity_for(key, order, "gt15", limit)
        res = run_ordered(table, lowered(EXPRS[:m]), lower_cond(CONDS["gt15"]), ora.lower(order), desc, limit, cap)
        check_ordered(res, key, EXPRS[:m], order, "gt15", desc, limit)


@pytest.mark.parametrize("limit", [5, 1000])
@pytest.mark.parametrize("m", [0, 1, 4, 5, 16])
def test_ordered_output_counts(m, limit):
    table, _ = device_table(BIG)
    res = run_ordered(table, lowered(EXPRS[:m]), lower_cond(CONDS["gt15"]), ora.lower("quantity"), True, limit, limit)
    check_ordered(res, BIG, EXPRS[:m], "quantity", "gt15", True, limit)


@pytest.mark.parametrize("limit", [5, 1000])
def test_ordered_null_outputs_and_row_base(limit):
    table, _ = device_table(BIG)
    args = (table, lowered(EXPRS[:6]), lower_cond(CONDS["gt15"]), ora.lower("price * quantity"), False, limit, limit)
    for kw in (dict(null_vals=(0, 5)), dict(keys=False), dict(rows=False, d_count=False),
               dict(null_vals=(0, 1, 2, 3), keys=False, rows=False), dict(null_vals=tuple(range(6)))):
        check_ordered(run_ordered(*args, **kw), BIG, EXPRS[:6], "price * quantity", "gt15", False, limit,
                      **{k: v for k, v in kw.items() if k != "d_count"})
    # global rows of a shard: row_base is added to the rows, the values are the same
    size = limit + 1
    bufs = [torch.full((size,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
    rb = torch.full((size,), -1, dtype=torch.int64, device="cuda")
    cnt = wx.select_ordered(table, lowered(EXPRS[:2]), lower_cond(CONDS["gt15"]), ora.lower("price"), True, limit,
                            launch(), [b.data_ptr() for b in bufs], 0, rb.data_ptr(), limit, row_base=1 << 36)
    no_keys = np.full(size, np.nan, np.float32)
    check_ordered((cnt, [b.cpu().numpy() for b in bufs], no_keys, rb.cpu().numpy()), BIG, EXPRS[:2], "price", "gt15",
                  True, limit, row_base=1 << 36, keys=False)


@pytest.mark.parametrize("limit", [5, 32, 33, 1000, -1])
def test_ordered_capacity_one_short(limit):
    n = wx.gather_tile_rows(4) + 1
    table, _ = device_table(n)
    need = capacity_for(n, "price", "gt15", limit)
    assert need > 0
    with pytest.raises(wx.WarpExecError) as ei:
        run_ordered(table, lowered(EXPRS[:2]), lower_cond(CONDS["gt15"]), ora.lower("price"), True, limit, need - 1)
    assert ei.value.status == wx.WX_ERR_CAPACITY and ei.value.count == need
    # the exact capacity is enough (a top-K limit above it reads the count on the host first)
    res = run_ordered(table, lowered(EXPRS[:2]), lower_cond(CONDS["gt15"]), ora.lower("price"), True, limit, need)
    check_ordered(res, n, EXPRS[:2], "price", "gt15", True, limit)


def test_ordered_few_passing_rows_under_a_small_limit():
    # 3 rows pass, LIMIT 5 / 32: the top-K route's device count (3) bounds the gather of `limit` positions
    n = wx.gather_tile_rows(4) + 1
    table, _ = device_table(n)
    price = columns(n)["price"]
    third = np.sort(price)[-3]
    cond = f"price >= {float(third)!r}"
    ht = ora.HostTable(columns(n))
    rk, ri = ora.project_filter(ht, "price", cond)
    assert len(ri) == 3
    o = np.argsort(-rk, kind="stable")
    for limit in (5, 32):
        for cap in (limit, 3):
            cnt, vals, kb, rb = run_ordered(table, lowered(EXPRS[:4]), ora.lower(cond), ora.lower("price"), True,
                                            limit, cap)
            assert cnt == 3 and np.array_equal(rb[:3], ri[o]) and (rb[3:] == -1).all()
            assert np.array_equal(bits(kb[:3]), bits(rk[o])) and (bits(kb[3:]) == SENTINEL).all()
            for j in range(4):
                rv = ora.project_filter(ht, EXPRS[j], cond)[0]
                assert np.array_equal(bits(vals[j][:3]), bits(rv[o])) and (bits(vals[j][3:]) == SENTINEL).all()


@pytest.mark.parametrize("desc", [True, False])
@pytest.mark.parametrize("key", [BIG, "nan"])
def test_route_parity(key, desc, monkeypatch):
    table, _ = device_table(key)
    for limit in (1, 5, 32):
        args = (table, lowered(EXPRS[:5]), lower_cond(CONDS["gt15"]), ora.lower("price"), desc, limit, limit)
        monkeypatch.delenv("WARPDB_ORDERED_ROUTE", raising=False)
        topk = run_ordered(*args)
        monkeypatch.setenv("WARPDB_ORDERED_ROUTE", "sort")
        sort = run_ordered(*args)
        check_ordered(sort, key, EXPRS[:5], "price", "gt15", desc, limit)
        assert topk[0] == sort[0]
        for a, b in zip(topk[1], sort[1]):
            assert np.array_equal(bits(a), bits(b))
        assert np.array_equal(bits(topk[2]), bits(sort[2])) and np.array_equal(topk[3], sort[3])


# ------------------------------------------------------------- host layer
@pytest.fixture(scope="module")
def small_db():
    from warpdb_amd import pywarpdb as pw

    return pw.WarpDB(TEST_CSV), ora.HostTable(read_csv(TEST_CSV))


@pytest.fixture(scope="module")
def big_db(tmp_path_factory):
    from warpdb_amd import pywarpdb as pw

    n = 100_003
    rng = np.random.default_rng(77)
    cols = {
        "price": rng.uniform(0, 40, n).astype(np.float32),
        "quantity": rng.integers(1, 101, n).astype(np.float32),
        "qi": rng.integers(-50, 51, n).astype(np.int32),
    }
    path = str(tmp_path_factory.mktemp("ordered") / "big.csv")
    write_csv(path, cols)
    D = pw.DataType
    return pw.WarpDB(path, [D.Float32, D.Float32, D.Int32], 0), ora.HostTable(cols)


HOST_EXPRS = ["price", "quantity", "price * quantity", "price * 0.5 - quantity", "quantity + 1"]


def host_reference(ht, exprs, where, order, desc, limit=-1, offset=0):
    rk, ri = ora.project_filter(ht, order, where or None)
    o = np.argsort(-rk if desc else rk, kind="stable")
    o = o[offset:] if limit < 0 else o[offset:offset + limit]
    return [ora.project_filter(ht, e, where or None)[0][o] for e in exprs], ri[o]


@pytest.mark.parametrize("which", ["small", "big"])
def test_query_select_ordered_vs_oracle(which, small_db, big_db):
    db, ht = small_db if which == "small" else big_db
    for where in ("", "price > 15"):
        for order, desc in (("price", True), ("quantity", False), ("price * quantity", True)):
            for limit, offset in ((-1, 0), (2, 1), (40, 3), (5, 10**7)):
                names, cols, rows = db.query_select_ordered(HOST_EXPRS, where, order, desc, limit, offset)
                assert names == ["price", "quantity", "expr2", "expr3", "expr4"]
                rv, rr = host_reference(ht, HOST_EXPRS, where, order, desc, limit, offset)
                assert rows.dtype == np.int64 and np.array_equal(rows, rr), (where, order, desc, limit, offset)
                for j in range(len(HOST_EXPRS)):
                    assert cols[j].dtype == np.float32 and np.array_equal(bits(cols[j]), bits(rv[j]))


@pytest.mark.parametrize("which", ["small", "big"])
def test_query_sql_ordered_vs_oracle_and_query_sql(which, small_db, big_db):
    db, ht = small_db if which == "small" else big_db
    items = ["price", "quantity", "price * quantity"]
    for tail, order, desc, limit, offset in (("ORDER BY price DESC LIMIT 3", "price", True, 3, 0),
                                             ("ORDER BY price * quantity ASC LIMIT 100", "price * quantity", False, 100, 0),
                                             ("ORDER BY price", "price", False, -1, 0),
                                             ("ORDER BY quantity DESC LIMIT 7 OFFSET 2", "quantity", True, 7, 2)):
        sql = f"SELECT {', '.join(items)} FROM t WHERE price > 15 {tail}"
        names, cols, rows = db.query_sql_ordered(sql)
        assert names == ["price", "quantity", "expr2"]
        rv, rr = host_reference(ht, items, "price > 15", order, desc, limit, offset)
        assert np.array_equal(rows, rr), sql
        for j, e in enumerate(items):
            assert np.array_equal(bits(cols[j]), bits(rv[j])), sql
            # column j is what the single-column query returns
            one = np.array(db.query_sql(f"SELECT {e} FROM t WHERE price > 15 {tail}"), np.float32)
            assert np.array_equal(bits(cols[j]), bits(one)), (sql, e)
    # one item is allowed; no WHERE
    names, cols, rows = db.query_sql_ordered("SELECT price * quantity FROM t ORDER BY quantity DESC LIMIT 4")
    rv, rr = host_reference(ht, ["price * quantity"], "", "quantity", True, 4)
    assert names == ["expr0"] and np.array_equal(rows, rr) and np.array_equal(bits(cols[0]), bits(rv[0]))


def test_query_rows_equals_query_select_picked_on_the_host(big_db):
    db, ht = big_db
    names, cols, rows = db.query_select(HOST_EXPRS, "price > 15")
    rng = np.random.default_rng(3)
    pick = rng.integers(0, len(rows), 5000)
    n2, c2, r2 = db.query_rows(HOST_EXPRS, rows[pick].tolist())
    assert n2 == names and np.array_equal(r2, rows[pick])
    for j in range(len(HOST_EXPRS)):
        assert np.array_equal(bits(c2[j]), bits(cols[j][pick]))
    n3, c3, r3 = db.query_rows(["price"], [])
    assert n3 == ["price"] and len(c3) == 1 and len(c3[0]) == 0 and len(r3) == 0
    for bad in (-1, ht.n, 1 << 40):
        with pytest.raises(RuntimeError, match=f"Row id out of range: {bad}"):
            db.query_rows(["price"], [0, bad, 1])


def test_host_layer_refusals(small_db):
    db, _ = small_db
    with pytest.raises(RuntimeError, match="at most 16"):
        db.query_select_ordered(["price"] * 17, "", "price")
    with pytest.raises(RuntimeError, match="Empty SELECT list"):
        db.query_select_ordered([], "", "price")
    with pytest.raises(RuntimeError, match="Unknown column"):
        db.query_select_ordered(["price", "nope + 1"], "", "price")
    with pytest.raises(RuntimeError, match="Empty ORDER BY"):
        db.query_select_ordered(["price"], "", " ")
    with pytest.raises(RuntimeError, match="ORDER BY expression.*Unknown column"):
        db.query_select_ordered(["price"], "", "nope")
    with pytest.raises(RuntimeError, match="Failed to parse expression"):
        db.query_rows(["SUM(price)"], [0])
    with pytest.raises(RuntimeError, match="query_rows takes at most 16"):
        db.query_rows(["price"] * 17, [0])
    for sql, msg in (("SELECT price, quantity FROM t", "needs an ORDER BY"),
                     ("SELECT quantity, SUM(price) FROM t GROUP BY quantity ORDER BY quantity", "GROUP BY"),
                     ("SELECT DISTINCT price, quantity FROM t ORDER BY price", "DISTINCT"),
                     ("SELECT price, SUM(price) FROM t ORDER BY price", "aggregates"),
                     ("SELECT price, SUM(price) OVER (PARTITION BY quantity) FROM t ORDER BY price", "window functions"),
                     ("SELECT price, quantity FROM t JOIN u ON price = quantity ORDER BY price", "JOIN"),
                     ("SELECT price, nope FROM t ORDER BY price", "Unknown column"),
                     ("SELECT FROM", "Failed to parse SQL")):
        with pytest.raises(RuntimeError, match=msg):
            db.query_sql_ordered(sql)
    # the row-order entry point keeps refusing what it refused
    with pytest.raises(RuntimeError, match="not supported"):
        db.query_sql_table("SELECT price, quantity FROM t ORDER BY price")


def test_arrow_struct_export_ordered(small_db):
    db, ht = small_db
    exprs = ["price", "price * quantity", "quantity"]
    arr_cap, sch_cap = db.query_arrow_select_ordered(exprs, "price > 15", "price", True, 2, 0)
    rv, rr = host_reference(ht, exprs, "price > 15", "price", True, 2)
    a = ArrowArray.from_address(_ptr(arr_cap, None))
    s = ArrowSchema.from_address(_ptr(sch_cap, None))
    assert s.format == b"+s" and s.n_children == 4 and a.n_children == 4 and a.length == 2 and a.n_buffers == 1
    want = [(b"price", b"f", np.float32, rv[0]), (b"expr1", b"f", np.float32, rv[1]),
            (b"quantity", b"f", np.float32, rv[2]), (b"row", b"l", np.int64, rr)]
    for j, (name, fmt, dt, values) in enumerate(want):
        cs, ca = s.children[j].contents, a.children[j].contents
        assert cs.name == name and cs.format == fmt and cs.n_children == 0
        assert ca.length == 2 and ca.n_buffers == 2 and not ca.buffers[0] and ca.null_count == 0
        got = np.ctypeslib.as_array(ctypes.cast(ca.buffers[1], ctypes.POINTER(np.ctypeslib.as_ctypes_type(dt))),
                                    shape=(2,))
        assert got.tolist() == values.tolist()
    del arr_cap, sch_cap
