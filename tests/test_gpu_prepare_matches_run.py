"""The prepare entry points name the program the run path launches.

wx_prepare / wx_prepare_multi / wx_prepare_gather and the run calls build
their module's identity with the same spec builders (codegen.cpp).  If the two
ever disagree nothing fails: build() warms one code object and the first query
compiles another.  So, per family: with an empty disk cache and an expression
no other test uses (a constant of its own, so the in-memory cache cannot hold
it either), prepare, note the compile count, run the matching query once, and
require that the count did not move and that the result equals the oracle.

The table holds integer-valued floats, so every product and every sum (of at
most 1000 of them) is an integer below 2^24, exact in float and in double:
sums compare exactly whatever the order of the additions.
"""
from __future__ import annotations

import numpy as np
import pytest

import oracle_lib as ora
from test_gpu_parity import bits, dev_table, launch

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from warpdb_amd import _warpexec as wx  # noqa: E402

N = 1000
COND = "price > 15"


def _columns():
    r = np.arange(N)
    return {"price": ((r * 7) % 40).astype(np.float32), "quantity": (r % 16).astype(np.int32)}


@pytest.fixture(scope="module")
def data():
    cols = _columns()
    table, tensors = dev_table(cols)
    for t in tensors.values():
        assert t.data_ptr() % 16 == 0
    return ora.HostTable(cols), table, tensors


@pytest.fixture()
def fresh_cache(tmp_path, monkeypatch):
    monkeypatch.setenv("WARPDB_KERNEL_CACHE", str(tmp_path))
    return tmp_path


def out(n, dtype=torch.float32, fill=float("nan")):
    t = torch.full((max(1, n),), fill, dtype=dtype, device="cuda")
    assert t.data_ptr() % 16 == 0
    return t


def prepared(prepare):
    """Run the prepare call; it compiled something, and returns the count after it."""
    before = wx.cache_stats()[0]
    prepare()
    after = wx.cache_stats()[0]
    assert after > before, "the case's expression was already cached: its constant is not unique"
    return after


def test_dense(data, fresh_cache):
    ht, table, _ = data
    e, c, L = "price * 1001", COND, launch()
    n0 = prepared(lambda: wx.prepare(table, wx.OP_DENSE, ora.lower(e), ora.lower(c), launch=L))
    vals = out(N, fill=-1.0)
    wx.project_filter(table, ora.lower(e), ora.lower(c), L, wx.MODE_DENSE, vals.data_ptr())
    assert wx.cache_stats()[0] == n0
    assert np.array_equal(bits(vals.cpu().numpy()), bits(ora.dense(ht, e, c, np.full(N, -1.0, np.float32))))


def test_compact_where(data, fresh_cache):
    ht, table, _ = data
    e, c, L = "price * 1002", COND, launch()
    n0 = prepared(lambda: wx.prepare(table, wx.OP_COMPACT, ora.lower(e), ora.lower(c), launch=L))
    vals, idx = out(N), out(N, torch.int64, -1)
    cnt = wx.project_filter(table, ora.lower(e), ora.lower(c), L, wx.MODE_COMPACT, vals.data_ptr(), idx.data_ptr(), 8,
                            0, want_count=True)
    assert wx.cache_stats()[0] == n0
    rv, ri = ora.project_filter(ht, e, c)
    assert cnt == len(ri) and np.array_equal(idx[:cnt].cpu().numpy(), ri)
    assert np.array_equal(bits(vals[:cnt].cpu().numpy()), bits(rv))


def test_sum(data, fresh_cache):
    ht, table, _ = data
    e, c, L = "price * 1003", COND, launch()
    n0 = prepared(lambda: wx.prepare(table, wx.OP_SUM, ora.lower(e), ora.lower(c), launch=L))
    got = wx.reduce_sum(table, ora.lower(e), ora.lower(c), L)
    assert wx.cache_stats()[0] == n0
    assert got == ora.reduce_sum(ht, e, c)


def test_sum_minmax(data, fresh_cache):
    ht, table, _ = data
    e, c, L = "price * 1004", COND, launch()
    n0 = prepared(lambda: wx.prepare(table, wx.OP_SUM, ora.lower(e), ora.lower(c), None, 1, launch=L))
    s, cnt, mn, mx = wx.reduce_stats(table, ora.lower(e), ora.lower(c), L)
    assert wx.cache_stats()[0] == n0
    rs, rc, rmn, rmx = ora.stats(ht, e, c)
    assert (s, cnt) == (rs, rc) and np.float32(mn) == rmn and np.float32(mx) == rmx


def group_outputs():
    return out(64, torch.int32, -1), out(64, torch.float64), out(64, torch.int64, -1)


def test_group(data, fresh_cache):
    ht, table, _ = data
    e, key, L = "price * 1005", "quantity", launch()
    n0 = prepared(lambda: wx.prepare(table, wx.OP_GROUP, ora.lower(e), None, ora.lower(key), 0, launch=L))
    k, s, c = group_outputs()
    ng = wx.group_sum(table, ora.lower(e), ora.lower(key), None, L, 0, 64, k.data_ptr(), s.data_ptr(), c.data_ptr())
    assert wx.cache_stats()[0] == n0
    rk, rs, rc = ora.group_sum(ht, e, key)
    assert ng == len(rk) == 16
    assert np.array_equal(k[:ng].cpu().numpy(), rk) and np.array_equal(c[:ng].cpu().numpy(), rc)
    assert np.array_equal(s[:ng].cpu().numpy(), rs)


def test_group_minmax(data, fresh_cache):
    ht, table, _ = data
    e, key, L = "price * 1006", "quantity", launch()
    n0 = prepared(lambda: wx.prepare(table, wx.OP_GROUP, ora.lower(e), None, ora.lower(key), 1, launch=L))
    k, s, c = group_outputs()
    mn, mx = out(64), out(64)
    ng = wx.group_agg(table, ora.lower(e), ora.lower(key), None, L, 0, 64, k.data_ptr(), s.data_ptr(), c.data_ptr(),
                      mn.data_ptr(), mx.data_ptr())
    assert wx.cache_stats()[0] == n0
    rk, rs, rc, rmn, rmx = ora.group_agg(ht, e, key)
    assert ng == len(rk) == 16
    assert np.array_equal(k[:ng].cpu().numpy(), rk) and np.array_equal(c[:ng].cpu().numpy(), rc)
    assert np.array_equal(s[:ng].cpu().numpy(), rs)
    assert np.array_equal(bits(mn[:ng].cpu().numpy()), bits(rmn))
    assert np.array_equal(bits(mx[:ng].cpu().numpy()), bits(rmx))


def test_topk_descending(data, fresh_cache):
    ht, table, _ = data
    e, L = "price * 1007 + quantity", launch()
    n0 = prepared(lambda: wx.prepare(table, wx.OP_TOPK, ora.lower(e), ora.lower(COND), None, 5, launch=L))
    keys, idx = out(5), out(5, torch.int64, -1)
    cnt = wx.topk(table, ora.lower(e), ora.lower(COND), None, 5, True, L, keys.data_ptr(), idx.data_ptr())
    assert wx.cache_stats()[0] == n0
    rk, ri, _ = ora.topk(ht, e, 5, True, COND)
    assert cnt == 5 == len(rk)
    assert np.array_equal(bits(keys.cpu().numpy()), bits(rk))
    # (price, quantity) repeats every 80 rows: equal keys may come from either row
    rows = idx.cpu().numpy()
    full = ora.project_filter(ht, e, None)[0]
    assert np.array_equal(bits(full[rows]), bits(rk)) and len(set(rows.tolist())) == 5


def test_prepare_multi(data, fresh_cache):
    ht, table, _ = data
    exprs, L = ["price * 1008", "price + 1009"], launch()
    low = [ora.lower(e) for e in exprs]
    n0 = prepared(lambda: wx.prepare_multi(table, low, ora.lower(COND), launch=L))
    bufs, idx = [out(N), out(N)], out(N, torch.int64, -1)
    cnt = wx.project_filter_multi(table, low, ora.lower(COND), L, [b.data_ptr() for b in bufs], idx.data_ptr(), 8, 0,
                                  want_count=True)
    assert wx.cache_stats()[0] == n0
    for e, b in zip(exprs, bufs):
        rv, ri = ora.project_filter(ht, e, COND)
        assert cnt == len(ri) and np.array_equal(idx[:cnt].cpu().numpy(), ri)
        assert np.array_equal(bits(b[:cnt].cpu().numpy()), bits(rv))


def test_prepare_gather(data, fresh_cache):
    ht, table, _ = data
    exprs, L = ["price * 1010", "price + 1011"], launch()
    low = [ora.lower(e) for e in exprs]
    n0 = prepared(lambda: wx.prepare_gather(table, low, launch=L))
    rows_h = (np.arange(300, dtype=np.int64) * 37) % N
    rows = torch.from_numpy(rows_h).cuda()
    bufs = [out(300), out(300)]
    wx.gather_multi(table, low, rows.data_ptr(), 8, 300, L, [b.data_ptr() for b in bufs])
    assert wx.cache_stats()[0] == n0
    for e, b in zip(exprs, bufs):
        assert np.array_equal(bits(b.cpu().numpy()), bits(ora.project_filter(ht, e, None)[0][rows_h]))


def test_util_sorts(fresh_cache):
    L = launch()
    wx.prepare(None, wx.OP_UTIL, launch=L)  # (its modules have no expression: another test may have loaded them)
    n0 = wx.cache_stats()[0]
    r = np.arange(N)
    vals_h = ((r * 389) % 251).astype(np.float32) - 100.0
    keys_h = ((r * 977) % 61).astype(np.int32) - 30
    v = torch.from_numpy(vals_h).cuda()
    wx.sort_float(v.data_ptr(), N, True, L)
    k, p = torch.from_numpy(keys_h).cuda(), torch.from_numpy(vals_h).cuda()
    wx.sort_pairs(k.data_ptr(), p.data_ptr(), N, True, L)
    assert wx.cache_stats()[0] == n0
    assert np.array_equal(bits(v.cpu().numpy()), bits(np.sort(vals_h, kind="stable")))
    order = np.argsort(keys_h, kind="stable")
    assert np.array_equal(k.cpu().numpy(), keys_h[order])
    assert np.array_equal(bits(p.cpu().numpy()), bits(vals_h[order]))
