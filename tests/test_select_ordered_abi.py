"""CPU tests of the ordered multi-column SELECT's C ABI (wx_gather_multi,
wx_prepare_gather, wx_gather_tile_rows, wx_select_ordered): the symbols exist,
the row gather compiles for gfx950 without a device, and every argument check
fires before any device call."""
from __future__ import annotations

import pytest

from warpdb_amd import _warpexec as wx

DISCOUNT_SRC = "__device__ float discount(float price, float rate) {\n    return price * rate;\n}\n"


def table(**cols):
    dt = {"f32": wx.FLOAT32, "i32": wx.INT32, "f64": wx.FLOAT64, "i64": wx.INT64, "str": wx.STRING}
    return wx.Table(1 << 20, [wx.Column(k, dt[v], (i + 1) << 20) for i, (k, v) in enumerate(cols.items())])


def no_custom():
    return wx.make_launch(flags=wx.F_NO_CUSTOM)


def test_symbols_and_version():
    lib = wx.load()
    for name in ("wx_gather_multi", "wx_prepare_gather", "wx_gather_tile_rows", "wx_select_ordered"):
        assert hasattr(lib, name) and name in wx.EXPORTED_SYMBOLS
    assert lib.wx_abi_version() == 1


def test_gather_tile_rows(monkeypatch):
    monkeypatch.delenv("WARPDB_EXTRA_DEFINES", raising=False)
    for m in (1, 2, 3, 4):
        t = wx.gather_tile_rows(m)
        assert t > 0 and t % (4 * 64) == 0  # whole waves of quads
    for m in (-1, 0, 5, 16):
        assert wx.gather_tile_rows(m) == 0
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_GATHER_BLOCK=128,WX_GATHER_UNROLL=3")
    assert [wx.gather_tile_rows(m) for m in (1, 2, 3, 4)] == [128 * 4 * 3] * 4
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_GATHER_BLOCK=100")
    assert wx.gather_tile_rows(1) == 0  # not whole waves
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_GATHER_UNROLL=9")
    assert wx.gather_tile_rows(1) == 0


EXPRS = ["(f[idx] + (float)i[idx])", "(float)d[idx]", "((float)key[idx] * 2.0f)", "(f[idx] * f[idx])"]


@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_prepare_gather_compiles_every_column_type(m):
    t = table(f="f32", i="i32", d="f64", key="i64", note="str")
    wx.prepare_gather(t, EXPRS[:m], no_custom())


def test_prepare_gather_with_custom_function():
    t = table(price="f32", quantity="i32")
    wx.prepare_gather(t, ["price[idx]", "discount(price[idx], 0.9f)", "(price[idx] * quantity[idx])"],
                      wx.make_launch(custom_src=DISCOUNT_SRC))


def test_prepare_gather_other_geometry_and_constant(monkeypatch):
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_GATHER_BLOCK=64,WX_GATHER_UNROLL=1")
    t = table(price="f32", quantity="f32")
    wx.prepare_gather(t, ["price[idx]", "quantity[idx]"], no_custom())
    wx.prepare_gather(t, ["0.0f"], no_custom())  # no column at all: the rows-only launch of wx_select_ordered


def test_compile_error_is_reported():
    t = table(price="f32")
    with pytest.raises(wx.WarpExecError) as ei:
        wx.prepare_gather(t, ["price[idx]", "invalid@"], no_custom())
    assert ei.value.status == wx.WX_ERR_COMPILE


def _gather(t, exprs, idx_bytes=8, count=16, d_rows=1 << 30):
    # device pointers are never dereferenced: every case fails its argument check first
    return wx.gather_multi(t, exprs, d_rows, idx_bytes, count, no_custom(), [1 << 31] * len(exprs))


def test_gather_argument_checks_need_no_device():
    t = table(price="f32", quantity="f32")
    for exprs in ([], ["price[idx]"] * 5):
        with pytest.raises(wx.WarpExecError, match="n_exprs") as ei:
            _gather(t, exprs)
        assert ei.value.status == wx.WX_ERR_INVALID
        with pytest.raises(wx.WarpExecError, match="n_exprs") as ei:
            wx.prepare_gather(t, exprs, no_custom())
        assert ei.value.status == wx.WX_ERR_INVALID
    for exprs in (["price[idx]", "  "], [" "], ["price[idx]", None, "quantity[idx]"]):
        with pytest.raises(wx.WarpExecError, match="Empty query expression") as ei:
            _gather(t, exprs)
        assert ei.value.status == wx.WX_ERR_INVALID
        with pytest.raises(wx.WarpExecError, match="Empty query expression") as ei:
            wx.prepare_gather(t, exprs, no_custom())
        assert ei.value.status == wx.WX_ERR_INVALID
    for idx_bytes in (0, 2, 16):
        with pytest.raises(wx.WarpExecError, match="idx_bytes") as ei:
            _gather(t, ["price[idx]"], idx_bytes=idx_bytes)
        assert ei.value.status == wx.WX_ERR_INVALID
    with pytest.raises(wx.WarpExecError, match="negative") as ei:
        _gather(t, ["price[idx]"], count=-1)
    assert ei.value.status == wx.WX_ERR_INVALID
    with pytest.raises(wx.WarpExecError, match="null row id") as ei:
        _gather(t, ["price[idx]"], d_rows=0)
    assert ei.value.status == wx.WX_ERR_INVALID


def _ordered(t, exprs, order="price[idx]", limit=5, capacity=64):
    return wx.select_ordered(t, exprs, None, order, True, limit, no_custom(), [1 << 31] * len(exprs),
                             d_out_keys=1 << 30, d_out_rows=1 << 29, capacity=capacity)


def test_select_ordered_argument_checks_need_no_device():
    t = table(price="f32", quantity="f32")
    with pytest.raises(wx.WarpExecError, match="n_exprs") as ei:
        _ordered(t, ["price[idx]"] * 17)
    assert ei.value.status == wx.WX_ERR_INVALID
    for exprs in (["price[idx]", "  "], [" "], ["price[idx]", None]):
        with pytest.raises(wx.WarpExecError, match="Empty query expression") as ei:
            _ordered(t, exprs)
        assert ei.value.status == wx.WX_ERR_INVALID
    for order in (None, "", "  \t"):
        for exprs in ([], ["price[idx]"]):
            with pytest.raises(wx.WarpExecError, match="Empty ORDER BY expression") as ei:
                _ordered(t, exprs, order=order)
            assert ei.value.status == wx.WX_ERR_INVALID
    with pytest.raises(wx.WarpExecError, match="capacity") as ei:
        _ordered(t, ["price[idx]"], capacity=-1)
    assert ei.value.status == wx.WX_ERR_INVALID


def test_pywarpdb_methods_exist():
    from warpdb_amd import pywarpdb as pw

    for name in ("query_select_ordered", "query_rows", "query_sql_ordered", "query_arrow_select_ordered"):
        assert hasattr(pw.WarpDB, name)
