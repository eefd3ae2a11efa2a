"""CPU tests that pin what the top-K GPU tests compare against.

ora.topk (oracle/warpdb_oracle.c, a streaming insertion) is checked against
an independent numpy statement of the same total order -- one np.lexsort over
(row, rank, is-NaN): NaN last in both directions, -0.0 == +0.0, ties by
ascending row, the first K of the passing rows -- on every layout
tests/test_gpu_topk_edges.py uses, at its sizes.  "Equal to the oracle" there
then means "correct".

wx_topk_plan, from which those GPU tests assert the regime they run in, is
checked against hand-computed launch plans.  No device is needed.
"""
from __future__ import annotations

import numpy as np
import pytest

import oracle_lib as ora
import topk_layouts as tl
from warpdb_amd import _warpexec as wx

KS = (1, 8, 17, 32)


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def check(cols, order, k, desc, where):
    with np.errstate(over="ignore"):
        key = cols[order].astype(np.float32)
    passing = cols["quantity"] > 50 if where else None
    rk, ri, _ = ora.topk(ora.HostTable(cols), order, k, desc, cond=tl.OCOND if where else None)
    nk, ni = tl.numpy_topk(key, k, desc, passing)
    assert len(ri) == len(ni) == min(k, len(key) if passing is None else int(passing.sum()))
    assert np.array_equal(ri, ni)
    assert np.array_equal(bits(rk), bits(nk))
    return ri


@pytest.mark.parametrize("desc", [True, False])
@pytest.mark.parametrize("layout", sorted(tl.LAYOUTS))
def test_oracle_topk_is_the_lexsort_order(layout, desc):
    for k in KS:
        cols = tl.table(tl.LAYOUTS[layout](tl.N, k, desc))
        for where in (False, True):
            check(cols, "price", k, desc, where)


@pytest.mark.parametrize("desc", [True, False])
def test_layouts_hold_what_they_claim(desc):
    # the layouts' own claims, from the numpy order: where the winners sit
    n = tl.N
    for k in KS:
        _, ri = tl.numpy_topk(tl.all_equal(n, k, desc), k, desc)
        assert np.array_equal(ri, np.arange(k))
        _, ri = tl.numpy_topk(tl.late_winners(n, k, desc), k, desc)
        assert set(ri) == set(tl.late_rows(n, k)) and n - 1 in ri and n % 4 != 0  # row n - 1: in a partial quad
        for f in (tl.one_thread_improving, tl.one_thread_worsening):
            _, ri = tl.numpy_topk(f(n, k, desc), k, desc)
            assert set(ri) == set(tl.one_thread_rows(k))
            # one thread's quads: the same lane of the same workgroup in every batch
            assert len({(r // 4) % 256 for r in ri}) == 1 and len({(r // tl.SPAN) % tl.GRID for r in ri}) == 1
        for s0, f in ((0, tl.tie_bound_first_span), (1, tl.tie_bound_other_workgroup)):
            p = f(n, k, desc)
            nk, ri = tl.numpy_topk(p, k, desc)
            assert ri[k - 1] == s0 * tl.SPAN + 17  # the first copy of the K-th best value
            assert int((p == nk[k - 1]).sum()) == len(tl.tie_rows(n, s0)) >= 41
        p = tl.sentinel(n, k, desc)
        worst = np.float32("-inf") if desc else np.float32("inf")
        assert int(np.isfinite(p).sum()) < k and int((p == worst).sum()) > k
        nk, ri = tl.numpy_topk(p, k, desc)
        held = ri[nk == worst]
        assert len(held) >= 1 and np.array_equal(held, np.flatnonzero(p == worst)[:len(held)])
        nk, _ = tl.numpy_topk(tl.nan_but_k_minus_1(n, k, desc), k, desc)
        assert int(np.isnan(nk).sum()) == 1 and np.isnan(nk[k - 1])


@pytest.mark.parametrize("desc", [True, False])
def test_oracle_topk_pass_counts(desc):
    # exactly 0, 1, K - 1 and K passing rows: the count is the passing rows'
    for k in KS:
        price = tl.uniform(tl.N, k, desc)
        for m in sorted({0, 1, k - 1, k}):
            ri = check(tl.table(price, tl.pass_exactly(tl.N, m)), "price", k, desc, True)
            assert len(ri) == m


@pytest.mark.parametrize("desc", [True, False])
def test_oracle_topk_seed_miss_layout(desc):
    n, span, seed_grid, seed_stride = 300_003, 1024, 128, 2048
    for k in (5, 17):
        p = tl.seed_miss(n, k, desc, span, seed_grid, seed_stride)
        ri = check(tl.table(p), "price", k, desc, False)
        assert all((r % seed_stride) >= span or r // seed_stride >= seed_grid for r in ri)


@pytest.mark.parametrize("desc", [True, False])
@pytest.mark.parametrize("col", ["a", "d", "c"])
def test_oracle_topk_typed_keys(col, desc):
    # the key is the column cast to float: distinct values collide, the row decides
    cols = dict(tl.typed_columns(tl.N), quantity=tl.quantity(tl.N))
    ri = check(cols, col, 5, desc, False)
    with np.errstate(over="ignore"):
        key = cols[col].astype(np.float32)
    assert len(np.unique(key)) < len(np.unique(cols[col]))  # column values collide as float keys
    assert len(np.unique(key[ri])) < len(ri)                # and the winners tie: the row index decided


# ------------------------------------------------------------- wx_topk_plan
def plan(n, k, cus):
    p = wx.topk_plan(n, k, cus)
    return p.grid, p.span_rows, p.max_batches, p.seed_grid, p.seed_stride_rows


def test_topk_plan_symbol():
    assert hasattr(wx.load(), "wx_topk_plan") and "wx_topk_plan" in wx.EXPORTED_SYMBOLS


def test_topk_plan_default_geometry(monkeypatch):
    monkeypatch.delenv("WARPDB_EXTRA_DEFINES", raising=False)
    # 256 CUs: at most 512 workgroups, spans of 256 threads x 8 quads x 4 rows
    assert plan(0, 5, 256) == (1, 8192, 0, 0, 0)
    assert plan(1, 5, 256) == (1, 8192, 1, 0, 0)
    # 42 003 rows = 10 501 quads: 42 workgroups of 256 quads each would do, one span holds them twice over
    assert plan(42_003, 5, 256) == (42, 8192, 1, 0, 0)
    # 1 000 003 rows = 250 001 quads = 123 spans (122 whole): 512 workgroups, 389 of them idle
    assert plan(1_000_003, 5, 256) == (512, 8192, 1, 0, 0)
    # 2^24 rows = 2 048 spans over 512 workgroups: 4 batches; the seed pass from K = 5 on,
    # 128 workgroups every 16th span
    assert plan(1 << 24, 5, 256) == (512, 8192, 4, 128, 16 * 8192)
    assert plan(1 << 24, 32, 256) == (512, 8192, 4, 128, 16 * 8192)
    assert plan(1 << 24, 4, 256) == (512, 8192, 4, 0, 0)
    assert plan((1 << 24) - 1, 5, 256) == (512, 8192, 4, 0, 0)
    # fewer CUs: the grid follows, the batches grow
    assert plan(1 << 24, 5, 64) == (128, 8192, 16, 128, 16 * 8192)
    # 2^32 + 5 rows: 524 289 span positions over 512 workgroups
    assert plan((1 << 32) + 5, 32, 256) == (512, 8192, 1025, 128, 4096 * 8192)


def test_topk_plan_follows_the_define_list(monkeypatch):
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", tl.SHRUNK)
    # 10 501 quads in spans of 256: 42 positions (the last 5 quads, the very last 3 rows), 21 per workgroup
    assert plan(tl.N, 5, 256) == plan(tl.N, 32, 8) == (2, 1024, 21, 0, 0)
    assert plan(0, 5, 256) == (1, 1024, 0, 0, 0)
    assert plan(1024, 5, 256) == (1, 1024, 1, 0, 0)  # the cap is a cap: one workgroup's worth of quads
    assert plan(1025, 5, 256) == (2, 1024, 1, 0, 0)
    assert plan(3 * 1024 + 1, 5, 256) == (2, 1024, 2, 0, 0)
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_UNROLL=1,WX_TOPK_GRID=2,WX_TOPK_SEED=2")
    # 41 whole spans: a seed workgroup for each, one span apart
    assert plan(tl.N, 5, 256) == plan(tl.N, 1, 256) == (2, 1024, 21, 41, 1024)
    # 292 whole spans: 128 seed workgroups two spans apart; 293 positions over two workgroups
    assert plan(300_003, 17, 256) == (2, 1024, 147, 128, 2048)
    assert plan(2044, 5, 256) == (2, 1024, 1, 0, 0)  # 511 quads, under two whole spans: no seed pass
    assert plan(2045, 5, 256) == (2, 1024, 1, 2, 1024)  # 512 quads
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_UNROLL=1")  # without the cap: 42 workgroups, one batch each
    assert plan(tl.N, 5, 256) == (42, 1024, 1, 0, 0)
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_TOPK_GRID=1000")  # a cap above the grid changes nothing
    assert plan(1 << 24, 5, 256) == (512, 8192, 4, 128, 16 * 8192)
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_TOPK_GRID=0")
    assert plan(1 << 24, 5, 256) == (512, 8192, 4, 128, 16 * 8192)
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_TOPK_SEED=0")
    assert plan(1 << 24, 5, 256) == (512, 8192, 4, 0, 0)
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_TOPK_SEED_MINK=9")
    assert plan(1 << 24, 8, 256)[3] == 0 and plan(1 << 24, 9, 256)[3] == 128


def test_topk_plan_refuses_bad_arguments(monkeypatch):
    monkeypatch.delenv("WARPDB_EXTRA_DEFINES", raising=False)
    for n, k in ((-1, 5), (10, 0), (10, 33)):
        with pytest.raises(wx.WarpExecError):
            wx.topk_plan(n, k, 256)
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_UNROLL=0")
    with pytest.raises(wx.WarpExecError):
        wx.topk_plan(10, 5, 256)
