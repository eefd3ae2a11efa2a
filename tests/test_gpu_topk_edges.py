"""GPU top-K edge tests: wx_topk against the CPU oracle where the scan's
carried bound does its work.

At the default geometry (one workgroup per 8 192 rows up to two per CU) a
table of a few million rows gives every workgroup at most one batch, so the
fast reject against the lane's own worst key, the bound T carried from batch
to batch, the grid-wide slots' re-read every 8th batch and the finalize's slot
reset never run.  Here the diagnostic defines WX_UNROLL=1,WX_TOPK_GRID=2 shrink
the geometry: a batch is 1 024 rows and two workgroups split the table, so a
42 003-row table gives each of them 21 batches, the last one ragged and ending
in a partial quad.  Every test asserts the regime it claims from wx_topk_plan
(batches, seed pass on or off) and fails when the plan says otherwise.

Every case compares with ora.topk on the same host arrays (pinned against
numpy by tests/test_topk_oracle.py): the count, the row indices, and the keys
and values bit for bit.  There is no tolerance: the operation has none.
The cost of a case is its hiprtc compile, so the parameters are what changes
the module (K, direction, WHERE, alignment, defines) and the data layouts loop
inside.
"""
from __future__ import annotations

import numpy as np
import pytest

import oracle_lib as ora
import synth
import topk_layouts as tl
from test_gpu_parity import bits, dev_table, launch

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from warpdb_amd import _warpexec as wx  # noqa: E402

SEEDED = tl.SHRUNK + ",WX_TOPK_SEED=2"
KEY_FILL, IDX_FILL = 0x7FC0BEEF, -7  # what the outputs hold before a call (a NaN with a payload)


def regime(monkeypatch, defines, n, k, batches=17, seeded=False):
    """Set the define list and assert what wx_topk_plan then says of the run."""
    if defines is None:
        monkeypatch.delenv("WARPDB_EXTRA_DEFINES", raising=False)
    else:
        monkeypatch.setenv("WARPDB_EXTRA_DEFINES", defines)
    p = wx.topk_plan(n, k, launch=launch())
    assert p.max_batches >= batches, (p.grid, p.span_rows, p.max_batches)
    if batches > 1:
        assert p.grid == tl.GRID and p.span_rows == tl.SPAN
    assert (p.seed_grid > 0) == seeded, p.seed_grid
    return p


def run(cols, k, desc, where=False, order=("price[idx]", "price"), select=None, row_base=0, offset=0, table=None,
        flags=wx.F_SYNC, want=(True, True, True)):
    """One wx_topk call against ora.topk; returns the oracle's (keys, rows)."""
    if table is None:
        table, _ = dev_table(cols, offset=offset)
    keys = torch.full((k,), KEY_FILL, dtype=torch.int32, device="cuda").view(torch.float32)
    idx = torch.full((k,), IDX_FILL, dtype=torch.int64, device="cuda")
    vals = torch.full((k,), KEY_FILL, dtype=torch.int32, device="cuda").view(torch.float32)
    cond, ocond = (tl.COND, tl.OCOND) if where else (None, None)
    ptrs = [t.data_ptr() if w else 0 for t, w in zip((keys, idx, vals), want)]
    if flags & wx.F_SYNC:
        m = wx.topk(table, order[0], cond, select[0] if select else None, k, desc, launch(flags), *ptrs,
                    row_base=row_base)
    else:  # asynchronous: the count through device memory, read after the stream has drained
        d_count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        assert wx.topk(table, order[0], cond, select[0] if select else None, k, desc, launch(flags), *ptrs,
                       row_base=row_base, d_count=d_count.data_ptr(), want_count=False) is None
        torch.cuda.current_stream().synchronize()
        m = int(d_count.item())
    rk, ri, rv = ora.topk(ora.HostTable(cols), order[1], k, desc, cond=ocond, select_expr=select[1] if select else None)
    assert m == len(ri)
    keys, idx, vals = keys.cpu().numpy(), idx.cpu().numpy(), vals.cpu().numpy()
    for got, ref, wanted, fill in ((bits(keys), bits(rk), want[0], KEY_FILL), (idx, ri + row_base, want[1], IDX_FILL),
                                   (bits(vals), bits(rv), want[2], KEY_FILL)):
        mm = m if wanted else 0
        assert np.array_equal(got[:mm], ref[:mm])
        assert (got[mm:] == fill).all()  # nothing written past the count, or to an output not asked for
    return rk, ri


# ------------------------------------------- a. K regimes over many batches
@pytest.mark.parametrize("where", [False, True], ids=["all", "where"])
@pytest.mark.parametrize("desc", [True, False], ids=["desc", "asc"])
@pytest.mark.parametrize("k", [1, 2, 8, 9, 16, 17, 32])
def test_k_regimes_many_batches(k, desc, where, monkeypatch):
    n = tl.N
    regime(monkeypatch, tl.SHRUNK, n, k)
    for name, make in tl.LAYOUTS.items():
        price = make(n, k, desc)
        # the tie layouts are about unfiltered rows: a WHERE would drop copies of the K-th best value
        qty = np.full(n, 99.0, np.float32) if where and name.startswith("tie_bound") else None
        try:
            rk, ri = run(tl.table(price, qty), k, desc, where)
        except AssertionError as e:
            raise AssertionError(f"layout {name}: {e}") from e
        # (unseeded, a bound reaches a wave only from rows scanned before, of smaller index unless the
        # workgroups race; test_seed_pass_many_batches runs the tie layouts with the bound known from batch 0)
        if name == "tie_bound_first_span":
            assert ri[k - 1] == 17
        if name == "tie_bound_other_workgroup":
            assert ri[k - 1] == tl.SPAN + 17
        if name == "all_equal" and not where:
            assert np.array_equal(ri, np.arange(k))
    if where:  # exactly 0, 1, K - 1 and K passing rows: the module is the same, the count the oracle's
        price = tl.uniform(n, k, desc)
        for m in sorted({0, 1, k - 1, k}):
            _, ri = run(tl.table(price, tl.pass_exactly(n, m)), k, desc, True)
            assert len(ri) == m


# ------------------------------------- b. span edges at the default geometry
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("desc", [True, False], ids=["desc", "asc"])
@pytest.mark.parametrize("k", [5, 12, 32])
def test_span_edges_default_geometry(k, desc, offset, monkeypatch):
    s = regime(monkeypatch, None, 1 << 20, k, batches=1).span_rows
    assert s == 8192
    for n in (0, 1, 3, 4, 5, s - 1, s, s + 1, 2 * s - 3, 2 * s + 4):
        price = (np.round(tl.uniform(n, k, desc) * 4.0) / 4.0).astype(np.float32)  # 160 values: ties everywhere
        if n > 8:
            price[[n - 1, n - 5]] = tl.good([3, 3], desc)  # winners in the last quads, tied
        _, ri = run(tl.table(price), k, desc, offset=offset)  # n = 0: count 0, no output touched (run checks)
        assert len(ri) == min(k, n)


# --------------------------------------------- c. state carried between calls
def _tables():
    hi = tl.table(synth.uniform_f32(tl.N, 51, 100.0, 200.0))
    lo = tl.table(synth.uniform_f32(tl.N, 52, 0.0, 1.0))
    return (hi, dev_table(hi)[0]), (lo, dev_table(lo)[0])


@pytest.mark.parametrize("flags", [wx.F_SYNC, 0], ids=["sync", "async"])
def test_bound_state_between_calls(flags, monkeypatch):
    # One stream, one workspace: the 64 bound slots a query leaves behind are
    # the next query's starting bound.  A rank left from the [100, 200] table
    # would turn away every row of the [0, 1] table (DESC), and a DESC rank
    # read as an ASC one is a bound no row meets.
    n = tl.N
    (hi, hi_dev), (lo, lo_dev) = _tables()
    regime(monkeypatch, tl.SHRUNK, n, 5)
    run(hi, 5, True, table=hi_dev, flags=flags)    # 1
    run(hi, 5, False, table=hi_dev, flags=flags)   # 2
    run(hi, 32, True, table=hi_dev, flags=flags)   # 3
    run(lo, 5, True, table=lo_dev, flags=flags)    # 4: every key below the previous queries' bounds
    run(lo, 5, False, table=lo_dev, flags=flags)
    run(hi, 5, False, table=hi_dev, flags=flags)   # and above an ascending query's
    # 5: calls the host refuses before any launch leave the state as it was
    with pytest.raises(wx.WarpExecError) as e:
        wx.topk(hi_dev, "price[idx]", None, None, 33, True, launch())
    assert e.value.status == wx.WX_ERR_UNSUPPORTED
    with pytest.raises(wx.WarpExecError) as e:
        wx.topk(hi_dev, "invalid@", None, None, 5, True, launch())
    assert e.value.status == wx.WX_ERR_COMPILE
    run(lo, 5, True, table=lo_dev, flags=flags)
    # 6: a seeded query (slot 0 raised before the scan), then an unseeded one
    regime(monkeypatch, SEEDED, n, 5, seeded=True)
    run(hi, 5, True, table=hi_dev, flags=flags)
    run(hi, 17, False, table=hi_dev, flags=flags)
    regime(monkeypatch, tl.SHRUNK, n, 5)
    run(lo, 5, True, table=lo_dev, flags=flags)
    run(lo, 5, False, table=lo_dev, flags=flags)


# ------------------------------------------- d. seed pass under many batches
@pytest.mark.parametrize("desc", [True, False], ids=["desc", "asc"])
@pytest.mark.parametrize("k", [5, 17])
def test_seed_pass_many_batches(k, desc, monkeypatch):
    n = tl.N
    regime(monkeypatch, SEEDED, n, k, seeded=True)
    # the seed's bound is known from batch 0 on and comes from rows all over the table: a row that
    # ties with it and has a smaller index than the rows it came from must still win (the tie layouts)
    for name in ("all_equal", "late_winners", "sentinel", "specials", "nan_but_k_minus_1", "uniform",
                 "tie_bound_first_span", "tie_bound_other_workgroup"):
        try:
            _, ri = run(tl.table(tl.LAYOUTS[name](n, k, desc)), k, desc)
        except AssertionError as e:
            raise AssertionError(f"layout {name}: {e}") from e
        if name.startswith("tie_bound"):
            assert ri[k - 1] == (17 if name == "tie_bound_first_span" else tl.SPAN + 17)
    # more spans than seed workgroups: the seed samples every other span, the winners sit in the rest
    n = 300_003
    p = regime(monkeypatch, SEEDED, n, k, seeded=True)
    assert p.seed_stride_rows >= 2 * p.span_rows
    run(tl.table(tl.seed_miss(n, k, desc, p.span_rows, p.seed_grid, p.seed_stride_rows)), k, desc)


# ----------------------------------------------------- e. typed ORDER BY keys
@pytest.mark.parametrize("desc", [True, False], ids=["desc", "asc"])
@pytest.mark.parametrize("col", ["a", "d", "c"], ids=["int32", "int64", "float64"])
def test_typed_order_keys(col, desc, monkeypatch):
    # the key is static_cast<float>(column): distinct integers collide above
    # 2^24 and the row index decides; doubles beyond FLT_MAX become infinities
    n = tl.N
    regime(monkeypatch, tl.SHRUNK, n, 5)
    cols = dict(tl.typed_columns(n), quantity=tl.quantity(n))
    run(cols, 5, desc, order=(f"{col}[idx]", col))
    run(cols, 5, desc, where=True, order=(f"{col}[idx]", col))


# ------------------------------------------------------------------ f. outputs
@pytest.mark.parametrize("desc", [True, False], ids=["desc", "asc"])
def test_outputs_row_base_select_and_nulls(desc, monkeypatch):
    n = tl.N
    regime(monkeypatch, tl.SHRUNK, n, 5)
    cols = tl.table(tl.late_winners(n, 5, desc))
    table, _ = dev_table(cols)
    select = ("discount(price[idx], 0.9f)", "discount(price, 0.9)")
    run(cols, 5, desc, table=table, select=select, row_base=1 << 33)
    for want in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        run(cols, 5, desc, table=table, select=select, row_base=1 << 33, want=want)
    run(cols, 5, desc, table=table, want=(True, True, True))  # no SELECT expression: the values are the keys


# ---------------------------------------------------------- g. ordered SELECT
@pytest.mark.parametrize("desc", [True, False], ids=["desc", "asc"])
@pytest.mark.parametrize("limit", [5, 32])
def test_ordered_select_routes_agree_many_batches(limit, desc, monkeypatch):
    # wx_select_ordered's top-K route (limit <= 32) runs this scan: under the
    # shrunken geometry it must equal the sort route, rows and bits
    n = tl.N
    regime(monkeypatch, tl.SHRUNK, n, limit)
    exprs = ["(price[idx] * quantity[idx])", "discount(price[idx], 0.9f)"]
    for name in ("all_equal", "specials"):
        cols = tl.table(tl.LAYOUTS[name](n, limit, desc))
        table, _ = dev_table(cols)
        got = {}
        for route in ("auto", "sort"):
            monkeypatch.setenv("WARPDB_ORDERED_ROUTE", route)
            vals = [torch.full((limit,), KEY_FILL, dtype=torch.int32, device="cuda").view(torch.float32)
                    for _ in exprs]
            keys = torch.full((limit,), KEY_FILL, dtype=torch.int32, device="cuda").view(torch.float32)
            rows = torch.full((limit,), IDX_FILL, dtype=torch.int64, device="cuda")
            m = wx.select_ordered(table, exprs, tl.COND, "price[idx]", desc, limit, launch(),
                                  [v.data_ptr() for v in vals], keys.data_ptr(), rows.data_ptr(), limit)
            got[route] = (m, rows.cpu().numpy(), bits(keys.cpu().numpy()), [bits(v.cpu().numpy()) for v in vals])
        monkeypatch.delenv("WARPDB_ORDERED_ROUTE")
        (m, rows, keys, vals), (sm, srows, skeys, svals) = got["auto"], got["sort"]
        rk, ri, _ = ora.topk(ora.HostTable(cols), "price", limit, desc, cond=tl.OCOND)
        assert m == sm == len(ri) == limit, name
        assert np.array_equal(rows, ri) and np.array_equal(srows, ri), name
        assert np.array_equal(keys, bits(rk)) and np.array_equal(skeys, bits(rk)), name
        for j, (a, b) in enumerate(zip(vals, svals)):
            assert np.array_equal(a, b), (name, j)
        rv0 = ora.project_filter(ora.HostTable(cols), "price * quantity", None)[0][ri]
        assert np.array_equal(vals[0], bits(rv0)), name
