"""CPU tests of the LDS-window GROUP BY's launch geometry and of the layouts
its GPU tests run.

A streaming workgroup of wx_group_sum, wx_group_multi or wx_join_group runs
one batch (a span of block * WX_UNROLL row quads) until a table holds more
spans than the grid holds workgroups: 16 waves per CU, 512 workgroups of 512
threads on 256 CUs, above 2 097 152 rows.  No test table is that large, so the
second trip through the stride loop, the lead state carried from one batch to
the next and the LDS bins gathered over several batches ran at benchmark sizes
only.  The diagnostic define WX_GROUP_GRID caps the grid instead;
wx_group_window_geometry states what a call then launches, with the
arithmetic of the run path (group_window_plan, group_window.cpp), and needs no
device.

Here: that call against the geometry worked by hand at 256 CUs and at 1, its
error returns, wx_group_hash_slot against the numpy formula, the row
placement against a case worked by hand, every layout's own claim -- "this
wave has exactly 15 lanes on the first lane's bin", "this key's bin is one past
the window", "these 300 keys share a home slot" -- at cus = 256 under the
defines the GPU tests use (tests/test_gpu_group_window_edges.py), and the
numpy reference of those tests against the oracle.
"""
from __future__ import annotations

import numpy as np
import pytest

import gw_layouts as gw
import oracle_lib as ora
from warpdb_amd import _warpexec as wx

CUS = 256
# family -> (threads per workgroup, workgroups per CU), by hand from the LDS each build needs
BY_HAND = {"group_sum": (512, 2), "group_agg": (512, 2), "sum2": (512, 2), "mix3": (512, 2), "all4": (1024, 1),
           "join_hash": (512, 2), "join_direct": (512, 2)}


def geometry(monkeypatch, defines, n, family="group_sum", cus=CUS):
    if defines is None:
        monkeypatch.delenv("WARPDB_EXTRA_DEFINES", raising=False)
    else:
        monkeypatch.setenv("WARPDB_EXTRA_DEFINES", defines)
    fam, ns, nq, form = gw.FAMILIES[family]
    return wx.group_window_geometry(n, ns, nq, fam, form, cus)


def test_symbols():
    lib = wx.load()
    for name in ("wx_group_window_geometry", "wx_group_table_slots", "wx_group_hash_slot"):
        assert hasattr(lib, name) and name in wx.EXPORTED_SYMBOLS
    assert (wx.GW_GROUP_SUM, wx.GW_GROUP_MULTI, wx.GW_JOIN_GROUP) == (gw.SUM, gw.MULTI, gw.JOIN)


def test_default_geometry_runs_one_batch_per_workgroup(monkeypatch):
    # the regression fact: what the other GROUP BY tests run never takes the stride loop's second trip
    for family, sizes in (("group_sum", (0, 1, 63, 4097, 300_001, 2_000_003)), ("mix3", (4097, 300_001)),
                          ("all4", (4097, 300_001)), ("join_hash", (300_001,)), ("join_direct", (300_001,))):
        for n in sizes:
            g = geometry(monkeypatch, None, n, family)
            assert g.max_batches == (1 if n else 0), (family, n)
    g = geometry(monkeypatch, None, 2_000_003)
    assert (g.block_threads, g.span_rows, g.grid) == (512, 4096, 512)      # 489 spans on 512 workgroups
    g = geometry(monkeypatch, None, 300_001)
    assert (g.grid, g.max_batches) == (147, 1)                            # 74 spans: every other workgroup idle
    assert geometry(monkeypatch, None, 512 * 4096).max_batches == 1
    assert geometry(monkeypatch, None, 512 * 4096 + 1).max_batches == 2
    g = geometry(monkeypatch, None, 10 ** 9)                              # the benchmark's table
    assert (g.grid, g.max_batches) == (512, 477)
    g = geometry(monkeypatch, None, 10 ** 9, "all4")
    assert (g.block_threads, g.span_rows, g.grid, g.max_batches) == (1024, 8192, 256, 477)
    assert (g.window_keys, g.hsort_max) == (gw.WINDOW, gw.HSORT_MAX) == (wx.GROUP_WINDOW_BINS, 4096)


@pytest.mark.parametrize("family", list(gw.FAMILIES))
def test_geometry_by_hand(family, monkeypatch):
    block, per_cu = BY_HAND[family]
    for cap in (None, 1, 3, 1000):
        defines = None if cap is None else f"WX_GROUP_GRID={cap}"
        for cus in (CUS, 1, 104):
            for n in (0, 1, 3, 4, 5, 4 * block - 1, 4 * block, 4 * block + 1, 8 * block, 8 * block + 1, 24 * block,
                      72 * block + 5, 80 * block - 3, 300_001, 2_000_003, 10 ** 9, 2 ** 31 + 11):
                g = geometry(monkeypatch, defines, n, family, cus)
                want = gw.manual_geometry(n, block, cus, per_cu, cap)
                got = (g.block_threads, g.span_rows, g.grid, g.max_batches)
                assert got == (want.block_threads, want.span_rows, want.grid, want.max_batches), (cap, cus, n)
                assert g.grid * g.max_batches * g.span_rows >= n
                assert (g.window_keys, g.hsort_max) == (gw.WINDOW, gw.HSORT_MAX)
                assert g.lead == (gw.LEAD if gw.FAMILIES[family][2] == 0 else 0)   # sum-only builds alone


def test_grid_cap_changes_the_grid_alone(monkeypatch):
    for family in gw.FAMILIES:
        S = geometry(monkeypatch, None, 1, family).span_rows
        n = 9 * S + 5
        base, g = geometry(monkeypatch, None, n, family), geometry(monkeypatch, gw.GRID3, n, family)
        assert base.grid == 19 and base.max_batches == 1
        assert (g.grid, g.max_batches) == (3, 4)                # ten spans: workgroup 0 runs a fourth
        for f, _ in g._fields_:
            if f not in ("grid", "max_batches"):
                assert getattr(g, f) == getattr(base, f), f
        assert geometry(monkeypatch, gw.GRID1, n, family).max_batches == 10
        assert geometry(monkeypatch, gw.GRID3, n, family, cus=1).grid == 2 // (S // 4096)    # fewer than the cap
        # the steady-state sizes: the batches the GPU tests claim
        sizes = gw.steady_sizes(g)
        assert sizes == [S - 1, S, S + 1, 3 * S, 9 * S + 5, 10 * S - 3]
        assert [geometry(monkeypatch, gw.GRID3, m, family).max_batches for m in sizes] == [1, 1, 1, 1, 4, 4]
        assert [geometry(monkeypatch, gw.GRID3, m, family).grid for m in sizes] == [2, 2, 3, 3, 3, 3]
    # other defines of the list are not mistaken for it; the unroll moves the span, the lead its threshold
    g = geometry(monkeypatch, "WX_GP_GRID=2,WX_GROUP_GRID=3,WX_UNROLL=4,WX_GROUP_LEAD=8", 9 * 4096 + 5)
    assert (g.grid, g.span_rows, g.max_batches, g.lead) == (3, 8192, 2, 8)


def test_geometry_refuses(monkeypatch):
    def status(defines=None, n=1000, ns=1, nq=0, fam=gw.SUM, form=0, cus=CUS):
        if defines is None:
            monkeypatch.delenv("WARPDB_EXTRA_DEFINES", raising=False)
        else:
            monkeypatch.setenv("WARPDB_EXTRA_DEFINES", defines)
        with pytest.raises(wx.WarpExecError) as e:
            wx.group_window_geometry(n, ns, nq, fam, form, cus)
        return e.value.status

    for bad in ("WX_GROUP_GRID=0", "WX_GROUP_GRID=-3", "WX_GROUP_GRID=x", "WX_GROUP_GRID=", "WX_GROUP_GRID=3,WX_UNROLL=0"):
        assert status(bad) == wx.WX_ERR_INVALID, bad
    for ok in ("WX_GROUP_GRID=1", "WX_GROUP_GRID=100000", "WX_GROUP_GRIDS=0"):
        monkeypatch.setenv("WARPDB_EXTRA_DEFINES", ok)
        wx.group_window_geometry(1000, 1, 0, gw.SUM, 0, CUS)
    assert status(n=-1) == wx.WX_ERR_INVALID
    assert status(fam=3) == wx.WX_ERR_INVALID and status(fam=-1) == wx.WX_ERR_INVALID
    assert status(ns=2) == wx.WX_ERR_INVALID and status(nq=2) == wx.WX_ERR_INVALID      # wx_group_sum: one value
    assert status(ns=0, nq=0, fam=gw.MULTI) == wx.WX_ERR_INVALID and status(ns=5, fam=gw.MULTI) == wx.WX_ERR_INVALID
    assert status(ns=1, fam=gw.JOIN, form=2) == wx.WX_ERR_INVALID


def test_hash_slot_is_the_numpy_formula():
    rng = np.random.default_rng(3)
    keys = np.concatenate([rng.integers(gw.I32_MIN, gw.I32_MAX + 1, 500), [0, -1, 1, gw.I32_MIN, gw.I32_MAX]])
    for slots in (1, 2, 4096, 8192, 1 << 21, 1 << 30):
        want = gw.hash_slot(keys, slots)
        assert [wx.group_hash_slot(int(k), slots) for k in keys] == want.tolist()
        assert want.min() >= 0 and want.max() < slots
    assert wx.group_hash_slot(7, 4096) == (7 * 2654435761) % 4096 and wx.group_hash_slot(0, 4096) == 0
    for bad in (0, -4096, 3, 4097, (1 << 30) + 1, 1 << 31):
        assert wx.group_hash_slot(7, bad) == -1


def test_place_by_hand():
    # 2 workgroups of 64 threads, 2 quads per thread: a span is 128 quads = 512 rows
    g = gw.manual_geometry(2000, 64, 1, 2)
    assert (g.grid, g.span_rows, g.max_batches) == (2, 512, 2)
    p = gw.place(g, 2000)
    at = lambda r: (p.wg[r], p.batch[r], p.u[r], p.wave[r], p.lane[r], p.e[r])  # noqa: E731
    assert at(0) == (0, 0, 0, 0, 0, 0) and at(7) == (0, 0, 0, 0, 1, 3)
    assert at(256) == (0, 0, 1, 0, 0, 0)          # the thread's second quad, a block of quads further on
    assert at(512) == (1, 0, 0, 0, 0, 0)          # the next span is the next workgroup's
    assert at(1024 + 4 * 63 + 2) == (0, 1, 0, 0, 63, 2)   # workgroup 0's second batch
    assert at(1999) == (1, 1, 1, 0, 51, 3)
    g = gw.manual_geometry(2000, 128, 1, 1)       # two waves
    p = gw.place(g, 2000)
    assert (p.wave[4 * 64], p.lane[4 * 64], p.u[4 * 128]) == (1, 0, 1)


def test_lead_layout(monkeypatch):
    for family in ("group_sum", "sum2"):
        g = geometry(monkeypatch, gw.GRID3, 9 * 4096 + gw.LEAD_TAIL_ROWS, family)
        lay = gw.lead(g)                  # asserts every case it is named for (check_lead)
        assert lay.n == 9 * 4096 + gw.LEAD_TAIL_ROWS and not lay.passing(True).all()
        # both sides of the window are fed, and exactly one row is dropped by the WHERE
        assert len(lay.general_keys()) == 3 and (lay.flag == 0).sum() == 1
    with pytest.raises(AssertionError):
        gw.lead(geometry(monkeypatch, gw.GRID3, 9 * 4096 + gw.LEAD_TAIL_ROWS, "group_agg"))   # no lead in that build


def test_steady_layouts(monkeypatch):
    for family in gw.FAMILIES:
        S = geometry(monkeypatch, None, 1, family).span_rows
        for n in gw.steady_sizes(geometry(monkeypatch, gw.GRID3, 9 * S, family)):
            gw.check_steady(gw.steady(n), geometry(monkeypatch, gw.GRID3, n, family))


def test_placement_layouts(monkeypatch):
    n = 9 * 4096 + 5
    assert gw.PLACEMENT_LOS == (-2 ** 31, -1024, 2 ** 31 - 2048)
    for lo in gw.PLACEMENT_LOS:
        lay = gw.placement(n, lo)         # asserts its pool (check_placement)
        keys = np.unique(lay.keys)
        assert len(keys) == len(lay.general_keys()) + len(lay.window_keys()) < gw.HSORT_MAX
    with pytest.raises(AssertionError):
        gw.Layout(np.zeros(4), gw.I32_MAX - 2046)     # the window would pass the largest key


def test_finalize_layouts():
    seen = set()
    for nh in gw.FIN_NH:
        for side in gw.FIN_SIDES:
            for nwin in gw.FIN_NWIN:
                lay = gw.finalize(nh, side, nwin)
                gen = lay.general_keys()
                nlo = int((gen < lay.key_lo).sum())
                seen.add((nh, nlo, nwin))
                assert lay.n == 2 * (nh + nwin) + -(-(nh + nwin) // 5)
    assert {(4096, 0, 2048), (4096, 4096, 0), (4097, 2048, 1), (4095, 2047, 2048), (0, 0, 0), (1, 1, 1), (2, 1, 2048)} <= seen
    assert gw.FIN_NH == (0, 1, 2, 4095, 4096, 4097)


def test_table_layouts(monkeypatch):
    g = geometry(monkeypatch, gw.GRID3, 9 * 4096 + 5)
    for slots in (8192, 1 << 21):
        for home in (slots // 2 + 11, slots - 1):
            lay = gw.cluster(g, 9 * 4096 + 5, slots, home)
            gen = lay.general_keys()
            homes = gw.hash_slot(gen, slots)
            assert (homes == home).sum() == gw.CLUSTER and [wx.group_hash_slot(int(k), slots) for k in gen] == homes.tolist()
    assert len(gw.overfull().general_keys()) == 5000


def test_numpy_reference_is_the_oracle(monkeypatch):
    # "equal to gw.exact_groups, bit for bit" in the GPU tests then means "equal to the oracle"
    g = geometry(monkeypatch, gw.GRID3, 9 * 4096 + gw.LEAD_TAIL_ROWS)
    for lay in (gw.lead(g), gw.steady(9 * 4096 + 5), gw.placement(9 * 4096 + 5, gw.I32_MIN), gw.finalize(4097, "split", 2048)):
        cols = lay.cols()
        for expr, vals in (("va", cols["va"]), ("va * vb", cols["va"] * cols["vb"]), ("vc", cols["vc"]), ("vd", cols["vd"])):
            for where in (False, True):
                want = ora.group_agg(ora.HostTable(cols), expr, "k", gw.OCOND if where else None)
                got = gw.exact_groups(cols["k"], vals, lay.passing(where))
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
                assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))
                assert np.array_equal(got[3].view(np.uint32), want[3].view(np.uint32))
                assert np.array_equal(got[4].view(np.uint32), want[4].view(np.uint32))
    # NaN skipped, a group of NaN alone, -0.0 returned as +0.0
    k = np.array([1, 1, 2, 3, 3, 3], np.int32)
    v = np.array([np.nan, 2.0, np.nan, -0.0, np.nan, -0.0], np.float32)
    want = ora.group_agg(ora.HostTable({"k": k, "v": v}), "v", "k")
    got = gw.numpy_groups(k, v, np.ones(6, bool))
    assert np.isnan(got[3][1]) and got[3][0] == 2.0 and not np.signbit(got[3][2]) and not np.signbit(got[4][2])
    for a, b in ((got[3], want[3]), (got[4], want[4])):
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint32), b[~np.isnan(b)].view(np.uint32))
    # the joined table of the join family: every seventh left row finds no right key
    cols, hit, rr = gw.join_left(gw.steady(4097))
    rc = gw.right_columns()
    assert len(np.unique(rc["rk"])) == gw.RIGHT_ROWS and rc["rk"].max() - rc["rk"].min() < 4096
    assert np.array_equal(np.isin(cols["kk"], rc["rk"]), hit) and 0 < (~hit).sum() < 4097 / 6
    pos = {int(k): i for i, k in enumerate(rc["rk"])}
    assert all(rc["rr"][pos[int(k)]] == r for k, r in zip(cols["kk"][hit][:200], rr[hit][:200]))
