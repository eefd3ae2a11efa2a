"""GPU tests of the multi-value GROUP BY (wx_group_multi.hip) through
wx_group_agg_multi and WarpDB::query_sql_grouped.

The reference of an M-value call is M separate oracle calls
(oracle_lib.group_agg), one per value expression.  Keys and counts are
compared exactly and MIN / MAX bit for bit.  Sums are compared bit for bit on
tables built so that the order of the adds cannot matter: every value,
products included, is a multiple of 2^-6 below 2^17 over at most 2^20 rows, so
every partial sum is a multiple of 2^-6 below 2^37 and exact in a double (the
oracle's sums are first checked to be unchanged under row reversal).  One
case uses ordinary floats and compares at the project's rtol = 1e-12.

Outputs are prefilled with sentinels and must be untouched at positions >=
the group count.
"""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest

import oracle_lib as ora
from test_gpu_parity import bits, dev_table, launch

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from warpdb_amd import _warpexec as wx  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEST_CSV = os.path.join(ROOT, "tests", "golden", "test.csv")

KEY = "k"
# name -> (value expressions, sum mask, min/max mask); S summed and Q min/max
# values: S + Q <= 4 runs two 512-thread workgroups per CU, more runs one of 1024
SPECS = {
    "sum2": (["va", "va * vb"], 0b11, 0b00),                # sums only, shared columns
    "sum4": (["va", "vb", "vc", "vd"], 0b1111, 0b0000),     # sums only, disjoint columns (S = 4)
    "mm3": (["va", "vc", "vd"], 0b000, 0b111),              # min/max only
    "mix3": (["va", "vc", "va * vb"], 0b101, 0b010),        # mixed, S + Q = 3
    "mix4": (["va", "va * vb", "vc", "vd"], 0b1011, 0b1100),  # mixed, S + Q = 5: one workgroup per CU
    "all4": (["va", "va * vb", "vc", "vd"], 0b1111, 0b1111),  # S = Q = 4: the widest
}
SIZES = [0, 1, 63, 4097, 300_001]
# name -> (key generator bounds [lo, hi), key_window_lo, capacity)
LAYOUTS = {
    "inside": (0, 1000, 0, 4096),          # every key in the window
    "straddle": (-3000, 3000, -500, 8000),  # negative keys, a window that does not start at 0, < 4096 keys outside
    "outside": (5000, 8000, 0, 4096),      # all outside, <= 4096 distinct: the LDS-sorted finalize
    "many": (10_000, 16_000, 0, 8192),     # ~6000 distinct outside keys: the device-sorted finalize
    "narrow": (5000, 6500, 0, 8192),       # outside the caller's window, but a span the window can be moved onto
}


@functools.lru_cache(maxsize=None)
def columns(n, layout, kind="exact"):
    """Host columns, shared by every test of this (n, layout): read, never written."""
    lo, hi, _, _ = LAYOUTS[layout]
    rng = np.random.default_rng(1000 + n + list(LAYOUTS).index(layout))
    if kind == "exact":  # multiples of 2^-6; |va * vb| < 2^16
        cols = {
            "k": rng.integers(lo, hi, n).astype(np.int32),
            "va": (rng.integers(0, 256 * 64, n) / 64.0).astype(np.float32),
            "vb": rng.integers(0, 256, n).astype(np.float32),
            "vc": (rng.integers(-64_000, 64_001, n) / 64.0).astype(np.float32),
            "vd": (rng.integers(-4_000_000, 4_000_001, n) / 64.0).astype(np.float32),
        }
    elif kind == "skew":  # 90 % of the rows on one key
        k = rng.integers(lo, hi, n).astype(np.int32)
        k[rng.random(n) < 0.9] = lo + 7
        cols = dict(columns(n, layout))
        cols["k"] = k
    else:  # ordinary floats
        cols = {
            "k": rng.integers(lo, hi, n).astype(np.int32),
            "va": rng.uniform(0, 40, n).astype(np.float32),
            "vb": rng.uniform(1, 100, n).astype(np.float32),
            "vc": rng.normal(0, 1000, n).astype(np.float32),
            "vd": rng.uniform(-1, 1, n).astype(np.float32),
        }
    for v in cols.values():
        v.setflags(write=False)
    return cols


@functools.lru_cache(maxsize=None)
def reference(n, layout, expr, cond=None, kind="exact"):
    """The oracle's groups for one value expression: (keys, sums, counts, mins, maxs)."""
    cols = columns(n, layout, kind)
    r = ora.group_agg(ora.HostTable(cols), expr, KEY, cond)
    if kind != "floats":  # the order of the adds cannot matter on these tables
        rev = ora.group_agg(ora.HostTable({k: v[::-1].copy() for k, v in cols.items()}), expr, KEY, cond)
        assert np.array_equal(r[0], rev[0]) and np.array_equal(r[1].view(np.uint64), rev[1].view(np.uint64))
    for x in r:
        x.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def device_table(n, layout, kind="exact", offset=0):
    return dev_table(columns(n, layout, kind), offset)[0]


def run(table, exprs, smask, qmask, key_lo, cap, cond=None, L=None, key=KEY):
    """One fused call; returns (groups, keys, counts, sums[j], mins[j], maxs[j]) as host arrays
    of all `cap` + 1 entries (None where not requested)."""
    m = len(exprs)
    room = max(1, cap) + 1
    dk = torch.full((room,), -77, dtype=torch.int32, device="cuda")
    dc = torch.full((room,), -77, dtype=torch.int64, device="cuda")
    ds = [torch.full((room,), -77.0, dtype=torch.float64, device="cuda") if smask >> j & 1 else None for j in range(m)]
    dn = [torch.full((room,), -77.0, dtype=torch.float32, device="cuda") if qmask >> j & 1 else None for j in range(m)]
    dx = [torch.full((room,), -77.0, dtype=torch.float32, device="cuda") if qmask >> j & 1 else None for j in range(m)]
    p = lambda ts: [0 if t is None else t.data_ptr() for t in ts]  # noqa: E731
    g = wx.group_agg_multi(table, [ora.lower(e) for e in exprs], ora.lower(key), ora.lower(cond) if cond else None,
                           L or launch(), key_lo, cap, dk.data_ptr(), dc.data_ptr(), p(ds), p(dn), p(dx))
    h = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return g, h(dk), h(dc), [h(t) for t in ds], [h(t) for t in dn], [h(t) for t in dx]


def same_floats(got, want):
    """Bit for bit, any NaN matching any NaN."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(want[~nan]))


def check(res, refs, smask, qmask, rtol=None):
    g, keys, cnts, sums, mins, maxs = res
    rk, _, rc, _, _ = refs[0]
    assert g == len(rk)
    assert np.array_equal(keys[:g], rk) and (keys[g:] == -77).all()
    assert np.array_equal(cnts[:g], rc) and (cnts[g:] == -77).all()
    for j, (k2, rs, c2, rmn, rmx) in enumerate(refs):
        assert np.array_equal(k2, rk) and np.array_equal(c2, rc)
        if smask >> j & 1:
            if rtol is None:
                assert np.array_equal(sums[j][:g].view(np.uint64), rs.view(np.uint64)), f"sum of value {j}"
            else:
                print(f"value {j}: max relative error of the sums "
                      f"{np.max(np.abs(sums[j][:g] - rs) / np.maximum(np.abs(rs), 1e-300)):.3e}")
                assert np.allclose(sums[j][:g], rs, rtol=rtol, atol=0.0), f"sum of value {j}"
            assert (sums[j][g:] == -77.0).all()
        if qmask >> j & 1:
            assert same_floats(mins[j][:g], rmn), f"min of value {j}"
            assert same_floats(maxs[j][:g], rmx), f"max of value {j}"
            assert not np.signbit(mins[j][:g][mins[j][:g] == 0]).any()
            assert (mins[j][g:] == -77.0).all() and (maxs[j][g:] == -77.0).all()


def run_and_check(n, layout, spec, cond=None, kind="exact", offset=0, rtol=None):
    exprs, smask, qmask = SPECS[spec]
    _, _, key_lo, cap = LAYOUTS[layout]
    res = run(device_table(n, layout, kind, offset), exprs, smask, qmask, key_lo, cap, cond)
    check(res, [reference(n, layout, e, cond, kind) for e in exprs], smask, qmask, rtol)
    return res


# quad tail, a single workgroup, many workgroups flushing the same bins; both workgroup geometries
@pytest.mark.parametrize("spec", ["mix3", "all4"])
@pytest.mark.parametrize("layout", ["inside", "straddle"])
@pytest.mark.parametrize("n", SIZES)
def test_row_counts(n, layout, spec):
    run_and_check(n, layout, spec)


@pytest.mark.parametrize("spec", list(SPECS))
def test_mask_combinations(spec):
    run_and_check(300_001, "straddle", spec)


@pytest.mark.parametrize("spec", ["sum2", "mix4"])
def test_all_keys_outside_the_window(spec):
    g = run_and_check(300_001, "outside", spec)[0]
    assert 2900 < g <= 3000


def test_device_sorted_finalize():
    g = run_and_check(300_001, "many", "mix4")[0]
    assert g > 4096  # more general keys than the finalize sorts in LDS


def test_window_moved_onto_the_sampled_key_range(monkeypatch):
    """capacity > 4096 on a table above the row floor (lowered here): the key sample, then its memo,
    place the window; a span too wide for it ("many") keeps the caller's window.  Same results."""
    monkeypatch.setenv("WARPDB_GP_MIN_ROWS", "1000")
    for layout in ("narrow", "narrow", "many"):
        run_and_check(300_001, layout, "mix3")


def test_capacity_too_small():
    exprs, smask, qmask = SPECS["mix4"]
    want = len(reference(300_001, "outside", "va")[0])
    with pytest.raises(wx.WarpExecError) as e:
        run(device_table(300_001, "outside"), exprs, smask, qmask, 0, 100)
    assert e.value.status == wx.WX_ERR_CAPACITY and e.value.count == want
    run_and_check(300_001, "outside", "mix4")  # and the next call sees clean accumulators


@pytest.mark.parametrize("spec", ["sum2", "sum4"])
def test_skewed_key_wave_combined_add(spec):
    run_and_check(300_001, "inside", spec, kind="skew")


def test_nan_and_signed_zero_minmax():
    n = 4097
    rng = np.random.default_rng(5)
    pool = np.array([np.nan, -0.0, 0.0, 1.5, -2.25, np.inf, -np.inf, 1e-40], np.float32)
    cols = {"k": rng.integers(-5, 60, n).astype(np.int32), "va": rng.choice(pool, n), "vb": np.ones(n, np.float32),
            "vc": rng.choice(pool[:3], n), "vd": rng.choice(pool, n)}
    cols["va"][cols["k"] == 3] = np.nan  # a group with no value at all
    cols["vc"][cols["k"] == 4] = -0.0    # only negative zeros
    exprs, smask, qmask = SPECS["mm3"]
    res = run(dev_table(cols)[0], exprs, smask, qmask, 0, 4096)
    refs = [ora.group_agg(ora.HostTable(cols), e, KEY) for e in exprs]
    check(res, refs, smask, qmask)
    g, keys, _, _, mins, maxs = res
    at = lambda k: int(np.nonzero(keys[:g] == k)[0][0])  # noqa: E731
    assert np.isnan(mins[0][at(3)]) and np.isnan(maxs[0][at(3)])
    assert bits(mins[1][at(4)]) == 0 and bits(maxs[1][at(4)]) == 0  # +0.0


def test_where_rejects_every_row():
    g = run_and_check(4097, "straddle", "sum2", cond="va > 1000")[0]
    assert g == 0


def test_unaligned_columns():
    run_and_check(4097, "straddle", "sum2", offset=1)
    run_and_check(300_001, "straddle", "sum2", offset=1)


def test_ordinary_floats():
    run_and_check(300_001, "straddle", "all4", kind="floats", rtol=1e-12)


def test_repeated_call_same_bits():
    a = run_and_check(300_001, "straddle", "all4")
    b = run_and_check(300_001, "straddle", "all4")
    for x, y in zip(a[3] + a[4] + a[5], b[3] + b[4] + b[5]):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def single(table, expr, key_lo, cap, minmax):
    dk = torch.empty(cap, dtype=torch.int32, device="cuda")
    ds = torch.empty(cap, dtype=torch.float64, device="cuda")
    dc = torch.empty(cap, dtype=torch.int64, device="cuda")
    dn = torch.empty(cap, dtype=torch.float32, device="cuda")
    dx = torch.empty(cap, dtype=torch.float32, device="cuda")
    if minmax:
        g = wx.group_agg(table, ora.lower(expr), ora.lower(KEY), None, launch(), key_lo, cap, dk.data_ptr(),
                         ds.data_ptr(), dc.data_ptr(), dn.data_ptr(), dx.data_ptr())
    else:
        g = wx.group_sum(table, ora.lower(expr), ora.lower(KEY), None, launch(), key_lo, cap, dk.data_ptr(),
                         ds.data_ptr(), dc.data_ptr())
    return tuple(t[:g].cpu().numpy() for t in (dk, ds, dc, dn, dx))


def test_each_slot_equals_the_single_value_call():
    n, layout = 300_001, "straddle"
    exprs, smask, qmask = SPECS["all4"]
    _, _, key_lo, cap = LAYOUTS[layout]
    table = device_table(n, layout)
    g, keys, cnts, sums, mins, maxs = run(table, exprs, smask, qmask, key_lo, cap)
    for j, e in enumerate(exprs):
        sk, ss, sc, sn, sx = single(table, e, key_lo, cap, True)
        assert np.array_equal(keys[:g], sk) and np.array_equal(cnts[:g], sc)
        assert np.array_equal(sums[j][:g].view(np.uint64), ss.view(np.uint64))
        assert same_floats(mins[j][:g], sn) and same_floats(maxs[j][:g], sx)


def test_shared_accumulators_are_left_idle():
    """multi (M = 4), wx_group_sum, multi (M = 2), wx_group_agg with MIN / MAX on one stream:
    each is correct only if the one before returned every shared accumulator to its idle value."""
    n, layout = 300_001, "straddle"
    _, _, key_lo, cap = LAYOUTS[layout]
    table = device_table(n, layout)
    run_and_check(n, layout, "all4")
    sk, ss, sc, _, _ = single(table, "va", key_lo, cap, False)
    rk, rs, rc, rmn, rmx = reference(n, layout, "va")
    assert np.array_equal(sk, rk) and np.array_equal(sc, rc) and np.array_equal(ss.view(np.uint64), rs.view(np.uint64))
    run_and_check(n, layout, "sum2")
    sk, ss, sc, sn, sx = single(table, "vc", key_lo, cap, True)
    rk, rs, rc, rmn, rmx = reference(n, layout, "vc")
    assert np.array_equal(sk, rk) and np.array_equal(sc, rc) and np.array_equal(ss.view(np.uint64), rs.view(np.uint64))
    assert same_floats(sn, rmn) and same_floats(sx, rmx)
    run_and_check(n, "outside", "mix4")  # and through the general-key table
    sk, ss, sc, _, _ = single(device_table(n, "outside"), "va", 0, 4096, False)
    rk, rs, rc, _, _ = reference(n, "outside", "va")
    assert np.array_equal(sk, rk) and np.array_equal(sc, rc) and np.array_equal(ss.view(np.uint64), rs.view(np.uint64))


def test_one_value_is_group_agg():
    n, layout = 4097, "straddle"
    _, _, key_lo, cap = LAYOUTS[layout]
    res = run(device_table(n, layout), ["vc"], 0b0, 0b1, key_lo, cap)  # MIN / MAX only: the sums go to scratch
    check(res, [reference(n, layout, "vc")], 0b0, 0b1)


# ------------------------------------------------------------------ facade
def write_csv(path, cols):
    with open(path, "w") as f:
        f.write(",".join(cols) + "\n")
        for row in zip(*cols.values()):
            f.write(",".join(repr(x.item()) for x in row) + "\n")


@pytest.fixture(scope="module")
def grouped_db(tmp_path_factory):
    from warpdb_amd import pywarpdb as pw

    n = 20_000
    cols = {k: v[:n] for k, v in columns(300_001, "inside").items()}
    cols["k"] = (cols["k"] % 37).astype(np.int32)
    path = str(tmp_path_factory.mktemp("grouped") / "grouped.csv")
    write_csv(path, cols)
    D = pw.DataType
    return pw.WarpDB(path, [D.Int32, D.Float32, D.Float32, D.Float32, D.Float32], 0), cols


def numpy_groups(cols, where=None):
    keep = np.ones(len(cols["k"]), bool) if where is None else where
    keys = np.unique(cols["k"][keep])
    rows = [keep & (cols["k"] == k) for k in keys]
    return keys, rows


def test_query_sql_grouped_on_test_csv():
    from warpdb_amd import pywarpdb as pw

    db = pw.WarpDB(TEST_CSV)
    names, cols = db.query_sql_grouped("SELECT quantity, SUM(price), MAX(price * quantity), COUNT(price), AVG(price * 2) "
                                       "FROM t GROUP BY quantity")
    assert names == ["quantity", "sum_1", "max_2", "count_3", "avg_4"]
    assert cols[0].tolist() == [2.0, 3.0, 4.0, 5.0] and cols[1].tolist() == [15.25, 10.5, 20.0, 30.0]
    assert cols[2].tolist() == [30.5, 31.5, 80.0, 150.0] and cols[3].tolist() == [1.0] * 4
    assert cols[4].tolist() == [30.5, 21.0, 40.0, 60.0]
    assert all(c.dtype == np.float32 for c in cols)
    # the single-value entry point still refuses it, with the old text
    with pytest.raises(RuntimeError, match="two different expressions"):
        db.query_sql_table("SELECT quantity, SUM(price), MAX(price * quantity) FROM t GROUP BY quantity")


def test_query_sql_grouped_vs_numpy(grouped_db):
    db, cols = grouped_db
    # five distinct value expressions (two chunks), HAVING on an aggregate that is not selected,
    # ORDER BY an aggregate DESC, LIMIT / OFFSET
    sql = ("SELECT k, SUM(va), AVG(va * vb), MIN(vc), MAX(vd), SUM(vb), COUNT(va), MAX(vc) FROM t WHERE va > 16 "
           "GROUP BY k HAVING SUM(vc + vd) > 0 ORDER BY SUM(va * vb) DESC LIMIT 9 OFFSET 2")
    names, out = db.query_sql_grouped(sql)
    assert names == ["k", "sum_1", "avg_2", "min_3", "max_4", "sum_5", "count_6", "max_7"]
    a, b = cols["va"].astype(np.float64), cols["vb"].astype(np.float64)
    keys, rows = numpy_groups(cols, cols["va"] > 16)
    f32 = lambda x: np.float32(x)  # noqa: E731
    cd = (cols["vc"] + cols["vd"]).astype(np.float64)  # the engine adds in float, then sums in double
    ab = (cols["va"] * cols["vb"]).astype(np.float64)
    table = [(ab[r].sum(), [f32(k), f32(a[r].sum()), f32(ab[r].sum() / r.sum()), cols["vc"][r].min(), cols["vd"][r].max(),
                            f32(b[r].sum()), f32(r.sum()), cols["vc"][r].max()])
             for k, r in zip(keys, rows) if cd[r].sum() > 0]
    table.sort(key=lambda t: -t[0])  # sums of exact values: no ties in practice, checked below
    assert len({t[0] for t in table}) == len(table)
    want = [t[1] for t in table][2:11]
    assert len(want) == 9
    for j in range(len(names)):
        assert np.array_equal(bits(out[j]), bits(np.array([w[j] for w in want], np.float32))), names[j]


def test_query_sql_grouped_row_order(grouped_db, monkeypatch):
    db, cols = grouped_db
    monkeypatch.setenv("WARPDB_GROUP_ROW_ORDER", "1")
    names, out = db.query_sql_grouped("SELECT k, SUM(va), SUM(va * vb), MAX(vc), AVG(vd) FROM t GROUP BY k")
    table, _ = dev_table(cols)
    cap = 4096
    L = launch(flags=wx.F_SYNC | wx.F_ROW_ORDER)
    for j, (e, f) in enumerate([("va", "sum"), ("va * vb", "sum"), ("vc", "max"), ("vd", "avg")], start=1):
        dk = torch.empty(cap, dtype=torch.int32, device="cuda")
        ds = torch.empty(cap, dtype=torch.float64, device="cuda")
        dc = torch.empty(cap, dtype=torch.int64, device="cuda")
        dn = torch.empty(cap, dtype=torch.float32, device="cuda")
        dx = torch.empty(cap, dtype=torch.float32, device="cuda")
        g = wx.group_agg(table, ora.lower(e), "k[idx]", None, L, 0, cap, dk.data_ptr(), ds.data_ptr(), dc.data_ptr(),
                         dn.data_ptr(), dx.data_ptr())
        s, c, x = ds[:g].cpu().numpy(), dc[:g].cpu().numpy(), dx[:g].cpu().numpy()
        want = {"sum": s, "max": x, "avg": s / c}[f].astype(np.float32)
        assert np.array_equal(out[0], dk[:g].cpu().numpy().astype(np.float32))
        assert np.array_equal(bits(out[j]), bits(want)), names[j]
