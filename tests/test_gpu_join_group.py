"""GPU tests of the JOIN under GROUP BY (wx_join_group.hip) through
wx_join_group_agg and WarpDB::attach / query_sql_joined_grouped (pywarpdb).

The reference materialises the inner join on the host with numpy (a
searchsorted over the sorted right keys, as test_gpu_join.expected does) and
runs oracle_lib.group_agg over the joined host table, once per value.  Keys,
counts and MIN / MAX are compared exactly.  Sums are compared bit for bit on
tables where the order of the adds cannot matter: every summed value is a
multiple of 2^-6 below 2^17 over at most 2^20 rows (va is on a 1/8 grid below
1024, rr on a 1/8 grid below 64, rd on a 1/4 grid below 1024), so every
partial sum is exact in a double; the oracle's sums are first checked to be
unchanged under row reversal.  One case uses ordinary floats at the project's
rtol = 1e-12.

Outputs are prefilled with sentinels and must be untouched at positions >=
the group count.  The table builders are test_gpu_join's; this file only adds
group-key columns to them.
"""
from __future__ import annotations

import functools
import os
import re

import numpy as np
import pytest

import oracle_lib as ora
from test_gpu_group_multi import check as check_groups
from test_gpu_group_multi import columns as gm_columns
from test_gpu_group_multi import reference as gm_reference
from test_gpu_group_multi import run as gm_run
from test_gpu_join import EXPECTED_FORM, assert_form, left_columns, right_columns, right_keys
from test_gpu_parity import bits, dev_table, launch

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from warpdb_amd import _warpexec as wx  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECT, HASH = wx.JOIN_DIRECT, wx.JOIN_HASH
COND = "pp > 0.5"                 # names left columns only: the probe follows the WHERE
COND_R = "pp > 0.5 AND rr > 0"    # names a right column: every row is probed first

# name -> (value expressions, sum mask, min/max mask)
SPECS = {
    "one": (["va * rr"], 0b1, 0b0),
    "sum2": (["va", "va * rr"], 0b11, 0b00),
    "mm3": (["va", "rr", "rl"], 0b000, 0b111),
    "mix3": (["va", "rd", "va * rr"], 0b101, 0b010),           # S + Q = 3: 512 threads in both forms
    "mix5": (["va", "va * rr", "rd", "ri"], 0b1011, 0b1100),   # S + Q = 5: one workgroup of 1024
    "all4": (["va", "va * rr", "rd", "rr"], 0b1111, 0b1111),   # S = Q = 4: the widest
}
# group key -> (key_window_lo, capacity)
KEYS = {
    "t7": (0, 4096),                 # a right attribute of 7 values, inside the window
    "t1k": (-500, 8000),             # ~1000 values in [-3000, 3000): a window not at 0, < 4096 keys outside it
    "kk": (0, 8192),                 # the left join key itself
    "lg": (0, 4096),                 # a left column
    "t7 * 100 + lg": (0, 4096),      # both sides
    "rd": (-100, 4096),              # a right double through the (int) cast
    "rl": (0, 8192),                 # a right int64 through the (int) cast
    "t6k": (0, 8192),                # ~5000 values outside the window: the device-sorted finalize
}


def unroll():
    """Row quads per thread and span (WX_UNROLL of the kernel source)."""
    with open(os.path.join(ROOT, "warpdb_amd", "csrc", "kernels", "wx_group_multi.hip")) as f:
        return int(re.search(r"#define WX_UNROLL (\d+)", f.read()).group(1))


def span_rows(spec, form):
    _, smask, qmask = SPECS[spec]
    block, _, _ = wx.join_group_geometry(bin(smask).count("1"), bin(qmask).count("1"), form)
    return block * unroll() * 4


@functools.lru_cache(maxsize=None)
def rcols(rname):
    c = dict(right_columns(rname))
    r = np.arange(len(c["rk"]), dtype=np.int64)
    c["t7"] = (r % 7).astype(np.int32)
    c["t1k"] = ((r * 31) % 1000 * 6 - 3000).astype(np.int32)
    c["t6k"] = (r % 6000 + 10_000).astype(np.int32)
    for v in c.values():
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def lcols(n, rname, hit_mode, kind="plain"):
    c = dict(left_columns(n, rname, hit_mode))
    c["lg"] = (np.arange(n, dtype=np.int64) * 13 % 50).astype(np.int32)
    if kind == "skew":  # 90 % of the rows on one right row, so on one group whatever the key
        rng = np.random.default_rng(n)
        kk = c["kk"].copy()
        kk[rng.random(n) < 0.9] = np.sort(right_keys(rname)[0])[3]
        c["kk"] = kk
        c["pp"] = np.where(rng.random(n) < 0.95, np.float32(1), c["pp"]).astype(np.float32)
    for v in c.values():
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def tables(n, rname, hit_mode, kind="plain", offset=0):
    return dev_table(lcols(n, rname, hit_mode, kind), offset)[0], dev_table(rcols(rname), offset)[0]


@functools.lru_cache(maxsize=None)
def joined(n, rname, hit_mode, kind="plain"):
    """The inner join on the host: every left row that finds its key, with the matched right row's columns."""
    lc, rc = lcols(n, rname, hit_mode, kind), rcols(rname)
    lk = lc["kk"].astype(np.int64)
    order = np.argsort(rc["rk"], kind="stable")
    skeys = rc["rk"][order].astype(np.int64)
    m = len(skeys)
    pos = np.minimum(np.searchsorted(skeys, lk), max(m - 1, 0))
    hit = (skeys[pos] == lk) if m else np.zeros(len(lk), bool)
    rrow = order[pos[hit]] if m else np.zeros(0, np.int64)
    out = {k: v[hit] for k, v in lc.items()}
    out.update({k: v[rrow] for k, v in rc.items()})
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(n, rname, hit_mode, expr, gkey, cond, kind="plain", exact=True):
    cols = joined(n, rname, hit_mode, kind)
    r = ora.group_agg(ora.HostTable(cols), expr, gkey, cond)
    if exact:  # the order of the adds cannot matter on these tables
        rev = ora.group_agg(ora.HostTable({k: v[::-1].copy() for k, v in cols.items()}), expr, gkey, cond)
        assert np.array_equal(r[0], rev[0]) and np.array_equal(r[1].view(np.uint64), rev[1].view(np.uint64))
    for x in r:
        x.setflags(write=False)
    return r


def run(lt, rt, exprs, smask, qmask, gkey, key_lo, cap, cond, want_count=True, d_n_groups=False):
    """One call; the result in test_gpu_group_multi.run's layout."""
    m = len(exprs)
    room = max(1, cap) + 1
    dk = torch.full((room,), -77, dtype=torch.int32, device="cuda")
    dc = torch.full((room,), -77, dtype=torch.int64, device="cuda")
    ds = [torch.full((room,), -77.0, dtype=torch.float64, device="cuda") if smask >> j & 1 else None for j in range(m)]
    dn = [torch.full((room,), -77.0, dtype=torch.float32, device="cuda") if qmask >> j & 1 else None for j in range(m)]
    dx = [torch.full((room,), -77.0, dtype=torch.float32, device="cuda") if qmask >> j & 1 else None for j in range(m)]
    ng = torch.full((1,), -5, dtype=torch.int64, device="cuda") if d_n_groups else None
    p = lambda ts: [0 if t is None else t.data_ptr() for t in ts]  # noqa: E731
    g = wx.join_group_agg(lt, rt, "kk[idx]", "rk", [ora.lower(e) for e in exprs], ora.lower(gkey),
                          ora.lower(cond) if cond else None, launch(), key_lo, cap, dk.data_ptr(), dc.data_ptr(), p(ds),
                          p(dn), p(dx), d_n_groups=ng.data_ptr() if d_n_groups else 0, want_count=want_count)
    if d_n_groups:
        torch.cuda.synchronize()
        assert g is None or g == int(ng.item())
        g = int(ng.item())
    h = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return g, h(dk), h(dc), [h(t) for t in ds], [h(t) for t in dn], [h(t) for t in dx]


def run_and_check(n, rname, hit_mode, spec, gkey="t7", cond=COND, kind="plain", offset=0, **kw):
    exprs, smask, qmask = SPECS[spec]
    key_lo, cap = KEYS[gkey]
    lt, rt = tables(n, rname, hit_mode, kind, offset)
    res = run(lt, rt, exprs, smask, qmask, gkey, key_lo, cap, cond, **kw)
    check_groups(res, [reference(n, rname, hit_mode, e, gkey, cond, kind) for e in exprs], smask, qmask)
    return res


def test_geometry_covers_both_block_sizes():
    assert {span_rows("mix3", f) for f in (DIRECT, HASH)} == {512 * unroll() * 4}
    assert {span_rows("all4", f) for f in (DIRECT, HASH)} == {1024 * unroll() * 4}


# quad tail, one workgroup, one row past one workgroup span of each block size, many workgroups
@pytest.mark.parametrize("spec", ["mix3", "all4"])
@pytest.mark.parametrize("rname", ["span4096", "span4097"])
def test_left_sizes(rname, spec, monkeypatch):
    monkeypatch.delenv("WARPDB_JOIN_FORM", raising=False)
    form = assert_form(rname)
    for n in sorted({0, 1, 63, span_rows("mix3", form) + 1, span_rows("all4", form) + 1, 300_001}):
        g = run_and_check(n, rname, "mix", spec)[0]
        assert g == (0 if n == 0 else min(g, 7)) and (n < 300_001 or g == 7)  # t7: at most 7 groups, all at 300 001 rows


@pytest.mark.parametrize("hit_mode", ["all", "none", "mix"])
@pytest.mark.parametrize("rname", ["empty", "one", "span4096", "span4097", "wide5000", "cluster_last", "big"])
def test_right_tables(rname, hit_mode, monkeypatch):
    monkeypatch.delenv("WARPDB_JOIN_FORM", raising=False)
    assert_form(rname)
    g = run_and_check(20_011, rname, hit_mode, "sum2")[0]
    if hit_mode == "none" or rname == "empty":
        assert g == 0
    else:
        assert g > 0


def test_direct_range_table_in_the_hash_form(monkeypatch):
    monkeypatch.setenv("WARPDB_JOIN_FORM", "hash")
    assert_form("span4096", monkeypatch)
    for hit_mode in ("all", "mix"):
        run_and_check(20_011, "span4096", hit_mode, "sum2")


@pytest.mark.parametrize("gkey,rname", [("t1k", "span4096"), ("kk", "wide5000"), ("lg", "span4097"),
                                        ("t7 * 100 + lg", "span4096"), ("rd", "span4097"), ("rl", "span4096"),
                                        ("t6k", "wide5000")])
def test_group_keys_and_window_layouts(gkey, rname, monkeypatch):
    monkeypatch.delenv("WARPDB_JOIN_FORM", raising=False)
    g, keys = run_and_check(300_001, rname, "mix", "mix3", gkey)[:2]
    key_lo = KEYS[gkey][0]
    outside = int(((keys[:g] < key_lo) | (keys[:g] >= key_lo + 2048)).sum())
    if gkey == "t1k":
        assert keys[0] < 0 and 0 < outside < 4096 and g - outside > 0  # the LDS-sorted finalize beside the window
    if gkey in ("kk", "t6k"):
        assert outside > 4096  # the device-sorted finalize


@pytest.mark.parametrize("rname", ["span4096", "wide5000"])
@pytest.mark.parametrize("spec", list(SPECS))
def test_mask_combinations(spec, rname, monkeypatch):
    """Every mask in both forms, with the WHERE over a right column (every row probed)."""
    monkeypatch.delenv("WARPDB_JOIN_FORM", raising=False)
    run_and_check(300_001, rname, "mix", spec, "t1k", COND_R)


@pytest.mark.parametrize("rname", ["span4096", "wide5000"])
@pytest.mark.parametrize("cond", [None, COND, COND_R])
def test_where_forms(cond, rname, monkeypatch):
    monkeypatch.delenv("WARPDB_JOIN_FORM", raising=False)
    run_and_check(20_011, rname, "mix", "sum2", "t7", cond)


@pytest.mark.parametrize("hit_mode", ["mix", "none"])
@pytest.mark.parametrize("rname", ["one", "span4096", "span4097", "wide5000", "cluster_last"])
def test_clamp_of_dropped_and_tail_rows(rname, hit_mode, monkeypatch):
    """With the right-column WHERE every row is probed: the dropped rows carry INT32_MIN, INT32_MAX, the keys
    just outside the span, gaps and keys of the cluster's home slot, and the last quad's rows past n_rows
    carry zero-filled registers."""
    monkeypatch.delenv("WARPDB_JOIN_FORM", raising=False)
    for n in (4097 + 2, 20_011):
        run_and_check(n, rname, hit_mode, "sum2", "t7", COND_R)


@pytest.mark.parametrize("rname", ["span4096", "wide5000"])
@pytest.mark.parametrize("spec", ["sum2", "mix3"])  # the wave-combined add, and the plain path
def test_skewed_group(spec, rname, monkeypatch):
    monkeypatch.delenv("WARPDB_JOIN_FORM", raising=False)
    g, _, cnts = run_and_check(300_001, rname, "all", spec, "t7", COND, kind="skew")[:3]
    assert cnts[:g].max() > 0.85 * cnts[:g].sum()


def test_ordinary_floats(monkeypatch):
    monkeypatch.delenv("WARPDB_JOIN_FORM", raising=False)
    exprs, smask, qmask = ["va * 0.37", "rr * 0.11 + va"], 0b11, 0b10
    n, rname = 300_001, "wide5000"
    lt, rt = tables(n, rname, "mix")
    res = run(lt, rt, exprs, smask, qmask, "t7", 0, 4096, COND)
    check_groups(res, [reference(n, rname, "mix", e, "t7", COND, exact=False) for e in exprs], smask, qmask, rtol=1e-12)


def test_unaligned_columns(monkeypatch):
    monkeypatch.delenv("WARPDB_JOIN_FORM", raising=False)
    run_and_check(20_011, "span4097", "mix", "sum2", offset=1)


def test_device_count_without_host_count(monkeypatch):
    monkeypatch.delenv("WARPDB_JOIN_FORM", raising=False)
    run_and_check(20_011, "span4096", "mix", "sum2", want_count=False, d_n_groups=True)
    lt, rt = tables(20_011, "empty", "mix")
    assert run(lt, rt, *SPECS["sum2"], "t7", 0, 4096, COND, want_count=False, d_n_groups=True)[0] == 0


def plain_group_multi_is_correct():
    """A plain wx_group_agg_multi with masks of its own: right only if the shared accumulators were idle."""
    n, layout, exprs, smask, qmask = 4097, "straddle", ["vc", "va", "vd"], 0b011, 0b110
    res = gm_run(dev_table(gm_columns(n, layout))[0], exprs, smask, qmask, -500, 8000)
    check_groups(res, [gm_reference(n, layout, e) for e in exprs], smask, qmask)


@pytest.mark.parametrize("rname", ["span4096", "wide5000"])
def test_failed_calls_leave_the_accumulators_idle(rname, monkeypatch):
    monkeypatch.delenv("WARPDB_JOIN_FORM", raising=False)
    n = 20_011
    lt, _ = tables(n, rname, "mix")
    rc = {k: v.copy() for k, v in rcols(rname).items()}
    dup = int(rc["rk"][17])
    rc["rk"][1234] = dup
    bad = dev_table(rc)[0]
    with pytest.raises(wx.WarpExecError, match=rf"JOIN: the right key is not unique \(key {dup}\)") as ei:
        run(lt, bad, *SPECS["mix5"], "t1k", *KEYS["t1k"], COND_R)
    assert ei.value.status == wx.WX_ERR_UNSUPPORTED
    run_and_check(n, rname, "mix", "sum2", "t1k", COND_R)
    plain_group_multi_is_correct()
    # more groups than the outputs hold: the call reports how many it found
    lt, rt = tables(n, rname, "mix")
    want = len(reference(n, rname, "mix", "va", "t1k", COND_R)[0])
    assert want > 100
    with pytest.raises(wx.WarpExecError) as ei:
        run(lt, rt, *SPECS["mix5"], "t1k", -500, 100, COND_R)
    assert ei.value.status == wx.WX_ERR_CAPACITY and ei.value.count == want
    run_and_check(n, rname, "mix", "mm3", "t1k", COND_R)
    plain_group_multi_is_correct()


def test_direct_then_hash_on_one_workspace(monkeypatch):
    monkeypatch.delenv("WARPDB_JOIN_FORM", raising=False)
    for rname in ("span4096", "wide5000", "span4096", "big"):
        run_and_check(20_011, rname, "mix", "sum2")


def test_prepared_module_is_the_one_the_run_uses(monkeypatch):
    monkeypatch.delenv("WARPDB_JOIN_FORM", raising=False)
    exprs, smask, qmask = ["va + 3", "rr - va"], 0b01, 0b10  # a shape no other test compiles
    n, rname = 4097, "span4097"
    lt, rt = tables(n, rname, "mix")
    wx.prepare_join_group(lt, rt, "kk[idx]", "rk", [ora.lower(e) for e in exprs], smask, qmask, ora.lower("t7"),
                          ora.lower(COND), launch(), EXPECTED_FORM[rname])
    before = wx.cache_stats()[0]
    res = run(lt, rt, exprs, smask, qmask, "t7", 0, 4096, COND)
    assert wx.cache_stats()[0] == before
    check_groups(res, [reference(n, rname, "mix", e, "t7", COND) for e in exprs], smask, qmask)


# ------------------------------------------------------------------ facade
def _write_csv(path, cols):
    with open(path, "w") as f:
        f.write(",".join(cols) + "\n")
        for row in zip(*cols.values()):
            f.write(",".join(repr(x.item()) for x in row) + "\n")


@pytest.fixture(scope="module")
def joined_db(tmp_path_factory):
    from warpdb_amd import pywarpdb as pw

    D = pw.DataType
    n, rname = 20_011, "span4097"
    lc = {k: lcols(n, rname, "mix")[k] for k in ("kk", "va", "pp", "lg")}
    rc = {k: rcols(rname)[k] for k in ("rk", "rr", "ri", "t7")}
    rc["va"] = rc["rr"] + np.float32(1)  # a name in both tables
    d = tmp_path_factory.mktemp("joined_grouped")
    _write_csv(d / "fact.csv", lc)
    _write_csv(d / "dim.csv", rc)
    db = pw.WarpDB(str(d / "fact.csv"), [D.Int32, D.Float32, D.Float32, D.Int32], 0)
    db.attach("dim", str(d / "dim.csv"), [D.Int32, D.Float32, D.Int32, D.Int32, D.Float32])
    return db, joined(n, rname, "mix")


def test_facade_every_aggregate_kind(joined_db):
    db, j = joined_db
    sql = ("SELECT dim.t7, SUM(t.va * rr), AVG(t.va), COUNT(*), MIN(ri), MAX(t.va * rr), SUM(lg) FROM t JOIN dim "
           "ON kk = dim.rk WHERE pp > 0.5 GROUP BY t7 HAVING SUM(rr + lg) > 0 ORDER BY SUM(t.va) DESC LIMIT 4 OFFSET 1")
    names, out = db.query_sql_joined_grouped(sql)
    assert names == ["t7", "sum_1", "avg_2", "count_3", "min_4", "max_5", "sum_6"]
    refs = {e: reference(20_011, "span4097", "mix", e, "t7", COND) for e in ("va * rr", "va", "ri", "lg", "rr + lg")}
    keys, _, cnts, _, _ = refs["va"]
    f32 = np.float32
    table = [(refs["va"][1][i], [f32(keys[i]), f32(refs["va * rr"][1][i]), f32(refs["va"][1][i] / cnts[i]), f32(cnts[i]),
                                 refs["ri"][3][i], refs["va * rr"][4][i], f32(refs["lg"][1][i])])
             for i in range(len(keys)) if refs["rr + lg"][1][i] > 0]
    table.sort(key=lambda t: -t[0])
    assert len({t[0] for t in table}) == len(table) >= 5  # no ties: the order is determined
    want = [t[1] for t in table][1:5]
    assert j["t7"].max() == 6
    for c in range(len(names)):
        assert np.array_equal(bits(out[c]), bits(np.array([w[c] for w in want], np.float32))), names[c]


def test_facade_answers_the_planner_table(joined_db, tmp_path):
    """Every row of join_group_errors.tsv against the whole facade: t(price, quantity, cust, id) JOIN u(id, rate, tier)."""
    from warpdb_amd import pywarpdb as pw

    D = pw.DataType
    (tmp_path / "t.csv").write_text("price,quantity,cust,id\n10.5,3,1,7\n20.0,4,2,8\n15.25,2,1,9\n30.0,5,3,7\n")
    (tmp_path / "u.csv").write_text("id,rate,tier\n1,0.5,10\n2,0.75,20\n4,2.0,10\n")
    db = pw.WarpDB(str(tmp_path / "t.csv"), [D.Float32, D.Int32, D.Int32, D.Int32], 0)
    db.attach("u", str(tmp_path / "u.csv"), [D.Int32, D.Float32, D.Int32])
    accepted = refused = 0
    with open(os.path.join(ROOT, "tests", "golden", "join_group_errors.tsv")) as f:
        for line in f:
            if line.startswith("#") or not line.strip():
                continue
            kind, sql, want = line.rstrip("\n").split("\t")
            if kind == "refuse":
                with pytest.raises(RuntimeError) as ei:
                    db.query_sql_joined_grouped(sql)
                assert str(ei.value) == want, sql
                refused += 1
            else:
                names, cols = db.query_sql_joined_grouped(sql)
                assert names == want.split(" | ")[5].split(","), sql
                assert len(cols) == len(names) and len({len(c) for c in cols}) == 1
                accepted += 1
    assert accepted >= 8 and refused >= 20
    # the headline query: rows 0, 2 (cust 1 -> tier 10) and 1 (cust 2 -> tier 20) match; price > 15 keeps 2 and 1
    names, cols = db.query_sql_joined_grouped("SELECT u.tier, SUM(price * u.rate), COUNT(*), MAX(price) FROM t JOIN u "
                                              "ON t.cust = u.id WHERE price > 15 GROUP BY u.tier")
    assert [c.tolist() for c in cols] == [[10.0, 20.0], [7.625, 15.0], [1.0, 1.0], [15.25, 20.0]]
    # the other entry points keep their refusals word for word
    with pytest.raises(RuntimeError, match="GROUP BY is not supported by query_sql_joined"):
        db.query_sql_joined("SELECT tier FROM t JOIN u ON cust = u.id GROUP BY tier")
    with pytest.raises(RuntimeError, match="JOIN is not supported by the execution engine"):
        db.query_sql_grouped("SELECT quantity, SUM(price) FROM t JOIN u ON quantity = price GROUP BY quantity")
