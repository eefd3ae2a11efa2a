"""GPU tests of the PK-FK equi-join (wx_join.hip) through wx_join_select,
WarpDB::attach / query_join / query_sql_joined and their pywarpdb bindings.

Expectations are computed here with numpy (a searchsorted over the sorted
right keys) and every comparison is bit-exact: the value columns lie on a 1/8
grid (|va| <= 1024, |rr| <= 64, so va * rr is exact in float32), the integer
and double columns convert to float32 the way the kernel's static_cast does,
and an unmatched row's right-side output is the kernel's quiet NaN
(0x7fc00000, numpy's).  Outputs are prefilled with a NaN / -1 sentinel and
must be untouched at positions >= count and in front of an offset pointer.

The clamp: the kernels probe EVERY row of a tile, rows the WHERE drops and
the zero-filled rows past n_rows included.  The left tables here give the
dropped rows keys that are absent from the right table -- INT32_MIN,
INT32_MAX, the values just outside the key span on both sides and gaps
between keys -- in valid queries whose answer is known; the results must not
change.
"""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest

from test_gpu_parity import bits, dev_table, launch

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from warpdb_amd import _warpexec as wx  # noqa: E402

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
COND = "(pp[idx] > 0.5f)"
COND_R = "(pp[idx] > 0.5f && rr[idx] > 0.0f)"
INNER, LEFT = wx.JOIN_INNER, wx.JOIN_LEFT
DIRECT, HASH = wx.JOIN_DIRECT, wx.JOIN_HASH
NAN_BITS = np.uint32(0x7fc00000)
HASH_MUL = np.uint64(0x9E3779B1)


def home_slots(keys, log2cap):
    """wx_join_hash_slot over an array (checked against the library in test_hash_slot_model)."""
    k = np.asarray(keys, np.int64).astype(np.uint64) & np.uint64(0xffffffff)
    return (((k * HASH_MUL) & np.uint64(0xffffffff)) >> np.uint64(32 - log2cap)).astype(np.int64)


def _cluster(slot, log2cap=10):
    """Keys of [0, 2^20) whose home slot in a 1024-slot table is `slot`: (300 members, absent ones)."""
    cand = np.arange(1 << 20, dtype=np.int64)
    same = cand[home_slots(cand, log2cap) == slot]
    assert len(same) >= 400
    return same[:300], same[300:400]


@functools.lru_cache(maxsize=None)
def right_keys(name):
    """(keys in right-row order, absent keys that are likely to collide or None)."""
    rng = np.random.default_rng(77)
    extra = None
    if name == "empty":
        k = np.zeros(0, np.int64)
    elif name == "one":
        k = np.array([7], np.int64)
    elif name == "span4096":  # span exactly 4096, negative start: the direct form's widest table
        mid = rng.choice(np.arange(-2999, -3000 + 4095), 2000, replace=False)
        k = np.concatenate([[-3000, -3000 + 4095], mid])
    elif name == "span4097":  # one key too wide for the direct form
        k = np.concatenate([[5, 5 + 4096], rng.choice(np.arange(6, 4000), 900, replace=False)])
    elif name == "wide5000":
        k = np.unique(np.concatenate([[I32_MIN, I32_MAX], rng.integers(I32_MIN, I32_MAX, 4998)]))
    elif name == "big":  # 2^17 rows
        k = np.unique(rng.integers(-(10 ** 9), 10 ** 9, (1 << 17) + 4096))[: 1 << 17]
    elif name == "cluster":  # 300 keys, one home slot in the middle of the table
        k, extra = _cluster(500)
    elif name == "cluster_last":  # home is the last slot: the probe wraps around
        k, extra = _cluster(1023)
    else:
        raise KeyError(name)
    k = np.asarray(k, np.int64)
    assert len(np.unique(k)) == len(k)
    k = k[rng.permutation(len(k))]  # right rows are in no key order
    k.setflags(write=False)
    return k, extra


EXPECTED_FORM = {"empty": HASH, "one": DIRECT, "span4096": DIRECT, "span4097": HASH, "wide5000": HASH, "big": HASH,
                 "cluster": HASH, "cluster_last": HASH}


@functools.lru_cache(maxsize=None)
def right_columns(name):
    k, _ = right_keys(name)
    m = len(k)
    r = np.arange(m, dtype=np.int64)
    cols = {
        "rk": k.astype(np.int32),
        "rr": (((r * 37) % 1025 - 512) / 8.0).astype(np.float32),
        "ri": ((r * 7919) % 100003 - 50000).astype(np.int32),
        "rd": ((r * 13) % 4099 / 4.0 - 300.0).astype(np.float64),
        "rl": ((r * 104729) % (1 << 22) - (1 << 21)).astype(np.int64),
    }
    for c in cols.values():
        c.setflags(write=False)
    return cols


@functools.lru_cache(maxsize=None)
def right_table(name, offset=0):
    return dev_table(right_columns(name), offset)


@functools.lru_cache(maxsize=None)
def left_columns(n, rname, hit_mode, key_shift=0):
    """kk + key_shift: the left key; va: a value; pp: 1 where the WHERE keeps the row.
    hit_mode all / none / mix: which of the passing rows find their key.  Dropped rows carry absent keys."""
    rng = np.random.default_rng(4000 + n % 9973)
    keys, extra = right_keys(rname)
    present = np.sort(keys)
    lo, hi = (int(present[0]), int(present[-1])) if len(present) else (0, 0)
    absent = [I32_MIN, I32_MAX, lo - 1, hi + 1, lo - 4096, hi + 4096]
    if len(present) > 1:
        gaps = np.setdiff1d(np.arange(lo, min(hi, lo + 8192)), present)
        absent += list(gaps[:64])
    if extra is not None:
        absent += list(extra)  # the same home slot as the cluster's members, but not in the table
    absent = np.array([a for a in absent if I32_MIN + key_shift <= a <= I32_MAX], np.int64)  # kk stays an int32
    absent = np.setdiff1d(absent, present)
    assert len(absent)
    p = (rng.random(n) < 0.7).astype(np.float32)
    miss = absent[rng.integers(0, len(absent), n)]
    if len(present) and hit_mode != "none":
        hitk = present[rng.integers(0, len(present), n)]
        if n >= 2:
            hitk[0], hitk[-1] = present[0], present[-1]
        take = np.ones(n, bool) if hit_mode == "all" else rng.random(n) < 0.7
        k = np.where(take, hitk, miss)
    else:
        k = miss
    k = np.where(p < 0.5, absent[np.arange(n) % len(absent)], k)
    kk = k - key_shift
    assert np.all((kk >= I32_MIN) & (kk <= I32_MAX))
    cols = {"kk": kk.astype(np.int32), "va": (rng.integers(-8192, 8193, n) / 8.0).astype(np.float32), "pp": p}
    for c in cols.values():
        c.setflags(write=False)
    return cols


@functools.lru_cache(maxsize=None)
def left_table(n, rname, hit_mode, key_shift=0, offset=0):
    return dev_table(left_columns(n, rname, hit_mode, key_shift), offset)


# expressions: lowered text -> (numpy over the left columns and the matched right rows, names a right column)
EXPRS = {
    "va[idx]": (lambda l, r: l["va"], False),
    "kk[idx]": (lambda l, r: l["kk"].astype(np.float32), False),
    "(va[idx] + 1.0f)": (lambda l, r: l["va"] + np.float32(1), False),
    "rr[idx]": (lambda l, r: r["rr"], True),
    "ri[idx]": (lambda l, r: r["ri"].astype(np.float32), True),
    "rd[idx]": (lambda l, r: r["rd"].astype(np.float32), True),
    "rl[idx]": (lambda l, r: r["rl"].astype(np.float32), True),
    "(va[idx] * rr[idx])": (lambda l, r: l["va"] * r["rr"], True),
    "(rr[idx] + 0.5f)": (lambda l, r: r["rr"] + np.float32(0.5), True),
}


def expected(lcols, rcols, exprs, join_type, cond=COND, key_shift=0):
    """(values per output, left row ids, matched right rows) by numpy."""
    lk = lcols["kk"].astype(np.int64) + key_shift
    order = np.argsort(rcols["rk"], kind="stable")
    skeys = rcols["rk"][order].astype(np.int64)
    m = len(skeys)
    pos = np.searchsorted(skeys, lk)
    hit = (pos < m) & (skeys[np.minimum(pos, max(m - 1, 0))] == lk) if m else np.zeros(len(lk), bool)
    rrow = np.where(hit, order[np.minimum(pos, max(m - 1, 0))] if m else 0, 0)
    # an unmatched row binds 0 for every right column
    at = {c: np.where(hit, v[rrow] if m else 0, 0).astype(v.dtype) for c, v in rcols.items()}
    keep = lcols["pp"] > 0.5
    if cond == COND_R:
        keep = keep & hit & (at["rr"] > 0)
    elif join_type == INNER:
        keep = keep & hit
    outs = []
    for e in exprs:
        fn, right = EXPRS[e]
        v = np.asarray(fn(lcols, at), np.float32).copy()
        if right:
            v[~hit] = np.float32(np.nan)
        outs.append(v[keep])
    return outs, np.nonzero(keep)[0].astype(np.int64), np.where(hit, rrow, -1)[keep].astype(np.int32)


def run(lt, rt, exprs, join_type=INNER, cond=COND, key="kk[idx]", offset=0, ids=8, row_base=0, null=(), rrow=True,
        d_count=False):
    """One call.  Returns (count, [full value buffers incl. the offset slack], id buffer, right-row buffer)."""
    n = lt.n_rows
    bufs = [torch.full((n + offset + 1,), float("nan"), dtype=torch.float32, device="cuda") for _ in exprs]
    idx = torch.full((n + offset + 1,), -1, dtype=torch.int64 if ids == 8 else torch.int32, device="cuda") if ids else None
    rr = torch.full((n + offset + 1,), -7, dtype=torch.int32, device="cuda") if rrow else None
    dc = torch.full((1,), -5, dtype=torch.int64, device="cuda") if d_count else None
    ptrs = [0 if j in null else b[offset:].data_ptr() for j, b in enumerate(bufs)]
    cnt = wx.join_select(lt, rt, key, "rk", exprs, cond, launch(), ptrs, join_type=join_type,
                         d_out_idx=idx[offset:].data_ptr() if ids else 0, idx_bytes=ids or 8, row_base=row_base,
                         d_out_right_row=rr[offset:].data_ptr() if rrow else 0,
                         d_count=dc.data_ptr() if d_count else 0, want_count=True)
    if d_count:
        assert int(dc.item()) == cnt
    return (cnt, [b.cpu().numpy() for b in bufs], None if idx is None else idx.cpu().numpy(),
            None if rr is None else rr.cpu().numpy())


def check(n, rname, hit_mode, exprs, join_type=INNER, cond=COND, key="kk[idx]", key_shift=0, offset=0, ids=8, row_base=0,
          null=(), rrow=True, d_count=False, table_offset=0):
    lt, _ = left_table(n, rname, hit_mode, key_shift, table_offset)
    rt, _ = right_table(rname, table_offset)
    cnt, bufs, idx, rr = run(lt, rt, exprs, join_type, cond, key, offset, ids, row_base, null, rrow, d_count)
    want, rows, rrows = expected(left_columns(n, rname, hit_mode, key_shift), right_columns(rname), exprs, join_type, cond,
                                 key_shift)
    assert cnt == len(rows)
    sent = bits(np.float32(np.nan))
    for j, (b, w) in enumerate(zip(bufs, want)):
        u = bits(b)
        if j in null:
            assert np.all(u == sent)
            continue
        assert np.array_equal(u[offset:offset + cnt], bits(w)), (j, exprs[j])
        assert np.all(u[:offset] == sent) and np.all(u[offset + cnt:] == sent), "written outside [0, count)"
    if idx is not None:
        assert np.array_equal(idx[offset:offset + cnt], (rows + row_base).astype(idx.dtype))
        assert np.all(idx[:offset] == -1) and np.all(idx[offset + cnt:] == -1)
    if rr is not None:
        assert np.array_equal(rr[offset:offset + cnt], rrows)
        assert np.all(rr[:offset] == -7) and np.all(rr[offset + cnt:] == -7)
    return cnt


def assert_form(rname, monkeypatch=None):
    k, _ = right_keys(rname)
    form, log2cap = wx.join_plan(len(k), int(k.min()) if len(k) else 0, int(k.max()) if len(k) else 0)
    if monkeypatch is None:
        assert form == EXPECTED_FORM[rname]
    else:
        assert form == HASH
    if form == HASH:
        assert (1 << log2cap) >= max(64, 2 * len(k)) and (1 << log2cap) < max(128, 4 * len(k))
    return form


AB = ["va[idx]", "rr[idx]"]


def test_hash_slot_model():
    rng = np.random.default_rng(3)
    keys = np.concatenate([[I32_MIN, I32_MAX, 0, -1, 1], rng.integers(I32_MIN, I32_MAX, 200)])
    for log2cap in (6, 10, 18, 27):
        got = np.array([wx.join_hash_slot(int(k), log2cap) for k in keys])
        assert np.array_equal(got, home_slots(keys, log2cap))
    for name, slot in (("cluster", 500), ("cluster_last", 1023)):
        k, extra = right_keys(name)
        assert wx.join_plan(len(k), int(k.min()), int(k.max())) == (HASH, 10)
        assert {wx.join_hash_slot(int(x), 10) for x in np.concatenate([k, extra])} == {slot}


def _sizes(form, nout=2, rrow=True):
    tile = wx.join_tile_rows(nout, form, rrow)
    assert tile > 0
    return [0, 1, tile - 1, tile, tile + 1, 3 * tile + 5, 40 * tile + 17]


@pytest.mark.parametrize("sched", ["deep", "ticket"])
@pytest.mark.parametrize("join_type", [INNER, LEFT])
@pytest.mark.parametrize("rname", ["span4096", "span4097"])
def test_left_sizes(rname, join_type, sched, monkeypatch):
    monkeypatch.delenv("WARPDB_JOIN_FORM", raising=False)
    monkeypatch.setenv("WARPDB_COMPACT_SCHED", sched)
    form = assert_form(rname)
    for n in _sizes(form):
        assert n <= 1 << 20
        check(n, rname, "mix", AB, join_type)


@pytest.mark.parametrize("join_type", [INNER, LEFT])
@pytest.mark.parametrize("hit_mode", ["all", "none", "mix"])
@pytest.mark.parametrize("rname", ["empty", "one", "span4096", "span4097", "wide5000", "cluster", "cluster_last"])
def test_right_tables(rname, hit_mode, join_type, monkeypatch):
    monkeypatch.delenv("WARPDB_JOIN_FORM", raising=False)
    monkeypatch.delenv("WARPDB_COMPACT_SCHED", raising=False)
    form = assert_form(rname)
    n = 3 * wx.join_tile_rows(2, form, True) + 5
    cnt = check(n, rname, hit_mode, AB, join_type)
    if join_type == INNER and (hit_mode == "none" or rname == "empty"):
        assert cnt == 0
    if join_type == LEFT:
        assert cnt == int((left_columns(n, rname, hit_mode)["pp"] > 0.5).sum())  # a LEFT join drops no row cond keeps


@pytest.mark.parametrize("join_type", [INNER, LEFT])
@pytest.mark.parametrize("rname", ["one", "span4096"])
def test_direct_capable_tables_in_the_hash_form(rname, join_type, monkeypatch):
    monkeypatch.setenv("WARPDB_JOIN_FORM", "hash")
    assert_form(rname, monkeypatch)
    n = 3 * wx.join_tile_rows(2, HASH, True) + 5
    for hit_mode in ("all", "none", "mix"):
        check(n, rname, hit_mode, AB, join_type)


@pytest.mark.parametrize("sched", ["deep", "ticket"])
def test_largest_case(sched, monkeypatch):
    """2^20 left rows against 2^17 right rows."""
    monkeypatch.delenv("WARPDB_JOIN_FORM", raising=False)
    monkeypatch.setenv("WARPDB_COMPACT_SCHED", sched)
    assert assert_form("big") == HASH
    check(1 << 20, "big", "mix", AB, LEFT)
    check(1 << 20, "big", "mix", AB, INNER)


@pytest.mark.parametrize("join_type", [INNER, LEFT])
@pytest.mark.parametrize("rname", ["span4096", "wide5000"])
def test_cond_over_a_right_column_keeps_matched_rows_only(rname, join_type, monkeypatch):
    monkeypatch.delenv("WARPDB_JOIN_FORM", raising=False)
    n = 2 * wx.join_tile_rows(2, EXPECTED_FORM[rname], True) + 3
    lt, _ = left_table(n, rname, "mix")
    rt, _ = right_table(rname)
    cnt, _, _, rr = run(lt, rt, AB, join_type, COND_R)
    assert cnt > 0 and np.all(rr[:cnt] >= 0)
    check(n, rname, "mix", AB, join_type, COND_R)


OUTPUT_LISTS = [
    ["rr[idx]"],
    ["va[idx]", "rr[idx]", "kk[idx]"],
    ["rr[idx]", "ri[idx]", "rd[idx]", "rl[idx]"],  # every right column type
    ["va[idx]", "rr[idx]", "(va[idx] * rr[idx])", "ri[idx]", "(va[idx] + 1.0f)", "(rr[idx] + 0.5f)"],  # two launches
]


@pytest.mark.parametrize("rrow", [True, False])
@pytest.mark.parametrize("rname", ["span4096", "wide5000"])
@pytest.mark.parametrize("exprs", OUTPUT_LISTS, ids=lambda e: str(len(e)))
def test_output_counts_and_types(exprs, rname, rrow, monkeypatch):
    monkeypatch.delenv("WARPDB_JOIN_FORM", raising=False)
    monkeypatch.delenv("WARPDB_COMPACT_SCHED", raising=False)
    form = EXPECTED_FORM[rname]
    n = 2 * wx.join_tile_rows(min(len(exprs), 4), form, rrow) + 7
    check(n, rname, "mix", exprs, LEFT, rrow=rrow)
    check(n, rname, "mix", exprs, INNER, rrow=rrow, d_count=True)


@pytest.mark.parametrize("sched", ["deep", "ticket"])
def test_ids_nulls_and_offsets(sched, monkeypatch):
    monkeypatch.delenv("WARPDB_JOIN_FORM", raising=False)
    monkeypatch.setenv("WARPDB_COMPACT_SCHED", sched)
    exprs = OUTPUT_LISTS[1]
    n = 3 * wx.join_tile_rows(3, HASH, True) + 5
    check(n, "wide5000", "mix", exprs, LEFT, ids=4, row_base=1000)
    check(n, "wide5000", "mix", exprs, LEFT, ids=8, row_base=(1 << 40) + 3)
    check(n, "wide5000", "mix", exprs, LEFT, ids=0)
    check(n, "wide5000", "mix", exprs, INNER, null=(0, 2))
    check(n, "wide5000", "mix", exprs, INNER, null=(0, 1, 2), rrow=False)
    for offset in (1, 3):  # misaligned outputs and misaligned columns
        check(n, "wide5000", "mix", exprs, LEFT, offset=offset, ids=4)
        check(n, "wide5000", "mix", exprs, LEFT, offset=offset, table_offset=offset)
    check(n, "wide5000", "mix", OUTPUT_LISTS[3], LEFT, offset=1, null=(4,))  # the second launch too


@pytest.mark.parametrize("rname", ["span4096", "span4097"])
def test_mixed_expression_and_key_expression(rname, monkeypatch):
    monkeypatch.delenv("WARPDB_JOIN_FORM", raising=False)
    n = 2 * wx.join_tile_rows(1, EXPECTED_FORM[rname], True) + 9
    for join_type in (INNER, LEFT):
        check(n, rname, "mix", ["(va[idx] * rr[idx])"], join_type)
        check(n, rname, "mix", ["(va[idx] * rr[idx])"], join_type, key="(kk[idx] + 1)", key_shift=1)


@pytest.mark.parametrize("force_hash", [False, True])
def test_duplicate_right_key_is_refused(force_hash, monkeypatch):
    monkeypatch.delenv("WARPDB_JOIN_FORM", raising=False)
    if force_hash:
        monkeypatch.setenv("WARPDB_JOIN_FORM", "hash")
    rc = {k: v.copy() for k, v in right_columns("span4096").items()}
    dup = int(rc["rk"][17])
    rc["rk"][1234] = dup
    rt, _ = dev_table(rc)
    n = 1000
    lt, _ = left_table(n, "span4096", "mix")
    for _ in range(2):
        with pytest.raises(wx.WarpExecError, match=rf"JOIN: the right key is not unique \(key {dup}\)") as ei:
            run(lt, rt, AB)
        assert ei.value.status == wx.WX_ERR_UNSUPPORTED
    check(n, "span4096", "mix", AB, LEFT)  # the next call on the same workspace succeeds
    # a wide table with a duplicate takes the hash form by itself
    rc = {k: v.copy() for k, v in right_columns("wide5000").items()}
    dup = int(rc["rk"][4000])
    rc["rk"][5] = dup
    rt, _ = dev_table(rc)
    with pytest.raises(wx.WarpExecError, match=rf"not unique \(key {dup}\)") as ei:
        run(lt, rt, AB)
    assert ei.value.status == wx.WX_ERR_UNSUPPORTED
    check(n, "wide5000", "mix", AB, INNER)


# ------------------------------------------------------------------ facade
# price, quantity: (10.5, 3), (20, 4), (15.25, 2), (30, 5)
TEST_CSV = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test.csv")


def _write_csv(path, cols):
    with open(path, "w") as f:
        f.write(",".join(cols) + "\n")
        for row in zip(*cols.values()):
            f.write(",".join(repr(x.item()) for x in row) + "\n")


def test_facade_on_test_csv(tmp_path):
    from warpdb_amd import pywarpdb as pw

    D = pw.DataType
    right = tmp_path / "dim.csv"
    right.write_text("id,rate,price\n4,0.5,100\n3,0.25,200\n9,2.0,300\n")
    db = pw.WarpDB(TEST_CSV)
    with pytest.raises(RuntimeError, match=r"Unknown table: u \(attach it first\)"):
        db.query_sql_joined("SELECT price FROM t JOIN u ON quantity = u.id")
    db.attach("u", str(right), [D.Int32, D.Float32, D.Float32])
    nan = float("nan")
    # inner: rows 0 and 1 match (quantity 3 and 4), in left row order
    names, cols, rows, rrows = db.query_sql_joined("SELECT t.price, rate, t.price * rate, u.price FROM t JOIN u "
                                                   "ON quantity = u.id")
    assert names == ["price", "rate", "expr2", "price"]
    assert rows.tolist() == [0, 1] and rrows.tolist() == [1, 0]
    assert [c.tolist() for c in cols] == [[10.5, 20.0], [0.25, 0.5], [2.625, 10.0], [200.0, 100.0]]
    # left outer: every row WHERE keeps; right-side items are NaN where nothing matched
    names, cols, rows, rrows = db.query_sql_joined("SELECT t.price, rate FROM t LEFT OUTER JOIN u ON u.id = quantity "
                                                   "WHERE t.price > 15")
    assert rows.tolist() == [1, 2, 3] and rrows.tolist() == [0, -1, -1]
    assert cols[0].tolist() == [20.0, 15.25, 30.0]
    assert bits(cols[1]).tolist() == bits(np.array([0.5, nan, nan], np.float32)).tolist()
    # a WHERE over a right column keeps matched rows only; LIMIT / OFFSET over the result rows
    _, cols, rows, rrows = db.query_sql_joined("SELECT rate FROM t LEFT JOIN u ON quantity = u.id WHERE rate > 0.3")
    assert rows.tolist() == [1] and rrows.tolist() == [0] and cols[0].tolist() == [0.5]
    _, cols, rows, rrows = db.query_sql_joined("SELECT quantity FROM t LEFT JOIN u ON quantity = u.id LIMIT 2 OFFSET 1")
    assert rows.tolist() == [1, 2] and rrows.tolist() == [0, -1] and cols[0].tolist() == [4.0, 2.0]
    _, cols, rows, _ = db.query_sql_joined("SELECT quantity FROM t INNER JOIN u ON quantity + 5 = u.id")
    assert rows.tolist() == [1] and cols[0].tolist() == [4.0]  # 4 + 5 = 9
    # query_join: the same from its parts
    names, cols, rows, rrows = db.query_join("u", "quantity", "id", ["quantity", "rate * 2", "u.price"], "", True)
    assert names == ["quantity", "expr1", "price"] and rows.tolist() == [0, 1, 2, 3] and rrows.tolist() == [1, 0, -1, -1]
    assert bits(cols[1]).tolist() == bits(np.array([0.5, 1.0, nan, nan], np.float32)).tolist()
    names, cols, rows, rrows = db.query_join("u", "quantity", "u.id", ["rate"], "quantity > 3")
    assert rows.tolist() == [1] and rrows.tolist() == [0] and cols[0].tolist() == [0.5]
    # refusals: the planner's, the engine's, and the other entry points' own
    with pytest.raises(RuntimeError, match="Ambiguous column: price"):
        db.query_sql_joined("SELECT price FROM t JOIN u ON quantity = u.id")
    with pytest.raises(RuntimeError, match="JOIN condition must be <left expression> = <right column>"):
        db.query_sql_joined("SELECT rate FROM t JOIN u ON quantity > u.id")
    with pytest.raises(RuntimeError, match="right_key_col must be a bare INT32 column"):
        db.query_sql_joined("SELECT t.price FROM t JOIN u ON quantity = rate")
    with pytest.raises(RuntimeError, match="GROUP BY is not supported by query_sql_joined"):
        db.query_sql_joined("SELECT rate FROM t JOIN u ON quantity = u.id GROUP BY rate")
    with pytest.raises(RuntimeError, match="Unknown table: v"):
        db.query_join("v", "quantity", "id", ["rate"])
    with pytest.raises(RuntimeError, match="JOIN is not supported by the execution engine"):
        db.query_sql_table("SELECT price, quantity FROM t JOIN u ON quantity = price")
    dup = tmp_path / "dup.csv"
    dup.write_text("id,rate\n4,0.5\n3,0.25\n4,2.0\n")
    db.attach("u", str(dup), [D.Int32, D.Float32])  # attaching again replaces the table
    with pytest.raises(RuntimeError, match=r"JOIN: the right key is not unique \(key 4\)"):
        db.query_sql_joined("SELECT rate FROM t JOIN u ON quantity = u.id")


def test_facade_vs_numpy(tmp_path):
    from warpdb_amd import pywarpdb as pw

    D = pw.DataType
    n = 20_011
    lcols, rcols = left_columns(n, "span4097", "mix"), {k: right_columns("span4097")[k] for k in ("rk", "rr", "ri")}
    _write_csv(tmp_path / "fact.csv", lcols)
    _write_csv(tmp_path / "dim.csv", rcols)
    db = pw.WarpDB(str(tmp_path / "fact.csv"), [D.Int32, D.Float32, D.Float32], 0)
    db.attach("dim", str(tmp_path / "dim.csv"), [D.Int32, D.Float32, D.Int32])
    exprs = ["va[idx]", "rr[idx]", "(va[idx] * rr[idx])", "ri[idx]", "kk[idx]"]
    for how, jt in (("JOIN", INNER), ("LEFT JOIN", LEFT)):
        names, cols, rows, rrows = db.query_sql_joined(f"SELECT va, rr, va * rr, ri, kk FROM t {how} dim ON kk = rk "
                                                       "WHERE pp > 0.5")
        want, wrows, wrrows = expected(lcols, right_columns("span4097"), exprs, jt)
        assert names == ["va", "rr", "expr2", "ri", "kk"]
        assert np.array_equal(rows, wrows) and np.array_equal(rrows, wrrows.astype(np.int64))
        for got, w in zip(cols, want):
            assert np.array_equal(bits(got), bits(w))
        names, cols, rows, rrows = db.query_sql_joined(f"SELECT rr FROM t {how} dim ON kk = rk WHERE pp > 0.5 "
                                                       "LIMIT 100 OFFSET 50")
        assert np.array_equal(rows, wrows[50:150]) and np.array_equal(bits(cols[0]), bits(want[1][50:150]))
        assert np.array_equal(rrows, wrrows[50:150].astype(np.int64))
