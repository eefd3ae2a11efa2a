"""CPU tests of the JOIN under GROUP BY (wx_join_group_agg, wx_join_group.hip):
the ABI is exported and parses as C11, the module compiles for gfx950 in both
forms, for one to four values, every mask kind and every column type without
a device, the geometry fits the LDS, the argument checks fire before any
device call, and the planner answers tests/golden/join_group_errors.tsv."""
from __future__ import annotations

import os
import subprocess

import pytest

from warpdb_amd import _warpexec as wx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INNER, LEFT, DIRECT, HASH = wx.JOIN_INNER, wx.JOIN_LEFT, wx.JOIN_DIRECT, wx.JOIN_HASH
LDS = 160 * 1024


def table(n=1 << 20, **cols):
    dt = {"f32": wx.FLOAT32, "i32": wx.INT32, "f64": wx.FLOAT64, "i64": wx.INT64, "str": wx.STRING}
    return wx.Table(n, [wx.Column(k, dt[v], (i + 1) << 20) for i, (k, v) in enumerate(cols.items())])


def no_custom(flags=0):
    return wx.make_launch(flags=wx.F_NO_CUSTOM | flags)


def fact():
    return table(price="f32", quantity="i32", cust="i32", wide="f64", big="i64")


def dim():
    return table(1000, id="i32", rate="f32", tier="i32", credit="f64", since="i64", label="str")


def test_symbols():
    lib = wx.load()
    for name in ("wx_join_group_agg", "wx_prepare_join_group", "wx_join_group_geometry"):
        assert hasattr(lib, name) and name in wx.EXPORTED_SYMBOLS
    assert lib.wx_abi_version() == 1


def test_header_parses_as_c11(tmp_path):
    c = tmp_path / "use.c"
    c.write_text('#include "warpexec.h"\n'
                 "int probe(const wx_table *l, const wx_table *r, const char *const *e, double *const *s,\n"
                 "          float *const *f, int32_t *k, int64_t *c) {\n"
                 "  int32_t block = 0, per_cu = 0, lds = 0;\n"
                 "  return (int)wx_join_group_agg(l, r, \"k\", \"id\", WX_JOIN_INNER, e, WX_GROUP_MAX_VALUES, \"g\", 0, 0,\n"
                 "                                0, 16, k, s, c, f, f, 0, c, 0, 0)\n"
                 "       + (int)wx_prepare_join_group(l, r, \"k\", \"id\", WX_JOIN_INNER, e, 2, 3u, 1u, \"g\", 0, 0, 1, 0, 0)\n"
                 "       + (int)wx_join_group_geometry(4, 4, 0, &block, &per_cu, &lds, 0, 0);\n}\n")
    r = subprocess.run(["cc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "include"), str(c)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


VALUES = ["(price[idx] * rate[idx])", "price[idx]", "credit[idx]", "(price[idx] + 1.0f)"]
# (sum mask, min/max mask) over 1 .. 4 values: sum-only, min/max-only, mixed
MASKS = {1: [(1, 0), (0, 1), (1, 1)], 2: [(3, 0), (0, 3), (1, 2)], 3: [(7, 0), (0, 7), (5, 6)],
         4: [(15, 0), (0, 15), (11, 12), (15, 15)]}


@pytest.mark.parametrize("n_vals", [1, 2, 3, 4])
@pytest.mark.parametrize("form", [DIRECT, HASH])
def test_prepare_compiles(form, n_vals):
    """Every mask kind; the WHERE alternates between none, left-only and one naming a right column."""
    conds = [None, "(price[idx] > 15.0f)", "(price[idx] > 15.0f && rate[idx] > 0.5f)"]
    for i, (sm, mm) in enumerate(MASKS[n_vals]):
        wx.prepare_join_group(fact(), dim(), "cust[idx]", "id", VALUES[:n_vals], sm, mm, "tier[idx]", conds[i % 3],
                              no_custom(), form)


@pytest.mark.parametrize("form", [DIRECT, HASH])
def test_prepare_every_column_type(form):
    # left f32 / i32 / f64 / i64 as values and in the key expressions; right columns of every type
    wx.prepare_join_group(fact(), dim(), "(cust[idx] + 1)", " id ",
                          ["price[idx]", "quantity[idx]", "wide[idx]", "big[idx]"], 0b0101, 0b1010,
                          "(tier[idx] * 100 + quantity[idx])", "(wide[idx] > 1.0)", no_custom(), form)
    wx.prepare_join_group(fact(), dim(), "(int)big[idx]", "id",
                          ["rate[idx]", "tier[idx]", "credit[idx]", "since[idx]"], 0b1111, 0b0110, "credit[idx]",
                          "(since[idx] > 5 && credit[idx] > 1.0)", no_custom(), form)
    wx.prepare_join_group(fact(), dim(), "cust[idx]", "id", ["((float)since[idx] + credit[idx])"], 1, 0, "since[idx]",
                          None, no_custom(), form)


def test_prepare_is_cached_and_reports_compile_errors():
    before = wx.cache_stats()[0]
    for _ in range(2):
        wx.prepare_join_group(fact(), dim(), "cust[idx]", "id", ["(price[idx] - 7.0f)"], 1, 1, "tier[idx]", None,
                              no_custom(), HASH)
    assert wx.cache_stats()[0] - before <= 2  # the build module and the grouped pass, compiled once
    with pytest.raises(wx.WarpExecError) as ei:
        wx.prepare_join_group(fact(), dim(), "cust[idx]", "id", ["invalid@"], 1, 0, "tier[idx]", None, no_custom())
    assert ei.value.status == wx.WX_ERR_COMPILE


def test_geometry():
    for form in (DIRECT, HASH):
        for s in range(5):
            for q in range(5):
                if s + q == 0:
                    continue
                block, per_cu, lds = wx.join_group_geometry(s, q, form)
                assert lds == 2048 * (4 + 8 * (s + q)) + (16 * 1024 if form == DIRECT else 0)
                assert per_cu * lds <= LDS
                assert (block, per_cu) in ((512, 2), (1024, 1)) and block * per_cu == 1024  # 16 waves per CU
                # two workgroups per CU wherever two fit
                assert per_cu == (2 if 2 * lds <= LDS else 1)
    # where the block size switches: S + Q = 4 still fits twice without the direct table, not with it
    assert wx.join_group_geometry(2, 1, DIRECT)[:2] == (512, 2)
    assert wx.join_group_geometry(2, 2, DIRECT)[:2] == (1024, 1)
    assert wx.join_group_geometry(2, 2, HASH)[:2] == (512, 2)
    assert wx.join_group_geometry(3, 2, HASH)[:2] == (1024, 1)
    assert wx.join_group_geometry(4, 4, DIRECT) == (1024, 1, 152 * 1024)  # the widest build
    for args in ((0, 0, 0), (5, 0, 0), (0, 5, 1), (-1, 1, 0), (1, 1, 2), (1, 1, -1)):
        with pytest.raises(wx.WarpExecError) as ei:
            wx.join_group_geometry(*args)
        assert ei.value.status == wx.WX_ERR_INVALID


def _run(left, right, vals, key="cust[idx]", rkey="id", gkey="tier[idx]", cond=None, join_type=INNER, flags=0,
         sums=True, mins=False):
    # device pointers are never dereferenced: every case fails its argument check first
    fake = [1 << 30] * len(vals)
    return wx.join_group_agg(left, right, key, rkey, vals, gkey, cond, no_custom(flags), 0, 16, 1 << 30, 1 << 30,
                             d_sums=fake if sums else None, d_mins=fake if mins else None, join_type=join_type)


def _both(match, status, left, right, vals, **kw):
    """The run path and the prepare path refuse alike."""
    with pytest.raises(wx.WarpExecError, match=match) as ei:
        _run(left, right, vals, **kw)
    assert ei.value.status == status
    n = len(vals)
    with pytest.raises(wx.WarpExecError, match=match) as ei:
        wx.prepare_join_group(left, right, kw.get("key", "cust[idx]"), kw.get("rkey", "id"), vals, (1 << n) - 1, 0,
                              kw.get("gkey", "tier[idx]"), kw.get("cond"), no_custom(), HASH,
                              kw.get("join_type", INNER))
    assert ei.value.status == status


def test_argument_checks_need_no_device():
    f, d = fact(), dim()
    one = ["rate[idx]"]
    for vals in ([], ["price[idx]"] * 5):
        _both("n_vals must be between 1 and 4", wx.WX_ERR_INVALID, f, d, vals)
    for vals, key, gkey in ((["  "], "cust[idx]", "tier[idx]"), (["price[idx]", None], "cust[idx]", "tier[idx]"),
                            (one, "  ", "tier[idx]"), (one, None, "tier[idx]"), (one, "cust[idx]", " "),
                            (one, "cust[idx]", None)):
        _both("Empty query expression", wx.WX_ERR_INVALID, f, d, vals, key=key, gkey=gkey)
    # a value with nothing requested
    with pytest.raises(wx.WarpExecError, match="value 0 has no aggregate requested") as ei:
        _run(f, d, one, sums=False)
    assert ei.value.status == wx.WX_ERR_INVALID
    with pytest.raises(wx.WarpExecError, match="value 1 has no aggregate requested") as ei:
        wx.prepare_join_group(f, d, "cust[idx]", "id", ["price[idx]", "rate[idx]"], 1, 0, "tier[idx]", None, no_custom())
    assert ei.value.status == wx.WX_ERR_INVALID
    with pytest.raises(wx.WarpExecError, match="beyond n_vals") as ei:
        wx.prepare_join_group(f, d, "cust[idx]", "id", one, 3, 0, "tier[idx]", None, no_custom())
    assert ei.value.status == wx.WX_ERR_INVALID
    # a column of both tables, wherever it is named
    both = table(1000, id="i32", price="f32", tier="i32")
    _both("column price is in both tables", wx.WX_ERR_INVALID, f, both, ["price[idx]"])
    _both("column price is in both tables", wx.WX_ERR_INVALID, f, both, ["quantity[idx]"], gkey="(int)price[idx]")
    _both("column price is in both tables", wx.WX_ERR_INVALID, f, both, ["quantity[idx]"], cond="(price[idx] > 1.0f)")
    _both("column price is in both tables", wx.WX_ERR_INVALID, f, both, ["quantity[idx]"], key="(int)price[idx]")
    # the left key names left columns only; the right key is a bare INT32 column of the right table
    _both("left_key_expr names the right column tier", wx.WX_ERR_INVALID, f, d, one, key="(cust[idx] + tier[idx])")
    for rkey in ("rate", "since", "nothere", "cust", "(id + 1)", "id[idx]", "", None):
        _both("right_key_col must be a bare INT32 column of the right table", wx.WX_ERR_INVALID, f, d, one, rkey=rkey)
    for jt in (-1, 2):
        _both("join_type", wx.WX_ERR_INVALID, f, d, one, join_type=jt)
    _both(r"LEFT JOIN under GROUP BY is not supported \(an unmatched row needs NULL-aware aggregates\)",
          wx.WX_ERR_UNSUPPORTED, f, d, one, join_type=LEFT)
    _both("cannot evaluate", wx.WX_ERR_UNSUPPORTED, f, d, ["label[idx]"])
    _both("more than 67108864 rows", wx.WX_ERR_UNSUPPORTED, f, table((1 << 26) + 1, id="i32", rate="f32", tier="i32"),
          one)
    with pytest.raises(wx.WarpExecError, match="form must be") as ei:
        wx.prepare_join_group(f, d, "cust[idx]", "id", one, 1, 0, "tier[idx]", None, no_custom(), 2)
    assert ei.value.status == wx.WX_ERR_INVALID
    with pytest.raises(wx.WarpExecError, match="row-order") as ei:
        _run(f, d, one, flags=wx.F_ROW_ORDER)
    assert ei.value.status == wx.WX_ERR_UNSUPPORTED


def test_column_limit_is_per_table():
    lcols = {f"c{i}": "f32" for i in range(18)}
    rcols = {f"r{i}": "f32" for i in range(18)}
    f, d = table(k="i32", **lcols), table(1000, id="i32", **rcols)
    vals = ["(" + " + ".join(f"c{i}[idx]" for i in range(j, 15, 4)) + " + " +
            " + ".join(f"r{i}[idx]" for i in range(j, 16, 4)) + ")" for j in range(4)]
    wx.prepare_join_group(f, d, "k[idx]", "id", vals, 15, 0, "k[idx]", None, no_custom())  # 16 left, 16 right
    for cond in ("(c15[idx] > 0.0f)", "(r16[idx] > 0.0f)"):
        with pytest.raises(wx.WarpExecError, match="16 columns") as ei:
            wx.prepare_join_group(f, d, "k[idx]", "id", vals, 15, 0, "k[idx]", cond, no_custom())
        assert ei.value.status == wx.WX_ERR_UNSUPPORTED


def test_planner_binary():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "bin/join_group_plan_test"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "bin", "join_group_plan_test")], capture_output=True,
                       text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "join_group_plan_test: all passed" in r.stdout
