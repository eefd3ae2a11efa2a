"""CPU tests of the join family (wx_join_select, wx_join.hip): the ABI is
exported and parses as C11, its modules compile for gfx950 in both forms and
both join types without a device, the plan and the hash function are what the
header says, the probe tile shrinks with what shares the LDS with it, and the
argument checks fire before any device call."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

from warpdb_amd import _warpexec as wx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISCOUNT_SRC = "__device__ float discount(float price, float rate) {\n    return price * rate;\n}\n"
INNER, LEFT, DIRECT, HASH = wx.JOIN_INNER, wx.JOIN_LEFT, wx.JOIN_DIRECT, wx.JOIN_HASH
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def table(n=1 << 20, **cols):
    dt = {"f32": wx.FLOAT32, "i32": wx.INT32, "f64": wx.FLOAT64, "i64": wx.INT64, "str": wx.STRING}
    return wx.Table(n, [wx.Column(k, dt[v], (i + 1) << 20) for i, (k, v) in enumerate(cols.items())])


def no_custom(flags=0):
    return wx.make_launch(flags=wx.F_NO_CUSTOM | flags)


def fact():
    return table(price="f32", quantity="i32", cust="i32")


def dim():
    return table(1000, id="i32", rate="f32", tier="i32", credit="f64", since="i64", label="str")


def test_symbols():
    lib = wx.load()
    for name in ("wx_join_select", "wx_prepare_join", "wx_join_tile_rows", "wx_join_plan", "wx_join_hash_slot"):
        assert hasattr(lib, name) and name in wx.EXPORTED_SYMBOLS
    assert lib.wx_abi_version() == 1
    assert (INNER, LEFT, DIRECT, HASH) == (0, 1, 0, 1)


def test_header_parses_as_c11(tmp_path):
    c = tmp_path / "use.c"
    c.write_text('#include "warpexec.h"\n'
                 "int probe(const wx_table *l, const wx_table *r, const char *const *e, float *const *o, int32_t *rr) {\n"
                 "  int32_t form = 0, cap = 0;\n"
                 "  return (int)wx_join_select(l, r, \"k\", \"id\", WX_JOIN_LEFT, e, 2, 0, 0, o, 0, 8, 0, rr, 0, 0, 0, 0)\n"
                 "       + (int)wx_prepare_join(l, r, \"k\", \"id\", WX_JOIN_INNER, e, 2, 0, 0, 1, 1, 0, 0)\n"
                 "       + (int)wx_join_tile_rows(WX_MAX_OUTPUTS, 0, 1) + (int)wx_join_plan(5, 0, 9, &form, &cap, 0, 0)\n"
                 "       + (int)wx_join_hash_slot(7, 6);\n}\n")
    r = subprocess.run(["cc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "include"), str(c)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


OUTPUTS = ["price[idx]", "rate[idx]", "(price[idx] * rate[idx])", "tier[idx]"]


@pytest.mark.parametrize("rrow", [False, True])
@pytest.mark.parametrize("join_type", [INNER, LEFT])
@pytest.mark.parametrize("form", [DIRECT, HASH])
def test_prepare_compiles_both_forms_and_types(form, join_type, rrow):
    """1 .. 4 outputs, a mixed expression, and a condition over a right column."""
    for m in (1, 2, 3, 4):
        wx.prepare_join(fact(), dim(), "cust[idx]", "id", OUTPUTS[:m], "(price[idx] > 15.0f)" if m % 2 else None,
                        no_custom(), join_type, rrow, form)
    wx.prepare_join(fact(), dim(), "cust[idx]", "id", ["(price[idx] * rate[idx])"],
                    "(price[idx] > 15.0f && rate[idx] > 0.5f)", no_custom(), join_type, rrow, form)


@pytest.mark.parametrize("form", [DIRECT, HASH])
def test_prepare_every_right_column_type_and_key_expression(form):
    wx.prepare_join(fact(), dim(), "(cust[idx] + 1)", "id", ["rate[idx]", "tier[idx]", "credit[idx]", "since[idx]"],
                    None, no_custom(), LEFT, True, form)
    wx.prepare_join(fact(), dim(), "(int)price[idx]", " id ", ["((float)since[idx] + credit[idx])"],
                    "(credit[idx] > 1.0)", no_custom(), INNER, False, form)


def test_prepare_six_outputs_and_custom_function():
    six = OUTPUTS + ["(price[idx] + 1.0f)", "discount(price[idx], rate[idx])"]
    before = wx.cache_stats()[0]
    wx.prepare_join(fact(), dim(), "cust[idx]", "id", six, "(price[idx] > 15.0f)", wx.make_launch(custom_src=DISCOUNT_SRC),
                    LEFT, True, HASH)
    wx.prepare_join(fact(), dim(), "cust[idx]", "id", six, "(price[idx] > 15.0f)", wx.make_launch(custom_src=DISCOUNT_SRC),
                    LEFT, True, HASH)
    assert wx.cache_stats()[0] - before <= 3  # the build module and two probe launches, compiled once


def test_compile_error_is_reported():
    with pytest.raises(wx.WarpExecError) as ei:
        wx.prepare_join(fact(), dim(), "cust[idx]", "id", ["invalid@"], None, no_custom())
    assert ei.value.status == wx.WX_ERR_COMPILE


def test_tile_rows(monkeypatch):
    monkeypatch.delenv("WARPDB_EXTRA_DEFINES", raising=False)
    budget, table_bytes = 150 * 1024, 4096 * 4
    for form in (DIRECT, HASH):
        for rrow in (False, True):
            rows = [wx.join_tile_rows(m, form, rrow) for m in (1, 2, 3, 4)]
            for m, r in zip((1, 2, 3, 4), rows):
                assert r > 0 and r % 256 == 0
                # two stage buffers (4 B per output, 4 more with the right row, a 2-byte offset) beside the table
                assert r * 2 * (4 * (m + rrow) + 2) + (table_bytes if form == DIRECT else 0) <= budget
                assert r <= wx.select_tile_rows(m) or m == 1
            assert rows == sorted(rows, reverse=True) and rows[3] < rows[0]  # shrinks with the outputs
        for m in (1, 2, 3, 4):  # the right row costs 4 more bytes per staged row, the direct table 16 KiB
            assert wx.join_tile_rows(m, form, True) <= wx.join_tile_rows(m, form, False)
            assert wx.join_tile_rows(m, DIRECT, False) <= wx.join_tile_rows(m, HASH, False)
    # the hash form without the right row stages what the select kernel stages: its geometry
    assert [wx.join_tile_rows(m, HASH, False) for m in (2, 3, 4)] == [wx.select_tile_rows(m) for m in (2, 3, 4)]
    lib = wx.load()
    for args in ((0, 0, 0), (5, 0, 0), (-1, 1, 0), (2, 2, 0), (2, -1, 0), (2, 0, 2), (2, 1, -1)):
        assert lib.wx_join_tile_rows(*args) == 0, args
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_COMPACT_GROUPS=1,WX_COMPACT_DWAVES=2")
    assert wx.join_tile_rows(2, DIRECT, True) == wx.join_tile_rows(4, HASH, False) == 512
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_COMPACT_GROUPS=9")
    assert wx.join_tile_rows(2, HASH, False) == 0
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_COMPACT_GROUPS=8,WX_COMPACT_DWAVES=15")
    assert wx.join_tile_rows(4, DIRECT, True) == 0  # does not fit


def test_plan(monkeypatch):
    monkeypatch.delenv("WARPDB_JOIN_FORM", raising=False)
    assert wx.join_plan(10, -5, -5 + 4095) == (DIRECT, 0)  # span 4096
    assert wx.join_plan(10, -5, -5 + 4096)[0] == HASH      # span 4097
    assert wx.join_plan(2, I32_MIN, I32_MAX)[0] == HASH
    assert wx.join_plan(1, I32_MAX, I32_MAX) == (DIRECT, 0)
    assert wx.join_plan(4096, I32_MIN, I32_MIN + 4095) == (DIRECT, 0)
    for n in (0, 1, 31, 32, 33, 64, 65, 1000, 5000, (1 << 17), (1 << 17) + 1, 1 << 26):
        form, log2cap = wx.join_plan(n, 0, I32_MAX)
        assert form == HASH
        cap = 1 << log2cap
        assert cap >= 2 * n and cap >= 64 and (cap == 64 or cap // 2 < 2 * n)  # the smallest such power of two
    assert wx.join_plan(1 << 26, 0, I32_MAX) == (HASH, 27)
    with pytest.raises(wx.WarpExecError, match="more than 67108864 rows") as ei:
        wx.join_plan((1 << 26) + 1, 0, I32_MAX)
    assert ei.value.status == wx.WX_ERR_UNSUPPORTED
    with pytest.raises(wx.WarpExecError) as ei:
        wx.join_plan(-1, 0, 0)
    assert ei.value.status == wx.WX_ERR_INVALID
    with pytest.raises(wx.WarpExecError) as ei:
        wx.join_plan(5, 3, 2)
    assert ei.value.status == wx.WX_ERR_INVALID
    monkeypatch.setenv("WARPDB_JOIN_FORM", "hash")  # the test hook
    assert wx.join_plan(10, -5, 100) == (HASH, 6)
    assert wx.join_plan(2000, 0, 4095) == (HASH, 12)


def test_hash_slot():
    rng = np.random.default_rng(5)
    keys = [I32_MIN, I32_MAX, -1, 0, 1] + [int(k) for k in rng.integers(I32_MIN, I32_MAX, 500)]
    for log2cap in range(6, 28):
        for k in keys:
            s = wx.join_hash_slot(k, log2cap)
            assert 0 <= s < (1 << log2cap)
            assert s == (((k & 0xffffffff) * 0x9E3779B1) & 0xffffffff) >> (32 - log2cap)
    for log2cap in (-1, 0, 5, 28, 32):
        assert wx.join_hash_slot(7, log2cap) == -1


def _call(left, right, exprs, key="cust[idx]", rkey="id", join_type=INNER, cond=None, flags=0, idx=0, idx_bytes=8,
          row_base=0):
    # device pointers are never dereferenced: every case fails its argument check first
    return wx.join_select(left, right, key, rkey, exprs, cond, no_custom(flags), [1 << 30] * len(exprs),
                          join_type=join_type, d_out_idx=idx, idx_bytes=idx_bytes, row_base=row_base)


def _both(match, status, left, right, exprs, **kw):
    """The run path and the prepare path refuse alike."""
    with pytest.raises(wx.WarpExecError, match=match) as ei:
        _call(left, right, exprs, **kw)
    assert ei.value.status == status
    with pytest.raises(wx.WarpExecError, match=match) as ei:
        wx.prepare_join(left, right, kw.get("key", "cust[idx]"), kw.get("rkey", "id"), exprs, kw.get("cond"),
                        no_custom(), kw.get("join_type", INNER))
    assert ei.value.status == status


def test_argument_checks_need_no_device():
    f, d = fact(), dim()
    one = ["rate[idx]"]
    for exprs in ([], ["price[idx]"] * 17):
        _both("n_exprs must be between 1 and 16", wx.WX_ERR_INVALID, f, d, exprs)
    wx.prepare_join(f, d, "cust[idx]", "id", [f"(price[idx] + {j}.0f)" for j in range(16)], None, no_custom())
    for exprs, key in ((["  "], "cust[idx]"), (["price[idx]", None], "cust[idx]"), (one, "  "), (one, None)):
        _both("Empty query expression", wx.WX_ERR_INVALID, f, d, exprs, key=key)
    for jt in (-1, 2, 7):
        _both("join_type", wx.WX_ERR_INVALID, f, d, one, join_type=jt)
    # the right key: a bare INT32 column of the right table
    for rkey in ("rate", "since", "nothere", "cust", "(id + 1)", "id[idx]", "", None):
        _both("right_key_col must be a bare INT32 column of the right table", wx.WX_ERR_INVALID, f, d, one, rkey=rkey)
    # a column of both tables
    both = table(1000, id="i32", price="f32")
    _both("column price is in both tables", wx.WX_ERR_INVALID, f, both, ["price[idx]"])
    _both("column price is in both tables", wx.WX_ERR_INVALID, f, both, ["id[idx]"], cond="(price[idx] > 1.0f)")
    _both("column price is in both tables", wx.WX_ERR_INVALID, f, both, ["id[idx]"], key="(int)price[idx]")
    wx.prepare_join(f, both, "cust[idx]", "id", ["quantity[idx]"], None, no_custom())  # unreferenced: no conflict
    # the left key names left columns only
    _both("left_key_expr names the right column tier", wx.WX_ERR_INVALID, f, d, one, key="(cust[idx] + tier[idx])")
    # strings cannot be evaluated, on either side
    _both("cannot evaluate", wx.WX_ERR_UNSUPPORTED, f, d, ["label[idx]"])
    # the right table's size
    _both("more than 67108864 rows", wx.WX_ERR_UNSUPPORTED, f, table((1 << 26) + 1, id="i32", rate="f32"), one)
    wx.prepare_join(f, table(1 << 26, id="i32", rate="f32"), "cust[idx]", "id", one, None, no_custom())
    with pytest.raises(wx.WarpExecError, match="form must be") as ei:
        wx.prepare_join(f, d, "cust[idx]", "id", one, None, no_custom(), INNER, False, 2)
    assert ei.value.status == wx.WX_ERR_INVALID
    # the run path's own checks
    with pytest.raises(wx.WarpExecError) as ei:
        _call(f, d, one, flags=wx.F_ROW_ORDER)
    assert ei.value.status == wx.WX_ERR_UNSUPPORTED
    with pytest.raises(wx.WarpExecError, match="idx_bytes") as ei:
        _call(f, d, one, idx=1 << 30, idx_bytes=2)
    assert ei.value.status == wx.WX_ERR_INVALID
    with pytest.raises(wx.WarpExecError, match="exceed int32") as ei:
        _call(f, d, one, idx=1 << 30, idx_bytes=4, row_base=(1 << 31) - 5)
    assert ei.value.status == wx.WX_ERR_INVALID


def test_column_limit_is_per_table():
    lcols = {f"c{i}": "f32" for i in range(18)}
    rcols = {f"r{i}": "f32" for i in range(18)}
    f, d = table(k="i32", **lcols), table(1000, id="i32", **rcols)
    exprs = ["(" + " + ".join(f"c{i}[idx]" for i in range(j, 15, 4)) + " + " +
             " + ".join(f"r{i}[idx]" for i in range(j, 16, 4)) + ")" for j in range(4)]
    wx.prepare_join(f, d, "k[idx]", "id", exprs, None, no_custom())  # 15 + the key on the left, 16 on the right
    with pytest.raises(wx.WarpExecError, match="16 columns") as ei:
        wx.prepare_join(f, d, "k[idx]", "id", exprs, "(c15[idx] > 0.0f)", no_custom())
    assert ei.value.status == wx.WX_ERR_UNSUPPORTED
    with pytest.raises(wx.WarpExecError, match="16 columns") as ei:
        wx.prepare_join(f, d, "k[idx]", "id", exprs, "(r16[idx] > 0.0f)", no_custom())
    assert ei.value.status == wx.WX_ERR_UNSUPPORTED


def test_program_text_of_other_families_is_unchanged():
    """A single-output compaction's program names nothing of the join family."""
    lib = wx.load()
    t = fact()
    src = ctypes.create_string_buffer(1 << 20)
    err = ctypes.create_string_buffer(4096)
    L = no_custom()
    st = lib.wx_prepare(ctypes.byref(t.c), wx.OP_COMPACT, b"price[idx]", None, None, 0, ctypes.byref(L), src, len(src),
                        err, len(err))
    assert st == 0, err.value
    text = src.value.decode()
    assert "wx_project_compact_deep" in text and "wx_join" not in text and "WX_JOIN_" not in text


def test_planner_binary():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "bin/join_plan_test"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "bin", "join_plan_test")], capture_output=True, text=True,
                       cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "join_plan_test: all passed" in r.stdout
