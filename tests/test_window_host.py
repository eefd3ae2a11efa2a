"""CPU tests of the window-aggregate family (wx_window_select, wx_window.hip,
plan_sql_windowed): the ABI is exported and parses as C11, its modules compile
for gfx950 in the dense and the search form without a device, the argument
checks fire before any device call, the broadcast tile shrinks with the
table it shares the LDS with, the kernel sources it builds on are untouched,
and the planner binary (tests/cpp/window_plan_test.cpp) passes."""
from __future__ import annotations

import ctypes
import hashlib
import importlib.util
import os
import re
import subprocess

import pytest

from warpdb_amd import _warpexec as wx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "warpdb_amd", "csrc", "kernels")
DISCOUNT_SRC = "__device__ float discount(float price, float rate) {\n    return price * rate;\n}\n"


def table(**cols):
    dt = {"f32": wx.FLOAT32, "i32": wx.INT32, "f64": wx.FLOAT64, "i64": wx.INT64, "str": wx.STRING}
    return wx.Table(1 << 20, [wx.Column(k, dt[v], (i + 1) << 20) for i, (k, v) in enumerate(cols.items())])


def no_custom(flags=0):
    return wx.make_launch(flags=wx.F_NO_CUSTOM | flags)


def test_symbols():
    lib = wx.load()
    for name in ("wx_window_select", "wx_prepare_window", "wx_window_tile_rows"):
        assert hasattr(lib, name) and name in wx.EXPORTED_SYMBOLS
    assert lib.wx_abi_version() == 1
    assert (wx.WIN_SUM, wx.WIN_AVG, wx.WIN_COUNT, wx.WIN_MIN, wx.WIN_MAX) == (0, 1, 2, 3, 4)


def test_header_parses_as_c11(tmp_path):
    c = tmp_path / "use.c"
    c.write_text('#include "warpexec.h"\n'
                 "int probe(const wx_table *t, const char *const *e, float *const *o) {\n"
                 "  const wx_window_item items[2] = {{\"v\", WX_WIN_SUM}, {\"v\", WX_WIN_MAX}};\n"
                 "  return (int)wx_window_select(t, e, 2, items, 2, \"k\", 0, 0, 0, 16, o, 0, 8, 0, 0, 0, 0, 0)\n"
                 "       + (int)wx_prepare_window(t, e, 2, items, 2, \"k\", 0, 0, 1, 0, 0)\n"
                 "       + (int)wx_window_tile_rows(WX_MAX_OUTPUTS, 2, 0) + WX_WIN_AVG + WX_WIN_COUNT + WX_WIN_MIN;\n}\n")
    r = subprocess.run(["cc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "include"), str(c)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("search", [False, True])
@pytest.mark.parametrize("key", ["k32[idx]", "k64[idx]", "(int)f[idx]", "d[idx]", "0"])
def test_prepare_compiles_every_column_type(key, search):
    t = table(f="f32", i="i32", d="f64", w="i64", k32="i32", k64="i64", note="str")
    # one launch of four outputs: two plain expressions beside a sum and a maximum of two values
    wx.prepare_window(t, ["(f[idx] + (float)i[idx])", "w[idx]"],
                      [("d[idx]", wx.WIN_AVG), ("((float)w[idx] * 2.0f)", wx.WIN_MAX)], key,
                      "(d[idx] > 1.0)" if search else None, no_custom(), search=search)


@pytest.mark.parametrize("search", [False, True])
def test_prepare_every_launch_shape(search):
    t = table(price="f32", quantity="i32")
    one = [("price[idx]", wx.WIN_SUM)]
    # no plain expression; 1 + 3; 4 + 0 items; nine outputs in three launches (the first all plain)
    wx.prepare_window(t, [], one, "quantity[idx]", None, no_custom(), search=search)
    wx.prepare_window(t, ["price[idx]", "quantity[idx]", "(price[idx] * 2.0f)"], one, "quantity[idx]",
                      "(price[idx] > 15.0f)", no_custom(), search=search)
    wx.prepare_window(t, [], [("price[idx]", a) for a in (wx.WIN_SUM, wx.WIN_AVG, wx.WIN_MIN, wx.WIN_MAX)],
                      "quantity[idx]", None, no_custom(), search=search)
    wx.prepare_window(t, [f"(price[idx] + {j}.0f)" for j in range(4)],
                      [("price[idx]", a) for a in (wx.WIN_SUM, wx.WIN_AVG, wx.WIN_COUNT, wx.WIN_MIN, wx.WIN_MAX)],
                      "quantity[idx]", "(price[idx] > 15.0f)", no_custom(), search=search)


def test_prepare_with_custom_function():
    t = table(price="f32", quantity="i32")
    for search in (False, True):
        wx.prepare_window(t, ["discount(price[idx], 0.9f)"], [("discount(price[idx], 0.5f)", wx.WIN_SUM)],
                          "quantity[idx]", "(price[idx] > 15.0f)", wx.make_launch(custom_src=DISCOUNT_SRC),
                          search=search)


def test_program_text_of_a_launch():
    """The window module is a WX_OP_COMPACT program with the window prelude; the select source stays out."""
    lib = wx.load()
    t = table(price="f32", quantity="i32")
    before = wx.cache_stats()[0]
    wx.prepare_window(t, ["price[idx]"], [("price[idx]", wx.WIN_SUM)], "quantity[idx]", None, no_custom())
    wx.prepare_window(t, ["price[idx]"], [("price[idx]", wx.WIN_SUM)], "quantity[idx]", None, no_custom())
    assert wx.cache_stats()[0] - before <= 3  # the table module, the grouped pass and one launch, compiled once
    # a single-output compaction's program names nothing of the window family
    src = ctypes.create_string_buffer(1 << 20)
    err = ctypes.create_string_buffer(4096)
    L = no_custom()
    st = lib.wx_prepare(ctypes.byref(t.c), wx.OP_COMPACT, b"price[idx]", None, None, 0, ctypes.byref(L), src, len(src),
                        err, len(err))
    assert st == 0, err.value
    text = src.value.decode()
    assert "wx_project_compact_deep" in text and "wx_window" not in text and "WX_WIN_" not in text


def test_compile_error_is_reported():
    t = table(price="f32", quantity="i32")
    with pytest.raises(wx.WarpExecError) as ei:
        wx.prepare_window(t, ["invalid@"], [("price[idx]", wx.WIN_SUM)], "quantity[idx]", None, no_custom())
    assert ei.value.status == wx.WX_ERR_COMPILE


def _call(t, exprs, items, part="quantity[idx]", flags=0, cap=16, key_lo=0, idx=0, idx_bytes=8, row_base=0):
    # device pointers are never dereferenced: every case fails its argument check first
    return wx.window_select(t, exprs, items, part, None, no_custom(flags), [1 << 30] * (len(exprs) + len(items)),
                            key_window_lo=key_lo, group_capacity=cap, d_out_idx=idx, idx_bytes=idx_bytes,
                            row_base=row_base)


def test_argument_checks_need_no_device():
    t = table(price="f32", quantity="i32")
    one = [("price[idx]", wx.WIN_SUM)]
    with pytest.raises(wx.WarpExecError, match="wx_project_filter_multi") as ei:
        _call(t, ["price[idx]"], [])
    assert ei.value.status == wx.WX_ERR_INVALID
    with pytest.raises(wx.WarpExecError, match="wx_project_filter_multi") as ei:
        wx.prepare_window(t, ["price[idx]"], [], "quantity[idx]", None, no_custom())
    assert ei.value.status == wx.WX_ERR_INVALID
    with pytest.raises(wx.WarpExecError, match="n_items") as ei:
        _call(t, [], one * 17)
    assert ei.value.status == wx.WX_ERR_INVALID
    with pytest.raises(wx.WarpExecError, match="at most 16") as ei:
        _call(t, ["price[idx]"] * 9, one * 8)
    assert ei.value.status == wx.WX_ERR_INVALID
    for exprs, items, part in ((["  "], one, "quantity[idx]"), (["price[idx]", None], one, "quantity[idx]"),
                               ([], [(" ", wx.WIN_SUM)], "quantity[idx]"), ([], [(None, wx.WIN_MAX)], "quantity[idx]"),
                               ([], one, "  ")):
        with pytest.raises(wx.WarpExecError, match="Empty query expression") as ei:
            _call(t, exprs, items, part=part)
        assert ei.value.status == wx.WX_ERR_INVALID
    for agg in (-1, 5, 99):
        with pytest.raises(wx.WarpExecError, match="unknown aggregate") as ei:
            _call(t, [], [("price[idx]", agg)])
        assert ei.value.status == wx.WX_ERR_INVALID
    # five distinct values are one too many; COUNTs take none, repeats share one
    five = [(f"(price[idx] + {j}.0f)", wx.WIN_SUM) for j in range(5)]
    with pytest.raises(wx.WarpExecError, match="distinct value expressions") as ei:
        _call(t, [], five)
    assert ei.value.status == wx.WX_ERR_INVALID
    with pytest.raises(wx.WarpExecError, match="distinct value expressions") as ei:
        wx.prepare_window(t, [], five, "quantity[idx]", None, no_custom())
    assert ei.value.status == wx.WX_ERR_INVALID
    wx.prepare_window(t, [], five[:4] + [(e, wx.WIN_MAX) for e, _ in five[:4]] +
                      [(f"(price[idx] * {j}.0f)", wx.WIN_COUNT) for j in range(8)], "quantity[idx]", None, no_custom())
    with pytest.raises(wx.WarpExecError) as ei:
        _call(t, [], one, flags=wx.F_ROW_ORDER)
    assert ei.value.status == wx.WX_ERR_UNSUPPORTED
    with pytest.raises(wx.WarpExecError, match="idx_bytes") as ei:
        _call(t, [], one, idx=1 << 30, idx_bytes=2)
    assert ei.value.status == wx.WX_ERR_INVALID
    with pytest.raises(wx.WarpExecError, match="exceed int32") as ei:
        _call(t, [], one, idx=1 << 30, idx_bytes=4, row_base=(1 << 31) - 5)
    assert ei.value.status == wx.WX_ERR_INVALID
    for cap in (0, -1, 1 << 31):
        with pytest.raises(wx.WarpExecError, match="group_capacity") as ei:
            _call(t, [], one, cap=cap)
        assert ei.value.status == wx.WX_ERR_INVALID
    with pytest.raises(wx.WarpExecError, match="key window") as ei:
        _call(t, [], one, key_lo=(1 << 31) - 100)
    assert ei.value.status == wx.WX_ERR_INVALID
    with pytest.raises(wx.WarpExecError) as ei:
        _call(table(price="f32", note="str"), [], [("price[idx]", wx.WIN_SUM)], part="note[idx]")
    assert ei.value.status == wx.WX_ERR_UNSUPPORTED


def test_column_limit_is_over_everything_referenced():
    cols = {f"c{i}": "f32" for i in range(18)}
    t = table(k="i32", **cols)
    plain = ["(" + " + ".join(f"c{i}[idx]" for i in range(j, 10, 4)) + ")" for j in range(4)]  # 10 columns
    items = [(f"c{i}[idx]", wx.WIN_SUM) for i in range(10, 14)]  # 14
    wx.prepare_window(t, plain, items, "k[idx]", "(c14[idx] > 0.0f)", no_custom())  # + key + cond = 16
    with pytest.raises(wx.WarpExecError, match="16 columns") as ei:
        wx.prepare_window(t, plain, items, "k[idx]", "(c14[idx] > c15[idx])", no_custom())
    assert ei.value.status == wx.WX_ERR_UNSUPPORTED


def test_tile_rows(monkeypatch):
    monkeypatch.delenv("WARPDB_EXTRA_DEFINES", raising=False)
    budget, bins = 150 * 1024, 2048
    for nout in range(1, wx.MAX_OUTPUTS + 1):
        row_bytes = 2 * (4 * nout + 2)
        rows = [wx.window_tile_rows(nout, k) for k in range(1, nout + 1)]
        for k, r in enumerate(rows, start=1):
            assert r > 0 and r % 256 == 0
            assert r * row_bytes + k * bins * 4 <= budget  # two stage buffers beside the table
            assert r // 256 <= 8 * 15  # at most 8 row quads per thread, 15 data waves
        assert rows == sorted(rows, reverse=True)
        # the search form needs no table: the select geometry
        assert wx.window_tile_rows(nout, 1, True) == wx.window_tile_rows(nout, nout, True) >= rows[0]
        if nout >= 2:
            assert wx.window_tile_rows(nout, 1, True) == wx.select_tile_rows(nout)
    assert wx.window_tile_rows(2, 2) < wx.window_tile_rows(2, 1)
    assert wx.window_tile_rows(4, 4) < wx.window_tile_rows(4, 1)
    # every (outputs, items) of a launch, dense form; the search form is the select table's
    dense = {1: [7680], 2: [6912, 6144], 3: [4608, 4608, 4608], 4: [3840, 3072, 3072, 3072]}
    for nout, rows in dense.items():
        assert [wx.window_tile_rows(nout, k) for k in range(1, nout + 1)] == rows
        assert wx.window_tile_rows(nout, 1, True) == [7680, 7680, 5376, 3840][nout - 1]
    lib = wx.load()
    for args in ((0, 1, 0), (5, 1, 0), (2, 0, 0), (2, 3, 0), (1, 2, 0), (-1, 1, 0), (2, -1, 0), (2, 1, 2), (2, 1, -1)):
        assert lib.wx_window_tile_rows(*args) == 0, args
    # the diagnostic define list shrinks it, as for wx_select_tile_rows
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_COMPACT_GROUPS=1,WX_COMPACT_DWAVES=2")
    assert wx.window_tile_rows(2, 1) == wx.window_tile_rows(4, 4, True) == 512
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_COMPACT_GROUPS=9")
    assert wx.window_tile_rows(2, 1) == 0
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_COMPACT_GROUPS=8,WX_COMPACT_DWAVES=15")
    assert wx.window_tile_rows(4, 4) == 0  # does not fit beside a 32 KiB table


def _module(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_program_text_has_one_body(monkeypatch):
    """A window module names its two kernels once each and takes their bodies from the shared source."""
    monkeypatch.delenv("WARPDB_EXTRA_DEFINES", raising=False)
    text = _module("test_select_multi_abi").program_text("window", 1, 1)
    assert "#define WX_WIN_NOUT 2\n#define WX_WIN_MASK 2\n" in text
    for hook, name in (("WX_CM_DEEP", "wx_window_compact_deep"), ("WX_CM_TICKET", "wx_window_compact_ticket")):
        assert text.count(name) == 1 and text.count(f"#define {hook} {name}\n") == 1
        assert len(re.findall(rf"\bvoid {hook}\(", text)) == 1
    assert "wx_select_compact" not in text and "#define WX_NOUT" not in text and "wx_select.hip\"" not in text
    assert text.count('#line 1 "wx_compact_multi.hip"') == 1
    assert text.rindex("#line 1 ") == text.index('#line 1 "wx_compact_multi.hip"')  # appended last


def _frozen(module):
    return _module(module).FROZEN


@pytest.mark.parametrize("module", ["test_select_multi_abi", "test_group_multi_host"])
def test_frozen_sources_unchanged(module):
    """The sources the window family is appended to keep the hashes the earlier families pinned."""
    frozen = _frozen(module)
    for name in ("wx_args.h", "wx_common.hip"):
        assert name in frozen
    for name, digest in frozen.items():
        with open(os.path.join(KERNELS, name), "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == digest, name


def test_planner_binary():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "bin/window_plan_test"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "bin", "window_plan_test")], capture_output=True,
                       text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "window_plan_test: all passed" in r.stdout
