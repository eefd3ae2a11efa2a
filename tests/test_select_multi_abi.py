"""CPU tests of the multi-output compaction's C ABI (wx_project_filter_multi,
wx_prepare_multi): the symbols exist, every module compiles for gfx950
without a device, the argument checks fire before any device call, and the
single-output kernel sources it builds on are untouched."""
from __future__ import annotations

import hashlib
import os
import re
import subprocess

import pytest

from warpdb_amd import _warpexec as wx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "warpdb_amd", "csrc", "kernels")
DISCOUNT_SRC = "__device__ float discount(float price, float rate) {\n    return price * rate;\n}\n"

# sha256 of the sources the single-output compaction is built from, as of the
# commit before the multi-output kernel was added: its code objects (keyed by
# source text) and the benchmark's traffic profile (keyed by these hashes)
# stay valid only while they do not change
FROZEN = {
    "wx_args.h": "e0d96028bf0e813ead6aa4a7e75bbae0a4363c761ffa7db9dca58998c4f30785",
    "wx_common.hip": "b852758b8f63c910e29d98da9face7f5156e1e424fa345b459921b0b2ab79779",
    "wx_compact.hip": "452b538eca6ba53e1e66749a010faf324e9a232a718f13fd60f4bc2b16ec239e",
}


def table(**cols):
    dt = {"f32": wx.FLOAT32, "i32": wx.INT32, "f64": wx.FLOAT64, "i64": wx.INT64, "str": wx.STRING}
    return wx.Table(1 << 20, [wx.Column(k, dt[v], (i + 1) << 20) for i, (k, v) in enumerate(cols.items())])


def no_custom():
    return wx.make_launch(flags=wx.F_NO_CUSTOM)


def test_symbols_and_version():
    lib = wx.load()
    assert hasattr(lib, "wx_project_filter_multi") and hasattr(lib, "wx_prepare_multi")
    assert lib.wx_abi_version() == 1
    assert wx.MAX_OUTPUTS == 4


@pytest.mark.parametrize("name", sorted(FROZEN))
def test_single_output_sources_unchanged(name):
    with open(os.path.join(KERNELS, name), "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == FROZEN[name]


def test_tile_rows_shrink_with_outputs(monkeypatch):
    monkeypatch.delenv("WARPDB_EXTRA_DEFINES", raising=False)
    rows = [wx.select_tile_rows(m) for m in (1, 2, 3, 4)]
    assert rows[0] == 12288  # the single-output geometry is what it was
    assert rows[0] > rows[1] > rows[2] > rows[3] > 0
    assert rows[1:] == [7680, 5376, 3840]  # as measured; the window broadcast starts from them
    for m, r in zip((2, 3, 4), rows[1:]):
        assert r % 256 == 0 and 2 * r * (4 * m + 2) <= 150 * 1024  # two stage buffers fit the LDS
    assert wx.select_tile_rows(0) == 0 and wx.select_tile_rows(5) == 0
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_COMPACT_GROUPS=1,WX_COMPACT_DWAVES=2")
    assert [wx.select_tile_rows(m) for m in (1, 2, 3, 4)] == [512] * 4
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_COMPACT_GROUPS=4,WX_COMPACT_DWAVES=12")
    assert wx.select_tile_rows(1) == 12288 and wx.select_tile_rows(2) == 0  # 12288 rows x 20 B do not fit
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_COMPACT_GROUPS=10,WX_COMPACT_DWAVES=3")
    assert wx.select_tile_rows(2) == 0  # a thread's keep bits (4 per quad) share one 32-bit word


def program_text(*args):
    """The program text of a multi-output module (tests/cpp/program_text.cpp: the code generator, no device)."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "bin/program_text"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "bin", "program_text"), *map(str, args)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_program_text_has_one_body(monkeypatch):
    """A select module names its two kernels once each and takes their bodies from the shared source."""
    monkeypatch.delenv("WARPDB_EXTRA_DEFINES", raising=False)
    text = program_text("select", 2)
    assert "#define WX_NOUT 2\n" in text
    for hook, name in (("WX_CM_DEEP", "wx_select_compact_deep"), ("WX_CM_TICKET", "wx_select_compact_ticket")):
        assert text.count(name) == 1 and text.count(f"#define {hook} {name}\n") == 1
        assert len(re.findall(rf"\bvoid {hook}\(", text)) == 1
    assert "wx_window_compact" not in text and "#define WX_WIN_" not in text and 'wx_window.hip"' not in text
    assert text.count('#line 1 "wx_compact_multi.hip"') == 1
    assert text.rindex("#line 1 ") == text.index('#line 1 "wx_compact_multi.hip"')  # appended last


EXPRS = ["(f[idx] + (float)i[idx])", "(float)d[idx]", "((float)key[idx] * 2.0f)", "(f[idx] * f[idx])"]


@pytest.mark.parametrize("m", [2, 3, 4])
@pytest.mark.parametrize("cond", [None, "(d[idx] > 1.0)"])
def test_prepare_multi_compiles_every_column_type(m, cond):
    t = table(f="f32", i="i32", d="f64", key="i64", note="str")
    wx.prepare_multi(t, EXPRS[:m], cond, no_custom())


def test_prepare_multi_with_custom_function():
    t = table(price="f32", quantity="i32")
    wx.prepare_multi(t, ["price[idx]", "discount(price[idx], 0.9f)", "(price[idx] * quantity[idx])"],
                     "(price[idx] > 15.0f)", wx.make_launch(custom_src=DISCOUNT_SRC))


def test_prepare_multi_tiny_tiles(monkeypatch):
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_COMPACT_GROUPS=1,WX_COMPACT_DWAVES=2")
    t = table(price="f32", quantity="f32")
    wx.prepare_multi(t, ["price[idx]", "quantity[idx]"], "(price[idx] > 15.0f)", no_custom())


def test_one_expression_is_the_single_output_module():
    t = table(price="f32", quantity="f32")
    e, c = "(price[idx] * quantity[idx] + 0.125f)", "(price[idx] > 15.0f)"
    wx.prepare(t, wx.OP_COMPACT, e, c, launch=no_custom())
    before = wx.cache_stats()[0]
    wx.prepare_multi(t, [e], c, no_custom())
    assert wx.cache_stats()[0] == before  # same source text: the cached code object


def test_compile_error_is_reported():
    t = table(price="f32")
    with pytest.raises(wx.WarpExecError) as ei:
        wx.prepare_multi(t, ["price[idx]", "invalid@"], None, no_custom())
    assert ei.value.status == wx.WX_ERR_COMPILE


def _call(t, exprs, mode=wx.MODE_COMPACT, **kw):
    # device pointers are never dereferenced: every case fails its argument check first
    return wx.project_filter_multi(t, exprs, None, no_custom(), [1 << 30] * len(exprs), mode=mode, **kw)


def test_argument_checks_need_no_device():
    t = table(price="f32", quantity="f32")
    for exprs in ([], ["price[idx]"] * 5):
        with pytest.raises(wx.WarpExecError) as ei:
            _call(t, exprs)
        assert ei.value.status == wx.WX_ERR_INVALID
        with pytest.raises(wx.WarpExecError) as ei:
            wx.prepare_multi(t, exprs, None, no_custom())
        assert ei.value.status == wx.WX_ERR_INVALID
    for exprs in (["price[idx]", "  "], [" "], ["price[idx]", None, "quantity[idx]"]):
        with pytest.raises(wx.WarpExecError, match="Empty query expression") as ei:
            _call(t, exprs)
        assert ei.value.status == wx.WX_ERR_INVALID
    for mode in (wx.MODE_DENSE, wx.MODE_DENSE_FILL):
        with pytest.raises(wx.WarpExecError) as ei:
            _call(t, ["price[idx]", "quantity[idx]"], mode=mode)
        assert ei.value.status == wx.WX_ERR_UNSUPPORTED
    with pytest.raises(wx.WarpExecError) as ei:
        _call(t, ["price[idx]", "quantity[idx]"], mode=7)
    assert ei.value.status == wx.WX_ERR_INVALID
    for m in (1, 2):
        with pytest.raises(wx.WarpExecError, match="idx_bytes") as ei:
            _call(t, ["price[idx]", "quantity[idx]"][:m], d_out_idx=1 << 31, idx_bytes=2)
        assert ei.value.status == wx.WX_ERR_INVALID
        with pytest.raises(wx.WarpExecError, match="int32") as ei:
            _call(t, ["price[idx]", "quantity[idx]"][:m], d_out_idx=1 << 31, idx_bytes=4, row_base=(1 << 31) - 5)
        assert ei.value.status == wx.WX_ERR_INVALID


def test_column_limit_is_over_the_union():
    cols = {f"c{i}": "f32" for i in range(18)}
    t = table(**cols)
    exprs = ["(" + " + ".join(f"c{i}[idx]" for i in range(j, 18, 4)) + ")" for j in range(4)]
    with pytest.raises(wx.WarpExecError) as ei:
        wx.prepare_multi(t, exprs, None, no_custom())
    assert ei.value.status == wx.WX_ERR_UNSUPPORTED
    wx.prepare_multi(t, ["c0[idx]", "c1[idx]"], "(c17[idx] > 0.0f)", no_custom())


def test_result_column_names():
    from warpdb_amd import pywarpdb as pw

    assert pw.result_column_names("SELECT price, quantity FROM t") == ["price", "quantity"]
    assert pw.result_column_names("SELECT price, price * quantity, quantity + 1 FROM t WHERE price > 1") == [
        "price", "expr1", "expr2"]
    assert pw.result_column_names("SELECT quantity, SUM(price), COUNT(price), AVG(price), MIN(price), MAX(price) "
                                  "FROM t GROUP BY quantity") == [
        "quantity", "sum_1", "count_2", "avg_3", "min_4", "max_5"]
    with pytest.raises(RuntimeError, match="Failed to parse SQL"):
        pw.result_column_names("SELECT FROM")
