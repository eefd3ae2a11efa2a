"""CPU tests of the multi-value GROUP BY (wx_group_agg_multi,
wx_prepare_group_multi, WarpDB::query_sql_grouped's planner): the symbols
exist, every module compiles for gfx950 without a device, the argument checks
fire before any device call, the header still parses as C11, and the
single-value kernel sources (whose cached code objects are keyed by their
text) are untouched."""
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

# sha256 of the sources wx_group_sum / wx_group_agg are built from, as of the
# commit before the multi-value kernel was added: every generated program
# starts with wx_args.h and wx_common.hip, and the code-object cache is keyed
# by the program text, so the single-value kernels stay instruction-identical
# (and their cached objects valid) only while these do not change
FROZEN = {
    "wx_args.h": "e0d96028bf0e813ead6aa4a7e75bbae0a4363c761ffa7db9dca58998c4f30785",
    "wx_common.hip": "b852758b8f63c910e29d98da9face7f5156e1e424fa345b459921b0b2ab79779",
    "wx_group.hip": "5a30eb707756263081cba29ec06c96a9857458ff59147523e3926e5b5a5d2c44",
    "wx_group_part.hip": "2043eb7a0b3f1048913e0ecfc3fe366d901bc5aa127a5b81ae4bf0b623f6fd37",  # + #ifndef WX_GP_DIRCH
    "wx_group_rows.hip": "3809bb618fd8d7714bb9490968143cc9dedc8635bb72971526a345452451f278",
}


def table(**cols):
    dt = {"f32": wx.FLOAT32, "i32": wx.INT32, "f64": wx.FLOAT64, "i64": wx.INT64, "str": wx.STRING}
    return wx.Table(1 << 20, [wx.Column(k, dt[v], (i + 1) << 20) for i, (k, v) in enumerate(cols.items())])


def no_custom():
    return wx.make_launch(flags=wx.F_NO_CUSTOM)


def test_symbols():
    lib = wx.load()
    assert hasattr(lib, "wx_group_agg_multi") and hasattr(lib, "wx_prepare_group_multi")
    assert lib.wx_abi_version() == 1


@pytest.mark.parametrize("name", sorted(FROZEN))
def test_single_value_sources_unchanged(name):
    with open(os.path.join(KERNELS, name), "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == FROZEN[name]


def test_single_value_spec_keys_and_programs_unchanged():
    """The GROUP program of a single-value call names no multi-value source or define."""
    import ctypes

    lib = wx.load()
    t = table(price="f32", quantity="i32")
    for k in (0, 1):
        src = ctypes.create_string_buffer(1 << 20)
        err = ctypes.create_string_buffer(4096)
        L = no_custom()
        st = lib.wx_prepare(ctypes.byref(t.c), wx.OP_GROUP, b"price[idx]", None, b"quantity[idx]", k, ctypes.byref(L),
                            src, len(src), err, len(err))
        assert st == 0, err.value
        text = src.value.decode()
        assert "wx_group_sum" in text and "wx_group_multi" not in text and "WX_GM_" not in text


def program_text(*args):
    """The program text of a module the C ABI does not hand out (tests/cpp/program_text.cpp: the code generator, no device)."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "bin/program_text"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "bin", "program_text"), *map(str, args)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_program_text_has_one_body(monkeypatch):
    """A multi-value or grouped-join module takes the window body and the block helpers from the shared sources,
    once each and ahead of the kernels; a single-value GROUP program holds neither."""
    monkeypatch.delenv("WARPDB_EXTRA_DEFINES", raising=False)
    for args in (("group_multi", 2, 0b01, 0b10), ("join_group", 1, 0b1, 0, "direct"),
                 ("join_group", 4, 0b0011, 0b1110, "hash", "left")):
        text = program_text(*args)
        kernels = text.index('#line 1 "wx_group_multi.hip"')
        for shared in ('#line 1 "wx_group_window.hip"', '#line 1 "wx_block.hip"'):
            assert text.count(shared) == 1 and text.index(shared) < kernels, args
        assert text.index('#line 1 "wx_block.hip"') < text.index('#line 1 "wx_group_window.hip"')
        assert text.count('#line 1 "wx_group_multi.hip"') == 1
        assert len(re.findall(r"\bvoid wx_group_multi_finalize\(", text)) == 1
        assert ('#line 1 "wx_join_group.hip"' in text) == (args[0] == "join_group")
    single = wx.prepare(table(price="f32", quantity="i32"), wx.OP_GROUP, "price[idx]", None, "quantity[idx]", 0,
                        launch=no_custom(), want_source=True)
    assert "wx_group_sum" in single and "wx_group_window.hip" not in single and "wx_block.hip" not in single


def test_header_parses_as_c11(tmp_path):
    c = tmp_path / "use.c"
    c.write_text('#include "warpexec.h"\n'
                 "int probe(const wx_table *t, const char *const *v, double *const *s, float *const *m) {\n"
                 "  return (int)wx_group_agg_multi(t, v, WX_GROUP_MAX_VALUES, \"k\", 0, 0, 0, 16, 0, s, 0, m, m, 0, 0, 0, 0)\n"
                 "       + (int)wx_prepare_group_multi(t, v, 2, 3u, 0u, \"k\", 0, 0, 0, 0);\n}\n")
    r = subprocess.run(["cc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "include"), str(c)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


VALS = ["(f[idx] + (float)i[idx])", "d[idx]", "((float)w[idx] * 2.0f)", "(f[idx] * f[idx])"]
# (sum mask, min/max mask) per M: sums only, min/max only, mixed, and for M = 4 also S = Q = 4
MASKS = {2: [(0b11, 0), (0, 0b11), (0b01, 0b10)],
         3: [(0b111, 0), (0, 0b111), (0b101, 0b011)],
         4: [(0b1111, 0), (0, 0b1111), (0b0011, 0b1110), (0b1111, 0b1111)]}


@pytest.mark.parametrize("key", ["k32[idx]", "k64[idx]", "(int)f[idx]", "d[idx]"])
@pytest.mark.parametrize("m", [2, 3, 4])
def test_prepare_compiles_every_column_type_and_mask(m, key):
    t = table(f="f32", i="i32", d="f64", w="i64", k32="i32", k64="i64", note="str")
    for n, (smask, qmask) in enumerate(MASKS[m]):
        wx.prepare_group_multi(t, VALS[:m], smask, qmask, key, "(d[idx] > 1.0)" if n % 2 else None, no_custom())


def test_prepare_with_custom_function():
    t = table(price="f32", quantity="i32")
    wx.prepare_group_multi(t, ["price[idx]", "discount(price[idx], 0.9f)"], 0b11, 0b10, "quantity[idx]",
                           "(price[idx] > 15.0f)", wx.make_launch(custom_src=DISCOUNT_SRC))


def test_one_value_is_the_single_value_module():
    t = table(price="f32", quantity="i32")
    e, k, c = "(price[idx] * 0.375f)", "quantity[idx]", "(price[idx] > 15.0f)"
    for mm in (0, 1):
        wx.prepare(t, wx.OP_GROUP, e, c, k, mm, launch=no_custom())
        before = wx.cache_stats()[0]
        wx.prepare_group_multi(t, [e], 1 - mm, mm, k, c, no_custom())
        assert wx.cache_stats()[0] == before  # same program text: the cached code object


def test_compile_error_is_reported():
    t = table(price="f32", quantity="i32")
    with pytest.raises(wx.WarpExecError) as ei:
        wx.prepare_group_multi(t, ["price[idx]", "invalid@"], 3, 0, "quantity[idx]", None, no_custom())
    assert ei.value.status == wx.WX_ERR_COMPILE


def _call(t, vals, key="quantity[idx]", flags=wx.F_NO_CUSTOM, sums="all", mins=None, cap=16, key_lo=0, d_keys=1 << 30):
    # device pointers are never dereferenced: every case fails its argument check first
    if sums == "all":
        sums = [1 << 30] * len(vals)
    return wx.group_agg_multi(t, vals, key, None, wx.make_launch(flags=flags), key_lo, cap, d_keys, 1 << 30, sums,
                              mins, None)


def test_argument_checks_need_no_device():
    t = table(price="f32", quantity="i32")
    two = ["price[idx]", "(price[idx] * 2.0f)"]
    for vals in ([], ["price[idx]"] * 5):
        with pytest.raises(wx.WarpExecError, match="n_vals") as ei:
            _call(t, vals)
        assert ei.value.status == wx.WX_ERR_INVALID
        with pytest.raises(wx.WarpExecError) as ei:
            wx.prepare_group_multi(t, vals, 1, 0, "quantity[idx]", None, no_custom())
        assert ei.value.status == wx.WX_ERR_INVALID
    for vals in (["price[idx]", "  "], [" "], ["price[idx]", None, "price[idx]"]):
        with pytest.raises(wx.WarpExecError, match="Empty query expression") as ei:
            _call(t, vals)
        assert ei.value.status == wx.WX_ERR_INVALID
    with pytest.raises(wx.WarpExecError, match="Empty query expression") as ei:
        _call(t, two, key=" ")
    assert ei.value.status == wx.WX_ERR_INVALID
    # a value with nothing requested: no sums array at all, or a null where value 1's pointers go
    for sums, mins in ((None, None), ([1 << 30, 0], None), ([1 << 30, 0], [1 << 30, 0])):
        with pytest.raises(wx.WarpExecError, match="no aggregate requested") as ei:
            _call(t, two, sums=sums, mins=mins)
        assert ei.value.status == wx.WX_ERR_INVALID
    with pytest.raises(wx.WarpExecError, match="no aggregate requested") as ei:
        _call(t, ["price[idx]"], sums=None)
    assert ei.value.status == wx.WX_ERR_INVALID
    with pytest.raises(wx.WarpExecError) as ei:
        _call(t, two, flags=wx.F_NO_CUSTOM | wx.F_ROW_ORDER)
    assert ei.value.status == wx.WX_ERR_UNSUPPORTED
    with pytest.raises(wx.WarpExecError, match="capacity") as ei:
        _call(t, two, cap=-1)
    assert ei.value.status == wx.WX_ERR_INVALID
    with pytest.raises(wx.WarpExecError, match="capacity") as ei:
        _call(t, two, d_keys=0)
    assert ei.value.status == wx.WX_ERR_INVALID
    with pytest.raises(wx.WarpExecError, match="key window") as ei:
        _call(t, two, key_lo=(1 << 31) - 100)
    assert ei.value.status == wx.WX_ERR_INVALID
    # prepare: every value needs a bit, none beyond n_vals
    for smask, qmask in ((0b01, 0), (0, 0b10), (0b111, 0), (0b11, 0b100), (0b11, 1 << 8)):
        with pytest.raises(wx.WarpExecError) as ei:
            wx.prepare_group_multi(t, two, smask, qmask, "quantity[idx]", None, no_custom())
        assert ei.value.status == wx.WX_ERR_INVALID


def test_column_limit_is_over_values_key_and_condition():
    cols = {f"c{i}": "f32" for i in range(18)}
    t = table(k="i32", **cols)
    vals = ["(" + " + ".join(f"c{i}[idx]" for i in range(j, 14, 4)) + ")" for j in range(4)]  # 14 columns
    wx.prepare_group_multi(t, vals, 0xF, 0, "k[idx]", "(c14[idx] > 0.0f)", no_custom())  # + key + cond = 16
    with pytest.raises(wx.WarpExecError) as ei:
        wx.prepare_group_multi(t, vals, 0xF, 0, "k[idx]", "(c14[idx] > c15[idx])", no_custom())
    assert ei.value.status == wx.WX_ERR_UNSUPPORTED


def test_planner_binary():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "bin/group_multi_plan_test"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "bin", "group_multi_plan_test")], capture_output=True,
                       text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "group_multi_plan_test: all passed" in r.stdout
