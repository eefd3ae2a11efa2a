"""CPU tests of the radix sort's geometry queries (wx_sort_tile_keys,
wx_sort_hist_span_keys): the symbols exist, the values follow the diagnostic
define list exactly as the run path's tile count does, an invalid geometry
answers 0, and the util modules compile for gfx950 under the tiny geometry
the GPU edge tests use (tests/test_gpu_sort_edges.py).  No device is needed."""
from __future__ import annotations

from warpdb_amd import _warpexec as wx

# the smallest tile the kernels allow: 256 threads (one per digit) x 2 keys
TINY_DEFINES = "WX_RS_BLOCK=256,WX_RS_ITEMS=2"
TINY_TILE = 512


def test_symbols():
    lib = wx.load()
    for name in ("wx_sort_tile_keys", "wx_sort_hist_span_keys"):
        assert hasattr(lib, name) and name in wx.EXPORTED_SYMBOLS


def test_sort_tile_keys(monkeypatch):
    monkeypatch.delenv("WARPDB_EXTRA_DEFINES", raising=False)
    assert wx.sort_tile_keys(0) == 1024 * 32 == 32768
    assert wx.sort_tile_keys(1) == 512 * 28 == 14336
    assert wx.sort_tile_keys(7) == wx.sort_tile_keys(True) == 14336  # any nonzero value: with payload
    assert wx.sort_hist_span_keys() == 1024 * 4 * 4 == 16384
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_RS_BLOCK=512,WX_RS_ITEMS=20")
    assert wx.sort_tile_keys(0) == wx.sort_tile_keys(1) == 512 * 20
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_DIAG=1,WX_RS_ITEMS=8")  # one of the two: the other keeps its default
    assert wx.sort_tile_keys(0) == 1024 * 8 and wx.sort_tile_keys(1) == 512 * 8
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", TINY_DEFINES)
    assert wx.sort_tile_keys(0) == wx.sort_tile_keys(1) == TINY_TILE
    assert wx.sort_hist_span_keys() == 16384  # not a tile define
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_RS_HUNROLL=2")
    assert wx.sort_hist_span_keys() == 1024 * 2 * 4
    assert wx.sort_tile_keys(0) == 32768


def test_refused_geometry_is_zero(monkeypatch):
    for defines in ("WX_RS_BLOCK=100", "WX_RS_ITEMS=65", "WX_RS_BLOCK=2048", "WX_RS_BLOCK=320,WX_RS_ITEMS=0",
                    "WX_RS_BLOCK=128"):
        monkeypatch.setenv("WARPDB_EXTRA_DEFINES", defines)
        assert wx.sort_tile_keys(0) == 0 and wx.sort_tile_keys(1) == 0, defines
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_RS_BLOCK=320")  # whole waves, in range
    assert wx.sort_tile_keys(0) == 320 * 32 and wx.sort_tile_keys(1) == 320 * 28
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_RS_HUNROLL=0")
    assert wx.sort_hist_span_keys() == 0


def test_util_modules_compile_under_the_tiny_geometry(monkeypatch):
    # wx_prepare(OP_UTIL) builds the key module (the define list's geometry)
    # and the key + payload module (rs_geometry's own defines, four look-back
    # words per round): both must compile for gfx950 with 512-key tiles.  (The
    # code-object cache is the ordinary one, keyed by the generated source: a
    # first run compiles both, ~10 s each, and the GPU tests then find them.)
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", TINY_DEFINES)
    wx.prepare(None, wx.OP_UTIL)
