"""CPU tests of the layouts the row-order GROUP BY's GPU tests run
(tests/ro_layouts.py) and of the host hooks those tests lean on.

The span path launches min(tiles, 2 * CUs) ranges, so on tables a test can
afford every range runs one tile and the scatter's cross-tile state (the runs
advanced per tile, the counters re-zeroed, the bases rebuilt) never matters.
WARPDB_RO_RANGES caps the ranges, wx_group_rows_last_call says what a call
did, wx_group_rows_geometry gives the sizes, and the layouts choose every
tile.  Here: the geometry against the kernels' constants, the record on a
workspace nothing ran on, wx_ro_range restated, and every layout's own claim.
"""
from __future__ import annotations

import numpy as np
import pytest

import ro_layouts as rl
from warpdb_amd import _warpexec as wx

NEW = ("wx_group_rows_geometry", "wx_group_rows_last_call", "wx_group_rows_last_values")


@pytest.fixture(scope="module")
def geom():
    return wx.group_rows_geometry()


@pytest.fixture(scope="module")
def lays(geom):
    return rl.all_layouts(geom)


def test_symbols_are_exported():
    lib = wx.load()
    for name in NEW:
        assert hasattr(lib, name) and name in wx.EXPORTED_SYMBOLS


def test_geometry_is_the_kernels(geom, monkeypatch):
    g = geom
    assert g.tile_rows == 512 * 16 and g.span_bins == 2048 and g.count_span_rows == 512 * 8
    assert g.fold_block_values == 64 * 8 and g.fold_blocks_ahead == 4 and g.fold_small == 4096
    assert g.starts_chunk == 256 * 16 and g.rle_wave_rows == 16384
    assert g.xf_chunk == 1 << 16 and g.xf_big == 4 << 20 and g.sample_rows == 64 * 1024
    # a tile is a whole number of count spans, and a count span of waves
    assert g.tile_rows % g.count_span_rows == 0 and g.count_span_rows % 64 == 0
    assert g.xf_big % g.xf_chunk == 0 and g.xf_chunk % g.fold_block_values == 0
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", "WX_XF_J=4,WX_XF_AHEAD=2")   # the fold's diagnostic defines are followed
    g2 = wx.group_rows_geometry()
    assert g2.fold_block_values == 256 and g2.fold_blocks_ahead == 2 and g2.tile_rows == g.tile_rows
    err = wx._err()
    assert wx.load().wx_group_rows_geometry(None, err, len(err)) == wx.WX_ERR_INVALID


def test_geometry_follows_the_kernel_sources(geom):
    """The sizes only the kernel sources name, read from them."""
    import os
    import re

    kdir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "warpdb_amd", "csrc", "kernels")
    src = {f: open(os.path.join(kdir, f)).read() for f in ("wx_args.h", "wx_group_rows.hip", "wx_util.hip",
                                                           "wx_group_part.hip")}

    def define(f, name):
        return int(eval(re.search(r"^#define %s (.+?)(?:\s*//.*)?$" % name, src[f], re.M).group(1), {}))

    assert geom.tile_rows == define("wx_args.h", "WX_RO_TILE_ROWS") == \
        define("wx_group_rows.hip", "WX_RO_BLOCK") * define("wx_group_rows.hip", "WX_RO_ITEMS")
    assert geom.span_bins == define("wx_group_rows.hip", "WX_RO_BINS")
    assert "constexpr wx_i64 SPAN = (wx_i64)WX_RO_BLOCK * 8;" in src["wx_group_rows.hip"]
    assert geom.count_span_rows == define("wx_group_rows.hip", "WX_RO_BLOCK") * 8
    assert geom.fold_block_values == 64 * define("wx_util.hip", "WX_XF_J")
    assert geom.fold_blocks_ahead == define("wx_util.hip", "WX_XF_AHEAD")
    assert geom.fold_small == define("wx_args.h", "WX_FOLD_SMALL")
    assert geom.starts_chunk == define("wx_args.h", "WX_GS_BLOCK") * define("wx_args.h", "WX_GS_PER")
    assert geom.xf_chunk == define("wx_args.h", "WX_XF_CHUNK") and geom.xf_big == define("wx_args.h", "WX_XF_BIG")
    # the sample: thread i of S reads row i * n / S, S the launch's threads
    assert "const wx_i64 wx_s = (wx_i64)gridDim.x * WX_GP_BLOCK;" in src["wx_group_part.hip"]
    assert geom.sample_rows % define("wx_args.h", "WX_GP_BLOCK") == 0


def test_record_is_zero_and_values_refused_on_a_fresh_stream():
    # a (device, stream) nothing ran on: host numbers only, so no device is needed (the stream is never used)
    for stream in (0x5EEE0, 0x5EEE8):
        L = wx.make_launch(device=0, stream=stream)
        r = wx.group_rows_last_call(L)
        assert (r.route, r.why, r.ranges, r.tiles, r.n_values, r.big_groups, r.big_chunks) == (0,) * 7
        with pytest.raises(wx.WarpExecError, match="no row-order GROUP BY") as ei:
            wx.group_rows_last_values(L, 0, 0)
        assert ei.value.status == wx.WX_ERR_INVALID
    err = wx._err()
    assert wx.load().wx_group_rows_last_call(None, None, err, len(err)) == wx.WX_ERR_INVALID
    assert (wx.RO_ROUTE_NONE, wx.RO_ROUTE_DIRECT, wx.RO_ROUTE_ORDINARY_SPAN, wx.RO_ROUTE_GENERAL_RUNS,
            wx.RO_ROUTE_GENERAL_ORDINARY) == (0, 1, 2, 3, 4)


def test_ro_range_covers_the_tiles_in_order(geom):
    T = geom.tile_rows
    for n in (1, T - 1, T, T + 1, 15 * T + 65, 16 * T, 17 * T - 1):
        tiles = -(-n // T)
        for ranges in range(1, tiles + 1):
            spans = [rl.ro_range(n, ranges, r, T) for r in range(ranges)]
            assert spans[0][0] == 0 and spans[-1][1] == tiles
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            assert all(1 <= t1 - t0 <= -(-tiles // ranges) for t0, t1 in spans)   # ranges <= tiles: none is empty


def test_every_layout_holds_its_claim(geom, lays):
    T, bins = geom.tile_rows, geom.span_bins
    assert len(lays) == len(rl.TAILS) + 2
    kinds, tails = set(), set()
    for name, lay in lays.items():
        assert lay.name == name and lay.n < 1 << 24 and lay.n_tiles == len(lay.kinds) >= rl.N_TILES
        kinds |= set(lay.kinds)
        tails.add(lay.n - (lay.n_tiles - 1) * T)
        c = lay.cols
        keep = lay.keep
        # the declared per-tile passing counts are the columns'
        assert np.add.reduceat(keep.astype(np.int64), np.arange(0, lay.n, T)).tolist() == lay.counts, name
        assert np.array_equal(c["rid"].astype(np.int64), np.arange(lay.n))           # exact and distinct
        # passing keys inside the span, dropped rows' keys outside it on both sides
        kk = c["kk"].astype(np.int64)
        assert kk[keep].min() >= rl.LO and kk[keep].max() < rl.LO + bins
        assert set(np.unique(kk[~keep]).tolist()) == {rl.I32_MIN, rl.I32_MAX, rl.LO - 1, rl.LO + bins}, name
        # the hot key's run goes on over many tiles, and over an empty tile between two of them
        hot = [int(((kk[t * T:(t + 1) * T] == rl.LO + rl.HOT) & keep[t * T:(t + 1) * T]).sum())
               for t in range(lay.n_tiles)]
        assert sum(1 for h in hot if h) >= 8, name
        assert any(lay.counts[t] == 0 and any(hot[:t]) and any(hot[t + 1:]) for t in range(lay.n_tiles)), name
        # the order the GPU tests expect is key-major and ascending in row within a key
        o = lay.order()
        ko = kk[o]
        assert len(o) == keep.sum() and (np.diff(ko) >= 0).all() and (np.diff(o)[np.diff(ko) == 0] > 0).all()
        # ranges of at least two tiles at every cap, unequal at caps 5 and 7
        for cap in rl.CAPS:
            sizes = [t1 - t0 for t0, t1 in (rl.ro_range(lay.n, cap, r, T) for r in range(cap))]
            assert min(sizes) >= 2 and sum(sizes) == lay.n_tiles, (name, cap)
            if cap in (5, 7):
                assert len(set(sizes)) > 1, (name, cap)
        # the strided sample sees the smallest and the largest passing key: the direct route's guess holds
        s = rl.sampled_rows(lay.n, geom.sample_rows)
        s = s[keep[s]]
        assert kk[s].min() == kk[keep].min() and kk[s].max() == kk[keep].max(), name
    assert kinds == set(rl.KINDS)
    assert tails == set(rl.TAILS) | {T}
    wide, narrow = lays["mixed_whole"], lays["narrow_tail_65"]
    assert np.array_equal(wide.groups()[0], np.arange(rl.LO, rl.LO + bins))          # every bin, the first and last too
    assert set(narrow.kinds) <= set(rl.NARROW)
    nk = narrow.groups()[0]
    assert nk.min() == rl.LO + rl.HOT - 28 and nk.max() == rl.LO + rl.HOT + 35       # a span of 64 keys


def test_tile_kinds_by_hand(geom):
    T, bins = geom.tile_rows, geom.span_bins
    rng = np.random.default_rng(1)
    b, keep, count = rl.tile("one_key_no_lane0", 130, T, bins, rng)
    assert count == 127 and np.flatnonzero(~keep).tolist() == [0, 64, 128] and set(b.tolist()) == {rl.HOT}
    b, keep, count = rl.tile("lane_parity", T, T, bins, rng)
    assert keep.all() and b[:4].tolist() == [rl.HOT, rl.HOT + 1, rl.HOT, rl.HOT + 1] and b[64] == rl.HOT
    b, keep, count = rl.tile("straddle", T, T, bins, rng)
    assert set(b.tolist()) == {rl.HOT - 1, rl.HOT} and (rl.HOT - 1) % 4 == 3 and rl.HOT % 4 == 0
    b, keep, count = rl.tile("mod_bins", T, T, bins, rng)
    assert np.bincount(b, minlength=bins).tolist() == [T // bins] * bins
    b, keep, count = rl.tile("extremes", T, T, bins, rng)
    assert set(b.tolist()) == {0, bins - 1} and 0.3 < (b == 0).mean() < 0.7
    for rows, want in ((T, T // 8), (3 * T // 8, 0), (3 * T // 8 + 5, 5), (T // 2 + 1, T // 8)):
        b, keep, count = rl.tile("one_wave", rows, T, bins, rng)
        assert count == want == keep.sum()
        assert not count or (np.flatnonzero(keep)[0] == 3 * T // 8)
    b, keep, count = rl.tile("last_row", 4097, T, bins, rng)
    assert count == 1 and np.flatnonzero(keep).tolist() == [4096]


def test_rle_ranges_by_hand(geom):
    W = geom.rle_wave_rows
    assert rl.rle_ranges(W - 1, W) == (1, W) and rl.rle_ranges(W, W) == (1, W)
    assert rl.rle_ranges(W + 1, W) == (2, (W // 2 + 1 + 63) // 64 * 64)
    n_blk, span = rl.rle_ranges(2 * W + 1, W)
    assert n_blk == 3 and span % 64 == 0 and (n_blk - 1) * span < 2 * W + 1 <= n_blk * span
    assert rl.sampled_rows(10, 4).tolist() == [0, 2, 5, 7]
