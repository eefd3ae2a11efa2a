"""CPU tests of the layouts the ordered compaction's GPU tests run
(tests/compact_layouts.py) and of the host hooks those tests lean on.

At the default geometry a compaction launches one workgroup per tile until a
table holds more tiles than the device keeps resident, so on tables a test can
afford no workgroup of the multi-output kernels ever runs the pipeline's
steady state (three tiles in flight), and uniformly random tables never pick
the shape of a tile's output run.  WARPDB_COMPACT_GRID caps the grid,
wx_compact_last_launch says what a call launched, and the layouts choose every
tile's count.  Here: the numpy statement of the store split against cases
worked by hand, every layout's own claim, and the report on a workspace
nothing has run on.  (A bad WARPDB_COMPACT_GRID is refused by the compacting
call itself, which needs a device: tests/test_gpu_compact_edges.py.)
"""
from __future__ import annotations

import numpy as np
import pytest

import compact_layouts as cl
from warpdb_amd import _warpexec as wx


def test_symbol_is_exported():
    assert hasattr(wx.load(), "wx_compact_last_launch") and "wx_compact_last_launch" in wx.EXPORTED_SYMBOLS


def test_last_launch_is_zero_on_a_fresh_stream():
    # a (device, stream) nothing ran on: host numbers only, so no device is needed (the stream is never used)
    for stream in (0x5EED0, 0x5EED8):
        g = wx.compact_last_launch(wx.make_launch(device=0, stream=stream))
        assert (g.tile_rows, g.n_tiles, g.grid, g.deep) == (0, 0, 0, 0)
    err = wx._err()
    assert wx.load().wx_compact_last_launch(None, None, err, len(err)) == wx.WX_ERR_INVALID


def test_split_by_hand():
    # (excl, tot) -> (head, body, tail)
    for (excl, tot), want in {
        (0, 0): (0, 0, 0), (0, 3): (0, 0, 3), (0, 4): (0, 4, 0), (0, 7): (0, 4, 3), (0, 512): (0, 512, 0),
        (1, 10): (10, 0, 0), (1, 31): (31, 0, 0), (1, 32): (31, 0, 1), (1, 134): (31, 100, 3), (1, 512): (31, 480, 1),
        (31, 0): (0, 0, 0), (31, 1): (1, 0, 0), (31, 43): (1, 40, 2), (31, 512): (1, 508, 3),
        (95, 6): (1, 4, 1), (64 + 17, 5): (5, 0, 0), (7, 25): (25, 0, 0),
    }.items():
        assert cl.split(excl, tot) == want, (excl, tot)
    for excl in range(0, 70):
        for tot in range(0, 80):
            h, b, t = cl.split(excl, tot)
            assert h + b + t == tot and 0 <= h < 32 and b % 4 == 0 and 0 <= t < 4
            assert b == 0 or (excl + h) % 32 == 0          # the body starts on a 32-element boundary
            assert h == min(tot, (32 - excl % 32) % 32)


def test_zero_runs():
    assert cl.zero_runs([1, 0, 0, 2, 0, 3, 0, 0, 0]) == [2, 1, 3] and cl.zero_runs([4, 5]) == []


def test_every_layout_holds_its_claim():
    lays = cl.all_layouts()   # every builder asserts the edge it is named for
    assert len(lays) == 11
    for name, lay in lays.items():
        assert 1 <= lay.n <= cl.MAX_ROWS, name
        assert lay.tile_rows in cl.DEFINES and name.endswith(str(lay.tile_rows))
        # the recorded shapes are the masks': exclusive offsets and counts per tile
        t = lay.tile_rows
        tots = np.add.reduceat(lay.keep.astype(np.int64), np.arange(0, lay.n, t))
        excl = np.concatenate([[0], np.cumsum(tots)[:-1]])
        assert [s[1] for s in lay.shapes] == tots.tolist(), name
        assert [s[0] for s in lay.shapes] == (excl % 32).tolist(), name
        assert all(s[2:] == cl.split(int(e), s[1]) for s, e in zip(lay.shapes, excl)), name
        assert np.array_equal(lay.rows, np.flatnonzero(lay.keep))
    assert lays["steady_512"].n_tiles == lays["steady_1024"].n_tiles == 48
    assert cl.STORE_CLASSES <= lays["store_shapes_512"].classes()
    assert sorted(cl.zero_runs(lays["empty_run_512"].tots))[-2:] == [70, 70]
    one_drop = lays["last_one_drop_512"]
    assert one_drop.shapes[-1][1] == 0 and one_drop.keep.sum() > 0 and one_drop.n % 512 == 1
    assert lays["last_exact_512"].n % 512 == 0 and lays["last_single_512"].n == 1
    # the random layouts never choose a run's shape: what (b) adds to (a)
    assert not cl.STORE_CLASSES <= lays["steady_512"].classes()


def test_join_columns_drop_through_the_probe_and_keep_the_mask():
    rk = cl.right_columns()["rk"].astype(np.int64)
    assert len(np.unique(rk)) == len(rk) and rk.min() == 0 and rk.max() == cl.RIGHT_SPAN - 1
    assert not np.isin(cl.ABSENT, rk).any()
    for name, lay in cl.all_layouts().items():
        base, inner, left = lay.cols(), lay.inner_cols(), lay.left_cols()
        assert np.array_equal(base["pp"] > 0.5, lay.keep)
        assert np.isin(base["kk"][lay.keep], rk).all()                      # the window's dense form: span <= 2048
        hit = np.isin(inner["kk"], rk)
        assert np.array_equal((inner["pp"] > 0.5) & hit, lay.keep), name    # what INNER keeps is the layout's mask
        assert np.array_equal((inner["pp"] > 0.5) & ~hit, lay.probe_drop)
        assert np.array_equal(left["pp"] > 0.5, lay.keep)
        assert np.array_equal(lay.keep & ~np.isin(left["kk"], rk), lay.left_miss)
        for c in (base, inner, left):
            assert np.array_equal(c["va"].astype(np.float64) * 8, np.arange(lay.n))   # exact and distinct
    big = cl.all_layouts()["steady_1024"]
    assert big.probe_drop.sum() > 1000 and big.left_miss.sum() > 1000


def test_position_masks_name_the_kernel_grid():
    pm = cl.position_masks(1024)
    assert np.flatnonzero(pm["element 3"])[:3].tolist() == [3, 7, 11]
    assert np.flatnonzero(pm["lane 63"]).tolist() == [252, 253, 254, 255, 508, 509, 510, 511,
                                                      764, 765, 766, 767, 1020, 1021, 1022, 1023]
    assert np.flatnonzero(pm["last wave"]).tolist() == list(range(256, 512)) + list(range(768, 1024))
    assert np.flatnonzero(pm["crossed"]).tolist() == list(range(256, 768))


@pytest.mark.parametrize("t", [512, 1024])
def test_defines_give_the_tile(t, monkeypatch):
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", cl.DEFINES[t])
    assert wx.select_tile_rows(1) == wx.select_tile_rows(2) == wx.select_tile_rows(4) == t
    assert wx.window_tile_rows(2, 1, False) == t
    for form in (wx.JOIN_DIRECT, wx.JOIN_HASH):
        assert wx.join_tile_rows(2, form, False) == wx.join_tile_rows(2, form, True) == t
