"""CPU tests of the range-partitioned GROUP BY's geometry and of the layouts
its GPU tests run.

At the default geometry a tile workgroup runs one tile until a table holds more
than 4 194 304 rows (256 CUs x 16 384 rows), so the software-pipelined tile
loop of wx_group_part_tiles, the plan's several / empty / trailing items and
the aggregation's later sweeps and directory rounds need tables no test can
afford.  The diagnostic defines WX_GP_GRID (a cap on the tile grid) and
WX_GP_DIRCH (directory words per aggregation round) shrink the geometry
instead; wx_group_part_geometry states what a pass then launches, with the
arithmetic of the run path (gp_plan, group.cpp), and needs no device.

Here: that call's invariants and error returns, the numpy statement of the
plan (gp_layouts.expected_plan) against a case worked by hand, the oracle's
grouped sums against numpy on the layouts, and every layout's own claim --
"some item is empty", "some e_g is k * chunk", "17 tiles in a row hold no row of
the partition" -- at cus = 256 under the defines the GPU tests use
(tests/test_gpu_group_part_edges.py).
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest

import gp_layouts as tl
import oracle_lib as ora
from warpdb_amd import _warpexec as wx

CUS = 256


def geometry(monkeypatch, defines, n, span=tl.SPAN23, cus=CUS):
    if defines is None:
        monkeypatch.delenv("WARPDB_EXTRA_DEFINES", raising=False)
    else:
        monkeypatch.setenv("WARPDB_EXTRA_DEFINES", defines)
    return wx.group_part_geometry(n, span, cus)


def test_symbols():
    lib = wx.load()
    for name in ("wx_group_part_geometry", "wx_group_part_passes"):
        assert hasattr(lib, name) and name in wx.EXPORTED_SYMBOLS


def test_default_geometry_runs_one_tile_per_workgroup(monkeypatch):
    # the regression fact: what tests/test_gpu_group_wide.py runs never takes the tile loop's second iteration
    g = geometry(monkeypatch, None, 1_500_007, 1_000_000)
    assert (g.tile_rows, g.n_tiles, g.grid, g.tiles_per_wg) == (16384, 92, 92, 1)
    assert (g.n_part, g.part_keys, g.chunk_rows, g.target_items) == (123, 8192, 65536, 4 * CUS)
    assert (g.work_cap, g.dir_chunk, g.agg_tiles_per_sweep) == (123 + 4 * CUS + 2, 4096, 128)
    assert geometry(monkeypatch, None, 4_000_000, 1_000_000).tiles_per_wg == 1   # the largest table of any test
    assert geometry(monkeypatch, None, 256 * 16384, 1_000_000).tiles_per_wg == 1
    assert geometry(monkeypatch, None, 256 * 16384 + 1, 1_000_000).tiles_per_wg == 2
    g = geometry(monkeypatch, None, 10 ** 9, 1_000_000)                          # the benchmark's table
    assert (g.n_tiles, g.grid, g.tiles_per_wg) == (61036, 256, 239)


def test_grid_cap_changes_the_grid_alone(monkeypatch):
    base = geometry(monkeypatch, None, tl.N_RAGGED)
    assert (base.grid, base.tiles_per_wg) == (12, 1)
    g = geometry(monkeypatch, tl.GRID3, tl.N_RAGGED)
    assert (g.grid, g.tiles_per_wg, g.n_tiles) == (3, 4, 12)
    for f, _ in g._fields_:
        if f not in ("grid", "tiles_per_wg"):
            assert getattr(g, f) == getattr(base, f), f
    assert g.target_items == 4 * CUS                                             # not the capped grid's
    g = geometry(monkeypatch, tl.GRID3, tl.N_ONE_ROW)
    assert (g.grid, g.tiles_per_wg, g.n_tiles) == (3, 5, 14)                     # the last workgroup owns 4
    g = geometry(monkeypatch, "WX_GP_GRID=1000", tl.N_RAGGED)                    # a cap above the grid: nothing
    assert (g.grid, g.tiles_per_wg) == (12, 1)
    g = geometry(monkeypatch, tl.GRID2_DIR40, tl.N_LONG, tl.LONG_PARTS * tl.PART)
    assert (g.grid, g.tiles_per_wg, g.n_tiles, g.dir_chunk) == (2, 66, 132, tl.DIRCH_SMALL)
    assert g.n_tiles > 3 * g.dir_chunk and (g.n_tiles % g.dir_chunk) % 8 != 0    # four rounds, the last one ragged


@pytest.mark.parametrize("cap", [None, 1, 2, 3, 7, 300, 5000])
def test_geometry_invariants(cap, monkeypatch):
    defines = None if cap is None else f"WX_GP_GRID={cap}"
    for cus in (1, 8, 104, 256, 304):
        for span in (2049, tl.SPAN23, 2 ** 24):
            for n in (1, 5, 16383, 16384, 16385, tl.N_RAGGED, 1_500_007, 256 * 16384, 256 * 16384 + 1, 10 ** 9,
                      2 ** 31 + 11):
                g = geometry(monkeypatch, defines, n, span, cus)
                assert g.n_tiles == -(-n // g.tile_rows)
                assert g.grid * g.tiles_per_wg >= g.n_tiles > (g.grid - 1) * g.tiles_per_wg
                assert 1 <= g.grid <= min(cus, 1024, cap or 1024)
                assert g.n_part == -(-span // g.part_keys) <= 2048
                assert g.work_cap == g.n_part + g.target_items + 2 <= 4096
                assert g.target_items == 4 * cus and g.chunk_rows == tl.CHUNK and g.tile_rows == tl.TILE
                assert g.part_keys == tl.PART and g.agg_tiles_per_sweep == 128 and g.dir_chunk == 4096


def test_geometry_refuses(monkeypatch):
    def status(defines, n=tl.N_RAGGED, span=tl.SPAN23, cus=CUS):
        with pytest.raises(wx.WarpExecError) as e:
            geometry(monkeypatch, defines, n, span, cus)
        return e.value.status

    for bad in ("WX_GP_GRID=0", "WX_GP_GRID=-3", "WX_GP_GRID=x", "WX_GP_DIRCH=0", "WX_GP_DIRCH=-1", "WX_GP_DIRCH=4097",
                "WX_GP_GRID=3,WX_GP_DIRCH=100000"):
        assert status(bad) == wx.WX_ERR_INVALID, bad
    for ok in ("WX_GP_DIRCH=1", "WX_GP_DIRCH=4096", "WX_GP_GRID=1"):
        geometry(monkeypatch, ok, tl.N_RAGGED)
    # only spans the partitioned kernels take: above the LDS window, at most 2048 partitions
    for span in (-1, 0, 1, 2048, 2 ** 24 + 1, 2 ** 32):
        assert status(None, span=span) == wx.WX_ERR_UNSUPPORTED, span
    assert status(None, n=0) == wx.WX_ERR_INVALID and status(None, n=-5) == wx.WX_ERR_INVALID
    # more work items than the plan kernel holds is an error, never a geometry
    assert status(None, span=2 ** 24, cus=512) == wx.WX_ERR_INTERNAL


def test_expected_plan_by_hand():
    # 3 workgroups of one 8-row tile, partitions of 10 keys, chunk 3
    g = SimpleNamespace(tile_rows=8, tiles_per_wg=1, grid=3, n_tiles=3, part_keys=10, chunk_rows=3, target_items=1000)
    keys = np.array([0, 3, 3, 3, 3, 3, 3, 14,     # workgroup 0: 7 rows of partition 0, 1 of partition 1
                     3, 25, 25, 25, 25, 25, 25, 25,   # workgroup 1: 1 of partition 0, 7 of partition 2
                     3, 3, 14, 14, 14, 14, 99, 99])   # workgroup 2: 2 of partition 0, 4 of partition 1, 2 dropped
    keep = np.ones(24, bool)
    keep[22:] = False
    plan, chunk = tl.expected_plan(g, keys, keep)
    assert chunk == 3 and sorted(plan) == [0, 1, 2]
    # partition 0: counts (7, 1, 2), e = (0, 7, 8), K = 4, b = #{e < 3, 6, 9} = 1, 1, 3
    assert list(plan[0]["e"]) == [0, 7, 8]
    assert plan[0]["items"] == [(0, 1), (1, 1), (1, 3), (3, 3)]
    assert tl.has_empty_middle(plan[0]) and tl.has_trailing(plan[0], 3) and not tl.has_exact_boundary(plan[0], 3)
    # partition 1: counts (1, 0, 4), e = (0, 1, 1), K = 2, b_1 = 3: the second item starts at G
    assert plan[1]["items"] == [(0, 3), (3, 3)] and tl.has_trailing(plan[1], 3)
    # partition 2: counts (0, 7, 0), e = (0, 0, 7), K = 3, b = #{e < 3, 6} = 2, 2
    assert plan[2]["items"] == [(0, 2), (2, 2), (2, 3)] and tl.has_empty_middle(plan[2])
    # e_g exactly on a chunk boundary belongs to the next item
    plan, _ = tl.expected_plan(g, np.array([5] * 6 + [99, 99] + [5] * 8 + [99] * 8), np.array([True] * 6 + [False] * 2 +
                                                                                             [True] * 8 + [False] * 8))
    assert list(plan[0]["e"]) == [0, 6, 14] and plan[0]["items"] == [(0, 1), (1, 1), (1, 2), (2, 2), (2, 3)]
    assert tl.has_exact_boundary(plan[0], 3)
    assert list(tl.tiles_with(g, keys, keep, 1)) == [True, False, True] and tl.longest_gap([1, 0, 0, 1, 0]) == 2


def _numpy_group_sum(lay, where):
    keep = lay.passing(where)
    k, inv = np.unique(lay.keys[keep], return_inverse=True)
    return k, np.bincount(inv, weights=tl.values(lay.n)[keep].astype(np.float64)), np.bincount(inv)


def _layouts(monkeypatch):
    """Every layout of the GPU tests at cus = 256; building one asserts what it is named for."""
    for n in (tl.N_RAGGED, tl.N_ONE_ROW, tl.N_WHOLE):
        g = geometry(monkeypatch, tl.GRID3, n)
        assert g.tiles_per_wg >= 3
        yield f"stage_{n}", tl.stage(n, g), g
    for name, (defines, n, counts, claims) in tl.heavy_cases().items():
        g = geometry(monkeypatch, defines, n)
        lay = tl.heavy(n, g, counts)
        tl.check_heavy(lay, g, claims)
        yield name, lay, g
    g = geometry(monkeypatch, tl.GRID3, tl.N_SPARSE)
    yield "sparse", tl.sparse(tl.N_SPARSE, g), g
    for defines in (tl.GRID2, tl.GRID2_DIR40):
        g = geometry(monkeypatch, defines, tl.N_LONG, tl.LONG_PARTS * tl.PART)
        yield "long", tl.long_items(tl.N_LONG, g), g


def test_layouts_hold_what_they_claim(monkeypatch):
    seen = set()
    for name, lay, g in _layouts(monkeypatch):
        seen.add(name)
        assert g.tiles_per_wg >= 3 and lay.n > (g.grid - 1) * g.tiles_per_wg * g.tile_rows, name
        assert tl.PART * (g.n_part - 1) < lay.span(False) <= tl.PART * g.n_part, name
        plan, _ = tl.expected_plan(g, lay.keys, lay.passing(False))
        assert max(plan) == g.n_part - 1 and sum(len(p["items"]) for p in plan.values()) <= g.work_cap, name
    assert len(seen) == 9
    # the claims between them: every edge of the plan is some layout's
    claims = {c for _, _, _, cs in tl.heavy_cases().values() for c in cs}
    assert claims == {"exact", "empty", "trailing"}
    assert {d for d, _, _, _ in tl.heavy_cases().values()} == {tl.GRID2, tl.GRID3}


def test_oracle_group_sum_is_the_numpy_fold(monkeypatch):
    # "equal to ora.group_sum, bit for bit" in the GPU tests then means "correct"
    for name, lay, _ in _layouts(monkeypatch):
        if name in ("long", "sparse", "stage_%d" % tl.N_WHOLE, "stage_%d" % tl.N_ONE_ROW):
            continue  # one table of each kind is enough here
        table = ora.HostTable(lay.cols())
        for where in (False, True):
            rk, rs, rc = ora.group_sum(table, "v", "k", tl.OCOND if where else None, capacity=1 << 20)
            nk, ns, nc = _numpy_group_sum(lay, where)
            assert np.array_equal(rk, nk) and np.array_equal(rc, nc), name
            assert np.array_equal(rs.view(np.int64), ns.view(np.int64)), name
