"""Table layouts for the range-partitioned GROUP BY tests, and the numpy
statement of its plan.

Shared by tests/test_group_part_geometry.py (CPU: every layout holds what it is
named for) and tests/test_gpu_group_part_edges.py (GPU: wx_group_sum against
the oracle on those layouts), so that a layout that stops hitting its edge
fails before it reaches a GPU.

The layouts are stated against the geometry wx_group_part_geometry reports: a
tile is `tile_rows` rows, tile workgroup g runs the tiles [g * tiles_per_wg,
(g + 1) * tiles_per_wg), a partition is `part_keys` keys counted from the
smallest passing key, and the plan cuts a partition's rows into work items of
whole workgroups (expected_plan below).  The diagnostic define WX_GP_GRID caps
the grid, so that a table of a few tiles gives every workgroup several.

Columns: `k` the key, `v` the value, `f` the WHERE flag (COND keeps f > 0).
Values are integers 1..61 that depend on the tile and the row: every double
sum is exact in any order, and a tile written out from the wrong stage
changes a sum.
"""
from __future__ import annotations

import numpy as np

TILE = 16384      # rows per tile
PART = 8192       # keys per partition
CHUNK = 65536     # the floor of a work item's rows
GRID3, GRID2, GRID2_DIR40 = "WX_GP_GRID=3", "WX_GP_GRID=2", "WX_GP_GRID=2,WX_GP_DIRCH=40"
DIRCH_SMALL = 40
COND, OCOND = "(f[idx] > 0.0f)", "f > 0"

N_RAGGED = 11 * TILE + 5    # GRID3: 4 tiles per workgroup, the last tile 5 rows (a partial quad)
N_ONE_ROW = 13 * TILE + 1   # GRID3: 5 tiles per workgroup, the last workgroup 4, the last tile one row
N_WHOLE = 12 * TILE         # GRID3: exactly 12 tiles
N_ITEMS3 = 27 * TILE + 5    # GRID3: 10 tiles per workgroup: one workgroup holds more than two chunks
N_ITEMS2 = 18 * TILE + 5    # GRID2: 10 and 9 tiles
N_SPARSE = 58 * TILE + 5    # GRID3: 20 tiles per workgroup
N_LONG = 131 * TILE + 7     # GRID2: 66 tiles per workgroup, 132 tiles per item
SPAN23 = 23 * PART - 100    # 23 partitions, the last one short
HASH = 2654435761


def values(n):
    i = np.arange(n, dtype=np.int64)
    return (1 + ((i // TILE) * 7 + i * 13) % 61).astype(np.float32)


class Layout:
    def __init__(self, keys, flag=None):
        self.keys = np.ascontiguousarray(keys, np.int64)
        self.n = len(self.keys)
        self.flag = np.ones(self.n, np.float32) if flag is None else np.ascontiguousarray(flag, np.float32)

    def passing(self, where):
        return self.flag > 0 if where else np.ones(self.n, bool)

    def lo(self, where):
        return int(self.keys[self.passing(where)].min())

    def span(self, where):
        k = self.keys[self.passing(where)]
        return int(k.max() - k.min() + 1)

    def cols(self, key_dtype=np.int32, val_dtype=np.float32):
        assert self.keys.min() >= -(2 ** 31) and self.keys.max() <= 2 ** 31 - 1
        return {"v": values(self.n).astype(val_dtype), "k": self.keys.astype(key_dtype), "f": self.flag}


# ------------------------------------------------------------------ the plan
def expected_plan(g, keys, passing):
    """wx_group_part_plan's arithmetic in numpy.  Returns (plan, chunk): plan[p]
    = {"counts": rows of partition p per workgroup, "e": their exclusive prefix
    e_g, "items": [(g0, g1), ...]} for every partition with a passing row, with
    K = ceil(rows / chunk) items, item k = [b_(k-1), b_k), b_k = #{g : e_g < k *
    chunk}, b_0 = 0, b_K = G."""
    keys = np.asarray(keys, np.int64)
    rows = np.flatnonzero(passing)
    if not len(rows):
        return {}, int(g.chunk_rows)
    part = (keys[rows] - keys[rows].min()) // g.part_keys
    wg = (rows // g.tile_rows) // g.tiles_per_wg
    n_part, grid = int(part.max()) + 1, int(g.grid)
    assert wg.max() < grid
    counts = np.bincount(wg * n_part + part, minlength=grid * n_part).reshape(grid, n_part)
    chunk = max(-(-len(rows) // int(g.target_items)), int(g.chunk_rows))
    plan = {}
    for p in np.flatnonzero(counts.sum(axis=0)):
        c = counts[:, p]
        e = np.cumsum(c) - c
        k_items = -(-int(c.sum()) // chunk)
        b = [0] + [int((e < k * chunk).sum()) for k in range(1, k_items)] + [grid]
        plan[int(p)] = {"counts": c, "e": e, "items": [(b[k], b[k + 1]) for k in range(k_items)]}
    return plan, chunk


def tiles_with(g, keys, passing, p):
    """Per tile: does partition p hold a passing row of it?"""
    keys = np.asarray(keys, np.int64)
    rows = np.flatnonzero(passing)
    part = (keys[rows] - keys[rows].min()) // g.part_keys
    out = np.zeros(int(g.n_tiles), bool)
    out[rows[part == p] // g.tile_rows] = True
    return out


def longest_gap(present):
    """The longest run of consecutive False."""
    best = cur = 0
    for x in present:
        cur = 0 if x else cur + 1
        best = max(best, cur)
    return best


# ------------------------------------------------------------------- layouts
def uniform(n, span, lo=0):
    """Hashed keys over [lo, lo + span), both ends present (the larger in the
    last row); a span of 2^20 or more holds 5000 evenly spaced keys."""
    i = np.arange(n, dtype=np.int64)
    if span >= 1 << 20:
        keys = lo + ((i * HASH) % 5000) * (span // 5000)
    else:
        keys = lo + (i * HASH) % span
    keys[0], keys[n - 1] = lo, lo + span - 1
    return Layout(keys)


STAGE_KINDS = ("one_part", "none", "4k+1", "uniform")
STAGE_KEPT = 4 * 1000 + 1


def stage_kind(t, tpw):
    """Tile t's kind: the four kinds in turn, rotated by one per workgroup."""
    return STAGE_KINDS[(t % tpw + t // tpw) % 4]


def stage(n, g):
    """Consecutive tiles of a workgroup that differ as much as tiles can: all
    rows in one partition (one run from 0 of the whole tile), a tile whose
    WHERE keeps nothing, a tile whose WHERE keeps 4k + 1 rows, a hashed tile."""
    lay = uniform(n, SPAN23)
    tpw, tile = int(g.tiles_per_wg), int(g.tile_rows)
    pinned = False
    for t in range(int(g.n_tiles)):
        a, b = t * tile, min(n, (t + 1) * tile)
        kind = stage_kind(t, tpw)
        if kind == "one_part":
            lay.keys[a:b] = PART * (t % 23) + np.arange(b - a) % 1000
        elif kind == "none":
            lay.flag[a:b] = 0
        elif kind == "4k+1":
            lay.flag[a:b] = 0
            lay.flag[a + 1:b:4][:STAGE_KEPT] = 1
        elif not pinned:  # both ends of the key range in rows that pass with and without the WHERE
            lay.keys[a], lay.keys[b - 1] = 0, SPAN23 - 1
            pinned = True
    assert pinned
    check_stage(lay, g)
    return lay


def check_stage(lay, g):
    tpw, tile = int(g.tiles_per_wg), int(g.tile_rows)
    assert tpw >= 3
    seen = set()
    for where in (False, True):
        assert lay.lo(where) == 0 and lay.span(where) == SPAN23
        keep = lay.passing(where)
        for t in range(int(g.n_tiles)):
            a, b = t * tile, min(lay.n, (t + 1) * tile)
            kind = stage_kind(t, tpw)
            kept = int(keep[a:b].sum())
            if kind == "one_part":
                assert kept == b - a and len(set(lay.keys[a:b] // PART)) == 1, t
            if kind == "none" and where:
                assert kept == 0, t       # tile t keeps no row
            if kind == "4k+1" and where and b - a == tile:
                assert kept == STAGE_KEPT and kept % 4 == 1, t
            if b - a == tile:
                seen.add((kind, t % tpw == 0, t % tpw == tpw - 1))
    kinds = {k for k, _, _ in seen}
    assert kinds == set(STAGE_KINDS)
    assert ("none", True, False) in seen       # a workgroup's first tile keeps nothing
    t_last = int(g.n_tiles) - 1
    assert stage_kind(t_last, tpw) == "none"   # and so does the table's last (ragged) tile


def heavy(n, g, counts, where_thins=True):
    """counts[w] rows of workgroup w on one key (5; row 0 holds key 0 of the
    same partition), the rest hashed over the partitions above it, the largest
    key in the last row.  The WHERE drops every third heavy row."""
    tpw, tile, grid = int(g.tiles_per_wg), int(g.tile_rows), int(g.grid)
    assert len(counts) == grid
    i = np.arange(n, dtype=np.int64)
    keys = PART + (i * HASH) % (SPAN23 - PART)
    keys[n - 1] = SPAN23 - 1
    flag = np.ones(n, np.float32)
    for w, c in enumerate(counts):
        a, b = w * tpw * tile, min(n - 1, (w + 1) * tpw * tile)   # row n - 1 stays the largest key
        assert 0 <= c <= b - a, (w, c, b - a)
        rows = a + (np.arange(c, dtype=np.int64) * (b - a)) // max(c, 1)
        keys[rows] = 5
        if where_thins:
            flag[rows[rows % 3 == 0]] = 0
    assert counts[0] > 0
    keys[0], flag[0] = 0, 1
    lay = Layout(keys, flag)
    plan, chunk = expected_plan(g, lay.keys, lay.passing(False))
    assert chunk == CHUNK and list(plan[0]["counts"]) == list(counts)
    return lay


def has_exact_boundary(item_plan, chunk):
    """Some workgroup's prefix e_g (g > 0) is a multiple k * chunk, 1 <= k < K."""
    k_items = len(item_plan["items"])
    return any(e > 0 and e % chunk == 0 and e // chunk < k_items for e in item_plan["e"][1:])


def has_empty_middle(item_plan):
    items = item_plan["items"]
    return any(g0 == g1 and g0 < items[-1][1] for g0, g1 in items[:-1])


def has_trailing(item_plan, grid):
    return item_plan["items"][-1] == (grid, grid)


# name -> (defines, n, per-workgroup rows of the heavy partition, claims)
def heavy_cases():
    w3 = 4 * TILE                        # rows of a GRID3 workgroup at N_RAGGED
    return {
        # all rows but the last on the heavy partition: e = (0, chunk, 2 chunk)
        "all_exact": (GRID3, N_RAGGED, (w3, w3, N_RAGGED - 2 * w3 - 1), ("exact",)),
        # 90 %: workgroup 0 holds more than two chunks (an empty item), the prefixes end below (K - 1) chunk
        "most_empty_trailing": (GRID3, N_ITEMS3, (10 * TILE, 120_000, 114_213), ("empty", "trailing")),
        "all_empty_trailing": (GRID2, N_ITEMS2, (10 * TILE, N_ITEMS2 - 10 * TILE - 1), ("empty", "trailing")),
        # 89 %: e_1 = 2 chunk exactly, so item 2 is empty and item 3 starts at workgroup 1
        "most_exact_empty": (GRID2, N_ITEMS2, (2 * CHUNK, 131_070), ("exact", "empty", "trailing")),
    }


def check_heavy(lay, g, claims):
    plan, chunk = expected_plan(g, lay.keys, lay.passing(False))
    hp = plan[0]
    assert len(hp["items"]) >= 3
    if "exact" in claims:
        assert has_exact_boundary(hp, chunk), hp
    if "empty" in claims:
        assert has_empty_middle(hp), hp
    if "trailing" in claims:
        assert has_trailing(hp, int(g.grid)), hp
    # thinned by the WHERE the counts are ragged: still several items
    tp, _ = expected_plan(g, lay.keys, lay.passing(True))
    assert len(tp[0]["items"]) >= 2 and all(c % 1024 for c in tp[0]["counts"])
    return hp


SPARSE_EVERY = 19


def sparse(n, g):
    """Partition 0 only in every 19th tile and in the last; partition 1 only in
    the first tile of each workgroup; the rest hashed over partitions 2..22."""
    tpw, tile, n_tiles = int(g.tiles_per_wg), int(g.tile_rows), int(g.n_tiles)
    i = np.arange(n, dtype=np.int64)
    keys = 2 * PART + (i * HASH) % (SPAN23 - 2 * PART)
    keys[n - 1] = SPAN23 - 1
    for t in range(n_tiles):
        a, b = t * tile, min(n - 1, (t + 1) * tile)
        if t % SPARSE_EVERY == 0 or t == n_tiles - 1:
            rows = a + (np.arange(min(37, b - a)) * 431) % (b - a)
            keys[rows] = (rows * 7) % PART
        if t % tpw == 0:
            rows = a + 1 + (np.arange(53) * 293) % (b - a - 1)
            keys[rows] = PART + (rows * 11) % PART
    keys[0] = 0
    lay = Layout(keys)
    check_sparse(lay, g)
    return lay


def check_sparse(lay, g):
    tpw, n_tiles = int(g.tiles_per_wg), int(g.n_tiles)
    assert lay.lo(False) == 0 and lay.span(False) == SPAN23
    t = np.arange(n_tiles)
    p0 = tiles_with(g, lay.keys, lay.passing(False), 0)
    assert np.array_equal(p0, (t % SPARSE_EVERY == 0) | (t == n_tiles - 1))
    assert longest_gap(p0) >= 17          # at least 17 consecutive tiles with no row of partition 0
    p1 = tiles_with(g, lay.keys, lay.passing(False), 1)
    assert np.array_equal(p1, t % tpw == 0) and p1.sum() == int(g.grid) >= 3
    plan, _ = expected_plan(g, lay.keys, lay.passing(False))
    assert plan[0]["items"] == [(0, int(g.grid))] and plan[1]["items"] == [(0, int(g.grid))]
    assert n_tiles % 8 != 0               # the item's last group of 8 tiles is short


LONG_PARTS = 64


def long_items(n, g):
    """Hashed keys over 64 partitions of fewer than `chunk` rows each: every
    partition is one item over all the table's tiles."""
    lay = uniform(n, LONG_PARTS * PART)
    plan, chunk = expected_plan(g, lay.keys, lay.passing(False))
    assert sorted(plan) == list(range(LONG_PARTS))
    for p in plan.values():
        assert p["items"] == [(0, int(g.grid))] and p["counts"].sum() <= chunk
    assert int(g.n_tiles) > int(g.agg_tiles_per_sweep)   # a wave's second sweep
    return lay
