"""Tables for the ordered compaction's tests, built tile by tile, and the
numpy statement of the store split of its pipelined kernels.

Shared by tests/test_compact_layouts.py (CPU: every layout holds the edge it
is named for) and tests/test_gpu_compact_edges.py (GPU: every compaction
family over them), so that both see the same tables.  numpy only.

A layout is a list of per-tile pass masks for a tile of T rows (the last one
may be shorter: a ragged table).  Row r of a tile belongs to row group
r // (4 * DTHREADS), data thread (r % (4 * DTHREADS)) // 4 -- wave thread // 64,
lane thread % 64 -- and element r % 4 of that thread's quad
(wx_compact.hip); the kernels rank a tile's passing rows in that order, which
is row order.  T = 512 is one group of two data waves, T = 1024 two groups.

The columns of a layout:
  pp  1.0 where the row is kept, else 0.0; the WHERE is pp > 0.5
  va  row / 8: distinct per row and exact in float32, so a misplaced row is
      a wrong value and not merely a wrong id
  kk  int32 key: a key of the right table (RIGHT_KEYS, all inside [0, 2047),
      so the window's dense form) on every kept row, an absent one elsewhere
For JOIN INNER the table is inner_cols(): pp is also 1.0 on `probe_drop`, a
seeded subset of the dropped rows, whose absent key makes the probe and not
the WHERE drop them; the rows kept are the layout's.  For JOIN LEFT it is
left_cols(): a seeded third of the kept rows carry an absent key (right row
-1, right-side values NaN), and every kept row stays.

The store split (wx_project_compact_deep, WX_CM_DEEP): a tile at exclusive
offset excl with tot passing rows writes positions [excl, end) as a scalar
head up to b0, a body of 16-byte stores up to b1 and a scalar tail.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

DWAVES = 2
DEFINES = {512: "WX_COMPACT_GROUPS=1,WX_COMPACT_DWAVES=2", 1024: "WX_COMPACT_GROUPS=2,WX_COMPACT_DWAVES=2"}
MAX_ROWS = 200_000
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1

RIGHT_SPAN = 2047                     # right keys lie in [0, 2047): key k is present unless k % 3 == 1
_ALL = np.arange(RIGHT_SPAN, dtype=np.int64)
PRESENT = _ALL[_ALL % 3 != 1]         # 0 and 2046 among them
ABSENT = np.concatenate([_ALL[_ALL % 3 == 1], [I32_MIN, I32_MAX, -1, RIGHT_SPAN, 5000, -4096]]).astype(np.int64)


def right_columns() -> Dict[str, np.ndarray]:
    """The right table of the join cases: rk unique, in no key order; rr on a 1/8 grid."""
    rng = np.random.default_rng(606)
    k = PRESENT[rng.permutation(len(PRESENT))]
    r = np.arange(len(k), dtype=np.int64)
    return {"rk": k.astype(np.int32), "rr": (((r * 37) % 1025 - 512) / 8.0).astype(np.float32)}


# ------------------------------------------------------------ the store split
def split(excl: int, tot: int) -> Tuple[int, int, int]:
    """(head, body, tail) of a tile's output run."""
    end = excl + tot
    b0 = min((excl + 31) & ~31, end)
    b1 = b0 + ((end - b0) & ~3)
    return b0 - excl, b1 - b0, end - b1


def store_classes(tile_rows: int, res: int, tot: int, head: int, body: int, tail: int) -> set:
    """The store shapes one tile's run belongs to (the classes layout (b) must cover)."""
    c = set()
    clamped = tot < (32 - res) % 32   # the next 32-boundary lies past the run's end: b0 is clamped to end
    if tot == 0:
        c.add("empty")
        if res == 31:
            c.add("clamped@31")       # one element short of the boundary: only an empty run ends before it
    if clamped and tot > 0:
        c.add("clamped@%d" % res)
    if res and tot == 32 - res:
        c.add("head to the boundary, nothing after")
    if res == 0 and 1 <= tot <= 3:
        c.add("tail only %d" % tot)
    if res == 0 and tot and tot % 4 == 0:
        c.add("body only")
    if body and tail and head in (1, 31):
        c.add("head %d + body + tail" % head)
    if body and tail:
        c.add("tail %d" % tail)
    if tot == tile_rows and res in (0, 1, 31):
        c.add("full@%d" % res)
    return c


STORE_CLASSES = frozenset(
    ["empty", "clamped@1", "clamped@17", "clamped@30", "clamped@31", "head to the boundary, nothing after",
     "tail only 1", "tail only 2", "tail only 3", "body only", "head 1 + body + tail", "head 31 + body + tail",
     "tail 1", "tail 2", "tail 3", "full@0", "full@1", "full@31"])


# ------------------------------------------------------------------ layouts
@dataclass
class Layout:
    name: str
    tile_rows: int
    keep: np.ndarray                      # bool per row: the rows every family must return
    probe_drop: np.ndarray                # bool per row: dropped rows that pass the INNER join's WHERE
    left_miss: np.ndarray                 # bool per row: kept rows whose LEFT join key is absent
    shapes: List[Tuple[int, int, int, int, int]] = field(default_factory=list)  # (excl % 32, tot, head, body, tail)

    @property
    def n(self) -> int:
        return len(self.keep)

    @property
    def n_tiles(self) -> int:
        return -(-self.n // self.tile_rows)

    @property
    def tots(self) -> np.ndarray:
        return np.array([s[1] for s in self.shapes], np.int64)

    @property
    def rows(self) -> np.ndarray:
        return np.nonzero(self.keep)[0].astype(np.int64)

    def classes(self) -> set:
        out = set()
        for s in self.shapes:
            out |= store_classes(self.tile_rows, *s)
        return out

    def _va(self):
        return (np.arange(self.n, dtype=np.int64) / 8.0).astype(np.float32)

    def _keys(self, absent_at):
        r = np.arange(self.n, dtype=np.int64)
        k = PRESENT[(r * 7919 + 13) % len(PRESENT)]
        return np.where(absent_at, ABSENT[(r * 31 + 5) % len(ABSENT)], k).astype(np.int32)

    def cols(self) -> Dict[str, np.ndarray]:
        """single-output, SELECT and window: WHERE pp > 0.5, PARTITION BY kk."""
        return _frozen({"kk": self._keys(~self.keep), "va": self._va(), "pp": self.keep.astype(np.float32)})

    def inner_cols(self) -> Dict[str, np.ndarray]:
        """JOIN INNER ON kk = rk WHERE pp > 0.5: the probe drops probe_drop, the WHERE the rest."""
        return _frozen({"kk": self._keys(~self.keep), "va": self._va(),
                        "pp": (self.keep | self.probe_drop).astype(np.float32)})

    def left_cols(self) -> Dict[str, np.ndarray]:
        """JOIN LEFT ON kk = rk WHERE pp > 0.5: left_miss rows stay, unmatched."""
        return _frozen({"kk": self._keys(~self.keep | self.left_miss), "va": self._va(),
                        "pp": self.keep.astype(np.float32)})


def _frozen(cols):
    for c in cols.values():
        c.setflags(write=False)
    return cols


def from_masks(name: str, tile_rows: int, masks: List[np.ndarray], seed: int = 1) -> Layout:
    assert masks and all(len(m) == tile_rows for m in masks[:-1]) and 1 <= len(masks[-1]) <= tile_rows
    keep = np.concatenate([np.asarray(m, bool) for m in masks])
    assert len(keep) <= MAX_ROWS
    rng = np.random.default_rng(9000 + seed)
    probe_drop = ~keep & (rng.random(len(keep)) < 0.4)
    left_miss = keep & (rng.random(len(keep)) < 0.33)
    shapes, excl = [], 0
    for m in masks:
        tot = int(np.count_nonzero(m))
        shapes.append((excl % 32, tot) + split(excl, tot))
        excl += tot
    lay = Layout(name, tile_rows, keep, probe_drop, left_miss, shapes)
    assert lay.n_tiles == len(masks) and excl == int(keep.sum())
    return lay


def _random_tile(rng, tile_rows, tot, rows=None):
    """tot passing rows at seeded random positions of a tile (of its first `rows` rows)."""
    rows = tile_rows if rows is None else rows
    m = np.zeros(rows, bool)
    m[rng.choice(rows, tot, replace=False)] = True
    return m


def _full(t):
    return np.ones(t, bool)


def _none(t):
    return np.zeros(t, bool)


def _one(t, row):
    m = np.zeros(t, bool)
    m[row] = True
    return m


def steady(tile_rows: int) -> Layout:
    """(a) 48 tiles, each of its own seeded selectivity in (0, 1); the last tile ragged."""
    rng = np.random.default_rng(100 + tile_rows)
    sel = rng.random(48)
    masks = [rng.random(tile_rows) < p for p in sel[:-1]]
    masks.append(rng.random(tile_rows - 101) < sel[-1])   # 411 / 923 rows: the last quad is partial
    lay = from_masks("steady", tile_rows, masks, 1)
    assert lay.n_tiles == 48 and lay.n % tile_rows and lay.n % 4 and lay.shapes[-1][1] > 0
    assert lay.tots.min() < tile_rows // 8 and lay.tots.max() > tile_rows - tile_rows // 8   # sparse and dense tiles
    return lay


# (excl % 32, tot) of the tiles layout (b) is built around; tot None: tile_rows.  Filler tiles steer the residue.
_STORE_TARGETS = [
    (5, 0), (31, 0), (1, 10), (17, 5), (30, 1), (7, 25), (0, 1), (0, 2), (0, 3), (0, 64), (0, 8),
    (31, 43), (1, 134), (0, 5), (0, 6), (0, 7), (31, 1 + 36 + 1), (1, 31 + 8 + 2), (12, 20 + 12 + 3),
    (0, None), (1, None), (31, None),
]


def store_shapes(tile_rows: int = 512) -> Layout:
    """(b) a chain of tiles whose (excl % 32, head, body, tail) covers STORE_CLASSES."""
    rng = np.random.default_rng(200 + tile_rows)
    masks, excl = [], 0
    for res, tot in _STORE_TARGETS:
        tot = tile_rows if tot is None else tot
        fill = (res - excl) % 32
        if fill:
            masks.append(_random_tile(rng, tile_rows, fill))
            excl += fill
        assert excl % 32 == res
        masks.append(_random_tile(rng, tile_rows, tot))
        excl += tot
    masks.append(_random_tile(rng, tile_rows, 9, rows=77))   # ragged end
    lay = from_masks("store_shapes", tile_rows, masks, 2)
    missing = STORE_CLASSES - lay.classes()
    assert not missing, missing
    return lay


def empty_run(tile_rows: int = 512) -> Layout:
    """(c) two runs of 70 all-drop tiles: the look-back crosses more than one 64-word window of zero aggregates."""
    rng = np.random.default_rng(300 + tile_rows)
    mixed = lambda: rng.random(tile_rows) < rng.uniform(0.2, 0.8)  # noqa: E731
    masks = [mixed() for _ in range(3)] + [_none(tile_rows)] * 70 + [mixed() for _ in range(5)] + \
            [_none(tile_rows)] * 70
    masks.append(_random_tile(rng, tile_rows, 50, rows=203))
    lay = from_masks("empty_run", tile_rows, masks, 3)
    assert [n for n in zero_runs(lay.tots) if n >= 65] == [70, 70] and lay.shapes[-1][1] > 0 and lay.n % tile_rows
    return lay


def zero_runs(tots) -> List[int]:
    """Lengths of the maximal runs of empty tiles."""
    runs, n = [], 0
    for t in list(tots) + [1]:
        if t == 0:
            n += 1
        elif n:
            runs.append(n)
            n = 0
    return runs


def full_tiles(tile_rows: int) -> Layout:
    """(d) runs of all-pass tiles between all-drop and single-row tiles (row 0 or row T - 1, the largest staged offset)."""
    t = tile_rows
    F, E, S0, SL = _full(t), _none(t), _one(t, 0), _one(t, t - 1)
    masks = [F, F, F, E, F, S0, F, F, SL, E, E, F, SL, S0, F, F, F, F, E, S0, SL, F]
    lay = from_masks("full_tiles", t, masks, 4)
    tots = lay.tots
    assert (tots == t).sum() == 12 and (tots == 1).sum() == 6 and (tots == 0).sum() == 4
    assert {s[0] for s in lay.shapes if s[1] == t} >= {0, 1, 2}   # full tiles at, and just off, a 32-boundary
    return lay


def last_tile(variant: str, tile_rows: int = 512) -> Layout:
    """(e) exact: n = m * T; one_pass: n = (m - 1) * T + 1, that row passing; one_drop: that row dropped after a
    full tile (the tile that writes the count is empty); single: one tile of one row."""
    t, m = tile_rows, 5
    rng = np.random.default_rng(500 + t)
    body = [rng.random(t) < 0.5 for _ in range(m - 2)]
    if variant == "exact":
        masks = body + [rng.random(t) < 0.5, rng.random(t) < 0.5]
    elif variant == "one_pass":
        masks = body + [rng.random(t) < 0.5, np.array([True])]
    elif variant == "one_drop":
        masks = body + [_full(t), np.array([False])]
    elif variant == "single":
        masks = [np.array([True])]
    else:
        raise KeyError(variant)
    lay = from_masks("last_" + variant, t, masks, 5)
    if variant == "exact":
        assert lay.n == m * t
    elif variant in ("one_pass", "one_drop"):
        assert lay.n == (m - 1) * t + 1 and lay.shapes[-1][1] == (variant == "one_pass")
    if variant == "one_drop":
        assert lay.shapes[-1][1] == 0 and lay.shapes[-2][1] == t and lay.keep.sum() > 0
    if variant == "single":
        assert lay.n == 1 and lay.n_tiles == 1 and lay.keep.all()
    return lay


LAST_VARIANTS = ("exact", "one_pass", "one_drop", "single")


def position_masks(tile_rows: int = 1024) -> Dict[str, np.ndarray]:
    """(f) tiles that pass only one kind of position of the (group, wave, lane, element) grid."""
    r = np.arange(tile_rows)
    per_group = 4 * 64 * DWAVES
    group, thread, elem = r // per_group, (r % per_group) // 4, r % 4
    wave, lane = thread // 64, thread % 64
    return {
        "element 3": elem == 3,
        "lane 63": lane == 63,
        "last wave": wave == DWAVES - 1,
        # ranked group-major: group 0's wave 1 (rows 256..511) comes before group 1's wave 0 (rows 512..767)
        "crossed": ((group == 1) & (wave == 0)) | ((group == 0) & (wave == 1)),
    }


def positions(tile_rows: int = 1024) -> Layout:
    assert tile_rows == 1024
    rng = np.random.default_rng(600)
    pm = position_masks(tile_rows)
    order = ["element 3", "lane 63", "last wave", "crossed", "crossed", "lane 63", "element 3", "last wave"]
    masks = []
    for i, k in enumerate(order):
        masks.append(pm[k])
        if i % 3 == 2:
            masks.append(_random_tile(rng, tile_rows, 37 + i))   # moves the next tile off the 32-boundary
    masks.append(pm["crossed"][: tile_rows - 300])               # ragged: the table ends inside group 1's wave 0
    lay = from_masks("positions", tile_rows, masks, 6)
    assert pm["element 3"].sum() == 256 and pm["lane 63"].sum() == 8 * DWAVES and pm["last wave"].sum() == 512
    assert pm["crossed"].sum() == 512 and pm["crossed"][256:768].all() and not pm["crossed"][:256].any()
    return lay


def all_layouts() -> Dict[str, Layout]:
    """Every (layout, tile size) the GPU tests run, by name."""
    out = {}
    for t in (512, 1024):
        out["steady_%d" % t] = steady(t)
        out["full_tiles_%d" % t] = full_tiles(t)
    out["store_shapes_512"] = store_shapes(512)
    out["empty_run_512"] = empty_run(512)
    for v in LAST_VARIANTS:
        out["last_%s_512" % v] = last_tile(v, 512)
    out["positions_1024"] = positions(1024)
    return out
