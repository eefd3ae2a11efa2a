"""Tables for the row-order GROUP BY's tests (WX_F_ROW_ORDER), built tile by
tile, and the numpy statements of the host arithmetic those tests lean on.

Shared by tests/test_ro_layouts.py (CPU: every layout holds what it claims)
and tests/test_gpu_group_rows_edges.py (GPU: every route over them), so that
both see the same tables.  numpy only.  Every size comes from the geometry
the caller passes (wx.group_rows_geometry()): tile rows T, bins of the span
path, the sample size.

The span path's scatter (wx_ro_scatter, wx_group_rows.hip) gives range r of R
the tiles [r * tiles // R, (r + 1) * tiles // R) and runs them in order; row p
of a tile belongs to wave p // (T / 8), item (p % (T / 8)) // 64 and lane
p % 64, and (wave, item, lane) is row order.  A row's bin is key - key_lo.

The columns of a layout:
  kk   int32 key: LO + bin on a passing row, a key outside [LO, LO + bins)
       on a row the WHERE drops (INT32_MIN, INT32_MAX, LO - 1, LO + bins in
       turn), so a kernel that looked at a dropped row's key would flag it
  rid  float32 row index: exact (every table has fewer than 2^24 rows), so the
       key-major value array names the row that landed in every slot
  va   float32 values over many binades: their double fold depends on order
  pp   1.0 where the row passes, else 0.0; the WHERE is pp > 0.5
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Tuple

import numpy as np

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
LO = -1000          # key of bin 0: the keys straddle zero
HOT = 700           # the bin most tile kinds share, so that its run continues from tile to tile
CAPS = (1, 2, 3, 5, 7)
TAILS = (1, 63, 64, 65, 4095, 4096, 4097, 8191)
N_TILES = 16        # of every table: >= 2 tiles per range at every cap, unequal ranges at caps 3, 5 and 7

KINDS = ("none", "one_key", "one_key_no_lane0", "lane_parity", "key_lane", "mod_bins", "extremes", "straddle",
         "first_row", "last_row", "one_wave", "random")
# kinds whose bins stay within [HOT - 28, HOT + 35]: a table of them has a narrow key span
NARROW = ("none", "one_key", "one_key_no_lane0", "lane_parity", "key_lane", "straddle", "first_row", "last_row",
          "one_wave")


def ro_range(n: int, ranges: int, r: int, tile_rows: int) -> Tuple[int, int]:
    """wx_ro_range: the tiles [t0, t1) of range r."""
    tiles = -(-n // tile_rows)
    return r * tiles // ranges, (r + 1) * tiles // ranges


def sampled_rows(n: int, sample_rows: int) -> np.ndarray:
    """wx_group_part_sample: thread i reads row i * n // S."""
    return (np.arange(sample_rows, dtype=np.int64) * n) // sample_rows


def rle_ranges(m: int, wave_rows: int) -> Tuple[int, int]:
    """(wave ranges, rows per range) of the run-length pass over m sorted rows (group_rows_general)."""
    n_blk = min(32768, max(1, -(-m // wave_rows)))
    return n_blk, (-(-m // n_blk) + 63) // 64 * 64


def tile(kind: str, rows: int, tile_rows: int, bins: int, rng) -> Tuple[np.ndarray, np.ndarray, int]:
    """(bin, passing, declared passing count) of one tile's first `rows` rows."""
    p = np.arange(rows, dtype=np.int64)
    wave_rows = tile_rows // 8
    lane, wave = p % 64, p // wave_rows
    b = np.full(rows, HOT, np.int64)
    keep = np.ones(rows, bool)
    count = rows
    if kind == "none":
        keep[:] = False
        count = 0
    elif kind == "one_key":            # the ballot alone: a wave's rows all in one packed 16-bit counter
        pass
    elif kind == "one_key_no_lane0":   # lane 0 not passing: 63 lanes add to one LDS address
        keep = lane != 0
        count = rows - (rows + 63) // 64
    elif kind == "lane_parity":        # lane 0's key by the ballot, the other by adds
        b = HOT + (lane & 1)
    elif kind == "key_lane":           # 64 keys per wave
        b = HOT - 28 + lane
    elif kind == "mod_bins":           # every bin, tile_rows / bins rows each
        b = p % bins
    elif kind == "extremes":           # only the first and the last bin
        b = np.where((p * 2654435761 >> 7) & 1, bins - 1, 0)
    elif kind == "straddle":           # bins 4j + 3 and 4j + 4: two threads' owned bins
        assert HOT % 4 == 0
        b = np.where((p * 40503 >> 5) & 1, HOT, HOT - 1)
    elif kind == "first_row":
        keep = p == 0
        count = 1
    elif kind == "last_row":
        keep = p == rows - 1
        count = 1
    elif kind == "one_wave":           # only wave 3's rows
        keep = wave == 3
        b = HOT - 10 + rng.integers(0, 21, rows)
        count = max(0, min(rows, 4 * wave_rows) - 3 * wave_rows)
    elif kind == "random":
        keep = rng.random(rows) < 0.6
        b = rng.integers(0, bins, rows)
        count = int(keep.sum())
    else:
        raise ValueError(kind)
    return b.astype(np.int64), keep, count


def spread(rng, n: int) -> np.ndarray:
    """1e7-, 1- and 1e-3-scale values interleaved, both signs."""
    scale = rng.choice(np.array([1e7, 1.0, 1e-3, -1.0, -1e7], np.float32), n)
    return (rng.uniform(0.0, 1.0, n).astype(np.float32) * scale).astype(np.float32)


def _frozen(cols: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    for v in cols.values():
        v.setflags(write=False)
    return cols


@dataclass
class Layout:
    name: str
    tile_rows: int
    bins: int
    kinds: List[str]          # per tile
    counts: List[int]         # per tile: the declared passing rows
    cols: Dict[str, np.ndarray]

    @property
    def n(self) -> int:
        return len(self.cols["kk"])

    @property
    def n_tiles(self) -> int:
        return -(-self.n // self.tile_rows)

    @property
    def keep(self) -> np.ndarray:
        return self.cols["pp"] > 0.5

    def order(self) -> np.ndarray:
        """The passing rows key-major, row order within a key: a stable sort of their keys."""
        idx = np.flatnonzero(self.keep)
        return idx[np.argsort(self.cols["kk"][idx], kind="stable")]

    def groups(self, scale: int = 1):
        """(keys, counts) of the passing rows, ascending."""
        k, c = np.unique(self.cols["kk"][self.keep].astype(np.int64) * scale, return_counts=True)
        return k.astype(np.int32), c.astype(np.int64)


def build(name: str, kinds: List[str], last_rows: int, geom, seed: int) -> Layout:
    T, bins = int(geom.tile_rows), int(geom.span_bins)
    rng = np.random.default_rng(seed)
    outside = np.array([I32_MIN, I32_MAX, LO - 1, LO + bins], np.int64)
    kk, pp, counts = [], [], []
    for i, kind in enumerate(kinds):
        rows = T if i + 1 < len(kinds) else last_rows
        b, keep, count = tile(kind, rows, T, bins, rng)
        assert 0 <= b.min() and b.max() < bins
        r = np.arange(rows, dtype=np.int64) + i * T
        kk.append(np.where(keep, LO + b, outside[(r * 7 + i) % 4]))
        pp.append(keep)
        counts.append(count)
    kk = np.concatenate(kk)
    pp = np.concatenate(pp)
    n = len(kk)
    assert n < 1 << 24
    cols = {"kk": kk.astype(np.int32), "rid": np.arange(n, dtype=np.float32), "va": spread(rng, n),
            "pp": pp.astype(np.float32)}
    return Layout(name, T, bins, list(kinds), counts, _frozen(cols))


# fifteen whole tiles of every kind -- the hot bin's run goes on through tiles
# of different kinds and through empty ones -- and a last tile per tail size
MIXED = ["mod_bins", "one_key", "none", "one_key_no_lane0", "lane_parity", "key_lane", "none", "extremes", "straddle",
         "first_row", "last_row", "one_wave", "random", "one_key", "none"]
LAST_KINDS = ["random", "one_key_no_lane0", "lane_parity", "straddle", "one_key", "key_lane", "mod_bins", "extremes",
              "one_key_no_lane0"]
NARROW_TILES = ["one_key", "none", "one_key_no_lane0", "lane_parity", "key_lane", "none", "straddle", "first_row",
                "last_row", "one_wave", "one_key", "straddle", "none", "lane_parity", "one_key_no_lane0", "key_lane"]


def all_layouts(geom) -> Dict[str, Layout]:
    T = int(geom.tile_rows)
    assert len(MIXED) == N_TILES - 1
    out = {}
    for i, tail in enumerate(TAILS + (T,)):
        name = "mixed_tail_%d" % tail if tail != T else "mixed_whole"
        out[name] = build(name, MIXED + [LAST_KINDS[i]], tail, geom, 7000 + i)
    # a key span of 64: the direct route centres it, the ordinary call's exact range is the span itself
    out["narrow_tail_65"] = build("narrow_tail_65", NARROW_TILES + ["one_key_no_lane0"], 65, geom, 7100)
    return out
