"""Key layouts for the top-K tests, and the numpy statement of top-K's order.

Shared by tests/test_topk_oracle.py (CPU: the oracle against numpy) and
tests/test_gpu_topk_edges.py (GPU: wx_topk against the oracle), so that both
see the same tables.  Every generator is seeded through tests/synth.py and
returns the float32 ORDER BY column `price`; `quantity` (the WHERE column) comes
from `table()`.

The layouts are stated against the scan's geometry (wx_topk_plan): span
position p covers rows [p * span, (p + 1) * span), workgroup b of a grid of g
runs positions b, b + g, ...; with WX_UNROLL=1 thread t of a workgroup reads
the one quad p * 256 + t of a position, rows 4 * (t + 256 * p) + e.
"""
from __future__ import annotations

import numpy as np

import synth

N = 42_003          # 42 span positions of 1 024 rows; the last holds 19 rows and ends in a 3-row quad
SPAN = 1024         # rows per batch span under WX_UNROLL=1
GRID = 2            # workgroups under WX_TOPK_GRID=2
SHRUNK = "WX_UNROLL=1,WX_TOPK_GRID=2"
COND, OCOND = "(quantity[idx] > 50.0f)", "quantity > 50"

F = np.float32
NAN = F("nan")


def _base(n, seed=41):
    return synth.uniform_f32(n, seed, 0.0, 40.0)


def good(j, desc):
    """Keys beyond the base range [0, 40), better for larger j in the query's direction."""
    j = np.asarray(j, dtype=np.float32)
    return (F(100.0) + j if desc else F(-100.0) - j).astype(F)


def one_thread_rows(k, span=SPAN, grid=GRID, thread=37, first=3):
    """K rows that one thread of one workgroup reads in consecutive batches
    (span positions first, first + grid, ...), four rows of its quad each."""
    quads_per_span = span // 4
    rows = [4 * (thread + quads_per_span * (first + grid * b)) + e for b in range((k + 3) // 4) for e in range(4)]
    return np.array(rows[:k], dtype=np.int64)


def late_rows(n, k):
    """The last K rows: the ragged final span with row n - 1 and the partial
    last quad (and, for K beyond its 19 rows, the end of the span before it,
    which the other workgroup scans)."""
    return np.arange(n - k, n, dtype=np.int64)


def tie_rows(n, s0, span=SPAN):
    """One row per span position from s0 on (the copies of the K-th best value)."""
    return np.arange(s0 * span + 17, n, span, dtype=np.int64)


def uniform(n, k, desc):
    return _base(n)


def ascending(n, k, desc):
    return np.sort(_base(n))


def descending(n, k, desc):
    return np.sort(_base(n))[::-1].copy()


def all_equal(n, k, desc):
    return np.full(n, 7.5, F)


def specials(n, k, desc):
    """A handful of distinct values with NaN, -0.0 and +0.0 mixed in."""
    u = synth.uniform_f32(n, 9, 0.0, 1.0)
    p = np.floor(synth.uniform_f32(n, 1, -3.0, 3.0)).astype(F)
    p[u < 0.05] = NAN
    p[(u >= 0.05) & (u < 0.3)] = F(-0.0)
    p[(u >= 0.3) & (u < 0.4)] = F(0.0)
    return p


def late_winners(n, k, desc):
    p = _base(n)
    rows = late_rows(n, k)
    p[rows] = good(synth.uniform_int(k, 5, 0, 7), desc)  # out of order, with ties
    return p


def one_thread_improving(n, k, desc):
    p = _base(n)
    p[one_thread_rows(k)] = good(np.arange(k), desc)
    return p


def one_thread_worsening(n, k, desc):
    p = _base(n)
    p[one_thread_rows(k)] = good(np.arange(k)[::-1], desc)
    return p


def _tie_bound(n, k, desc, s0):
    # K - 1 strictly best rows late in the table (every other row from the
    # end), the K-th best value once per span position from s0 on, the rest
    # worse.  The K-th output must be the copy of span s0.
    p = _base(n)
    p[tie_rows(n, s0)] = good(0, desc)
    p[n - 1 - 2 * np.arange(k - 1, dtype=np.int64)] = good(1 + np.arange(k - 1), desc)
    return p


def tie_bound_first_span(n, k, desc):
    return _tie_bound(n, k, desc, 0)


def tie_bound_other_workgroup(n, k, desc):
    return _tie_bound(n, k, desc, 1)


def sentinel(n, k, desc):
    """Fewer than K finite keys (and one key of the best infinity when K >= 3)
    over a table of the worst infinity -- the scan's own "no bound" / "row
    failed WHERE" value -- and NaN on every fifth row."""
    worst, best = (F("-inf"), F("inf")) if desc else (F("inf"), F("-inf"))
    p = np.full(n, worst, F)
    p[4::5] = NAN
    n_best = 1 if k >= 3 else 0
    n_fin = max(0, (k - 1 - n_best) // 2)
    fin = (n - 2 - 1031 * np.arange(n_fin, dtype=np.int64)) % n   # spread over both workgroups' spans
    if n_fin:
        p[fin] = good(synth.uniform_int(n_fin, 6, 0, 3), desc)
    if n_best:
        p[n // 2 + 1] = best
    return p


def all_nan(n, k, desc):
    return np.full(n, NAN, F)


def nan_but_k_minus_1(n, k, desc):
    p = np.full(n, NAN, F)
    # every 1 301st row back from n - 1 302: whole spans of both workgroups, their lanes' lists full of NaN by then
    rows = (n - 1 - 1301 * (1 + np.arange(k - 1, dtype=np.int64))) % n
    if k > 1:
        p[rows] = good(synth.uniform_int(k - 1, 8, 0, 5), desc)
    return p


LAYOUTS = {f.__name__: f for f in (
    uniform, ascending, descending, all_equal, specials, late_winners, one_thread_improving, one_thread_worsening,
    tie_bound_first_span, tie_bound_other_workgroup, sentinel, all_nan, nan_but_k_minus_1)}


def seed_miss(n, k, desc, span, seed_grid, seed_stride):
    """The K best rows outside every span the seed pass samples (workgroup j of
    the seed reads rows [j * seed_stride, j * seed_stride + span))."""
    sampled = np.zeros(n, bool)
    for j in range(seed_grid):
        sampled[j * seed_stride: j * seed_stride + span] = True
    free = np.flatnonzero(~sampled)
    assert len(free) >= k, "the seed pass samples (nearly) the whole table"
    rows = free[np.linspace(0, len(free) - 1, k).astype(np.int64)]
    p = _base(n)
    p[rows] = good(synth.uniform_int(k, 7, 0, 7), desc)
    return p


def quantity(n, seed=2):
    return synth.uniform_int(n, seed, 1, 100).astype(F)


def table(price, qty=None):
    return {"price": np.ascontiguousarray(price, F), "quantity": quantity(len(price)) if qty is None else qty}


def pass_exactly(n, m):
    """A quantity column under which exactly m rows pass COND, the last row among them."""
    q = np.full(n, 1.0, F)
    if m:
        q[np.unique(np.linspace(n - 1, 0, m).astype(np.int64))] = F(99.0)
        assert int((q > 50).sum()) == m
    return q


def typed_columns(n):
    """ORDER BY columns that are not float: distinct values that collide once
    cast to float (the row index then decides), and doubles beyond FLT_MAX."""
    a = ((1 << 24) - 40 + synth.uniform_int(n, 11, 0, 120)).astype(np.int32)       # straddles 2^24
    d = ((1 << 40) + synth.uniform_int(n, 12, -3000, 3000) * 50_000).astype(np.int64)  # float steps of 2^17
    c = synth.uniform_int(n, 13, -50, 50).astype(np.float64) * 0.25
    c[1::2] += 1e-12                                                                # pairs that round to one float
    big = synth.uniform_int(n, 14, 0, 999)
    c[big == 0] = 1e39
    c[big == 1] = -1e39
    c[big == 2] = 3.5e38                                                            # beyond FLT_MAX: rounds to inf
    return {"a": a, "d": d, "c": c}


# ------------------------------------------------------------------ numpy
def numpy_topk(key, k, desc, passing=None):
    """Rows and keys of ORDER BY key [DESC] LIMIT k among `passing`: NaN last
    in both directions, -0.0 == +0.0, ties by ascending row."""
    with np.errstate(over="ignore"):
        key = np.asarray(key).astype(F)
    rows = np.arange(len(key), dtype=np.int64) if passing is None else np.flatnonzero(passing).astype(np.int64)
    kk = key[rows].astype(np.float64)
    nan = np.isnan(kk)
    rank = np.where(nan, 0.0, -kk if desc else kk) + 0.0   # + 0.0: one zero
    order = np.lexsort((rows, rank, nan))[:k]
    return key[rows[order]], rows[order]
