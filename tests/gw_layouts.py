"""Table layouts for the tests of the LDS-window GROUP BY (wx_group_sum,
wx_group_multi, wx_join_group, their finalizes and the general-key table).

Shared by tests/test_group_window_layouts.py (CPU: every layout holds what it
is named for) and tests/test_gpu_group_window_edges.py (GPU: the kernels
against numpy on those layouts), so that a layout that stops hitting its edge
fails before it reaches a GPU.

The layouts are stated against the geometry wx_group_window_geometry reports.
With q = r >> 2 and e = r & 3, row r is element e of thread tid = q % block
in round u = (q % span) / block of span s = q / span (span = block * unroll
quads), and span s is batch s / grid of workgroup s % grid.  The diagnostic
define WX_GROUP_GRID caps the grid, so that a table of a few spans gives every
workgroup several batches.  A wave's lanes at one (batch, u, e) evaluate their
rows together: that is where the wave-combined add (WX_GROUP_LEAD) decides.

Columns: `k` the key, `f` the WHERE flag (COND keeps f > 0), and the values
of tests/test_gpu_group_multi.py: va a multiple of 2^-6 below 256, vb an
integer below 256 (va * vb below 2^16), vc and vd multiples of 2^-6 below 2^10
and 2^16; the join's rr is a multiple of 2^-3 below 64 (va * rr a multiple of
2^-9 below 2^14).  Over fewer than 2^17 rows every partial sum is a multiple
of 2^-9 below 2^33, exact in a double: sums are compared bit for bit.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

WINDOW = 2048      # keys of the LDS window
HSORT_MAX = 4096   # general keys the finalize sorts in LDS
LEAD = 16          # lanes on one bin from which a wave adds once
GRID3, GRID1 = "WX_GROUP_GRID=3", "WX_GROUP_GRID=1"
COND, OCOND = "(f[idx] > 0.0f)", "f > 0"
I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
HASH_MUL = 2654435761
HASH_INV = pow(HASH_MUL, -1, 2 ** 32)
SUM, MULTI, JOIN = 0, 1, 2      # wx_group_window_geometry's families
DIRECT, HASH = 0, 1             # join forms

# name -> (family, summed values, MIN / MAX values, join form): the streaming kernels' builds
FAMILIES = {
    "group_sum": (SUM, 1, 0, 0),
    "group_agg": (SUM, 1, 1, 0),
    "sum2": (MULTI, 2, 0, 0),       # sums only: the wave-combined add
    "mix3": (MULTI, 2, 1, 0),       # S + Q = 3: 512 threads
    "all4": (MULTI, 4, 4, 0),       # S + Q = 8: 1024 threads
    "join_hash": (JOIN, 2, 1, HASH),
    "join_direct": (JOIN, 2, 1, DIRECT),
}


def manual_geometry(n, block, cus, per_cu, cap=None, unroll=2):
    """The geometry by hand: one workgroup per `block` quads up to per_cu per CU, capped."""
    nq = (n + 3) // 4
    grid = max(1, min(-(-nq // block), cus * per_cu, cap or 1 << 40))
    span = block * unroll
    return SimpleNamespace(block_threads=block, span_rows=4 * span, grid=grid,
                           max_batches=-(-(-(-nq // span)) // grid))


def place(g, n):
    """Where each of n rows runs: arrays wg, batch, u, tid, wave, lane, e."""
    r = np.arange(n, dtype=np.int64)
    q, e = r >> 2, r & 3
    block, span = int(g.block_threads), int(g.span_rows) // 4
    s = q // span
    tid = q % block
    return SimpleNamespace(wg=s % int(g.grid), batch=s // int(g.grid), u=(q % span) // block, tid=tid, wave=tid >> 6,
                           lane=tid & 63, e=e, span=s)


def values(n, seed=0):
    rng = np.random.default_rng(77 + seed)
    return {
        "va": (rng.integers(0, 256 * 64, n) / 64.0).astype(np.float32),
        "vb": rng.integers(0, 256, n).astype(np.float32),
        "vc": (rng.integers(-64_000, 64_001, n) / 64.0).astype(np.float32),
        "vd": (rng.integers(-4_000_000, 4_000_001, n) / 64.0).astype(np.float32),
    }


class Layout:
    def __init__(self, keys, key_lo, flag=None, seed=0):
        self.keys = np.ascontiguousarray(keys, np.int64)
        self.n = len(self.keys)
        self.key_lo = int(key_lo)
        self.flag = np.ones(self.n, np.float32) if flag is None else np.ascontiguousarray(flag, np.float32)
        self.seed = seed
        assert self.n < 1 << 17 and (not self.n or (self.keys.min() >= I32_MIN and self.keys.max() <= I32_MAX))
        assert I32_MIN <= self.key_lo <= I32_MAX - (WINDOW - 1)

    def bins(self):
        """(u32)(key - key_lo), as the kernels compute it."""
        return (self.keys - self.key_lo) % (1 << 32)

    def inside(self):
        return self.bins() < WINDOW

    def passing(self, where):
        return self.flag > 0 if where else np.ones(self.n, bool)

    def cols(self):
        c = {"k": self.keys.astype(np.int32), "f": self.flag}
        c.update(values(self.n, self.seed))
        return c

    def general_keys(self, where=False):
        """The distinct passing keys outside the window, ascending."""
        return np.unique(self.keys[self.passing(where) & ~self.inside()])

    def window_keys(self, where=False):
        return np.unique(self.keys[self.passing(where) & self.inside()])


# ------------------------------------------------------------- steady state
STEADY_LO, STEADY_KEYS = -500, (-3000, 3000)


def steady_sizes(g3):
    """The row counts of the steady-state cases from the span S and the grid G = 3 of the capped geometry."""
    S, G = int(g3.span_rows), 3
    return [S - 1, S, S + 1, G * S, 3 * G * S + 5, (3 * G + 1) * S - 3]


def steady(n, seed=1):
    """Random keys over [-3000, 3000) around the window [-500, 1548): every batch feeds the LDS and the table."""
    rng = np.random.default_rng(500 + seed + n)
    return Layout(rng.integers(STEADY_KEYS[0], STEADY_KEYS[1], n), STEADY_LO, seed=seed)


def check_steady(lay, g):
    """Every batch of every workgroup holds rows inside and rows outside the window."""
    p = place(g, lay.n)
    ins = lay.inside()
    for s in range(int(p.span.max()) + 1):
        rows = p.span == s
        if rows.sum() >= 64:
            assert ins[rows].any() and (~ins[rows]).any(), s
    assert len(lay.general_keys()) < HSORT_MAX


# ----------------------------------------------------------- lead decisions
LEAD_LO = 1000


def _base_bins(p):
    """Bins below 1900, distinct over the lanes of a wave at every (batch, u, e)."""
    return (p.lane * 29 + p.wave * 7 + p.u * 3 + p.e) % WINDOW


def sel(p, wg, batch, wave=None, u=None, e=None):
    m = (p.wg == wg) & (p.batch == batch)
    for name, v in (("wave", wave), ("u", u), ("e", e)):
        if v is not None:
            m &= getattr(p, name) == v
    return m


def sharers(lay, p, wg, batch, wave, u, e, where=True):
    """What a wave sees at one (batch, u, e): (active lanes, the first lane passes, its bin, lanes on that bin)."""
    rows = np.flatnonzero(sel(p, wg, batch, wave, u, e))
    rows = rows[np.argsort(p.lane[rows])]
    if not len(rows):
        return 0, False, None, 0
    ok = lay.passing(where)[rows]
    b = lay.bins()[rows]
    first_ok = bool(ok[0]) and p.lane[rows[0]] == 0
    return len(rows), first_ok, int(b[0]), int((ok & (b == b[0])).sum())


# name -> (workgroup, batch, wave) of the wave a case of the lead table lives in
LEAD_SLOTS = {
    "share15": (0, 0, 0), "share16": (0, 0, 1), "share64": (0, 0, 2), "first_dropped": (0, 0, 3),
    "first_outside": (0, 0, 4), "all_above": (0, 0, 5), "bin2047": (0, 0, 6), "all_below": (0, 0, 7),
    "late_rounds": (2, 1, 0),
}
LEAD_BINS = {"share15": 1901, "share16": 1902, "share64": 1903, "first_dropped": 1904, "skew0": 1905, "skew2": 1906,
             "tail": 1907, "late16": 1908, "late40": 1909, "late20": 1910}
LEAD_TAIL_ROWS = 3 * 256 + 4 * 37 + 2   # the last span: three full waves, 37 quads and half a quad of the fourth


def lead(g):
    """One table over three batches of three workgroups and a ragged tenth span, a case per wave (LEAD_SLOTS):
    15, 16 and 64 lanes on the first lane's bin; a first lane the WHERE drops; a first lane outside the window;
    whole waves on key_lo + 2048, on bin 2047 and on key_lo - 1; workgroup 1 skewed in batches 0 and 2 and uniform
    in batch 1; later rounds of a lead batch with 40 sharers that exclude, and 20 that include, the first lane; a
    last partial span on one key."""
    G, S = int(g.grid), int(g.span_rows)
    assert G == 3
    n = 3 * G * S + LEAD_TAIL_ROWS
    p = place(g, n)
    lo = LEAD_LO
    keys = lo + _base_bins(p)
    flag = np.ones(n, np.float32)
    at = lambda name, **kw: sel(p, *LEAD_SLOTS[name], **kw)  # noqa: E731
    first = dict(u=0, e=0)
    keys[at("share15", **first) & (p.lane % 4 == 0) & (p.lane < 60)] = lo + LEAD_BINS["share15"]   # lanes 0, 4 .. 56
    keys[at("share16", **first) & (p.lane % 4 == 0)] = lo + LEAD_BINS["share16"]                    # lanes 0, 4 .. 60
    keys[at("share64")] = lo + LEAD_BINS["share64"]                                                  # every round
    keys[at("first_dropped", **first)] = lo + LEAD_BINS["first_dropped"]
    flag[at("first_dropped", **first) & (p.lane == 0)] = 0
    keys[at("first_outside", **first) & (p.lane == 0)] = lo + WINDOW + 5
    keys[at("all_above")] = lo + WINDOW
    keys[at("bin2047")] = lo + WINDOW - 1
    keys[at("all_below")] = lo - 1
    keys[sel(p, 1, 0)] = lo + LEAD_BINS["skew0"]
    keys[sel(p, 1, 2)] = lo + LEAD_BINS["skew2"]
    keys[at("late_rounds", **first) & (p.lane < 16)] = lo + LEAD_BINS["late16"]
    keys[at("late_rounds", u=1, e=1) & (p.lane >= 24)] = lo + LEAD_BINS["late40"]
    keys[at("late_rounds", u=1, e=2) & (p.lane < 20)] = lo + LEAD_BINS["late20"]
    keys[p.span == 3 * G] = lo + LEAD_BINS["tail"]
    lay = Layout(keys, lo, flag, seed=2)
    check_lead(lay, g)
    return lay


def check_lead(lay, g):
    p = place(g, lay.n)
    lo = lay.key_lo
    assert int(g.lead) == LEAD and int(g.block_threads) == 512 and int(g.grid) == 3
    assert int(g.max_batches) == 4 and p.batch.max() == 3
    see = lambda name, u=0, e=0: sharers(lay, p, *LEAD_SLOTS[name], u, e)  # noqa: E731
    assert see("share15") == (64, True, LEAD_BINS["share15"], LEAD - 1)
    assert see("share16") == (64, True, LEAD_BINS["share16"], LEAD)
    for u in range(2):
        for e in range(4):
            assert see("share64", u, e) == (64, True, LEAD_BINS["share64"], 64)
            assert see("all_above", u, e) == (64, True, WINDOW, 64)              # one past the window
            assert see("bin2047", u, e) == (64, True, WINDOW - 1, 64)            # the window's last bin
            assert see("all_below", u, e) == (64, True, (1 << 32) - 1, 64)       # the bin wraps
    active, first_ok, b0, same = see("first_dropped")
    assert (active, first_ok, b0, same) == (64, False, LEAD_BINS["first_dropped"], 63)
    active, first_ok, b0, same = see("first_outside")
    assert active == 64 and first_ok and b0 == WINDOW + 5 and same == 1
    # workgroup 1: every wave skewed in batches 0 and 2, no wave of batch 1 with two lanes on a bin
    for wave in range(8):
        assert sharers(lay, p, 1, 0, wave, 0, 0) == (64, True, LEAD_BINS["skew0"], 64)
        assert sharers(lay, p, 1, 2, wave, 1, 3) == (64, True, LEAD_BINS["skew2"], 64)
        for u in range(2):
            for e in range(4):
                assert sharers(lay, p, 1, 1, wave, u, e)[3] == 1
    # a lead batch whose later rounds hold many sharers without, and a few with, the first lane
    assert see("late_rounds") == (64, True, LEAD_BINS["late16"], LEAD)
    rows = np.flatnonzero(sel(p, *LEAD_SLOTS["late_rounds"], u=1, e=1))
    assert see("late_rounds", 1, 1)[3] == 1 and (lay.bins()[rows] == LEAD_BINS["late40"]).sum() == 40
    assert see("late_rounds", 1, 2) == (64, True, LEAD_BINS["late20"], 20)
    # the last span: workgroup 0's fourth batch, one key, the fourth wave cut inside a quad
    tail = np.flatnonzero(p.span == 9)
    assert len(tail) == LEAD_TAIL_ROWS and (p.wg[tail] == 0).all() and (p.batch[tail] == 3).all()
    assert (lay.keys[tail] == lo + LEAD_BINS["tail"]).all() and (p.u[tail] == 0).all()
    assert sharers(lay, p, 0, 3, 2, 0, 0)[0] == 64 and sharers(lay, p, 0, 3, 3, 0, 0)[0] == 38
    assert sharers(lay, p, 0, 3, 3, 0, 2)[0] == 37 and sharers(lay, p, 0, 3, 4, 0, 0)[0] == 0
    # no case's key is anyone else's
    for name, b in LEAD_BINS.items():
        assert b >= 1900 and (_base_bins(p) != b).all(), name


# --------------------------------------------------------- window placement
PLACEMENT_LOS = (I32_MIN, -1024, I32_MAX - (WINDOW - 1))


def placement_pool(key_lo):
    pool = [key_lo - 1, key_lo, key_lo + WINDOW - 1, key_lo + WINDOW, I32_MIN, I32_MAX, 0, -1]
    return sorted({k for k in pool if I32_MIN <= k <= I32_MAX})


def placement(n, key_lo):
    """Every third row a key of the pool (the window's ends and their neighbours, the int32 ends, 0, -1), the
    others random window keys."""
    rng = np.random.default_rng(900 + key_lo % 1000)
    keys = key_lo + rng.integers(0, WINDOW, n)
    pool = np.array(placement_pool(key_lo), np.int64)
    r = np.arange(0, n, 3)
    keys[r] = pool[(r // 3) % len(pool)]
    lay = Layout(keys, key_lo, seed=3)
    check_placement(lay)
    return lay


def check_placement(lay):
    lo = lay.key_lo
    pool = placement_pool(lo)
    assert set(pool) <= set(lay.keys.tolist())
    gen, win = lay.general_keys(), lay.window_keys()
    assert {lo, lo + WINDOW - 1} <= set(win.tolist()) and len(win) > 1000
    if lo > I32_MIN:
        assert lo - 1 in gen and I32_MIN in gen
        assert lay.bins()[lay.keys == lo - 1][0] == (1 << 32) - 1
    if lo + WINDOW <= I32_MAX:
        assert lo + WINDOW in gen and I32_MAX in gen
    if lo == I32_MAX - (WINDOW - 1):   # the smallest key lands one past the window's last bin
        assert lay.bins()[lay.keys == I32_MIN][0] == WINDOW and I32_MAX in win
    if lo == I32_MIN:
        assert len(gen[gen < lo]) == 0 and {0, -1, I32_MAX} <= set(gen.tolist())
    assert set((0, -1)) <= set(win.tolist()) or set((0, -1)) <= set(gen.tolist())


# ------------------------------------------------------ finalize boundaries
FIN_LO = -500
FIN_NH = (0, 1, 2, HSORT_MAX - 1, HSORT_MAX, HSORT_MAX + 1)
FIN_SIDES = ("below", "above", "split")
FIN_NWIN = (0, 1, WINDOW)


def finalize(nh, side, nwin, key_lo=FIN_LO):
    """nh general keys all below, all above or split around the window, and nwin window groups (2048: every bin);
    two rows per key and a third for every fifth, in a shuffled order."""
    nlo = {"below": nh, "above": 0, "split": nh // 2}[side]
    below = key_lo - 1 - 3 * np.arange(nlo, dtype=np.int64)
    above = key_lo + WINDOW + 5 * np.arange(nh - nlo, dtype=np.int64)
    win = key_lo + (np.arange(nwin, dtype=np.int64) if nwin == WINDOW else np.array([777], np.int64)[:nwin])
    ks = np.concatenate([below, win, above])
    keys = np.concatenate([ks, ks, ks[::5]])
    np.random.default_rng(nh * 7 + nwin).shuffle(keys)
    lay = Layout(keys, key_lo, seed=4)
    gen = lay.general_keys()
    assert len(gen) == nh and int((gen < key_lo).sum()) == nlo and len(lay.window_keys()) == nwin
    return lay


# ---------------------------------------------------- the general-key table
def hash_slot(keys, slots):
    """The home slot of each key in a table of `slots` slots (wx_group_hash_slot, in numpy)."""
    k = (np.asarray(keys, np.int64) % (1 << 32)).astype(np.uint64)   # the product wraps at 2^64: its low word is exact
    return ((k * np.uint64(HASH_MUL)) & np.uint64(slots - 1)).astype(np.int64)


def cluster_keys(count, slots, home, key_lo):
    """`count` distinct int32 keys outside the window whose home slot is `home`: the hash is a multiplication by an
    odd number, so the keys are the products of its inverse with the words whose low bits are `home`."""
    words = home + slots * np.arange(min(2 * count + WINDOW, (1 << 32) // slots), dtype=np.int64)
    keys = ((words.astype(np.uint64) * np.uint64(HASH_INV)) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    keys = np.where(keys >= 1 << 31, keys - (1 << 32), keys)
    keys = keys[((keys - key_lo) % (1 << 32)) >= WINDOW][:count]
    assert len(keys) == count == len(np.unique(keys)) and (hash_slot(keys, slots) == home).all()
    return keys


TABLE_LO = 100
CLUSTER = 300


def cluster(g, n, slots, home):
    """300 keys of one home slot (and 0 and -1, outside the window) laid out so that the 64 lanes of every wave
    hold 64 different keys of the cluster at every (batch, u, e): they claim their slots at once."""
    ck = cluster_keys(CLUSTER, slots, home, TABLE_LO)
    p = place(g, n)
    idx = (p.lane + 64 * p.wave + 61 * (p.u * 4 + p.e) + 97 * p.span) % CLUSTER
    keys = ck[idx]
    keys[5::1001] = 0
    keys[6::1001] = -1
    lay = Layout(keys, TABLE_LO, seed=5)
    for wave in (0, int(p.wave.max())):
        rows = np.flatnonzero(sel(p, 0, 0, wave, 0, 0))
        assert len(rows) == 64 and len(np.unique(lay.keys[rows])) == 64
    gen = lay.general_keys()
    assert len(gen) == CLUSTER + 2 and {0, -1} <= set(gen.tolist()) and not lay.inside().any()
    assert (hash_slot(ck, slots) == home).all()
    return lay


def overfull(n=20_000, distinct=5000):
    """More distinct keys outside the window than a 4096-slot table holds."""
    r = np.arange(n, dtype=np.int64)
    lay = Layout(TABLE_LO + WINDOW + 3 * ((r * 7919) % distinct), TABLE_LO, seed=6)
    assert len(lay.general_keys()) == distinct > 4096
    return lay


# ------------------------------------------------------------ the join's side
RIGHT_ROWS = 1000


def right_columns():
    """A right table of 1000 unique keys 10, 13, .. in a shuffled order (a span the direct form takes) and a value
    rr on a 1/8 grid below 64."""
    rng = np.random.default_rng(31)
    rk = (10 + 3 * rng.permutation(RIGHT_ROWS)).astype(np.int32)
    return {"rk": rk, "rr": (rng.integers(0, 512, RIGHT_ROWS) / 8.0).astype(np.float32)}


def join_left(lay):
    """The left columns of a layout: its columns and a join key kk that finds a right row, except in every
    seventh row.  Returns (columns, hit, the matched rr per row)."""
    rc = right_columns()
    r = np.arange(lay.n, dtype=np.int64)
    rrow = (r * 13) % RIGHT_ROWS
    hit = r % 7 != 3
    cols = lay.cols()
    cols["kk"] = np.where(hit, rc["rk"][rrow], rc["rk"][rrow] + 1).astype(np.int32)   # 11, 14, ..: no right key
    return cols, hit, rc["rr"][rrow]


# ------------------------------------------------------------- the reference
def numpy_groups(keys, vals, keep):
    """GROUP BY in numpy: (keys ascending, float64 sums added in row order, int64 counts, float32 minima and
    maxima with NaN skipped -- NaN when a group has no other value -- and -0.0 returned as +0.0)."""
    keys, vals = np.asarray(keys)[keep], np.asarray(vals, np.float32)[keep]
    uk, inv = np.unique(keys, return_inverse=True)
    sums = np.zeros(len(uk), np.float64)
    np.add.at(sums, inv, vals.astype(np.float64))
    counts = np.bincount(inv, minlength=len(uk)).astype(np.int64)
    mins = np.full(len(uk), np.nan, np.float32)
    maxs = np.full(len(uk), np.nan, np.float32)
    np.fmin.at(mins, inv, vals)
    np.fmax.at(maxs, inv, vals)
    mins[mins == 0] = 0.0
    maxs[maxs == 0] = 0.0
    return uk.astype(np.int32), sums, counts, mins, maxs


def exact_groups(keys, vals, keep):
    """numpy_groups, after checking that the order of the adds cannot matter on this table."""
    r = numpy_groups(keys, vals, keep)
    rev = numpy_groups(np.asarray(keys)[::-1], np.asarray(vals)[::-1], np.asarray(keep)[::-1])
    assert np.array_equal(r[0], rev[0]) and np.array_equal(r[1].view(np.uint64), rev[1].view(np.uint64))
    return r
