"""Row-order GROUP BY (WX_F_ROW_ORDER) at the edges of its kernels: many tiles
per range, the key-major order itself, every route, and the fold's sizes.

The span path launches min(tiles, 2 * CUs) ranges, so a table a test can
afford gives every workgroup one tile; WARPDB_RO_RANGES=<n> caps the ranges
so that one workgroup runs many tiles in order (the runs carried from tile to
tile, the counters re-zeroed, the bases rebuilt, a partial tile after whole
ones).  wx_group_rows_last_call says which route a call took and what it
launched, wx_group_rows_last_values copies the row-ordered value array out,
and wx_group_rows_geometry gives every size the tables are built from.

Order is observed, not inferred: the value is the row index, so the copied
array must be the passing rows in a stable sort of their keys (numpy), slot by
slot.  Sums are compared with the sequential double fold (np.add.accumulate
in float64, the oracle's fold) bit for bit, counts, keys, routes and row ids
for equality; there is no tolerance anywhere.  Output buffers carry a guard
tail and a sentinel prefill and must be untouched from the group count on.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import ro_layouts as rl

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from warpdb_amd import _warpexec as wx  # noqa: E402
from test_gpu_parity import dev_table  # noqa: E402

GUARD = 64
SENT_KEY, SENT_CNT, SENT_SUM = 0x5A5A5A5A, -77, 0x7FF8C0DEC0DE0001   # the sum's is a NaN no fold produces
SENT_F32 = 0x7FC0BEEF
WHERE = "(pp[idx] > 0.5f)"
LAYOUTS = ["mixed_tail_%d" % t for t in rl.TAILS] + ["mixed_whole", "narrow_tail_65"]
_KEEP = []   # every table stays allocated: a later table at a reused address would meet this one's memo / miss counter


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for v in ("WARPDB_GROUP_ROWS", "WARPDB_RO_RANGES", "WARPDB_XF_BIG", "WARPDB_FOLD_SMALL", "WARPDB_EXTRA_DEFINES"):
        monkeypatch.delenv(v, raising=False)


@functools.lru_cache(maxsize=None)
def geom():
    return wx.group_rows_geometry()


@functools.lru_cache(maxsize=None)
def layouts():
    return rl.all_layouts(geom())


@functools.lru_cache(maxsize=None)
def layout_table(name):
    t, tensors = dev_table(layouts()[name].cols)
    _KEEP.append(tensors)
    return t


@functools.lru_cache(maxsize=None)
def layout_reference(name, scale):
    """(order, keys, counts, exact sums of rid, first row, last row) of a layout: numpy, once."""
    lay = layouts()[name]
    order = lay.order()
    keys, counts = lay.groups(scale)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    sums = np.add.reduceat(order.astype(np.float64), starts)   # integers below 2^41: exact in any order
    for a in (order, keys, counts, sums):
        a.setflags(write=False)
    return order, keys, counts, sums, order[starts], order[starts + counts - 1]


def table_of(cols):
    t, tensors = dev_table(cols)
    _KEEP.append(tensors)
    return t


def launch(flags=wx.F_ROW_ORDER):
    return wx.make_launch(device=0, stream=torch.cuda.current_stream().cuda_stream, flags=flags)


def two_cus():
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


class Outputs:
    """Group outputs of `cap` entries and a guard tail, prefilled with sentinels."""

    def __init__(self, cap, agg=False):
        self.cap = cap
        self.keys = torch.full((cap + GUARD,), SENT_KEY, dtype=torch.int32, device="cuda")
        self.sums = torch.full((cap + GUARD,), SENT_SUM, dtype=torch.int64, device="cuda")
        self.cnts = torch.full((cap + GUARD,), SENT_CNT, dtype=torch.int64, device="cuda")
        self.mins = self.maxs = None
        if agg:
            self.mins = torch.full((cap + GUARD,), SENT_F32, dtype=torch.int32, device="cuda")
            self.maxs = torch.full((cap + GUARD,), SENT_F32, dtype=torch.int32, device="cuda")

    def run(self, t, val, key, cond):
        if self.mins is not None:
            self.g = wx.group_agg(t, val, key, cond, launch(), 0, self.cap, self.keys.data_ptr(), self.sums.data_ptr(),
                                  self.cnts.data_ptr(), self.mins.data_ptr(), self.maxs.data_ptr())
        else:
            self.g = wx.group_sum(t, val, key, cond, launch(), 0, self.cap, self.keys.data_ptr(),
                                  self.sums.data_ptr(), self.cnts.data_ptr())
        self.untouched_from(self.g)
        g = self.g
        self.k = self.keys[:g].cpu().numpy()
        self.s = self.sums[:g].cpu().numpy().view(np.float64)
        self.c = self.cnts[:g].cpu().numpy()
        if self.mins is not None:
            self.mn = self.mins[:g].cpu().numpy().view(np.float32)
            self.mx = self.maxs[:g].cpu().numpy().view(np.float32)
        return self

    def untouched_from(self, g):
        torch.cuda.synchronize()
        assert bool((self.keys[g:] == SENT_KEY).all()), "keys written at or beyond the group count"
        assert bool((self.sums[g:] == SENT_SUM).all()), "sums written at or beyond the group count"
        assert bool((self.cnts[g:] == SENT_CNT).all()), "counts written at or beyond the group count"
        if self.mins is not None:
            assert bool((self.mins[g:] == SENT_F32).all()) and bool((self.maxs[g:] == SENT_F32).all())


def record():
    return wx.group_rows_last_call(launch())


def copied_values(n_expected):
    """The last call's row-ordered value array, through a buffer with a guard tail."""
    buf = torch.full((n_expected + GUARD,), SENT_F32, dtype=torch.int32, device="cuda")
    n = wx.group_rows_last_values(launch(wx.F_SYNC), buf.data_ptr(), n_expected + GUARD)
    torch.cuda.synchronize()
    assert n == n_expected
    assert bool((buf[n:] == SENT_F32).all()), "the copy wrote beyond the array"
    return buf[:n].cpu().numpy().view(np.float32)


def fold(v):
    """The sequential double fold of float32 values in the order given."""
    with np.errstate(invalid="ignore"):   # +inf then -inf is a NaN, as in the kernels
        return np.add.accumulate(np.concatenate([[0.0], np.asarray(v, np.float32).astype(np.float64)]))[-1]


def assert_sums(got, want, what=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, np.flatnonzero(np.isnan(got) != nan)[:8])
    bad = np.flatnonzero(bits(got[~nan]) != bits(want[~nan]))
    assert bad.size == 0, (what, bad[:8], got[~nan][bad[:8]], want[~nan][bad[:8]])


# ------------------------------------------------------------ stable order
ROUTES = ["cap1", "cap2", "cap3", "cap5", "cap7", "uncapped", "ordinary", "minmax", "general", "keys5000"]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", LAYOUTS)
def test_stable_order_observed(name, route, monkeypatch):
    """The value is the row index: the copied value array must hold the passing
    rows key-major, ascending within a key -- slot by slot -- on every route,
    with one workgroup running 16, 8, 5-6, 3-4 and 2-3 tiles (caps 1 .. 7)."""
    lay = layouts()[name]
    t = layout_table(name)
    scale = 5000 if route == "keys5000" else 1
    order, keys, counts, sums, first, last = layout_reference(name, scale)
    key = "(kk[idx] * 5000)" if route == "keys5000" else "kk[idx]"
    uncapped = min(lay.n_tiles, two_cus())
    want_ranges = uncapped
    if route.startswith("cap"):
        monkeypatch.setenv("WARPDB_RO_RANGES", route[3:])
        want_ranges = int(route[3:])
    elif route == "ordinary":   # the exact key range of the ordinary call, three ranges
        monkeypatch.setenv("WARPDB_GROUP_ROWS", "ordinary")
        monkeypatch.setenv("WARPDB_RO_RANGES", "3")
        want_ranges = 3
    elif route == "minmax":
        monkeypatch.setenv("WARPDB_RO_RANGES", "5")
        want_ranges = 5
    elif route == "general":
        monkeypatch.setenv("WARPDB_GROUP_ROWS", "general")
    out = Outputs(len(keys) + 3, agg=route == "minmax").run(t, "rid[idx]", key, WHERE)
    r = record()
    want = {
        "ordinary": (wx.RO_ROUTE_ORDINARY_SPAN, wx.RO_WHY_NOT_TRIED),
        "minmax": (wx.RO_ROUTE_ORDINARY_SPAN, wx.RO_WHY_NOT_TRIED),
        "general": (wx.RO_ROUTE_GENERAL_RUNS, wx.RO_WHY_NOT_TRIED),
        "keys5000": (wx.RO_ROUTE_GENERAL_RUNS, wx.RO_WHY_WIDE),
    }.get(route, (wx.RO_ROUTE_DIRECT, wx.RO_WHY_NONE))
    assert (r.route, r.why) == want
    if want[0] == wx.RO_ROUTE_GENERAL_RUNS:
        assert (r.ranges, r.tiles) == (0, 0)
    else:
        assert (r.ranges, r.tiles) == (want_ranges, lay.n_tiles)
    assert r.n_values == len(order) and (r.big_groups, r.big_chunks) == (0, 0)
    got = copied_values(len(order))
    rows = got.astype(np.int64)
    wrong = np.flatnonzero(rows != order)
    assert wrong.size == 0, (len(wrong), wrong[:8], rows[wrong[:8]], order[wrong[:8]])
    assert out.g == len(keys) and np.array_equal(out.k, keys) and np.array_equal(out.c, counts)
    assert_sums(out.s, sums)
    if route == "minmax":   # a group's smallest and largest row index: its first and last row
        assert np.array_equal(out.mn.astype(np.int64), first) and np.array_equal(out.mx.astype(np.int64), last)


@pytest.mark.parametrize("cap", ["1", "3", "7", None])
def test_capped_ranges_fold_order_dependent_values(cap, monkeypatch):
    """Values over many binades (their fold depends on order) through capped
    ranges: bit-equal to the sequential fold and the same at every cap."""
    name = "mixed_tail_4097"
    lay = layouts()[name]
    if cap:
        monkeypatch.setenv("WARPDB_RO_RANGES", cap)
    order, keys, counts, *_ = layout_reference(name, 1)
    out = Outputs(len(keys)).run(layout_table(name), "va[idx]", "kk[idx]", WHERE)
    assert record().route == wx.RO_ROUTE_DIRECT and record().ranges == (int(cap) if cap else min(lay.n_tiles, two_cus()))
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    va = lay.cols["va"][order]
    want = np.array([fold(va[s:s + c]) for s, c in zip(starts, counts)])
    assert np.array_equal(copied_values(len(order)).view(np.uint32), va.view(np.uint32))
    assert np.array_equal(out.k, keys) and np.array_equal(out.c, counts)
    assert_sums(out.s, want)


@pytest.mark.parametrize("bad", ["0", "-3", "two", "1.5", "4x"])
def test_bad_range_cap_is_refused(bad, monkeypatch):
    t = layout_table("narrow_tail_65")
    monkeypatch.setenv("WARPDB_RO_RANGES", bad)
    out = Outputs(128)
    with pytest.raises(wx.WarpExecError, match="WARPDB_RO_RANGES") as ei:
        out.run(t, "rid[idx]", "kk[idx]", WHERE)
    assert ei.value.status == wx.WX_ERR_INVALID
    out.untouched_from(0)   # refused before anything was enqueued
    r = record()
    assert (r.route, r.why, r.ranges, r.tiles, r.n_values) == (0, 0, 0, 0, 0)
    with pytest.raises(wx.WarpExecError, match="no row-order GROUP BY"):
        wx.group_rows_last_values(launch(), 0, 0)


def test_range_cap_above_the_tiles_is_clamped(monkeypatch):
    lay = layouts()["narrow_tail_65"]
    monkeypatch.setenv("WARPDB_RO_RANGES", "1000000")
    Outputs(128).run(layout_table("narrow_tail_65"), "rid[idx]", "kk[idx]", WHERE)
    r = record()
    assert r.route == wx.RO_ROUTE_DIRECT and r.ranges == min(lay.n_tiles, two_cus()) and r.tiles == lay.n_tiles
    # the copy refuses a buffer that is too small
    small = torch.full((8 + GUARD,), SENT_F32, dtype=torch.int32, device="cuda")
    with pytest.raises(wx.WarpExecError) as ei:
        wx.group_rows_last_values(launch(wx.F_SYNC), small.data_ptr(), 8)
    assert ei.value.status == wx.WX_ERR_CAPACITY and bool((small == SENT_F32).all())


# ------------------------------------------------------------ value streams
def adversarial(rng, kind, m):
    """One group's m values of kind 0 .. 9: the streams of
    test_gpu_group_row_order._adversarial_groups, at a chosen length."""
    if kind == 0:    # ties: 2^30 first, then odd / even multiples of 2^-23 (half of u = 2^-22)
        x = rng.integers(-8, 9, m).astype(np.float32) * np.float32(2.0 ** -23)
        x[0] = 2.0 ** 30
    elif kind == 1:  # cancellation through zero
        x = np.where(rng.random(m) < 0.5, 1e7, -1e7).astype(np.float32) + rng.uniform(-1, 1, m).astype(np.float32)
    elif kind == 2:  # prices
        x = rng.uniform(0.0, 40.0, m).astype(np.float32)
    elif kind == 3:  # a NaN midway
        x = rng.uniform(0.0, 40.0, m).astype(np.float32)
        x[m // 2] = np.float32("nan")
    elif kind == 4:  # +inf, then -inf: NaN (one value: -inf)
        x = rng.uniform(0.0, 1.0, m).astype(np.float32)
        x[m // 3] = np.float32("inf")
        x[2 * m // 3] = np.float32("-inf")
    elif kind == 5:  # denormals and tiny values under a large sum
        x = (rng.integers(1, 1 << 20, m).astype(np.float32) * np.float32(2.0 ** -149)).astype(np.float32)
        x[::97] = np.float32(3.0e6)
    elif kind == 6:  # hovering at 2^20: +-x steps across the power of two
        x = (rng.choice(np.array([1.0, -1.0], np.float32), m) * rng.uniform(0.0, 3.0, m)).astype(np.float32)
        x[0] = 2.0 ** 20
    elif kind == 7:  # negative sums crossing binades
        x = -rng.uniform(0.0, 1000.0, m).astype(np.float32)
    elif kind == 8:  # float-max values: a double sum far above the float range
        x = np.full(m, 3.0e38, np.float32)
    else:            # mixed scales, negative too
        x = rl.spread(rng, m)
    return x.astype(np.float32)


def interleaved(rng, sizes, streams):
    """Rows of len(sizes) groups interleaved in row order: (group label per row, values)."""
    label = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    v = np.empty(len(label), np.float32)
    for i, x in enumerate(streams):
        v[label == i] = x   # ascending rows: the group's values in row order
    return label, v


def expected_folds(label, v, n_groups):
    return np.array([fold(v[label == i]) for i in range(n_groups)])


# ---------------------------------------------------------- fold size edges
def fold_sizes():
    g = geom()
    B, F = g.fold_block_values, g.fold_small
    A = g.fold_blocks_ahead
    assert A == 4   # the sizes below name the ring's edges as multiples of the blocks in flight
    return [1, 2, 63, 64, 65, B - 1, B, B + 1, A * B - 1, A * B, A * B + 1, 2 * A * B - 1, 2 * A * B + 1, F - 1, F,
            F + 1]


@functools.lru_cache(maxsize=None)
def fold_case(rot):
    rng = np.random.default_rng(900 + rot)
    sizes = fold_sizes()
    kinds = [(3 * i + rot) % 10 for i in range(len(sizes))]   # over rot 0 .. 9 every size meets every kind
    label, v = interleaved(rng, sizes, [adversarial(rng, k, m) for k, m in zip(kinds, sizes)])
    want = expected_folds(label, v, len(sizes))
    return label.astype(np.int32), v, want, np.array(sizes, np.int64)


@pytest.mark.parametrize("route", ["span", "general", "general_wave"])
@pytest.mark.parametrize("rot", range(10))
def test_fold_size_edges(rot, route, monkeypatch):
    """One group per size around the fold's block (B), its ring of blocks in
    flight (4B, 8B) and the one-lane fold's limit (F), rows interleaved, every
    adversarial value kind at every size: equal to the sequential fold."""
    label, v, want, sizes = fold_case(rot)
    keys = label if route == "span" else label * 5000
    if route == "general_wave":
        monkeypatch.setenv("WARPDB_FOLD_SMALL", "0")
    out = Outputs(len(sizes)).run(table_of({"kk": keys.astype(np.int32), "va": v}), "va[idx]", "kk[idx]", None)
    r = record()
    if route == "span":
        assert (r.route, r.why) == (wx.RO_ROUTE_DIRECT, wx.RO_WHY_NONE)
    else:
        assert (r.route, r.why) == (wx.RO_ROUTE_GENERAL_RUNS, wx.RO_WHY_WIDE)
    assert r.n_values == len(v) and r.big_groups == 0
    assert out.g == len(sizes) and np.array_equal(out.k, np.unique(keys)) and np.array_equal(out.c, sizes)
    assert_sums(out.s, want, route)


# ------------------------------------------------------- chunked big groups
CHUNK_KINDS = ["prices", "mix", "ties", "cancel", "negative", "nan2", "inf_last"]


def chunk_stream(rng, kind, m, C):
    if kind == "prices":
        x = rng.uniform(0.0, 40.0, m).astype(np.float32)
    elif kind == "mix":       # 1e7 / 1 / 1e-3 scales
        scale = rng.choice(np.array([1e7, 1.0, 1e-3], np.float32), m)
        x = (rng.uniform(0.0, 1.0, m).astype(np.float32) * scale).astype(np.float32)
    elif kind == "ties":      # multiples of 2^-20 under a mid-binade 1.5 * 2^33 start (u = 2^-19)
        x = (rng.integers(-8, 9, m).astype(np.float32) * np.float32(2.0 ** -20)).astype(np.float32)
        x[0] = np.float32(1.5 * 2.0 ** 33)
    elif kind == "cancel":    # the running sum crosses zero again and again: the approximate binade is wrong
        x = np.where(rng.random(m) < 0.5, 1e7, -1e7).astype(np.float32) + rng.uniform(-1, 1, m).astype(np.float32)
    elif kind == "negative":
        x = -rng.uniform(0.0, 1000.0, m).astype(np.float32)
    elif kind == "nan2":      # a NaN in the second chunk
        x = rng.uniform(0.0, 40.0, m).astype(np.float32)
        x[C + (m - C) // 2] = np.float32("nan")
    elif kind == "inf_last":  # +inf in the last chunk
        x = rng.uniform(0.0, 40.0, m).astype(np.float32)
        x[m - 1 - (m - 1) % C // 2] = np.float32("inf")
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


def chunk_tables():
    """name -> group sizes in key order (C: one chunk; a size above C is chunked)."""
    C = geom().xf_chunk
    return {
        "one": [37, C, 513, C + 1, 1],                                            # C itself is not chunked
        "two": [2 * C + 1, 5000, 1, 2 * C - 1],                                   # a big group first and last
        "three": [C + 1, 37, C, 513, 2 * C, 1, 2 * C - 1, 64],
        "five": [2 * C + 1, 37, C + 1, 1, C, 2 * C, 5000, 2 * C - 1, 513, C + 1],
    }


@functools.lru_cache(maxsize=None)
def chunk_case(name, shift):
    C = geom().xf_chunk
    sizes = chunk_tables()[name]
    rng = np.random.default_rng(1300 + len(sizes) * 10 + shift)
    streams, j = [], shift
    for m in sizes:
        if m > C:
            streams.append(chunk_stream(rng, CHUNK_KINDS[j % len(CHUNK_KINDS)], m, C))
            j += 1
        else:
            streams.append(chunk_stream(rng, "mix" if m % 2 else "prices", m, C))
    label, v = interleaved(rng, sizes, streams)
    return label.astype(np.int32), v, expected_folds(label, v, len(sizes)), np.array(sizes, np.int64)


def test_chunk_cases_cover_every_kind_and_count():
    C = geom().xf_chunk
    tabs = chunk_tables()
    assert [sum(1 for m in s if m > C) for s in tabs.values()] == [1, 2, 3, 5]
    assert {m for s in tabs.values() for m in s if m >= C} == {C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1}
    assert any(s[0] > C for s in tabs.values()) and any(s[-1] > C for s in tabs.values())
    seen = set()
    for name, s in tabs.items():
        for shift in (0, 3):
            n_big = sum(1 for m in s if m > C)
            seen |= {CHUNK_KINDS[(shift + i) % len(CHUNK_KINDS)] for i in range(n_big)}
    assert seen == set(CHUNK_KINDS)
    x = chunk_stream(np.random.default_rng(0), "inf_last", C + 1, C)
    assert np.flatnonzero(np.isinf(x)).tolist() == [C]           # a last chunk of one value: the +inf itself
    x = chunk_stream(np.random.default_rng(0), "nan2", 2 * C + 1, C)
    assert C <= np.flatnonzero(np.isnan(x))[0] < 2 * C


@pytest.mark.parametrize("route", ["span", "general"])
@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("name", ["one", "two", "three", "five"])
def test_chunked_big_groups_small(name, shift, route, monkeypatch):
    """WARPDB_XF_BIG at one chunk: groups of C + 1 .. 2C + 1 rows are folded
    in chunks (a last chunk of 1 value, of C - 1, of exactly C), a group of C
    is not; 1, 2, 3 and 5 chunked groups with small ones between (the entry
    search), every value kind.  Every group equals the sequential fold."""
    C = geom().xf_chunk
    monkeypatch.setenv("WARPDB_XF_BIG", str(C))
    label, v, want, sizes = chunk_case(name, shift)
    keys = label if route == "span" else label * 5000
    out = Outputs(len(sizes) + 1).run(table_of({"kk": keys.astype(np.int32), "va": v}), "va[idx]", "kk[idx]", None)
    r = record()
    assert r.route == (wx.RO_ROUTE_DIRECT if route == "span" else wx.RO_ROUTE_GENERAL_RUNS)
    big = sizes[sizes > C]
    assert (r.big_groups, r.big_chunks) == (len(big), int((-(-big // C)).sum())) and r.n_values == len(v)
    assert out.g == len(sizes) and np.array_equal(out.k, np.unique(keys)) and np.array_equal(out.c, sizes)
    assert_sums(out.s, want, (name, route))


def test_chunked_group_of_65_chunks(monkeypatch):
    """One group of 64 C + 1 rows: 65 chunk records, one more than the combine
    reads at a time, and a last chunk of one value."""
    C = geom().xf_chunk
    monkeypatch.setenv("WARPDB_XF_BIG", str(C))
    n = 64 * C + 1
    rng = np.random.default_rng(65)
    v = chunk_stream(rng, "mix", n, C)
    out = Outputs(4).run(table_of({"kk": np.full(n, 7, np.int32), "va": v}), "va[idx]", "kk[idx]", None)
    r = record()
    assert (r.route, r.big_groups, r.big_chunks, r.n_values) == (wx.RO_ROUTE_DIRECT, 1, 65, n)
    assert r.tiles == -(-n // geom().tile_rows) and r.ranges == min(r.tiles, two_cus())
    assert out.g == 1 and out.k[0] == 7 and out.c[0] == n
    assert_sums(out.s, [fold(v)])


# ------------------------------------------------------ general-path edges
def rle_sizes():
    W = geom().rle_wave_rows
    return [W - 1, W, W + 1, 2 * W + 1]


def run_general(keys, v, cap, agg=False):
    return Outputs(cap, agg=agg).run(table_of({"kk": keys.astype(np.int32), "va": v}), "va[idx]", "kk[idx]", None)


@pytest.mark.parametrize("i", range(4))
def test_general_single_run(i, monkeypatch):
    monkeypatch.setenv("WARPDB_GROUP_ROWS", "general")
    m = rle_sizes()[i]
    v = rl.spread(np.random.default_rng(m), m)
    out = run_general(np.full(m, -42), v, 1)   # capacity == groups == 1
    r = record()
    assert (r.route, r.why, r.n_values) == (wx.RO_ROUTE_GENERAL_RUNS, wx.RO_WHY_NOT_TRIED, m)
    assert out.g == 1 and out.k[0] == -42 and out.c[0] == m
    assert_sums(out.s, [fold(v)])
    assert np.array_equal(copied_values(m).view(np.uint32), v.view(np.uint32))


@pytest.mark.parametrize("i", range(4))
def test_general_every_row_its_own_group(i, monkeypatch):
    """groups == rows: capacity == m holds them exactly (the guard tail
    untouched), capacity == m - 1 is the capacity error."""
    monkeypatch.setenv("WARPDB_GROUP_ROWS", "general")
    m = rle_sizes()[i]
    rng = np.random.default_rng(100 + m)
    keys = rng.permutation(m).astype(np.int64) * 3 - 7
    v = rl.spread(rng, m)
    out = run_general(keys, v, m)
    assert record().route == wx.RO_ROUTE_GENERAL_RUNS
    o = np.argsort(keys, kind="stable")
    assert out.g == m and np.array_equal(out.k, keys[o]) and np.array_equal(out.c, np.ones(m, np.int64))
    assert_sums(out.s, 0.0 + v[o].astype(np.float64))
    assert np.array_equal(copied_values(m).view(np.uint32), v[o].view(np.uint32))
    short = Outputs(m - 1)
    with pytest.raises(wx.WarpExecError) as ei:
        short.run(table_of({"kk": keys.astype(np.int32), "va": v}), "va[idx]", "kk[idx]", None)
    assert ei.value.status == wx.WX_ERR_CAPACITY
    short.untouched_from(m - 1)
    assert record().route == wx.RO_ROUTE_NONE


@pytest.mark.parametrize("shape", ["boundary", "straddle"])
@pytest.mark.parametrize("i", [2, 3])
def test_general_runs_at_wave_range_boundaries(i, shape, monkeypatch):
    """Runs of the sorted keys that start exactly where a wave's range of the
    run-length pass starts, and runs of two rows that straddle that place."""
    monkeypatch.setenv("WARPDB_GROUP_ROWS", "general")
    m = rle_sizes()[i]
    n_blk, span = rl.rle_ranges(m, geom().rle_wave_rows)
    assert n_blk >= 2
    rng = np.random.default_rng(200 + m)
    edges = [k * span for k in range(1, n_blk)]
    cuts = set(rng.integers(1, m, 40).tolist()) - {e + d for e in edges for d in (-1, 0, 1)}
    cuts |= set(edges) if shape == "boundary" else {e + d for e in edges for d in (-1, 1)}
    bounds = np.array([0] + sorted(cuts) + [m])
    sizes = np.diff(bounds)
    label = np.repeat(np.arange(len(sizes)), sizes)       # sorted position -> group
    perm = rng.permutation(m)                             # table row -> sorted-key rank, shuffled
    keys = (label[perm] * 7 - 1000).astype(np.int64)
    v = rl.spread(rng, m)
    out = run_general(keys, v, len(sizes))
    assert record().route == wx.RO_ROUTE_GENERAL_RUNS
    o = np.argsort(keys, kind="stable")
    assert np.array_equal(copied_values(m).view(np.uint32), v[o].view(np.uint32))
    assert out.g == len(sizes) and np.array_equal(out.k, np.unique(keys)) and np.array_equal(out.c, sizes)
    assert_sums(out.s, [fold(v[o][a:b]) for a, b in zip(bounds[:-1], bounds[1:])])


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_general_after_the_ordinary_call_at_the_starts_chunk(d, monkeypatch):
    """MIN / MAX asked: the ordinary call's groups, their first rows by the
    chunked scan of wx_group_starts_* at G - 1, G and G + 1 groups."""
    monkeypatch.setenv("WARPDB_GROUP_ROWS", "general")
    groups = geom().starts_chunk + d
    rng = np.random.default_rng(300 + d)
    keys = rng.permutation(np.concatenate([np.arange(groups), np.arange(groups), rng.integers(0, groups, 5)])) * 9 - 50
    m = len(keys)
    v = rl.spread(rng, m)
    out = run_general(keys, v, groups + 2, agg=True)
    r = record()
    assert (r.route, r.why, r.n_values) == (wx.RO_ROUTE_GENERAL_ORDINARY, wx.RO_WHY_NOT_TRIED, m)
    o = np.argsort(keys, kind="stable")
    uk, cnt = np.unique(keys, return_counts=True)
    starts = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    assert out.g == groups and np.array_equal(out.k, uk) and np.array_equal(out.c, cnt)
    assert np.array_equal(copied_values(m).view(np.uint32), v[o].view(np.uint32))
    assert_sums(out.s, [fold(v[o][s:s + c]) for s, c in zip(starts, cnt)])
    assert np.array_equal(out.mn.view(np.uint32), np.minimum.reduceat(v[o], starts).view(np.uint32))
    assert np.array_equal(out.mx.view(np.uint32), np.maximum.reduceat(v[o], starts).view(np.uint32))


# ------------------------------------------------------------- route choice
def route_table(case, outlier=None, wide=False, drop_sampled=False):
    """Slightly more rows than the sample, keys 0 .. 99, one planted row the
    strided sample does not read.  Every case has its own row count, so no
    table meets another's memo or miss counter."""
    S = geom().sample_rows
    n = S + 37 + case
    rng = np.random.default_rng(500 + case)
    sampled = rl.sampled_rows(n, S)
    unsampled = np.setdiff1d(np.arange(n), sampled)
    assert len(unsampled) == n - S
    kk = rng.integers(0, 5000 if wide else 100, n).astype(np.int64)
    kk[sampled[:2]] = (0, 4999 if wide else 99)      # the sample sees the whole base range
    row = int(unsampled[len(unsampled) // 2])
    assert row not in set(sampled.tolist())
    if outlier is not None:
        kk[row] = outlier
    pp = np.ones(n, np.float32)
    if drop_sampled:
        pp[sampled] = 0.0
    cols = {"kk": kk.astype(np.int32), "va": rl.spread(rng, n), "pp": pp}
    keep = pp > 0.5
    o = np.flatnonzero(keep)[np.argsort(kk[keep], kind="stable")]
    uk, cnt = np.unique(kk[keep], return_counts=True)
    starts = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    want = np.array([fold(cols["va"][o][s:s + c]) for s, c in zip(starts, cnt)])
    return table_of(cols), uk, cnt, want, cols["va"][o]


def check_route(t, uk, cnt, want, ordered, cond, route, why, cap=None):
    out = Outputs(len(uk) if cap is None else cap).run(t, "va[idx]", "kk[idx]", cond)
    r = record()
    assert r.route == route and (why is None or r.why == why)
    assert out.g == len(uk) and np.array_equal(out.k, uk) and np.array_equal(out.c, cnt)
    assert_sums(out.s, want)
    assert np.array_equal(copied_values(len(ordered)).view(np.uint32), ordered.view(np.uint32))
    return r.why


def test_route_unsampled_outlier_inside_the_centred_span():
    # 100 sampled keys centred in 2048: the span reaches 974 below and 973 above them
    t, *ref = route_table(0, outlier=1000)
    for _ in range(2):   # the second call takes the memo's exact range, which holds the outlier
        check_route(t, *ref, None, wx.RO_ROUTE_DIRECT, wx.RO_WHY_NONE)   # capacity == groups: the guard tail untouched


def test_route_miss_then_sixteen_calls_of_ordinary_first():
    """An unsampled key outside the centred span but within 2048 of the rest:
    the count kernel flags it, the call goes ordinary first, and so do the
    next 16 calls without trying (group_rows_direct's counter starts at 16
    and a call passes while it is above 0); call 18 samples again, and misses
    again.  The same bits on every call."""
    t, *ref = route_table(1, outlier=1500)
    whys = [check_route(t, *ref, None, wx.RO_ROUTE_ORDINARY_SPAN, None) for _ in range(18)]
    assert whys == [wx.RO_WHY_OUTSIDE] + [wx.RO_WHY_RECENT_MISS] * 16 + [wx.RO_WHY_OUTSIDE]


def test_route_outlier_beyond_the_span_goes_general_with_the_ordinary_groups():
    t, *ref = route_table(2, outlier=5000)
    check_route(t, *ref, None, wx.RO_ROUTE_GENERAL_ORDINARY, wx.RO_WHY_OUTSIDE)
    check_route(t, *ref, None, wx.RO_ROUTE_GENERAL_ORDINARY, wx.RO_WHY_RECENT_MISS)
    t, *ref = route_table(3, outlier=-3000)
    check_route(t, *ref, None, wx.RO_ROUTE_GENERAL_ORDINARY, wx.RO_WHY_OUTSIDE)


def test_route_where_drops_every_sampled_row():
    t, uk, cnt, want, ordered = route_table(4, drop_sampled=True)
    assert cnt.sum() == 37 + 4   # only the unsampled rows pass
    check_route(t, uk, cnt, want, ordered, WHERE, wx.RO_ROUTE_ORDINARY_SPAN, wx.RO_WHY_NO_SAMPLE)


def test_route_sampled_keys_wider_than_the_span():
    t, *ref = route_table(5, wide=True)
    check_route(t, *ref, None, wx.RO_ROUTE_GENERAL_RUNS, wx.RO_WHY_WIDE)


def test_route_direct_capacity_edges():
    """capacity == groups - 1 on the direct route is the capacity error with
    nothing written from the capacity on; the next call on the workspace
    succeeds at capacity == groups."""
    t, uk, cnt, want, ordered = route_table(6)
    short = Outputs(len(uk) - 1)
    with pytest.raises(wx.WarpExecError) as ei:
        short.run(t, "va[idx]", "kk[idx]", None)
    assert ei.value.status == wx.WX_ERR_CAPACITY
    short.untouched_from(len(uk) - 1)
    assert record().route == wx.RO_ROUTE_NONE
    check_route(t, uk, cnt, want, ordered, None, wx.RO_ROUTE_DIRECT, wx.RO_WHY_NONE)
