"""GPU tests of the radix sort (wx_radix.hip, warpexec/sort.cpp) at the edges
of its live geometry and in the regimes the parity tests do not reach.

The tile sizes come from wx.sort_tile_keys (keys / key + payload) and the
histogram's span from wx.sort_hist_span_keys, so the sizes follow the
kernels when their geometry changes.  Covered here:

  a. tile boundaries (T - 1 .. 5T + 1) of every tile kernel behind the ABI;
  b. sorted, reverse-sorted and one-hot inputs (sparse look-back words);
  c. ~2 000-tile look-back chains under a 512-key diagnostic geometry;
  d. the histogram's software-pipelined loop and its special-key flag;
  e. 0 .. 4 executed passes and a skipped middle pass, for every buffer
     arrangement (in place, from a column, src == dst, pairs, and the
     row-order GROUP BY's column-reading pair sort);
  f. the status words' epoch wrap with one status buffer reused by sorts of
     different tile counts;
  g. the head route of ORDER BY .. LIMIT next to the full route.

Reference: NumPy's stable argsort of the keys (`v` ascending, `-v` descending
for floats, `-keys.astype(int64)` for ints): NaN last in both directions,
-0.0 == +0.0, input order among equals.  Keys are compared bit for bit,
payloads (the input positions: they prove stability) exactly, and every
buffer a sort writes carries sentinels in front of and behind the sorted
range that must come back unchanged.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle_lib as ora
import synth
from test_gpu_parity import _sort_input, dev_table, launch
from test_sort_geometry_abi import TINY_DEFINES, TINY_TILE

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from warpdb_amd import _warpexec as wx  # noqa: E402

# The data starts PAD elements into its allocation: 16-byte aligned like a
# fresh allocation (the histogram's vector loads), with sentinels in front.
PAD = 4
F_SENT = np.float32(-12345.5)
I_SENT = np.int32(-77)
DIRS = (True, False)
EDGES = ["T-1", "T", "T+1", "2T-1", "2T", "2T+1", "5T", "5T+1"]


def edge(name, t):
    """EDGES entry -> element count for tile size t."""
    mult, _, rest = name.partition("T")
    return int(mult or 1) * t + int(rest or 0)


def tile(pairs):
    t = wx.sort_tile_keys(1 if pairs else 0)
    assert t > 0
    return t


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def order_f(v, asc):
    return np.argsort(v if asc else -v, kind="stable")


def order_i(k, asc):
    return np.argsort(k if asc else -k.astype(np.int64), kind="stable")


def order_keys(a, asc=True):
    """The 32-bit order key the kernels sort by: wx::f2ord for floats, the
    sign flip for ints, complemented for a descending sort; a NaN's key is
    the largest in both directions."""
    b = u32(a).copy()
    if a.dtype == np.int32:
        k = b ^ np.uint32(0x80000000)
        return k if asc else ~k
    nan = (b & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    b[b == np.uint32(0x80000000)] = 0  # -0.0 == +0.0
    k = np.where(b >> np.uint32(31) != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    if not asc:
        k = ~k
    k[nan] = np.uint32(0xffffffff)
    return k


def varying_bytes(a):
    """Which of the order key's four bytes differ between keys: the radix
    passes sort.cpp executes (a constant digit's pass is skipped)."""
    k = order_keys(a)
    return [bool((((k >> np.uint32(8 * p)) & np.uint32(255)) != ((k[0] >> np.uint32(8 * p)) & np.uint32(255))).any())
            for p in range(4)]


def has_special(v):
    b = u32(v)
    return bool((((b & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)) | (b == np.uint32(0x80000000))).any())


def padded(a, sentinel):
    """Device buffer [PAD sentinels | a | 1 sentinel]; the pointer to a's first element."""
    buf = torch.empty(len(a) + PAD + 1, dtype=torch.float32 if a.dtype == np.float32 else torch.int32, device="cuda")
    buf.fill_(float(sentinel) if a.dtype == np.float32 else int(sentinel))
    buf[PAD:PAD + len(a)].copy_(torch.from_numpy(a if a.flags.writeable else a.copy()))  # (shared inputs are read-only)
    return buf, buf[PAD:].data_ptr()


def expect(buf, ref, sentinel, what, head=None):
    """The sorted range equals ref bit for bit (its first `head` elements
    when given) and the sentinels around it are unchanged."""
    h = buf.cpu().numpy()
    n = len(ref)
    k = n if head is None else head
    assert np.array_equal(u32(h[PAD:PAD + k]), u32(ref[:k])), what
    assert (h[:PAD] == sentinel).all(), what + ": written in front of the buffer"
    assert h[PAD + n] == sentinel, what + ": written behind the buffer"


def check_float(v, asc, entry="sort_float"):
    """sort_float (in place), sort_float_from into a separate buffer, or sort_float_from with src == dst."""
    n = len(v)
    ref = v[order_f(v, asc)]
    if entry == "from":
        src, ps = padded(v, F_SENT)
        dst, pd = padded(np.full(n, 4321.0, np.float32), np.float32(-654.0))
        wx.sort_float_from(ps, pd, n, asc, launch())
        expect(dst, ref, np.float32(-654.0), f"{entry} asc={asc}")
        expect(src, v, F_SENT, f"{entry} asc={asc}: the source was written")
        return
    buf, p = padded(v, F_SENT)
    if entry == "sort_float":
        wx.sort_float(p, n, asc, launch())
    else:
        assert entry == "from_same"
        wx.sort_float_from(p, p, n, asc, launch())
    expect(buf, ref, F_SENT, f"{entry} asc={asc}")


def check_pairs(keys, asc):
    """sort_by_key (float keys) or sort_pairs (int32 keys); payload = input position."""
    n = len(keys)
    assert n < (1 << 24)  # positions are exact in float32
    pos = np.arange(n, dtype=np.float32)
    if keys.dtype == np.float32:
        order, ksent, fn = order_f(keys, asc), F_SENT, wx.sort_by_key
    else:
        order, ksent, fn = order_i(keys, asc), I_SENT, wx.sort_pairs
    bk, pk = padded(keys, ksent)
    bv, pv = padded(pos, F_SENT)
    fn(pk, pv, n, asc, launch())
    expect(bk, keys[order], ksent, f"{fn.__name__} keys asc={asc}")
    expect(bv, pos[order], F_SENT, f"{fn.__name__} payload asc={asc}")


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def general_mix(n):
    v = _sort_input(n, 11)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def plain_mix(n):
    """The mix with no key the plain order flip would misplace: NaN -> +inf, -0.0 -> +0.0."""
    v = _sort_input(n, 11)
    v[np.isnan(v)] = np.float32(np.inf)
    v[(v == 0) & np.signbit(v)] = np.float32(0.0)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def full_range_ints(n, seed=6):
    k = (synth.uniform_int(n, seed, 0, (1 << 32) - 1) - (1 << 31)).astype(np.int32)
    k[:3] = [np.iinfo(np.int32).min, np.iinfo(np.int32).max, 0]
    k[n // 2:n // 2 + min(1000, n // 4)] = 7  # a long run of ties
    k.setflags(write=False)
    return k


def full_range_floats(n, seed):
    """Random bit patterns: every exponent and both signs, NaN patterns and -0.0 included."""
    return synth.uniform_int(n, seed, 0, (1 << 32) - 1).astype(np.uint32).view(np.float32)


def skewed_ints(n):
    # the keys of test_sort_ranking_modes_agree: one digit skewed next to a full-range digit
    rng = np.random.default_rng(n)
    return np.where(rng.random(n) < 0.7, rng.integers(0, 3, n), rng.integers(-2**31, 2**31 - 1, n)).astype(np.int32)


# ------------------------------------------- a. tile boundaries, every kernel
@pytest.mark.parametrize("mix", ["general", "plain"])
@pytest.mark.parametrize("size", EDGES)
def test_tile_edges_sort_float(size, mix):
    # general: wx_radix_tile_k_f_*; plain: wx_radix_tile_k_fp_* -- the variant
    # follows from the input, which is checked
    n = edge(size, tile(False))
    v = general_mix(n) if mix == "general" else plain_mix(n)
    assert has_special(v) == (mix == "general")
    if mix == "general":
        assert np.isnan(v).any() and ((v == 0) & np.signbit(v)).any()
    for asc in DIRS:
        check_float(v, asc)


@pytest.mark.parametrize("size", EDGES)
def test_tile_edges_sort_float_from(size):
    n = edge(size, tile(False))
    for asc in DIRS:
        check_float(general_mix(n), asc, "from")


@pytest.mark.parametrize("mix", ["general", "plain"])
@pytest.mark.parametrize("size", EDGES)
def test_tile_edges_sort_by_key(size, mix):
    # wx_radix_tile_kv_f_* / kv_fp_*
    n = edge(size, tile(True))
    v = general_mix(n) if mix == "general" else plain_mix(n)
    assert has_special(v) == (mix == "general")
    for asc in DIRS:
        check_pairs(v, asc)


@pytest.mark.parametrize("size", EDGES)
def test_tile_edges_sort_pairs(size):
    # wx_radix_tile_kv_i_*
    n = edge(size, tile(True))
    keys = full_range_ints(n)
    assert keys.min() == np.iinfo(np.int32).min and keys.max() == np.iinfo(np.int32).max
    for asc in DIRS:
        check_pairs(keys, asc)


# ------------------------------------------------ b. sparse look-back words
def sparse_input(kind, n, t, ints):
    """Sorted / reverse-sorted full-range keys (in the top-digit pass most
    digits are absent from most tiles: the walk sums runs of zero {A} words)
    or one-hot keys (all equal but one key in tile 0 and one in the last tile)."""
    if kind == "one_hot":
        a = np.full(n, 7, np.int32) if ints else np.full(n, 1.0, np.float32)
        a[3] = -5 if ints else 2.0
        a[n - 1] = 100_000 if ints else 0.5
        assert n - 1 >= (n - 1) // t * t >= 4 * t  # the second odd key sits in the last of >= 5 tiles
        return a
    if ints:
        a = np.sort(full_range_ints(n, seed=13))
    else:
        f = full_range_floats(n, 17)
        a = f[order_f(f, True)]
    return np.ascontiguousarray(a[::-1]) if kind == "reverse" else a


@pytest.mark.parametrize("kind", ["sorted", "reverse", "one_hot"])
def test_sparse_lookback_sort_float(kind):
    t = tile(False)
    v = sparse_input(kind, 5 * t + 1, t, False)
    for asc in DIRS:
        check_float(v, asc)


@pytest.mark.parametrize("kind", ["sorted", "reverse", "one_hot"])
def test_sparse_lookback_sort_pairs(kind):
    t = tile(True)
    keys = sparse_input(kind, 5 * t + 1, t, True)
    for asc in DIRS:
        check_pairs(keys, asc)


# ------------------------------------------------------------ c. long chains
LONG = 1_000_003  # ~1 950 tiles of 512 keys


@pytest.fixture
def tiny_tiles(monkeypatch):
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", TINY_DEFINES)
    assert wx.sort_tile_keys(0) == TINY_TILE and wx.sort_tile_keys(1) == TINY_TILE


def test_long_chain_sort_float(tiny_tiles):
    v = general_mix(LONG)
    for asc in DIRS:
        check_float(v, asc)


def test_long_chain_sort_pairs(tiny_tiles):
    keys = skewed_ints(LONG)
    for asc in DIRS:
        check_pairs(keys, asc)


def test_long_chain_sorted_input(tiny_tiles):
    f = full_range_floats(LONG, 19)
    v = f[order_f(f, True)]
    for asc in DIRS:
        check_float(v, asc)


# ------------------------- d. the histogram's pipelined loop and its flag
def hist_layout():
    """(n, S, C): workgroup 0 of the histogram owns two whole spans (its
    prefetch runs once with `more` true and once false), workgroup 1 one
    whole span and the partial one, and three keys take the scalar tail."""
    s = wx.sort_hist_span_keys()
    c = torch.cuda.get_device_properties(0).multi_processor_count
    n = (c + 1) * s + s // 2 + 3
    assert s > 0 and n // s > c, "the pipelined loop would not run"
    assert n % 4 == 3
    return n, s, c


@functools.lru_cache(maxsize=None)
def hist_base(n):
    v = plain_mix(n).copy()
    v.setflags(write=False)
    return v


@pytest.mark.parametrize("where", ["second_span", "partial_span", "scalar_tail"])
@pytest.mark.parametrize("special", ["neg_zero", "nan"])
def test_hist_pipelined_loop_special_key(special, where, monkeypatch):
    n, s, c = hist_layout()
    at = {"second_span": c * s + s // 3, "partial_span": (c + 1) * s + s // 4, "scalar_tail": n - 2}[where]
    assert {"second_span": c * s <= at < (c + 1) * s, "partial_span": (c + 1) * s <= at < n - 3,
            "scalar_tail": at >= n - 3}[where]
    v = hist_base(n).copy()
    assert not has_special(v)
    if special == "neg_zero":
        # +0.0 before and behind it: a wrong key map changes the order of the bit patterns
        v[5] = v[at - 7] = v[min(at + 1, n - 1)] = np.float32(0.0)
        v[at] = np.float32(-0.0)
    else:
        v[at] = np.float32(np.nan)
    b = u32(v)
    assert int((((b & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)) | (b == np.uint32(0x80000000))).sum()) == 1
    for asc in DIRS:
        for plain in (None, "0"):
            if plain is None:
                monkeypatch.delenv("WARPDB_RS_PLAIN", raising=False)
            else:
                monkeypatch.setenv("WARPDB_RS_PLAIN", plain)
            check_float(v, asc)


def test_hist_pipelined_loop_no_special_key(monkeypatch):
    n, _, _ = hist_layout()
    v = hist_base(n)
    assert not has_special(v)
    for asc in DIRS:
        for plain in (None, "0"):
            if plain is None:
                monkeypatch.delenv("WARPDB_RS_PLAIN", raising=False)
            else:
                monkeypatch.setenv("WARPDB_RS_PLAIN", plain)
            check_float(v, asc)


def test_hist_pipelined_loop_int_keys():
    # wx_radix_hist_i_a / _i_d
    n, _, _ = hist_layout()
    keys = full_range_ints(n)
    for asc in DIRS:
        check_pairs(keys, asc)


def test_hist_scalar_path_at_the_same_size():
    # a view one element into its allocation: the histogram's scalar loads
    n, _, _ = hist_layout()
    v = general_mix(n)
    buf = torch.full((n + 2,), float(F_SENT), dtype=torch.float32, device="cuda")
    buf[1:n + 1].copy_(torch.from_numpy(v.copy()))
    wx.sort_float(buf[1:].data_ptr(), n, False, launch())
    h = buf.cpu().numpy()
    assert np.array_equal(u32(h[1:n + 1]), u32(v[order_f(v, False)]))
    assert h[0] == F_SENT and h[n + 1] == F_SENT


# ----------------- e. executed passes 0 .. 4, every buffer arrangement
def float_keyset(name, n):
    """Positive floats built from bit patterns, the top byte constant (0x3f),
    so the number of varying bytes is known by construction."""
    r = lambda seed, hi: synth.uniform_int(n, seed, 0, hi - 1).astype(np.uint32)  # noqa: E731
    if name == "p0":
        return np.full(n, 7.5, np.float32)
    if name == "p1":
        return (np.uint32(0x3F800000) + r(3, 1 << 8)).view(np.float32)
    if name == "p2":
        return (np.uint32(0x3F800000) + r(4, 1 << 16)).view(np.float32)
    if name == "p3":  # 0.5 .. 2: 24 varying bits under a constant top byte
        return (np.uint32(0x3F000000) | r(5, 1 << 24)).view(np.float32)
    if name == "p4":
        return _sort_input(n, 23)
    assert name == "skip_mid"  # bytes 0 and 2 vary, byte 1 is constant
    return (np.uint32(0x3F800000) | r(7, 1 << 8) | (r(8, 1 << 7) << np.uint32(16))).view(np.float32)


def int_keyset(name, n):
    r = lambda seed, hi: synth.uniform_int(n, seed, 0, hi - 1).astype(np.int32)  # noqa: E731
    if name == "p0":
        return np.full(n, 41, np.int32)
    if name in ("p1", "p2", "p3"):
        return r(int(name[1]), 1 << (8 * int(name[1])))
    if name == "p4":
        return np.array(full_range_ints(n))
    assert name == "skip_mid"
    return r(7, 1 << 8) | (r(8, 1 << 8) << 16)


PASSES = {"p0": [False] * 4, "p1": [True, False, False, False], "p2": [True, True, False, False],
          "p3": [True, True, True, False], "p4": [True] * 4, "skip_mid": [True, False, True, False]}


@pytest.mark.parametrize("keyset", list(PASSES))
@pytest.mark.parametrize("entry", ["sort_float", "from", "from_same", "sort_by_key"])
def test_executed_passes_float_keys(entry, keyset):
    # (Which buffer the column-reading sort's last pass lands in is chosen so
    # that no copy back is needed; a wrong choice costs that copy and changes
    # no result, so it cannot be seen from here.  What is pinned is the result,
    # the untouched source and the sentinels for every number of passes.)
    n = 2 * tile(entry == "sort_by_key") + 1
    v = float_keyset(keyset, n)
    assert varying_bytes(v) == PASSES[keyset]  # the passes that run, from the keys themselves
    for asc in DIRS:
        if entry == "sort_by_key":
            check_pairs(v, asc)
        else:
            check_float(v, asc, entry)


@pytest.mark.parametrize("keyset", list(PASSES))
def test_executed_passes_sort_pairs(keyset):
    n = 2 * tile(True) + 1
    keys = int_keyset(keyset, n)
    assert varying_bytes(keys) == PASSES[keyset]
    for asc in DIRS:
        check_pairs(keys, asc)


@pytest.mark.parametrize("keyset", ["p1", "p2", "skip_mid", "p3"])
def test_executed_passes_group_rows_general(keyset, monkeypatch):
    """The row-order GROUP BY's general path with a bare int32 key column, a
    bare float value column and no WHERE: the pair sort reads both columns in
    place (src0 / src_v) and hands back whichever buffers its last pass wrote
    (res_k / res_v) -- after 1, 2 (adjacent or around a skipped pass) and 3
    executed passes.  Keys, counts exact; sums bit for bit (the oracle's
    sequential fold); both columns unwritten."""
    monkeypatch.setenv("WARPDB_GROUP_ROWS", "general")
    n = 2 * tile(True) + 1
    if keyset == "p3":  # at most 4 096 distinct 3-byte keys: the capacity stays small
        pool = np.unique(synth.uniform_int(4096, 21, 0, (1 << 24) - 1)).astype(np.int32)
        keys = pool[synth.uniform_int(n, 22, 0, len(pool) - 1)]
    else:
        keys = int_keyset(keyset, n)
    assert varying_bytes(keys) == PASSES[keyset]
    rng = np.random.default_rng(n)
    scale = rng.choice(np.array([1e7, 1.0, 1e-3], np.float32), n)  # sums that depend on the fold order
    cols = {"price": (rng.uniform(0.0, 1.0, n).astype(np.float32) * scale).astype(np.float32),
            "quantity": np.ascontiguousarray(keys)}
    cap = 1 << 16
    table, tensors = dev_table(cols)
    gk = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    gs = torch.full((cap,), float("nan"), dtype=torch.float64, device="cuda")
    gc = torch.full((cap,), -1, dtype=torch.int64, device="cuda")
    L = wx.make_launch(device=0, stream=torch.cuda.current_stream().cuda_stream, flags=wx.F_ROW_ORDER)
    g = wx.group_sum(table, "price[idx]", "quantity[idx]", None, L, 0, cap, gk.data_ptr(), gs.data_ptr(),
                     gc.data_ptr())
    rk, rs, rc = ora.group_sum(ora.HostTable(cols), "price", "quantity", capacity=cap)
    assert g == len(rk) == len(np.unique(keys))
    assert np.array_equal(gk[:g].cpu().numpy(), rk) and np.array_equal(gc[:g].cpu().numpy(), rc)
    assert np.array_equal(gs[:g].cpu().numpy().view(np.uint64), rs.view(np.uint64))
    assert np.array_equal(u32(tensors["price"].cpu().numpy()), u32(cols["price"])), "the value column was written"
    assert np.array_equal(tensors["quantity"].cpu().numpy(), cols["quantity"]), "the key column was written"


# --------------------------- f. epoch wrap over a reused status buffer
def test_epoch_wrap_sort_float():
    """25 four-pass sorts on one stream: one at 8T + 1 sizes the status buffer,
    then the sizes cycle through T + 1, 8T + 1 and 3T, so more than 63 passes
    (WX_RS_EPOCHS) reuse the same words for different tile counts and the
    epoch counter wraps.  Every result is compared in full."""
    t = tile(False)
    sizes = [8 * t + 1] + [(t + 1, 8 * t + 1, 3 * t)[i % 3] for i in range(24)]
    for i, n in enumerate(sizes):
        v = full_range_floats(n, 100 + i)
        assert varying_bytes(v) == [True] * 4
        check_float(v, i % 2 == 0)
    assert 4 * len(sizes) > 63 + 32


def test_epoch_wrap_sort_pairs():
    t = tile(True)
    sizes = [8 * t + 1] + [(t + 1, 8 * t + 1, 3 * t)[i % 3] for i in range(20)]
    for i, n in enumerate(sizes):
        keys = (synth.uniform_int(n, 200 + i, 0, (1 << 32) - 1) - (1 << 31)).astype(np.int32)
        assert varying_bytes(keys) == [True] * 4
        check_pairs(keys, i % 2 == 0)
    assert 4 * len(sizes) > 63


# ------------------------------------ g. the head route of LIMIT, small n
LIMITS = ["1", "100", "n//8", "n//2"]


def limit_of(name, n):
    return {"1": 1, "100": 100, "n//8": n // 8, "n//2": n // 2}[name]


@functools.lru_cache(maxsize=None)
def limit_keys(n):
    v = synth.uniform_f32(n, 41, 0.0, 40.0)
    v = np.where(v > 0, v, np.float32(20.0)).astype(np.float32)  # (0, 40)
    v.setflags(write=False)
    return v


def takes_head_route(v, limit, asc):
    """sort.cpp's rule restated from the data: the sorted order's first
    `limit` keys lie in the top-digit buckets up to the one holding rank
    limit - 1; the head route runs when those buckets hold at most n / 4 keys."""
    top = (order_keys(v, asc) >> np.uint32(24)).astype(np.int64)
    counts = np.bincount(top, minlength=256)
    if counts.max() == len(v) or not limit < len(v):
        return False
    cum = np.cumsum(counts)
    head = int(cum[np.searchsorted(cum, max(limit, 1), side="left")])
    return head <= len(v) // 4


def test_limit_cases_cover_both_routes():
    routes = set()
    for pairs in (False, True):
        n = 8 * tile(pairs) + 1
        for name in LIMITS:
            for asc in DIRS:
                routes.add(takes_head_route(limit_keys(n), limit_of(name, n), asc))
    assert routes == {True, False}


@pytest.mark.parametrize("limit", LIMITS)
def test_limit_head_sort_float(limit):
    n = 8 * tile(False) + 1
    v = limit_keys(n)
    k = limit_of(limit, n)
    for asc in DIRS:
        buf, p = padded(v, F_SENT)
        wx.sort_float_limit(p, n, k, asc, launch())
        expect(buf, v[order_f(v, asc)], F_SENT, f"limit {k} asc={asc} head={takes_head_route(v, k, asc)}", head=k)


@pytest.mark.parametrize("limit", LIMITS)
def test_limit_head_sort_by_key(limit):
    n = 8 * tile(True) + 1
    v = limit_keys(n)
    k = limit_of(limit, n)
    pos = np.arange(n, dtype=np.float32)
    for asc in DIRS:
        order = order_f(v, asc)
        bk, pk = padded(v, F_SENT)
        bv, pv = padded(pos, F_SENT)
        wx.sort_by_key_limit(pk, pv, n, k, asc, launch())
        what = f"limit {k} asc={asc} head={takes_head_route(v, k, asc)}"
        expect(bk, v[order], F_SENT, what + " keys", head=k)
        expect(bv, pos[order], F_SENT, what + " payload", head=k)
