"""GPU tests of the range-partitioned GROUP BY (wx_group_part.hip) where its
loops go round: many tiles per workgroup, several / empty / trailing plan
items, long and sparse aggregation items.

At the default geometry a tile workgroup runs ONE tile until a table holds more
than 256 x 16 384 rows, so in tests/test_gpu_group_wide.py the software-
pipelined tile loop of wx_group_part_tiles (the previous tile's write-out at
the top of an iteration, the next tile's loads under the LDS phases, the
per-workgroup totals carried over tiles) never takes a second iteration, the
plan never cuts an empty or a trailing item, and the aggregation never stages
a second directory round.  Here the diagnostic defines WX_GP_GRID=3 / 2 cap
the tile grid and WX_GP_DIRCH=40 shortens a directory round, so tables of 12
to 132 tiles reach all of that.

Every case goes through wx.group_sum with capacity > 4096 and
WARPDB_GP_MIN_ROWS=0, and first calls regime(): it sets the defines and
asserts the geometry wx_group_part_geometry reports for the live device
(tiles_per_wg >= 3, the grid, dir_chunk, n_part).  run() then asserts, from
the workspace's pass counter, which route the call took: a query that
finished through the LDS window + global hash, or at one tile per workgroup,
fails here although its result is right.  The layouts (tests/gp_layouts.py)
assert on the CPU the edge each is named for.

Values are small integers, so every double sum is exact in any order: keys,
counts and sums are compared bit for bit with ora.group_sum (pinned against
numpy by tests/test_group_part_geometry.py).  One uniform-float case keeps the
1e-12 relative bound of tests/test_gpu_group_wide.py.  The cost of a case is
its hiprtc compile: the parameters are what changes the module (defines,
WHERE, alignment, column types) and the layouts loop inside.
"""
from __future__ import annotations

import numpy as np
import pytest

import gp_layouts as tl
import oracle_lib as ora
from test_gpu_parity import dev_table, launch

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from warpdb_amd import _warpexec as wx  # noqa: E402

CAP = 1 << 20
KEY_FILL = -7
# The key range of a call is remembered per (expressions, device pointers,
# rows); a freed table's memory handed to the next one would make that table's
# first pass a guess (two passes where a case expects one).  Tables stay alive.
_KEEP = []


def regime(monkeypatch, defines, n, span, grid, n_part=None, dir_chunk=4096, guess="0"):
    """Set the hooks and assert what wx_group_part_geometry then says of a pass
    over n rows and `span` keys on the live device."""
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", defines)
    monkeypatch.setenv("WARPDB_GP_MIN_ROWS", "0")
    monkeypatch.setenv("WARPDB_GP_GUESS", guess)
    monkeypatch.delenv("WARPDB_GROUP_PARTITION", raising=False)
    g = wx.group_part_geometry(n, span, launch=launch())
    assert g.tiles_per_wg >= 3 and g.grid == grid, (g.grid, g.tiles_per_wg)
    assert g.n_tiles > (g.grid - 1) * g.tiles_per_wg and g.tile_rows == tl.TILE
    assert g.dir_chunk == dir_chunk and g.chunk_rows == tl.CHUNK and g.part_keys == tl.PART
    assert g.n_part == (n_part if n_part is not None else -(-span // tl.PART))
    return g


def upload(cols, offset=0):
    table, tensors = dev_table(cols, offset=offset)
    _KEEP.append((table, tensors))
    return table, tensors


def call(table, where, cap=CAP):
    """One wx_group_sum: (keys, sums, counts, passes it took)."""
    k = torch.full((cap + 64,), KEY_FILL, dtype=torch.int32, device="cuda")
    s = torch.zeros(cap, dtype=torch.float64, device="cuda")
    c = torch.zeros(cap, dtype=torch.int64, device="cuda")
    before = wx.group_part_passes(launch())
    try:
        g = wx.group_sum(table, "v[idx]", "k[idx]", tl.COND if where else None, launch(), 0, cap, k.data_ptr(),
                         s.data_ptr(), c.data_ptr())
    finally:
        passes = wx.group_part_passes(launch()) - before
    assert (k[g:g + 64] == KEY_FILL).all()  # nothing written past the groups
    return k[:g].cpu().numpy(), s[:g].cpu().numpy(), c[:g].cpu().numpy(), passes


def check(got, cols, where, passes=1, rtol=None):
    gk, gs, gc, took = got
    assert took == passes, f"{took} partitioned passes, expected {passes}"
    rk, rs, rc = ora.group_sum(ora.HostTable(cols), "v", "k", tl.OCOND if where else None, capacity=CAP)
    assert np.array_equal(gk, rk) and np.array_equal(gc, rc)
    if rtol is None:
        assert np.array_equal(gs.view(np.int64), rs.view(np.int64))
    else:
        np.testing.assert_allclose(gs, rs, rtol=rtol, atol=0)
    return len(rk)


def run(lay, where, name="", passes=1, offset=0, **types):
    cols = lay.cols(**types)
    table, _ = upload(cols, offset)
    try:
        return check(call(table, where), cols, where, passes)
    except AssertionError as e:
        raise AssertionError(f"layout {name} (n = {lay.n}, where = {where}): {e}") from e


WHERE = pytest.mark.parametrize("where", [False, True], ids=["all", "where"])


def _uniform_cases():
    """(name, n, span, key_lo): the sizes at 23 partitions, the partition counts
    at the ragged size, both ends of the int32 range."""
    for n in (tl.N_RAGGED, tl.N_ONE_ROW, tl.N_WHOLE):
        yield f"uniform_{n}", n, tl.SPAN23, 0
    yield "one_partition", tl.N_RAGGED, 5000, 7
    yield "2048_partitions", tl.N_RAGGED, 2 ** 24, -40_000
    yield "from_int32_min", tl.N_ONE_ROW, tl.SPAN23, -(2 ** 31)
    yield "to_int32_max", tl.N_RAGGED, tl.SPAN23, 2 ** 31 - tl.SPAN23
    yield "2048_partitions_from_int32_min", tl.N_WHOLE, 2 ** 24, -(2 ** 31)
    yield "2048_partitions_to_int32_max", tl.N_ONE_ROW, 2 ** 24, 2 ** 31 - 2 ** 24


# --------------------------------------------- a. many tiles per workgroup
def test_many_tiles_per_workgroup(monkeypatch):
    for name, n, span, lo in _uniform_cases():
        g = regime(monkeypatch, tl.GRID3, n, span, grid=3)
        assert g.tiles_per_wg == (5 if n == tl.N_ONE_ROW else 4)
        lay = tl.uniform(n, span, lo)
        assert lay.span(False) == span and lay.lo(False) == lo
        groups = run(lay, False, name)
        assert groups == len(np.unique(lay.keys))
    # uniform float values: double sums in another order than the oracle's, to 1e-12
    n = tl.N_RAGGED
    regime(monkeypatch, tl.GRID3, n, tl.SPAN23, grid=3)
    cols = tl.uniform(n, tl.SPAN23).cols()
    cols["v"] = np.random.default_rng(7).uniform(0.0, 40.0, n).astype(np.float32)
    check(call(upload(cols)[0], False), cols, False, rtol=1e-12)


# ------------------------------------------------------------ b. stage reuse
@WHERE
def test_stage_reuse_between_unlike_tiles(where, monkeypatch):
    for n in (tl.N_RAGGED, tl.N_ONE_ROW):
        g = regime(monkeypatch, tl.GRID3, n, tl.SPAN23, grid=3)
        run(tl.stage(n, g), where, "stage")


# ------------------------------------------------------------- c. plan items
@WHERE
@pytest.mark.parametrize("defines", [tl.GRID3, tl.GRID2], ids=["grid3", "grid2"])
def test_plan_items_of_a_heavy_partition(defines, where, monkeypatch):
    ran = 0
    for name, (d, n, counts, claims) in tl.heavy_cases().items():
        if d != defines:
            continue
        g = regime(monkeypatch, defines, n, tl.SPAN23, grid=3 if defines == tl.GRID3 else 2)
        lay = tl.heavy(n, g, counts)
        tl.check_heavy(lay, g, claims)   # the live geometry cuts the items the layout is named for
        run(lay, where, name)
        ran += 1
    assert ran == 2


# ------------------------------------------------------ d. sparse partitions
def test_sparse_partitions(monkeypatch):
    n = tl.N_SPARSE
    g = regime(monkeypatch, tl.GRID3, n, tl.SPAN23, grid=3)
    assert g.tiles_per_wg == 20
    run(tl.sparse(n, g), False, "sparse")


# --------------------------------------------------------------- e. long items
@pytest.mark.parametrize("defines", [tl.GRID2, tl.GRID2_DIR40], ids=["second_sweep", "directory_rounds"])
def test_long_items(defines, monkeypatch):
    n, span = tl.N_LONG, tl.LONG_PARTS * tl.PART
    rounds = defines == tl.GRID2_DIR40
    g = regime(monkeypatch, defines, n, span, grid=2, n_part=tl.LONG_PARTS,
               dir_chunk=tl.DIRCH_SMALL if rounds else 4096)
    assert g.n_tiles == 132 > g.agg_tiles_per_sweep == 128
    if rounds:
        assert g.n_tiles > 3 * g.dir_chunk and (g.n_tiles % g.dir_chunk) % 8 != 0
    run(tl.long_items(n, g), False, "long")


# ------------------------------------------------------- f. unaligned columns
@WHERE
def test_unaligned_columns(where, monkeypatch):
    for n in (tl.N_RAGGED, tl.N_ONE_ROW, tl.N_WHOLE):
        g = regime(monkeypatch, tl.GRID3, n, tl.SPAN23, grid=3)
        run(tl.stage(n, g) if where else tl.uniform(n, tl.SPAN23), where, "unaligned", offset=1)


# ------------------------------------------------- g. int64 keys, f64 values
@WHERE
def test_int64_keys_and_f64_values(where, monkeypatch):
    for n in (tl.N_RAGGED, tl.N_ONE_ROW, tl.N_WHOLE):
        g = regime(monkeypatch, tl.GRID3, n, tl.SPAN23, grid=3)
        run(tl.stage(n, g) if where else tl.uniform(n, tl.SPAN23), where, "typed", key_dtype=np.int64,
            val_dtype=np.float64)


# ------------------------------------------------ h. re-plan from a late tile
def test_replan_from_the_last_tile(monkeypatch):
    n = tl.N_RAGGED
    g = regime(monkeypatch, tl.GRID3, n, tl.SPAN23, grid=3)
    last_tile = (g.n_tiles - 1) * g.tile_rows
    assert n - last_tile == 5 and g.n_tiles - 1 == g.grid * g.tiles_per_wg - 1   # the last workgroup's last tile
    # 3000 distinct keys over the 23 partitions: the window + hash route of the last step then holds
    # fewer than 4096 keys outside its window and needs no key sort (a module of its own to compile)
    lay = tl.uniform(n, tl.SPAN23)
    lay.keys[1:n - 1] = ((np.arange(1, n - 1, dtype=np.int64) * tl.HASH) % 3000) * (tl.SPAN23 // 3000)
    assert lay.span(False) == tl.SPAN23 and len(np.unique(lay.keys)) <= 3002
    cols = lay.cols()
    table, tensors = upload(cols)
    check(call(table, False), cols, False, passes=1)
    check(call(table, False), cols, False, passes=1)   # from the remembered range

    def rewrite(keys):
        cols["k"] = keys.astype(np.int32)
        tensors["k"].copy_(torch.from_numpy(cols["k"]))

    # the only keys outside the remembered range sit in the last tile of the last workgroup, one on
    # each side: the pass counts them, aggregates nothing, and the query goes round over the exact range
    keys = lay.keys.copy()
    keys[n - 1], keys[n - 4] = tl.SPAN23 + 70_000, -30_000
    rewrite(keys)
    regime(monkeypatch, tl.GRID3, n, int(keys.max() - keys.min() + 1), grid=3)
    check(call(table, False), cols, False, passes=2)
    # nothing left over from the aborted pass (partition totals and counts, partial windows)
    check(call(table, False), cols, False, passes=1)
    # a remembered range whose exact range is wider than 2^24 keys: the aborted pass, then the
    # LDS window + global hash
    keys[n - 2] = 2 ** 25
    rewrite(keys)
    with pytest.raises(wx.WarpExecError) as e:
        wx.group_part_geometry(n, int(keys.max() - keys.min() + 1), launch=launch())
    assert e.value.status == wx.WX_ERR_UNSUPPORTED
    check(call(table, False), cols, False, passes=1)


def test_replan_after_a_sampled_guess(monkeypatch):
    # WARPDB_GP_GUESS=1: the first range is a 65 536-row sample's, widened by an eighth; keys far
    # outside it in the last tile only (no sampled row) send the query round again
    n = tl.N_RAGGED
    lay = tl.uniform(n, tl.SPAN23)
    sampled = np.arange(65536, dtype=np.int64) * (n // 65536) + (np.arange(65536, dtype=np.int64) * (n % 65536)) // 65536
    assert n - 2 not in sampled and n - 2 >= (tl.N_RAGGED // tl.TILE) * tl.TILE
    lay.keys[n - 2] = 3 * tl.SPAN23
    regime(monkeypatch, tl.GRID3, n, 3 * tl.SPAN23 + 1, grid=3, guess="1")
    run(lay, False, "sampled guess", passes=2)


# ----------------------------------------------------------------- i. capacity
def test_capacity_error_then_exact(monkeypatch):
    n = tl.N_RAGGED
    regime(monkeypatch, tl.GRID3, n, tl.SPAN23, grid=3)
    lay = tl.uniform(n, tl.SPAN23)
    cols = lay.cols()
    table, _ = upload(cols)
    small = 5000   # above 4096: the partitioned route, far fewer than the ~1.2e5 groups
    k = torch.empty(small, dtype=torch.int32, device="cuda")
    s = torch.empty(small, dtype=torch.float64, device="cuda")
    c = torch.empty(small, dtype=torch.int64, device="cuda")
    before = wx.group_part_passes(launch())
    with pytest.raises(wx.WarpExecError) as e:
        wx.group_sum(table, "v[idx]", "k[idx]", None, launch(), 0, small, k.data_ptr(), s.data_ptr(), c.data_ptr())
    assert e.value.status == wx.WX_ERR_CAPACITY
    assert wx.group_part_passes(launch()) - before == 1
    # the first `small` groups are the oracle's: the emit clips, it does not scramble
    rk, rs, rc = ora.group_sum(ora.HostTable(cols), "v", "k", None, capacity=CAP)
    assert len(rk) > small
    assert np.array_equal(k.cpu().numpy(), rk[:small]) and np.array_equal(c.cpu().numpy(), rc[:small])
    assert np.array_equal(s.cpu().numpy().view(np.int64), rs[:small].view(np.int64))
    check(call(table, False), cols, False, passes=1)
