"""GPU tests of the LDS-window GROUP BY (wx_group_sum, wx_group_multi,
wx_join_group, wx_group_finalize, wx_group_multi_finalize and the general-key
table behind them) where its loops go round and its decisions flip: several
batches per workgroup, the wave-combined add's thresholds, windows at the ends
of the int32 range, the finalize's sort and capacity boundaries, and probing in
the general-key table.

At the default geometry a streaming workgroup runs ONE batch until a table
holds more than two million rows, so in the other GROUP BY tests the stride
loop never takes a second trip.  Here the diagnostic define WX_GROUP_GRID=3
(=1 in one case) caps the grid, so tables of ten spans give workgroup 0 four
batches.  Every case first calls regime(): it sets the define and asserts what
wx_group_window_geometry reports for the live device; a case that ran at one
batch per workgroup fails here although its result is right.  The layouts
(tests/gw_layouts.py) assert on the CPU the edge each is named for, from the
same geometry.

The reference is numpy in float64 / int64 (gw_layouts.numpy_groups: np.unique,
np.add.at, MIN / MAX with NaN skipped and -0.0 returned as +0.0), checked once
against the oracle (test_reference_is_the_oracle; more of it without a GPU in
tests/test_group_window_layouts.py).  Values are multiples of 2^-6 (2^-9 for
the join's product) bounded so that every partial sum is exact in a double,
and each table's reference sums are first checked to be unchanged under row
reversal: every comparison is exact -- keys, counts, the bits of sums, minima
and maxima.  Outputs are prefilled with a sentinel that must survive at every
position >= the group count, and every case runs twice on its workspace: the
second run is right only if the first returned every accumulator to idle.

The cost of a case is its hiprtc compile: a module is named by its family,
its WHERE, its alignment and the define list, so the layouts loop inside the
tests and the families are the parameters.
"""
from __future__ import annotations

import numpy as np
import pytest

import gw_layouts as gw
import oracle_lib as ora
from test_gpu_parity import dev_table, launch

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from warpdb_amd import _warpexec as wx  # noqa: E402

SENT = -77
# family -> (entry point, value expressions, sum mask, min/max mask); gw.FAMILIES has the geometry side
CALLS = {
    "group_sum": ("sum", ["va"], 0b1, 0b0),
    "group_agg": ("agg", ["vc"], 0b1, 0b1),
    "sum2": ("multi", ["va", "va * vb"], 0b11, 0b00),
    "mix3": ("multi", ["va", "vc", "va * vb"], 0b101, 0b010),
    "all4": ("multi", ["va", "va * vb", "vc", "vd"], 0b1111, 0b1111),
    "join_hash": ("join", ["va", "va * rr"], 0b11, 0b10),
    "join_direct": ("join", ["va", "va * rr"], 0b11, 0b10),
}
for _f, (_, _e, _s, _q) in CALLS.items():   # the two tables describe the same builds
    assert gw.FAMILIES[_f][1:3] == (bin(_s).count("1"), bin(_q).count("1"))


def regime(monkeypatch, family, n, defines=gw.GRID3, grid=3, batches=None):
    """Set the hooks and assert what wx_group_window_geometry then says of a call over n rows on the live device."""
    monkeypatch.setenv("WARPDB_EXTRA_DEFINES", defines)
    if family == "join_hash":
        monkeypatch.setenv("WARPDB_JOIN_FORM", "hash")
    else:
        monkeypatch.delenv("WARPDB_JOIN_FORM", raising=False)
    if family == "join_direct":
        rk = gw.right_columns()["rk"]
        assert wx.join_plan(len(rk), int(rk.min()), int(rk.max()))[0] == wx.JOIN_DIRECT
    fam, ns, nq, form = gw.FAMILIES[family]
    g = wx.group_window_geometry(n, ns, nq, fam, form, launch=launch())
    assert g.grid == max(1, min(grid, -(-((n + 3) // 4) // g.block_threads))), (g.grid, n)
    assert g.block_threads == (1024 if family == "all4" else 512) and g.span_rows == 8 * g.block_threads
    assert (g.window_keys, g.hsort_max) == (gw.WINDOW, gw.HSORT_MAX)
    if batches is not None:
        assert g.max_batches == batches, (g.max_batches, batches)
    return g


# ------------------------------------------------------------------ running
def upload(family, lay, offset=0):
    """(device tables, host value arrays by expression, the rows a call keeps beside its WHERE)."""
    if CALLS[family][0] == "join":
        cols, hit, rr = gw.join_left(lay)
        tables = (dev_table(cols, offset)[0], dev_table(gw.right_columns(), offset)[0])
        vals = {"va": cols["va"], "va * rr": cols["va"] * rr}
    else:
        cols = lay.cols()
        hit = np.ones(lay.n, bool)
        tables = (dev_table(cols, offset)[0],)
        vals = {"va": cols["va"], "va * vb": cols["va"] * cols["vb"], "vc": cols["vc"], "vd": cols["vd"]}
    return tables, vals, hit


def call(family, tables, key_lo, cap, where=False, L=None):
    """One call; (groups, keys, counts, sums[j], mins[j], maxs[j]) as host arrays of cap + 2 entries (None where
    not requested).  A WarpExecError carries them as `.outputs`."""
    kind, exprs, smask, qmask = CALLS[family]
    m, room = len(exprs), cap + 2
    full = lambda dt, want=True: torch.full((room,), SENT, dtype=dt, device="cuda") if want else None  # noqa: E731
    dk, dc = full(torch.int32), full(torch.int64)
    ds = [full(torch.float64, smask >> j & 1) for j in range(m)]
    dn = [full(torch.float32, qmask >> j & 1) for j in range(m)]
    dx = [full(torch.float32, qmask >> j & 1) for j in range(m)]
    p = lambda ts: [0 if t is None else t.data_ptr() for t in ts]  # noqa: E731
    host = lambda: (dk.cpu().numpy(), dc.cpu().numpy(), *[[None if t is None else t.cpu().numpy() for t in ts]  # noqa: E731
                                                           for ts in (ds, dn, dx)])
    L = L or launch()
    low = [ora.lower(e) for e in exprs]
    cond = gw.COND if where else None
    try:
        if kind == "sum":
            g = wx.group_sum(tables[0], low[0], "k[idx]", cond, L, key_lo, cap, dk.data_ptr(), ds[0].data_ptr(),
                             dc.data_ptr())
        elif kind == "agg":
            g = wx.group_agg(tables[0], low[0], "k[idx]", cond, L, key_lo, cap, dk.data_ptr(), ds[0].data_ptr(),
                             dc.data_ptr(), dn[0].data_ptr(), dx[0].data_ptr())
        elif kind == "multi":
            g = wx.group_agg_multi(tables[0], low, "k[idx]", cond, L, key_lo, cap, dk.data_ptr(), dc.data_ptr(), p(ds),
                                   p(dn), p(dx))
        else:
            g = wx.join_group_agg(tables[0], tables[1], "kk[idx]", "rk", low, "k[idx]", cond, L, key_lo, cap,
                                  dk.data_ptr(), dc.data_ptr(), p(ds), p(dn), p(dx))
    except wx.WarpExecError as e:
        e.outputs = host()
        raise
    return (g, *host())


def same_f32(got, want):
    """Bit for bit, any NaN matching any NaN."""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def compare(family, outs, refs, upto):
    """The first `upto` groups are the reference's, everything behind them the sentinel."""
    _, exprs, smask, qmask = CALLS[family]
    keys, cnts, sums, mins, maxs = outs
    rk, _, rc, _, _ = refs[0]
    assert np.array_equal(keys[:upto], rk[:upto]) and (keys[upto:] == SENT).all()
    assert np.array_equal(cnts[:upto], rc[:upto]) and (cnts[upto:] == SENT).all()
    for j, (k2, rs, c2, rmn, rmx) in enumerate(refs):
        assert np.array_equal(k2, rk) and np.array_equal(c2, rc)
        if smask >> j & 1:
            assert np.array_equal(sums[j][:upto].view(np.uint64), rs[:upto].view(np.uint64)), f"sum of {exprs[j]}"
            assert (sums[j][upto:] == SENT).all()
        if qmask >> j & 1:
            assert same_f32(mins[j][:upto], rmn[:upto]), f"min of {exprs[j]}"
            assert same_f32(maxs[j][:upto], rmx[:upto]), f"max of {exprs[j]}"
            assert (mins[j][upto:] == SENT).all() and (maxs[j][upto:] == SENT).all()


def references(family, lay, vals, hit, where=False):
    keep = lay.passing(where) & hit
    return [gw.exact_groups(lay.keys, vals[e], keep) for e in CALLS[family][1]]


def run(family, lay, cap, where=False, offset=0, L=None, name=""):
    """The layout through the family twice on one workspace, each result exactly the reference; returns the groups."""
    tables, vals, hit = upload(family, lay, offset)
    refs = references(family, lay, vals, hit, where)
    try:
        for _ in range(2):
            g, *outs = call(family, tables, lay.key_lo, cap, where, L)
            assert g == len(refs[0][0]), (g, len(refs[0][0]))
            compare(family, outs, refs, g)
    except AssertionError as e:
        raise AssertionError(f"{family}, layout {name} (n = {lay.n}, where = {where}, offset = {offset}): {e}") from e
    return g


def test_reference_is_the_oracle():
    lay = gw.steady(9 * 4096 + 5)
    cols = lay.cols()
    for expr, vals in (("va * vb", cols["va"] * cols["vb"]), ("vc", cols["vc"])):
        want = ora.group_agg(ora.HostTable(cols), expr, "k")
        got = gw.exact_groups(cols["k"], vals, np.ones(lay.n, bool))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
        assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))
        assert same_f32(got[3], want[3]) and same_f32(got[4], want[4])


# ---------------------------------------------------------- 1. steady state
@pytest.mark.parametrize("family", list(CALLS))
def test_steady_state(family, monkeypatch):
    S = regime(monkeypatch, family, 1, grid=1).span_rows
    sizes = gw.steady_sizes(regime(monkeypatch, family, 9 * S))
    assert sizes == [S - 1, S, S + 1, 3 * S, 9 * S + 5, 10 * S - 3]
    for n, batches in zip(sizes, (1, 1, 1, 1, 4, 4)):
        g = regime(monkeypatch, family, n, batches=batches)
        lay = gw.steady(n)
        gw.check_steady(lay, g)
        run(family, lay, 8000, name="steady")
    # at least three batches per workgroup, the last span ragged, and every load guarded
    n = sizes[4]
    g = regime(monkeypatch, family, n, batches=4)
    assert g.max_batches >= 3 and g.grid * (g.max_batches - 1) * g.span_rows < n
    run(family, gw.steady(n), 8000, offset=1, name="steady, unaligned")


def test_steady_state_one_workgroup(monkeypatch):
    """WX_GROUP_GRID=1: one workgroup gathers all ten batches in its LDS bins before the one flush."""
    n = 9 * 4096 + 5
    g = regime(monkeypatch, "group_sum", n, defines=gw.GRID1, grid=1, batches=10)
    lay = gw.steady(n)
    gw.check_steady(lay, g)
    run("group_sum", lay, 8000, name="steady, one workgroup")


# --------------------------------------------------------- 2. lead decisions
@pytest.mark.parametrize("family", ["group_sum", "sum2"])
def test_lead_decisions(family, monkeypatch):
    n = 9 * 4096 + gw.LEAD_TAIL_ROWS
    g = regime(monkeypatch, family, n, batches=4)
    assert g.lead == gw.LEAD
    lay = gw.lead(g)      # asserts each wave's case from the live geometry (gw.check_lead)
    assert lay.n == n
    groups = run(family, lay, 4096, where=True, name="lead")
    assert groups == len(np.unique(lay.keys))
    # without the WHERE the dropped first lane joins its 63 sharers
    run(family, lay, 4096, where=False, name="lead, no WHERE")


# ------------------------------------------------------- 3. window placement
@pytest.mark.parametrize("family", ["group_sum", "mix3", "join_hash"])
def test_window_placement(family, monkeypatch):
    n = 9 * 4096 + 5
    regime(monkeypatch, family, n, batches=4)
    for lo in gw.PLACEMENT_LOS:
        lay = gw.placement(n, lo)
        tables, vals, hit = upload(family, lay)
        refs = references(family, lay, vals, hit)
        for _ in range(2):
            g, keys, *rest = call(family, tables, lo, 4096)
            assert g == len(refs[0][0])
            compare(family, (keys, *rest), refs, g)
            k = keys[:g].astype(np.int64)
            assert (np.diff(k) > 0).all()          # ascending across below, window and above
            gen = lay.general_keys()
            nb, na = int((k < lo).sum()), int((k >= lo + gw.WINDOW).sum())
            assert (nb, na) == (int((gen < lo).sum()), int((gen >= lo + gw.WINDOW).sum())) and nb + na == len(gen)
            assert (nb > 0 or lo == gw.I32_MIN) and (na > 0 or lo + gw.WINDOW > gw.I32_MAX)
    # a window that would pass the largest key is refused before anything runs
    lay = gw.placement(n, gw.PLACEMENT_LOS[2])
    tables, _, _ = upload(family, lay)
    with pytest.raises(wx.WarpExecError) as e:
        call(family, tables, gw.I32_MAX - 2046, 4096)
    assert e.value.status == wx.WX_ERR_INVALID
    run(family, lay, 4096, name="after the refusal")


# ----------------------------------------------------- 4. finalize boundaries
@pytest.mark.parametrize("family", ["group_agg", "mix3"])
def test_finalize_boundaries(family, monkeypatch):
    seen = 0
    for nh in gw.FIN_NH:
        for side in gw.FIN_SIDES:
            for nwin in gw.FIN_NWIN:
                lay = gw.finalize(nh, side, nwin)
                regime(monkeypatch, family, lay.n)
                total = nh + nwin
                # capacity == total: every group written, the sentinel behind the last one untouched
                assert run(family, lay, total, name=f"finalize {nh} {side} {nwin}") == total
                seen += 1
    assert seen == 54


@pytest.mark.parametrize("family", ["group_agg", "mix3"])
def test_capacity_one_short(family, monkeypatch):
    # the overflowing (largest) group in the window, then in the table
    for name, lay in (("window", gw.finalize(2, "below", gw.WINDOW)), ("table", gw.finalize(gw.HSORT_MAX - 1, "above", 1))):
        regime(monkeypatch, family, lay.n)
        tables, vals, hit = upload(family, lay)
        refs = references(family, lay, vals, hit)
        total = len(refs[0][0])
        last = int(refs[0][0][-1])
        assert (name == "window") == (lay.key_lo <= last < lay.key_lo + gw.WINDOW)
        for _ in range(2):
            with pytest.raises(wx.WarpExecError) as e:
                call(family, tables, lay.key_lo, total - 1)
            assert e.value.status == wx.WX_ERR_CAPACITY and e.value.count == total
            compare(family, e.value.outputs, refs, total - 1)     # nothing at or past the capacity
            g, *outs = call(family, tables, lay.key_lo, total)     # and the next call is correct
            assert g == total
            compare(family, outs, refs, total)


# ------------------------------------------------- 5. the general-key table
def fresh_stream():
    """A torch stream no GROUP BY has run on (the runtime keeps one workspace per stream, torch a pool of streams)."""
    for _ in range(40):
        s = torch.cuda.Stream()
        if wx.group_table_slots(wx.make_launch(device=0, stream=s.cuda_stream)) == 0:
            return s
    raise AssertionError("no unused stream")


def next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


@pytest.mark.parametrize("family", ["group_sum", "sum2"])
def test_table_clusters(family, monkeypatch):
    n = 9 * 4096 + 5
    g = regime(monkeypatch, family, n, batches=4)
    run(family, gw.steady(n), 8000, name="warm-up")
    slots = wx.group_table_slots(launch())       # this stream's table as earlier tests left it: it only grows
    assert slots >= 16384 and slots & (slots - 1) == 0
    for k in (0, -1, 12345, gw.I32_MIN, gw.I32_MAX):
        assert wx.group_hash_slot(k, slots) == int(gw.hash_slot([k], slots)[0])
    for home in (slots // 2 + 11, slots - 1):      # the middle of the table; the last slot: probing wraps
        lay = gw.cluster(g, n, slots, home)
        assert all(wx.group_hash_slot(int(k), slots) == home for k in lay.general_keys() if k not in (0, -1))
        assert run(family, lay, 4096, name=f"cluster at {home} of {slots}") == gw.CLUSTER + 2
        assert wx.group_table_slots(launch()) == slots


@pytest.mark.parametrize("family", ["group_sum", "sum2"])
def test_table_size_and_overflow_on_a_fresh_stream(family, monkeypatch):
    regime(monkeypatch, family, 20_000)
    full, ordinary = gw.overfull(), gw.steady(9 * 4096 + 5)
    t_full, _, _ = upload(family, full)
    torch.cuda.synchronize()
    with torch.cuda.stream(fresh_stream()):
        assert wx.group_table_slots(launch()) == 0           # a workspace of its own: no GROUP BY yet
        # capacity 16: 4096 slots for 5000 distinct keys outside the window
        for _ in range(2):
            with pytest.raises(wx.WarpExecError) as e:
                call(family, t_full, full.key_lo, 16)
            assert e.value.status == wx.WX_ERR_CAPACITY and e.value.count == 4096    # every slot taken
            assert wx.group_table_slots(launch()) == 4096 == next_pow2(max(4096, 2 * 16))
            keys = e.value.outputs[0]
            assert (keys[16:] == SENT).all() and (np.diff(keys[:16].astype(np.int64)) > 0).all()
            assert np.isin(keys[:16], full.general_keys()).all()
        # the table was returned empty: an ordinary call on the same stream
        run(family, ordinary, 8000, name="after the overflow")
        assert wx.group_table_slots(launch()) == next_pow2(max(4096, 2 * 8000)) == 16384
        run(family, gw.finalize(2, "split", 1), 3, name="a small capacity keeps the larger table")
        assert wx.group_table_slots(launch()) == 16384
        torch.cuda.current_stream().synchronize()
