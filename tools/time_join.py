#!/usr/bin/env python3
"""Time the PK-FK equi-join (wx_join_select) on the headline's shape: `price`
f32 U[0, 40), WHERE price > 15 (62.5 % pass), a left key uniform over the
right table's keys (every row matches), int32 row ids, against right tables
of 1e3 (direct form, and the hash form forced), 1e5, 1e6 and 1e7 rows (hash
form), for 1, 2 and 4 outputs, half of them right columns (the single output
is a right column), INNER and LEFT.

Per case, in one process on one device, call by call in turn:
  join    the whole wx_join_select call, host clock around the call and a
          device synchronisation (key range, the two host reads, the build,
          the probing compaction),
  probe   its probing compaction alone by HIP events (WX_F_TIME),
  build   the whole call over an empty left table: everything but the probe;
the floor the feature is held against:
  select  wx_project_filter_multi with the same number of outputs over the
          left table alone (the key column standing in for each right
          column, so the call reads price and the key, as the probe does):
          whole call, and its kernel by HIP events.
`probe/select` compares the two compaction kernels, which move the same
left-side bytes.  (The select call is timed here, in the same process; the
multi-output body it shares with the probe is this commit's.  README's select
row holds the figures of the commit before: 2.23 / 2.73 / 4.14 ms for 1 / 2 /
4 outputs.)

The last case is the one fixed condition: the hash probe at 1e5 right keys
with one right-column output against the window family's search form over
1e5 partition keys with one plain and one window output (the lookup a wide
key range had before), both by HIP events, in this process; the tool prints
the two and exits non-zero if the probe is not the faster.  Every figure is
the median of `reps` calls after `warm` warm-up calls (past the clock ramp).

usage: python tools/time_join.py [rows] [reps] [warm] [out-file]
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from warpdb_amd import _warpexec as wx  # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10 ** 9
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 11
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 5
out_path = sys.argv[4] if len(sys.argv) > 4 else None
assert reps >= 10, "the median of at least 10 calls"

COND = "(price[idx] > 15.0f)"
OUTPUTS = {  # outputs: (the join's expressions, the select call's stand-ins)
    1: (["rate[idx]"], ["fk[idx]"]),
    2: (["price[idx]", "rate[idx]"], ["price[idx]", "fk[idx]"]),
    4: (["price[idx]", "(price[idx] * 2.0f)", "rate[idx]", "bonus[idx]"],
        ["price[idx]", "(price[idx] * 2.0f)", "fk[idx]", "(fk[idx] + 1)"]),
}
RIGHTS = [(10 ** 3, False), (10 ** 3, True), (10 ** 5, False), (10 ** 6, False), (10 ** 7, False)]  # (rows, force hash)

stream = torch.cuda.current_stream().cuda_stream
L = wx.make_launch(stream=stream, flags=wx.F_NO_CUSTOM)
Lt = wx.make_launch(stream=stream, flags=wx.F_NO_CUSTOM | wx.F_TIME)
lines = []
probe_ms = {}  # (right rows, outputs, join type) -> median probe time, the planned form


def emit(s):
    print(s, flush=True)
    lines.append(s)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def med(xs):
    return statistics.median(xs)


emit(f"# tools/time_join.py: {n:.0e} left rows, price f32 U[0,40), WHERE price > 15, every row matches, int32 row "
     f"ids; whole calls by the host clock, kernels by HIP events, median of {reps} after {warm}")
emit(f"# {torch.cuda.get_device_name(0)}")
price = torch.empty(n, dtype=torch.float32, device="cuda")
wx.fill_synthetic(price.data_ptr(), wx.FLOAT32, n, 1, 0, 0.0, 40.0, L)
fk = torch.empty(n, dtype=torch.int32, device="cuda")
outs = [torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(4)]
ids = torch.empty(n, dtype=torch.int32, device="cuda")
cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
left = wx.Table.from_tensors(price=price, fk=fk)
empty = wx.Table(0, [wx.Column("price", wx.FLOAT32, 0), wx.Column("fk", wx.INT32, 0)])

for n_right, force_hash in RIGHTS:
    # the right table: keys 0 .. n_right - 1 in random row order, two f32 value columns
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    rkey = torch.randperm(n_right, device="cuda", generator=gen).to(torch.int32)
    rate = torch.rand(n_right, device="cuda", generator=gen)
    bonus = torch.rand(n_right, device="cuda", generator=gen)
    right = wx.Table.from_tensors(id=rkey, rate=rate, bonus=bonus)
    wx.fill_synthetic(fk.data_ptr(), wx.INT32, n, 9, 1, 0, n_right - 1, L)
    if force_hash:
        os.environ["WARPDB_JOIN_FORM"] = "hash"
    else:
        os.environ.pop("WARPDB_JOIN_FORM", None)
    form, log2cap = wx.join_plan(n_right, 0, n_right - 1)
    for m, (exprs, stand_in) in OUTPUTS.items():
        ptrs = [o.data_ptr() for o in outs[:m]]

        def select(launch):
            wx.project_filter_multi(left, stand_in, COND, launch, ptrs, ids.data_ptr(), 4, 0, cnt.data_ptr())

        for _ in range(warm):
            select(L)
        wx.check(L)
        wx.timing_read()
        ts, tk = [], []
        for _ in range(reps):
            ts.append(wall(lambda: select(L)))
            select(Lt)
            tk.append(wx.timing_read()[0])
        for jt, jname in ((wx.JOIN_INNER, "inner"), (wx.JOIN_LEFT, "left")):
            def join(launch, table=left):
                wx.join_select(table, right, "fk[idx]", "id", exprs, COND, launch, ptrs, join_type=jt,
                               d_out_idx=ids.data_ptr(), idx_bytes=4, d_count=cnt.data_ptr())

            for _ in range(warm):
                join(L)
            wx.check(L)
            wx.timing_read()
            tj, tp, tb = [], [], []
            for _ in range(reps):
                tj.append(wall(lambda: join(L)))
                join(Lt)
                tp.append(wx.timing_read()[0])
                tb.append(wall(lambda: join(L, empty)))
            wx.check(L)
            join(L)
            count = int(cnt.item())
            if not force_hash:
                probe_ms[(n_right, m, jname)] = med(tp)
            emit(f"right {n_right:9d}  {'direct' if form == wx.JOIN_DIRECT else f'hash 2^{log2cap}':9s}  outputs {m}  "
                 f"{jname:5s}  join {med(tj):8.3f} ms  probe {med(tp):8.3f} ms  build {med(tb):7.3f} ms  | "
                 f"select {med(ts):8.3f} ms (kernel {med(tk):8.3f} ms)  | probe/select {med(tp) / med(tk):.3f}  "
                 f"passing {count / n:.3f}")
    del right, rkey, rate, bonus
os.environ.pop("WARPDB_JOIN_FORM", None)
probe_1e5 = probe_ms[(10 ** 5, 1, "inner")]
# the window family's search form at 1e5 keys, (plain, window) = (1, 1), as tools/time_window.py times it
wide = torch.empty(n, dtype=torch.int32, device="cuda")
wx.fill_synthetic(wide.data_ptr(), wx.INT32, n, 9, 1, 0, 99_999, L)
wtable = wx.Table.from_tensors(price=price, wide=wide)
wptrs = [o.data_ptr() for o in outs[:2]]


def window(launch):
    wx.window_select(wtable, ["price[idx]"], [("price[idx]", wx.WIN_SUM)], "wide[idx]", COND, launch, wptrs,
                     group_capacity=1 << 17, d_out_idx=ids.data_ptr(), idx_bytes=4, d_count=cnt.data_ptr())


for _ in range(warm):
    window(L)
wx.check(L)
wx.timing_read()
tw = []
for _ in range(reps):
    window(Lt)
    tw.append(wx.timing_read()[0])
search_ms = med(tw)
ok = probe_1e5 < search_ms
emit(f"condition: hash probe at 1e5 right keys, 1 right-column output {probe_1e5:.3f} ms  <  window search form at "
     f"1e5 keys {search_ms:.3f} ms: {'holds' if ok else 'FAILS'} ({search_ms / probe_1e5:.2f} x)")
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
sys.exit(0 if ok else 1)
