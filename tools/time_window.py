#!/usr/bin/env python3
"""Time the window aggregates (wx_window_select) on the headline's shape:
`price` f32 U[0, 40), `quantity` int32 U{0..999}, WHERE price > 15 (62.5 %
pass), for (plain, window) output counts (1, 1), (2, 2) and (0, 4), with
int32 row ids.

Per shape, in one process on one device, call by call in turn:
  window     the whole wx_window_select call, host clock around the call and a
             device synchronisation (grouped pass, the two host reads, the
             table launch, the broadcast compaction), and
  broadcast  its broadcast compaction alone by HIP events (WX_F_TIME);
the yardsticks the feature is held against:
  group      wx_group_agg_multi over the same distinct values with the same
             aggregates, whole call as above, and
  select     wx_project_filter_multi with the same number of outputs over the
             same columns, the key column standing in for each window item
             (so the call reads price and the key, as the broadcast does):
             whole call, and its kernel by HIP events.
`ratio` is window / (group + select), whole calls; `bcast/select` compares
the two compaction kernels, which move the same bytes (8 B/row read, 4 B per
output and per row id written for each passing row).  The search form is
timed on the same table (forced, WARPDB_WINDOW_FORM=search) and over a second
key column of 100 000 distinct keys.  Every figure is the median of `reps`
calls after `warm` warm-up calls (past the clock ramp).

usage: python tools/time_window.py [rows] [reps] [warm] [out-file]
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
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 15
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 10
out_path = sys.argv[4] if len(sys.argv) > 4 else None
assert reps >= 10, "the median of at least 10 calls"

COND = "(price[idx] > 15.0f)"
P, PQ = "price[idx]", "(price[idx] * quantity[idx])"
SHAPES = {  # (plain, window): plain expressions, window items, the select call's stand-ins
    (1, 1): ([P], [(P, wx.WIN_SUM)]),
    (2, 2): ([P, PQ], [(P, wx.WIN_SUM), (PQ, wx.WIN_MAX)]),
    (0, 4): ([], [(P, wx.WIN_SUM), (P, wx.WIN_AVG), (P, wx.WIN_MIN), (P, wx.WIN_MAX)]),
}

stream = torch.cuda.current_stream().cuda_stream
L = wx.make_launch(stream=stream, flags=wx.F_NO_CUSTOM)
Lt = wx.make_launch(stream=stream, flags=wx.F_NO_CUSTOM | wx.F_TIME)
lines = []


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


emit(f"# tools/time_window.py: {n:.0e} rows, price f32 U[0,40), WHERE price > 15, int32 row ids; whole calls by the "
     f"host clock, kernels by HIP events, median of {reps} after {warm}")
emit(f"# {torch.cuda.get_device_name(0)}")
price = torch.empty(n, dtype=torch.float32, device="cuda")
wx.fill_synthetic(price.data_ptr(), wx.FLOAT32, n, 1, 0, 0.0, 40.0, L)
keys = {}
for name, hi in (("quantity", 999), ("wide", 99_999)):
    keys[name] = torch.empty(n, dtype=torch.int32, device="cuda")
    wx.fill_synthetic(keys[name].data_ptr(), wx.INT32, n, 9, 1, 0, hi, L)
outs = [torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(4)]
ids = torch.empty(n, dtype=torch.int32, device="cuda")
CAP = 1 << 17
gk = torch.empty(CAP, dtype=torch.int32, device="cuda")
gc = torch.empty(CAP, dtype=torch.int64, device="cuda")
gs = [torch.empty(CAP, dtype=torch.float64, device="cuda") for _ in range(2)]
gn = [torch.empty(CAP, dtype=torch.float32, device="cuda") for _ in range(2)]
gx = [torch.empty(CAP, dtype=torch.float32, device="cuda") for _ in range(2)]
ng = torch.zeros(1, dtype=torch.int64, device="cuda")


def measure(table, key_col, plain, items, form):
    """Medians (ms): window whole, broadcast kernels, group whole, select whole, select kernel; count, groups."""
    part = f"{key_col}[idx]"
    # items name `quantity` as a value: on the wide-key table that column is the value all the same
    m = len(plain) + len(items)
    vals, sm, qm = [], [], []
    for e, a in items:
        if e not in vals:
            vals.append(e)
            sm.append(False)
            qm.append(False)
        j = vals.index(e)
        if a in (wx.WIN_MIN, wx.WIN_MAX):
            qm[j] = True
        else:
            sm[j] = True
    stand_in = plain + [part] * len(items)
    ptrs = [o.data_ptr() for o in outs[:m]]
    if form == "search":
        os.environ["WARPDB_WINDOW_FORM"] = "search"
    else:
        os.environ.pop("WARPDB_WINDOW_FORM", None)

    def window(launch):
        return wx.window_select(table, plain, items, part, COND, launch, ptrs, group_capacity=CAP,
                                d_out_idx=ids.data_ptr(), idx_bytes=4, d_count=ng.data_ptr())

    def group(launch):
        wx.group_agg_multi(table, vals, part, COND, launch, 0, CAP, gk.data_ptr(), gc.data_ptr(),
                           [t.data_ptr() if s else 0 for t, s in zip(gs, sm)],
                           [t.data_ptr() if q else 0 for t, q in zip(gn, qm)],
                           [t.data_ptr() if q else 0 for t, q in zip(gx, qm)], ng.data_ptr(), want_count=False)

    def select(launch):
        wx.project_filter_multi(table, stand_in, COND, launch, ptrs, ids.data_ptr(), 4, 0, ng.data_ptr())

    for _ in range(warm):
        window(L)
        group(L)
        select(L)
    wx.check(L)
    wx.timing_read()
    tw, tb, tg, ts, tk = [], [], [], [], []
    for _ in range(reps):
        tw.append(wall(lambda: window(L)))
        window(Lt)
        tb.append(wx.timing_read()[0])
        tg.append(wall(lambda: group(L)))
        ts.append(wall(lambda: select(L)))
        select(Lt)
        tk.append(wx.timing_read()[0])
    wx.check(L)
    select(L)
    count = int(ng.item())
    group(L)
    groups = int(ng.item())
    os.environ.pop("WARPDB_WINDOW_FORM", None)
    return med(tw), med(tb), med(tg), med(ts), med(tk), count, groups


for key_col, forms in (("quantity", ("dense", "search")), ("wide", ("search",))):
    table = wx.Table.from_tensors(price=price, quantity=keys["quantity"], **({"wide": keys["wide"]} if key_col == "wide" else {}))
    for (a, b), (plain, items) in SHAPES.items():
        if key_col == "wide" and (a, b) != (1, 1):
            continue
        for form in forms:
            w_ms, b_ms, g_ms, s_ms, k_ms, count, groups = measure(table, key_col, plain, items, form)
            m = a + b
            bytes_row = 8 + (count / n) * 4 * (m + 1)
            emit(f"keys {groups:6d}  ({a}, {b})  {form:6s}  window {w_ms:8.3f} ms  broadcast {b_ms:8.3f} ms  | "
                 f"group {g_ms:8.3f} ms  select {s_ms:8.3f} ms (kernel {k_ms:8.3f} ms)  | "
                 f"ratio {w_ms / (g_ms + s_ms):.3f}  bcast/select {b_ms / k_ms:.3f}  "
                 f"broadcast {bytes_row * n / (b_ms * 1e-3) / 1e12:.2f} TB/s of its {bytes_row:.1f} B/row  "
                 f"passing {count / n:.3f}")
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
