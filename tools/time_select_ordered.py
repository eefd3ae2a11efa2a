#!/usr/bin/env python3
"""Time the ordered multi-column SELECT (wx_select_ordered) against what the
single-column entry points offer for the same result, and the row gather
(wx_gather_multi) alone, on the headline data (price f32 U[0,40), quantity f32
U{1..100}) with WHERE price > 15 ORDER BY price DESC.

ordered: LIMIT 10, LIMIT 1000 and no LIMIT, M = 1..4.  "fused" is one
  wx_select_ordered call (keys + int64 rows + M value columns); "separate" is
  M wx_topk calls with select_expr (LIMIT <= 32) or M wx_order_head calls
  (otherwise).  HIP events around the whole calls (several kernels and, on the
  sort route, host reads of the count), the two variants alternating call by
  call, median of `reps` after `warm`.
gather: wx_gather_multi alone (HIP events around the kernel, WX_F_TIME) at
  1e3 / 1e6 / 1e8 / 6.25e8 uniformly random int32 ids over the table, M = 1..4,
  for every geometry in GEOMETRIES: ids per second, and the line model -- each
  gathered element of each referenced column fetches at least one 64-byte
  line for 4 useful bytes (fetched / useful >= 16 when no line is reused).

usage: python tools/time_select_ordered.py ordered|gather [rows,rows,...] [reps] [warm] [out-file]
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from warpdb_amd import _warpexec as wx  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "ordered"
rows_list = [int(float(x)) for x in (sys.argv[2] if len(sys.argv) > 2 else "1e8,1e9").split(",")]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 15
warm = int(sys.argv[4]) if len(sys.argv) > 4 else 3
out_path = sys.argv[5] if len(sys.argv) > 5 else None
assert mode in ("ordered", "gather") and reps >= 10, "ordered|gather, the median of at least 10 calls"

EXPRS = ["price[idx]", "quantity[idx]", "(price[idx] * quantity[idx])", "(price[idx] + quantity[idx])"]
COND, ORDER = "(price[idx] > 15.0f)", "price[idx]"
GEOMETRIES = [(256, 1), (256, 2), (256, 4), (512, 2), (1024, 1), (64, 2)]  # (WX_GATHER_BLOCK, WX_GATHER_UNROLL)
ID_COUNTS = [1000, 10**6, 10**8, 625 * 10**6]

stream = torch.cuda.current_stream().cuda_stream
L = wx.make_launch(stream=stream, flags=wx.F_NO_CUSTOM)
Lt = wx.make_launch(stream=stream, flags=wx.F_NO_CUSTOM | wx.F_TIME)
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)
    if out_path:  # kept current: a long run leaves what it measured
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def make_table(n):
    price = torch.empty(n, dtype=torch.float32, device="cuda")
    qty = torch.empty(n, dtype=torch.float32, device="cuda")
    wx.fill_synthetic(price.data_ptr(), wx.FLOAT32, n, 1, 0, 0.0, 40.0, L)
    wx.fill_synthetic(qty.data_ptr(), wx.FLOAT32, n, 2, 1, 1, 100, L)
    return wx.Table.from_tensors(price=price, quantity=qty)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def run_ordered(n):
    table = make_table(n)
    passing = wx.project_filter(table, ORDER, COND, L, wx.MODE_COMPACT, 0, 0, 8, 0, want_count=True)
    for limit in (10, 1000, -1):
        cap = passing if limit < 0 else limit
        outs = [torch.empty(cap, dtype=torch.float32, device="cuda") for _ in range(4)]
        keys = torch.empty(cap, dtype=torch.float32, device="cuda")
        rows = torch.empty(cap, dtype=torch.int64, device="cuda")
        # the separate calls' outputs: top-K arrays, or one head record
        sk = torch.empty(32, dtype=torch.float32, device="cuda")
        si = torch.empty(32, dtype=torch.int64, device="cuda")
        sv = torch.empty(32, dtype=torch.float32, device="cuda")
        rec = torch.empty(8 + 16 * cap, dtype=torch.uint8, device="cuda") if limit < 0 or limit > 32 else None
        for m in (1, 2, 3, 4):
            def fused():
                return wx.select_ordered(table, EXPRS[:m], COND, ORDER, True, limit, L,
                                         [o.data_ptr() for o in outs[:m]], keys.data_ptr(), rows.data_ptr(), cap)

            def separate():
                for j in range(m):
                    if rec is None:
                        wx.topk(table, ORDER, COND, EXPRS[j], limit, True, L, sk.data_ptr(), si.data_ptr(),
                                sv.data_ptr())
                    else:
                        wx.order_head(table, ORDER, COND, EXPRS[j], cap, True, L, rec.data_ptr(), cap)

            for _ in range(warm):
                fused()
                separate()
            tf, ts = [], []
            for _ in range(reps):
                tf.append(event_ms(fused))
                ts.append(event_ms(separate))
            count = fused()
            # the last separate call's values against the fused column m - 1
            if rec is None:
                same = torch.equal(sv[:count].view(torch.int32), outs[m - 1][:count].view(torch.int32)) and \
                    torch.equal(si[:count], rows[:count])
            else:
                vals = rec[8 + 4 * cap:8 + 8 * cap].view(torch.float32)
                rr = rec[8 + 8 * cap:].view(torch.int64)
                same = torch.equal(vals[:count].view(torch.int32), outs[m - 1][:count].view(torch.int32)) and \
                    torch.equal(rr[:count], rows[:count])
            f_ms, s_ms = statistics.median(tf), statistics.median(ts)
            emit(f"rows {n:.0e}  LIMIT {'none' if limit < 0 else limit:>5}  M={m}  fused {f_ms:9.3f} ms  separate "
                 f"{s_ms:9.3f} ms  ratio {f_ms / s_ms:.3f}  rows out {count}  identical={same}")
        del outs, keys, rows, rec
        torch.cuda.empty_cache()


def run_gather(n):
    table = make_table(n)
    ids = torch.randint(0, n, (max(ID_COUNTS),), dtype=torch.int32, device="cuda")
    outs = [torch.empty(max(ID_COUNTS), dtype=torch.float32, device="cuda") for _ in range(4)]
    n_cols = {1: 1, 2: 2, 3: 2, 4: 2}  # columns the first m expressions reference
    for block, unroll in GEOMETRIES:
        os.environ["WARPDB_EXTRA_DEFINES"] = f"WX_GATHER_BLOCK={block},WX_GATHER_UNROLL={unroll}"
        for count in ID_COUNTS:
            for m in (1, 2, 3, 4):
                def call(launch):
                    wx.gather_multi(table, EXPRS[:m], ids.data_ptr(), 4, count, launch,
                                    [o.data_ptr() for o in outs[:m]])

                for _ in range(warm):
                    call(L)
                wx.check(L)
                wx.timing_read()
                t = []
                for _ in range(reps):
                    call(Lt)
                    t.append(wx.timing_read()[0])
                ms = statistics.median(t)
                line_gb = count * n_cols[m] * 64 / 1e9
                emit(f"table {n:.0e}  block {block:4d} unroll {unroll}  ids {count:.2e}  M={m}  {ms:9.4f} ms  "
                     f"{count / (ms * 1e-3):.3e} ids/s  >= {line_gb / (ms * 1e-3) / 1e3:.3f} TB/s of 64-byte lines "
                     f"for {count * (4 * n_cols[m] + 4 + 4 * m) / (ms * 1e-3) / 1e12:.3f} TB/s of useful bytes")
    os.environ.pop("WARPDB_EXTRA_DEFINES", None)


emit(f"# tools/time_select_ordered.py {mode}: WHERE {COND} ORDER BY {ORDER} DESC, median of {reps} after {warm}")
emit(f"# {torch.cuda.get_device_name(0)}; default gather tile per M: " +
     ", ".join(f"{m}: {wx.gather_tile_rows(m)}" for m in (1, 2, 3, 4)))
for n in rows_list:
    (run_ordered if mode == "ordered" else run_gather)(n)
