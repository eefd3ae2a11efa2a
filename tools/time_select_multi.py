#!/usr/bin/env python3
"""Time one fused M-output compaction (wx_project_filter_multi) against the M
single-output wx_project_filter calls it replaces, on the headline query and
data (price f32 U[0,40), quantity f32 U{1..100}, WHERE price > 15, int32 row
ids), by HIP events around the kernels (WX_F_TIME).

In the separate runs only the first call writes the row ids.  Every figure is
the median of `reps` calls after `warm` warm-up calls; the two variants
alternate call by call, so clock and thermal drift hit both alike.  The byte
model (bytes per row): separate 8 M + 0.625 (4 M + 4), fused
8 + 0.625 (4 M + 4).

usage: python tools/time_select_multi.py [rows,rows,...] [reps] [warm] [out-file]
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from warpdb_amd import _warpexec as wx  # noqa: E402

rows_list = [int(float(x)) for x in (sys.argv[1] if len(sys.argv) > 1 else "1e8,1e9").split(",")]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 15
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 3
out_path = sys.argv[4] if len(sys.argv) > 4 else None
assert reps >= 10, "the median of at least 10 calls"

EXPRS = ["(price[idx] * quantity[idx])", "price[idx]", "quantity[idx]", "(price[idx] + quantity[idx])"]
COND = "(price[idx] > 15.0f)"
HBM_TBS = 8.0  # MI355X peak

stream = torch.cuda.current_stream().cuda_stream
L = wx.make_launch(stream=stream, flags=wx.F_NO_CUSTOM)
Lt = wx.make_launch(stream=stream, flags=wx.F_NO_CUSTOM | wx.F_TIME)
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


emit(f"# tools/time_select_multi.py: headline query, {COND}, int32 row ids, HIP events, median of {reps} after {warm}")
emit(f"# {torch.cuda.get_device_name(0)}; tile rows per M: " +
     ", ".join(f"{m}: {wx.select_tile_rows(m)}" for m in (1, 2, 3, 4)))
for n in rows_list:
    price = torch.empty(n, dtype=torch.float32, device="cuda")
    qty = torch.empty(n, dtype=torch.float32, device="cuda")
    wx.fill_synthetic(price.data_ptr(), wx.FLOAT32, n, 1, 0, 0.0, 40.0, L)
    wx.fill_synthetic(qty.data_ptr(), wx.FLOAT32, n, 2, 1, 1, 100, L)
    table = wx.Table.from_tensors(price=price, quantity=qty)
    outs = [torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(4)]
    seps = [torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(4)]
    ids_f = torch.empty(n, dtype=torch.int32, device="cuda")
    ids_s = torch.empty(n, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    for m in (2, 3, 4):
        def fused(launch):
            wx.project_filter_multi(table, EXPRS[:m], COND, launch, [o.data_ptr() for o in outs[:m]],
                                    ids_f.data_ptr(), 4, 0, cnt.data_ptr())

        def separate(launch):
            for j in range(m):
                wx.project_filter(table, EXPRS[j], COND, launch, wx.MODE_COMPACT, seps[j].data_ptr(),
                                  ids_s.data_ptr() if j == 0 else 0, 4, 0, cnt.data_ptr())

        for _ in range(warm):
            fused(L)
            separate(L)
        wx.check(L)
        wx.timing_read()
        tf, ts = [], []
        for _ in range(reps):
            fused(Lt)
            tf.append(wx.timing_read()[0])
            separate(Lt)
            ms, launches = wx.timing_read()
            assert launches == m
            ts.append(ms)
        wx.check(L)
        passing = int(cnt.item())
        same = torch.equal(ids_f[:passing], ids_s[:passing]) and all(
            torch.equal(outs[j][:passing].view(torch.int32), seps[j][:passing].view(torch.int32)) for j in range(m))
        f_ms, s_ms = statistics.median(tf), statistics.median(ts)
        frac = passing / n
        model_f = 8 + frac * (4 * m + 4)
        model_s = 8 * m + frac * (4 * m + 4)
        emit(f"rows {n:.0e}  M={m}  fused {f_ms:8.4f} ms  separate {s_ms:8.4f} ms  ratio {f_ms / s_ms:.3f} "
             f"(byte model {model_f / model_s:.3f})  fused {model_f * n / (f_ms * 1e-3) / 1e12:.2f} TB/s of its "
             f"{model_f:.2f} B/row = {model_f * n / (f_ms * 1e-3) / 1e12 / HBM_TBS:.3f} of {HBM_TBS:.0f} TB/s  "
             f"passing {frac:.4f}  identical={same}")
    del price, qty, table, outs, seps, ids_f, ids_s
    torch.cuda.empty_cache()
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
