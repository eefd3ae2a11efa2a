#!/usr/bin/env python3
"""Time one fused M-value GROUP BY (wx_group_agg_multi) against the M
single-value calls it replaces, on C3's shape: int32 keys U{0..999} and value
expressions over M distinct f32 columns, no WHERE, by HIP events around the
stage-1 kernels (WX_F_TIME; the one-workgroup finalize of either variant is
not in the figure).

Per M three builds of the fused kernel: `sum` (every value summed) against M
wx_group_sum calls, `minmax` (every value with MIN / MAX only) and `both`
(every value with SUM, MIN and MAX) against M wx_group_agg calls with MIN /
MAX.  Every figure is the median of `reps` calls after `warm` warm-up calls
(past the clock ramp); the two variants alternate call by call in one
process, so clock and thermal drift hit both alike.  The byte model (bytes
per row): separate 8 M, fused 4 + 4 M.

usage: python tools/time_group_multi.py [rows,rows,...] [reps] [warm] [out-file]
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from warpdb_amd import _warpexec as wx  # noqa: E402

rows_list = [int(float(x)) for x in (sys.argv[1] if len(sys.argv) > 1 else "1e9").split(",")]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 15
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 20
out_path = sys.argv[4] if len(sys.argv) > 4 else None
assert reps >= 10, "the median of at least 10 calls"

VALS = ["v0[idx]", "v1[idx]", "v2[idx]", "v3[idx]"]
KEY = "k[idx]"
CAP = 2048
HBM_TBS = 8.0  # MI355X peak

stream = torch.cuda.current_stream().cuda_stream
L = wx.make_launch(stream=stream, flags=wx.F_NO_CUSTOM)
Lt = wx.make_launch(stream=stream, flags=wx.F_NO_CUSTOM | wx.F_TIME)
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


emit(f"# tools/time_group_multi.py: GROUP BY k (1000 int32 keys), M distinct f32 value columns, HIP events around "
     f"the stage-1 kernels, median of {reps} after {warm}")
emit(f"# {torch.cuda.get_device_name(0)}")
for n in rows_list:
    k = torch.empty(n, dtype=torch.int32, device="cuda")
    wx.fill_synthetic(k.data_ptr(), wx.INT32, n, 9, 1, 0, 999, L)
    vs = [torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(4)]
    for j, v in enumerate(vs):
        wx.fill_synthetic(v.data_ptr(), wx.FLOAT32, n, 1 + j, 0, 0.0, 40.0, L)
    table = wx.Table.from_tensors(k=k, v0=vs[0], v1=vs[1], v2=vs[2], v3=vs[3])
    dk = torch.empty(CAP, dtype=torch.int32, device="cuda")
    dc = torch.empty(CAP, dtype=torch.int64, device="cuda")
    ds = [torch.empty(CAP, dtype=torch.float64, device="cuda") for _ in range(4)]
    dn = [torch.empty(CAP, dtype=torch.float32, device="cuda") for _ in range(4)]
    dx = [torch.empty(CAP, dtype=torch.float32, device="cuda") for _ in range(4)]
    sk = torch.empty(CAP, dtype=torch.int32, device="cuda")
    sc = torch.empty(CAP, dtype=torch.int64, device="cuda")
    ss = [torch.empty(CAP, dtype=torch.float64, device="cuda") for _ in range(4)]
    sn = [torch.empty(CAP, dtype=torch.float32, device="cuda") for _ in range(4)]
    sx = [torch.empty(CAP, dtype=torch.float32, device="cuda") for _ in range(4)]
    ng = torch.zeros(1, dtype=torch.int64, device="cuda")
    for m in (2, 3, 4):
        for build in ("sum", "minmax", "both"):
            sums = build != "minmax"
            mm = build != "sum"

            def fused(launch):
                wx.group_agg_multi(table, VALS[:m], KEY, None, launch, 0, CAP, dk.data_ptr(), dc.data_ptr(),
                                   [t.data_ptr() for t in ds[:m]] if sums else None,
                                   [t.data_ptr() for t in dn[:m]] if mm else None,
                                   [t.data_ptr() for t in dx[:m]] if mm else None, ng.data_ptr(), want_count=False)

            def separate(launch):
                for j in range(m):
                    if mm:
                        wx.group_agg(table, VALS[j], KEY, None, launch, 0, CAP, sk.data_ptr(), ss[j].data_ptr(),
                                     sc.data_ptr(), sn[j].data_ptr(), sx[j].data_ptr(), ng.data_ptr(),
                                     want_count=False)
                    else:
                        wx.group_sum(table, VALS[j], KEY, None, launch, 0, CAP, sk.data_ptr(), ss[j].data_ptr(),
                                     sc.data_ptr(), ng.data_ptr(), want_count=False)

            for _ in range(warm):
                fused(L)
                separate(L)
            wx.check(L)
            wx.timing_read()
            tf, ts = [], []
            for _ in range(reps):
                fused(Lt)
                ms, launches = wx.timing_read()
                assert launches == 1
                tf.append(ms)
                separate(Lt)
                ms, launches = wx.timing_read()
                assert launches == m
                ts.append(ms)
            wx.check(L)
            g = int(ng.item())
            same = torch.equal(dk[:g], sk[:g]) and torch.equal(dc[:g], sc[:g])
            for j in range(m):
                if sums:  # atomics in any order: compare at the project's tolerance
                    same = same and torch.allclose(ds[j][:g], ss[j][:g], rtol=1e-12, atol=0.0)
                if mm:
                    same = same and torch.equal(dn[j][:g], sn[j][:g]) and torch.equal(dx[j][:g], sx[j][:g])
            f_ms, s_ms = statistics.median(tf), statistics.median(ts)
            s_, q_ = (m if sums else 0), (m if mm else 0)
            model_f, model_s = 4 + 4 * m, 8 * m
            emit(f"rows {n:.0e}  M={m}  {build:6s} S={s_} Q={q_} block {512 if s_ + q_ <= 4 else 1024}  "
                 f"fused {f_ms:8.4f} ms  separate {s_ms:8.4f} ms  ratio {f_ms / s_ms:.3f} "
                 f"(byte model {model_f / model_s:.3f})  fused {model_f * n / (f_ms * 1e-3) / 1e12:.2f} TB/s of its "
                 f"{model_f} B/row = {model_f * n / (f_ms * 1e-3) / 1e12 / HBM_TBS:.3f} of {HBM_TBS:.0f} TB/s  "
                 f"groups {g}  same={same}")
    del k, vs, table
    torch.cuda.empty_cache()
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
