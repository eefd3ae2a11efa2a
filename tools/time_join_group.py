#!/usr/bin/env python3
"""Time the JOIN under GROUP BY (wx_join_group_agg) on the headline's shape:
`price` f32 U[0, 40), WHERE price > 15 (62.5 % pass), a left key uniform over
the right table's keys (every row matches), right tables of 1e3 (direct form),
1e5 and 1e6 rows (hash form), grouping by a right attribute of 7 and of 1000
values, SUM of one and of four values.

Per case, in one process on one device, call by call in turn:
  (a) fused   the whole wx_join_group_agg call by the host clock around the
              call and a device synchronisation (key range, the two host
              reads, the build, the grouped pass, the finalize), and its
              grouped pass alone by HIP events (WX_F_TIME);
  (b) today   the route without it: wx_join_select materialising the group
              attribute and the values (no row ids), wx_cast of the attribute
              back to int32, wx_group_agg_multi over the materialised columns;
              whole route by the host clock;
  (c) floor   wx_group_agg_multi over the left table alone with the same value
              count and no probe (the key is fk % groups, the foreign key
              standing in for each right column): whole call, and its kernel
              by HIP events.
The gate: (a) is faster than (b) in every case (it does strictly less work:
the same probes, no per-row stores, no second pass); the tool exits non-zero
otherwise.  (a) / (c) is reported only.  Every figure is the median of `reps`
calls after `warm` warm-up calls.

usage: python tools/time_join_group.py [rows] [reps] [warm] [out-file]
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
# values: (the join's expressions, the floor's stand-ins over the left table)
VALUES = {
    1: (["(price[idx] * rate[idx])"], ["(price[idx] * fk[idx])"]),
    4: (["(price[idx] * rate[idx])", "price[idx]", "rate[idx]", "(price[idx] + bonus[idx])"],
        ["(price[idx] * fk[idx])", "price[idx]", "fk[idx]", "(price[idx] + fk[idx])"]),
}
RIGHTS = [10 ** 3, 10 ** 5, 10 ** 6]
GROUPS = [7, 1000]
CAP = 4096

stream = torch.cuda.current_stream().cuda_stream
L = wx.make_launch(stream=stream, flags=wx.F_NO_CUSTOM)
Lt = wx.make_launch(stream=stream, flags=wx.F_NO_CUSTOM | wx.F_TIME)
lines = []
ok = True


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


emit(f"# tools/time_join_group.py: {n:.0e} left rows, price f32 U[0,40), WHERE price > 15, every row matches; whole "
     f"calls by the host clock, kernels by HIP events, median of {reps} after {warm}")
emit(f"# {torch.cuda.get_device_name(0)}")
price = torch.empty(n, dtype=torch.float32, device="cuda")
wx.fill_synthetic(price.data_ptr(), wx.FLOAT32, n, 1, 0, 0.0, 40.0, L)
fk = torch.empty(n, dtype=torch.int32, device="cuda")
mat = [torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(5)]  # the materialised attribute + values
mkey = torch.empty(n, dtype=torch.int32, device="cuda")
left = wx.Table.from_tensors(price=price, fk=fk)
d_keys = torch.empty(CAP, dtype=torch.int32, device="cuda")
d_cnts = torch.empty(CAP, dtype=torch.int64, device="cuda")
d_sums = [torch.empty(CAP, dtype=torch.float64, device="cuda") for _ in range(4)]
results = {}

for n_right in RIGHTS:
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    rkey = torch.randperm(n_right, device="cuda", generator=gen).to(torch.int32)
    rate = torch.rand(n_right, device="cuda", generator=gen)
    bonus = torch.rand(n_right, device="cuda", generator=gen)
    wx.fill_synthetic(fk.data_ptr(), wx.INT32, n, 9, 1, 0, n_right - 1, L)
    form, log2cap = wx.join_plan(n_right, 0, n_right - 1)
    for groups in GROUPS:
        tier = (rkey % groups).to(torch.int32)
        right = wx.Table.from_tensors(id=rkey, rate=rate, bonus=bonus, tier=tier)
        for m, (exprs, stand_in) in VALUES.items():
            sums = [s.data_ptr() for s in d_sums[:m]]

            def fused(launch):
                return wx.join_group_agg(left, right, "fk[idx]", "id", exprs, "tier[idx]", COND, launch, 0, CAP,
                                         d_keys.data_ptr(), d_cnts.data_ptr(), sums)

            def today():
                cnt = wx.join_select(left, right, "fk[idx]", "id", ["tier[idx]"] + exprs, COND, L,
                                     [t.data_ptr() for t in mat[:m + 1]], want_count=True)
                wx.cast(mat[0].data_ptr(), wx.FLOAT32, mkey.data_ptr(), wx.INT32, cnt, L)
                cols = [wx.Column("gk", wx.INT32, mkey.data_ptr())]
                cols += [wx.Column(f"v{j}", wx.FLOAT32, mat[j + 1].data_ptr()) for j in range(m)]
                return wx.group_agg_multi(wx.Table(cnt, cols), [f"v{j}[idx]" for j in range(m)], "gk[idx]", None, L, 0,
                                          CAP, d_keys.data_ptr(), d_cnts.data_ptr(), sums)

            def floor(launch):
                return wx.group_agg_multi(left, stand_in, f"(fk[idx] % {groups})", COND, launch, 0, CAP,
                                          d_keys.data_ptr(), d_cnts.data_ptr(), sums)

            for _ in range(warm):
                ga, gb, gc = fused(L), today(), floor(L)
            assert ga == gb == gc == min(groups, n_right), (ga, gb, gc)
            wx.check(L)
            wx.timing_read()
            ta, tak, tb, tc, tck = [], [], [], [], []
            for _ in range(reps):
                ta.append(wall(lambda: fused(L)))
                fused(Lt)
                tak.append(wx.timing_read()[0])
                tb.append(wall(today))
                tc.append(wall(lambda: floor(L)))
                floor(Lt)
                tck.append(wx.timing_read()[0])
            wx.check(L)
            a, b, c = med(ta), med(tb), med(tc)
            results[(n_right, groups, m)] = (a, b, c)
            good = a < b
            ok = ok and good
            emit(f"right {n_right:8d}  {'direct' if form == wx.JOIN_DIRECT else f'hash 2^{log2cap}':9s}  groups {groups:4d}  "
                 f"values {m}  (a) fused {a:8.3f} ms (pass {med(tak):8.3f} ms)  (b) today {b:8.3f} ms  "
                 f"(c) floor {c:8.3f} ms (kernel {med(tck):8.3f} ms)  | b/a {b / a:5.2f}  a/c {a / c:5.2f}  "
                 f"pass/kernel {med(tak) / med(tck):5.2f}  {'' if good else 'GATE FAILS'}")
        del right, tier
    del rkey, rate, bonus
emit(f"gate: (a) fused faster than (b) today in every case: {'holds' if ok else 'FAILS'}")
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
sys.exit(0 if ok else 1)
