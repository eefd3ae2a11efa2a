// group_window.cpp -- what the LDS-window GROUP BY families share on the host:
// the accumulator planes of the multi-value window (do_group_multi,
// do_join_group), and for those and do_group_sum the device sort of many
// general keys and the finalize launch.
#include "wx_host.hpp"

namespace wx {

int popcount4(int m) { return (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1) + ((m >> 3) & 1); }

// The launch geometry of the streaming kernel of one LDS-window GROUP BY
// over n_rows rows: the one statement of it (do_group_sum, do_group_multi and
// do_join_group launch it, wx_group_window_geometry reports it).  ns summed
// and nq MIN / MAX values; family WX_GW_GROUP_SUM (wx_group_sum, with
// WX_MINMAX when nq == 1), WX_GW_GROUP_MULTI or WX_GW_JOIN_GROUP in the join
// form `form`.  One workgroup per `block` row quads up to 16 waves per CU;
// workgroup b runs the spans b, b + grid, ... of block * WX_UNROLL quads
// each, one batch per span.  WX_GROUP_GRID=<g> (diagnostic define) caps the
// grid and changes nothing else, so that a small table runs many batches per
// workgroup.
GroupWindowPlan group_window_plan(int64_t n_rows, int ns, int nq, int family, int form, int cus,
                                  const std::string &extra) {
  if (n_rows < 0) fail(WX_ERR_INVALID, "negative row count");
  if (cus < 1) fail(WX_ERR_INVALID, "GROUP BY: no compute units");
  if (ns < 0 || ns > WX_GM_MAX || nq < 0 || nq > WX_GM_MAX || ns + nq < 1)
    fail(WX_ERR_INVALID, "n_sums and n_minmax must be between 0 and " + std::to_string(WX_GM_MAX) +
                             ", and one of them at least 1");
  GroupWindowPlan P;
  int per_cu = 0;
  if (family == WX_GW_GROUP_SUM) {
    if (ns != 1 || nq > 1) fail(WX_ERR_INVALID, "wx_group_sum carries one sum and at most one MIN / MAX");
    P.block = WX_GBLOCK;                // 512 at two per CU: profiles/r03/abl_group_grid.txt
    per_cu = 4 * WX_BLOCK / WX_GBLOCK;  // 16 waves per CU
  } else if (family == WX_GW_GROUP_MULTI) {
    P.block = WX_GM_BLOCK(ns, nq);
    per_cu = WX_GM_PER_CU(ns, nq);
  } else if (family == WX_GW_JOIN_GROUP) {
    if (form != WX_JOIN_FORM_DIRECT && form != WX_JOIN_FORM_HASH)
      fail(WX_ERR_INVALID, "form must be 0 (direct) or 1 (hash)");
    P.block = WX_JG_BLOCK(ns, nq, form);
    per_cu = WX_JG_PER_CU(ns, nq, form);
  } else {
    fail(WX_ERR_INVALID, "family must be 0 (group_sum), 1 (group_multi) or 2 (join_group)");
  }
  const int cap = define_value(extra, "WX_GROUP_GRID", INT32_MAX);
  if (cap < 1) fail(WX_ERR_INVALID, "WX_GROUP_GRID must be at least 1");
  const int unroll = define_value(extra, "WX_UNROLL", 2);  // the kernels' default
  if (unroll < 1) fail(WX_ERR_INVALID, "WX_UNROLL must be at least 1");
  const int f256 = P.block / WX_BLOCK;
  const int64_t nq4 = (n_rows + 3) / 4;
  P.grid = std::min<unsigned>(grid_for((nq4 + f256 - 1) / f256, cus, per_cu), (unsigned)cap);
  const int64_t span = (int64_t)P.block * unroll;
  P.span_rows = span * 4;
  // workgroup 0 runs the most batches: every grid-th of the span positions
  P.max_batches = ((nq4 + span - 1) / span + P.grid - 1) / P.grid;
  P.lead = nq ? 0 : define_value(extra, "WX_GROUP_LEAD", 16);  // sum-only builds carry the wave-combined add
  return P;
}

// A plane buffer of at least `bytes`, every byte `fill` when freshly
// allocated: the finalize leaves the planes idle, so an old one is as it
// should be.
void ensure_planes(Workspace &w, hipStream_t s, Buf &b, size_t bytes, int fill) {
  if (b.p && b.bytes >= bytes) return;
  ensure(w, b, bytes, false);
  WX_HIP(hipMemsetAsync(b.p, fill, b.bytes, s));
}

// The workspace's accumulators for ns summed and nq MIN / MAX values and a
// table that holds `capacity` groups at half load.
WxGroupPlanes group_planes(Workspace &w, hipStream_t s, int ns, int nq, int64_t capacity, int key_lo) {
  ensure_group_table(w, s, next_pow2(std::max<int64_t>(4096, 2 * capacity)));
  const size_t hcap = w.g_hcap;
  ensure(w, w.g_win_cnt, WX_GROUP_WINDOW * 8, true);
  ensure(w, w.g_ctrs, 64, true);
  if (ns) {
    ensure_planes(w, s, w.gm_win_sum, (size_t)ns * WX_GROUP_WINDOW * 8, 0);
    ensure_planes(w, s, w.gm_sum, (size_t)ns * hcap * 8, 0);
  }
  if (nq) {
    ensure_planes(w, s, w.gm_win_min, (size_t)nq * WX_GROUP_WINDOW * 4, 0xff);
    ensure_planes(w, s, w.gm_win_max, (size_t)nq * WX_GROUP_WINDOW * 4, 0);
    ensure_planes(w, s, w.gm_min, (size_t)nq * hcap * 4, 0xff);
    ensure_planes(w, s, w.gm_max, (size_t)nq * hcap * 4, 0);
  }
  WxGroupPlanes g;
  g.win_cnt = static_cast<wx_u64 *>(w.g_win_cnt.p);
  g.win_sum = static_cast<double *>(w.gm_win_sum.p);
  g.win_min = static_cast<wx_u32 *>(w.gm_win_min.p);
  g.win_max = static_cast<wx_u32 *>(w.gm_win_max.p);
  g.h_tag = static_cast<wx_u64 *>(w.g_tag.p);
  g.h_cnt = static_cast<wx_u64 *>(w.g_cnt.p);
  g.h_used = static_cast<wx_u32 *>(w.g_used.p);
  g.h_sum = static_cast<double *>(w.gm_sum.p);
  g.h_min = static_cast<wx_u32 *>(w.gm_min.p);
  g.h_max = static_cast<wx_u32 *>(w.gm_max.p);
  g.ctrs = static_cast<wx_u64 *>(w.g_ctrs.p);
  g.hmask = (wx_u32)(hcap - 1);
  g.key_lo = key_lo;
  return g;
}

// More than WX_GROUP_HSORT_MAX general keys (possible only when the caller
// allows that many groups and some row was streamed): sorted on the device
// for the finalize, else null.  The entries are gathered by `own`'s
// wx_group_gather (the single-value module) or, without one, by the util
// module's wx_group_gather_keys, which names no expression.
const wx_u64 *sort_general_keys(Op &op, Module *own, wx_u64 *ctrs, wx_u32 *h_used, wx_u64 *h_tag, int64_t capacity,
                                bool any_rows) {
  if (capacity <= WX_GROUP_HSORT_MAX || !any_rows) return nullptr;
  int64_t nh = 0;
  WX_HIP(hipMemcpyAsync(&nh, ctrs, 8, hipMemcpyDeviceToHost, op.s));
  WX_HIP(hipStreamSynchronize(op.s));
  if (nh <= WX_GROUP_HSORT_MAX) return nullptr;
  int64_t npad = WX_SORT_LDS;
  while (npad < nh) npad <<= 1;
  ensure(op.w, op.w.g_sorted, (size_t)npad * 8, false);
  WxGroupGatherArgs ga;
  ga.ctrs = ctrs;
  ga.h_used = h_used;
  ga.h_tag = h_tag;
  ga.keys = static_cast<wx_u64 *>(op.w.g_sorted.p);
  ga.npad = npad;
  const hipFunction_t gather =
      own ? own->fn("wx_group_gather") : util_module(op.L.device, true)->fn("wx_group_gather_keys");
  launch(gather, grid_for(npad, op.d.cus, 8), &ga, op.s);
  bitonic_u64(op.L.device, ga.keys, npad, op.s);
  return ga.keys;
}

// The finalize: its own one-workgroup launch (1024 threads: WX_GFIN_BLOCK,
// WX_GMF_BLOCK) after the possible key sort, then the count for the host.
void finish_group(Op &op, hipFunction_t finalize, void *fin_args, int64_t *ng, int64_t *h_n_groups) {
  launch(finalize, 1, fin_args, op.s, false, 1024);
  if (h_n_groups) {  // read before the error check: a capacity error still reports the count
    WX_HIP(hipStreamSynchronize(op.s));
    WX_HIP(hipMemcpy(h_n_groups, ng, 8, hipMemcpyDeviceToHost));
  }
  if ((op.L.flags & WX_F_SYNC) || h_n_groups) check_errors(op.w);
}

}  // namespace wx
