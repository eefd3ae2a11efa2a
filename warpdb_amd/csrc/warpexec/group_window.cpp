// group_window.cpp -- what the LDS-window GROUP BY families share on the host:
// the accumulator planes of the multi-value window (do_group_multi,
// do_join_group), and for those and do_group_sum the device sort of many
// general keys and the finalize launch.
#include "wx_host.hpp"

namespace wx {

int popcount4(int m) { return (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1) + ((m >> 3) & 1); }

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
