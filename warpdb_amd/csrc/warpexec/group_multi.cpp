// group_multi.cpp -- GROUP BY over several value expressions in one pass
// (wx_group_multi.hip): the LDS window + global hash with one accumulator
// plane per requested aggregate.
#include "wx_host.hpp"

namespace wx {

void do_group_multi(const wx_table *t, const char *const *val_exprs, int32_t n_vals, const char *key_expr,
                    const char *cond, const wx_launch *Lp, int32_t key_lo, int64_t capacity, int32_t *d_keys,
                    double *const *d_sums, int64_t *d_counts, float *const *d_mins, float *const *d_maxs,
                    int64_t *d_n_groups, int64_t *h_n_groups) {
  check_table(t);
  check_group_multi_exprs(val_exprs, n_vals, key_expr);
  int smask = 0, qmask = 0;
  for (int32_t j = 0; j < n_vals; ++j) {
    if (d_sums && d_sums[j]) smask |= 1 << j;
    if ((d_mins && d_mins[j]) || (d_maxs && d_maxs[j])) qmask |= 1 << j;
  }
  check_group_multi_masks(n_vals, smask, qmask);
  const wx_launch L = launch_of(Lp);
  if (n_vals == 1) {
    // wx_group_agg itself (same module, same cache entry); it always writes
    // the sums, so sums nobody asked for land in workspace scratch
    double *sums = d_sums ? d_sums[0] : nullptr;
    if (!sums && capacity > 0 && !(L.flags & WX_F_ROW_ORDER)) {
      Op op(L);
      ensure(op.w, op.w.gm_scratch, (size_t)capacity * 8, false);
      sums = static_cast<double *>(op.w.gm_scratch.p);
    }
    do_group_sum(t, val_exprs[0], key_expr, cond, Lp, key_lo, capacity, d_keys, sums, d_counts, d_n_groups,
                 h_n_groups, d_mins ? d_mins[0] : nullptr, d_maxs ? d_maxs[0] : nullptr);
    return;
  }
  if (L.flags & WX_F_ROW_ORDER)
    fail(WX_ERR_UNSUPPORTED, "row-order sums are not available for several value expressions (one call per value)");
  if (capacity < 0 || (capacity > 0 && (!d_keys || !d_counts)))
    fail(WX_ERR_INVALID, "group outputs must hold `capacity` entries");
  if ((int64_t)key_lo + WX_GROUP_WINDOW - 1 > INT32_MAX) fail(WX_ERR_INVALID, "key window out of range");
  const Spec spec = group_multi_spec(t, val_exprs, n_vals, smask, qmask, key_expr, cond, L);
  const int ns = popcount4(smask), nq = popcount4(qmask);
  Op op(L, spec);
  Workspace &w = op.w;
  int64_t *ng = count_slot(w, w.g_ngroups, d_n_groups);
  // A caller expecting many groups on a large table: the key range of the
  // single-value call over the first value (its memo, else its 65 536-row
  // sample) -- used only to move the window onto a span that fits it.
  if (capacity > WX_GROUP_HSORT_MAX && t->n_rows >= gp_min_rows() && t->n_rows > 0 &&
      env_or("WARPDB_GROUP_PARTITION", "1") != "0") {
    const Spec single = group_spec(t, val_exprs[0], key_expr, cond, L, false);
    const uint64_t mkey = gp_memo_key(single, t, single.cols);
    if (w.gp_memo.size() > 256) w.gp_memo.clear();
    KeyRange r;
    auto it = w.gp_memo.find(mkey);
    const bool from_memo = it != w.gp_memo.end() && (!it->second.window || it->second.uses < 16);
    if (from_memo) {
      r.any = true;
      r.lo = it->second.lo;
      r.hi = it->second.hi;
      ++it->second.uses;
    } else {
      // (the single-value module is fetched only here, where it is needed: a
      // first use compiles it under the operation lock, which a fetch ahead of
      // every call would avoid at the price of compiling it for calls that
      // never use it)
      const std::shared_ptr<Module> smod = get_module(L.device, single, true);
      r = sample_keys(t, single.cols, smod.get(), w, op.s, op.timed);
      if (r.any) {
        const int64_t margin = std::max<int64_t>(r.span() / 8, 64);
        r.lo = std::max<int64_t>(INT32_MIN, r.lo - margin);
        r.hi = std::min<int64_t>(INT32_MAX, r.hi + margin);
      }
    }
    if (r.any && r.span() <= WX_GROUP_WINDOW) {
      key_lo = (int32_t)std::min<int64_t>(r.lo, INT32_MAX - (WX_GROUP_WINDOW - 1));
      if (!from_memo) w.gp_memo[mkey] = Workspace::GpMemo{r.lo, r.hi, true, 0};
    }
  }
  WxGroupMultiArgs a;
  fill_cols(t, spec.cols, a.col);
  a.n_rows = t->n_rows;
  a.acc = group_planes(w, op.s, ns, nq, capacity, key_lo);
  WxGroupMultiFinArgs f{};
  f.acc = a.acc;
  f.out_keys = d_keys;
  f.out_counts = reinterpret_cast<wx_i64 *>(d_counts);
  for (int32_t j = 0; j < n_vals; ++j) {
    f.out_sums[j] = d_sums ? d_sums[j] : nullptr;
    f.out_mins[j] = d_mins ? d_mins[j] : nullptr;
    f.out_maxs[j] = d_maxs ? d_maxs[j] : nullptr;
  }
  f.n_groups_out = reinterpret_cast<wx_i64 *>(ng);
  f.capacity = capacity;
  if (t->n_rows > 0) {
    // 16 waves per CU (WX_GM_PER_CU workgroups of WX_GM_BLOCK threads), one row quad per thread
    const GroupWindowPlan P = group_window_plan(t->n_rows, ns, nq, WX_GW_GROUP_MULTI, 0, op.d.cus, spec.extra);
    launch(op.mod->fn("wx_group_multi"), P.grid, &a, op.s, op.timed, (unsigned)P.block);
  }
  f.sorted = sort_general_keys(op, nullptr, a.acc.ctrs, a.acc.h_used, a.acc.h_tag, capacity, t->n_rows > 0);
  finish_group(op, op.mod->fn("wx_group_multi_finalize"), &f, ng, h_n_groups);
}

}  // namespace wx
