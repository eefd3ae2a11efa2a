// join_group.cpp -- JOIN under GROUP BY (wx_join_group.hip): the right
// table's direct or hash table (join.cpp's build), then one pass over the
// left table that probes it and adds the kept rows into wx_group_multi's
// accumulators, then wx_group_multi's finalize.
#include "wx_host.hpp"

namespace wx {

namespace {
void masks_of(int32_t n_vals, double *const *d_sums, float *const *d_mins, float *const *d_maxs, int &smask,
              int &qmask) {
  smask = qmask = 0;
  for (int32_t j = 0; j < n_vals; ++j) {
    if (d_sums && d_sums[j]) smask |= 1 << j;
    if ((d_mins && d_mins[j]) || (d_maxs && d_maxs[j])) qmask |= 1 << j;
  }
}
}  // namespace

void do_prepare_join_group(const wx_table *left, const wx_table *right, const char *left_key_expr,
                           const char *right_key_col, int32_t join_type, const char *const *val_exprs, int32_t n_vals,
                           int sum_mask, int mm_mask, const char *group_key_expr, const char *cond,
                           const wx_launch *Lp, int32_t form) {
  (void)check_join_group_args(left, right, left_key_expr, right_key_col, join_type, val_exprs, n_vals, group_key_expr,
                              cond);
  check_group_multi_masks(n_vals, sum_mask, mm_mask);
  const wx_launch L = launch_of(Lp);
  const Spec spec = join_group_spec(left, right, val_exprs, n_vals, sum_mask, mm_mask, form, left_key_expr,
                                    group_key_expr, cond, L);
  prepare_module(L, join_table_spec());
  prepare_module(L, spec);
}

void do_join_group(const wx_table *left, const wx_table *right, const char *left_key_expr, const char *right_key_col,
                   int32_t join_type, const char *const *val_exprs, int32_t n_vals, const char *group_key_expr,
                   const char *cond, const wx_launch *Lp, int32_t key_lo, int64_t capacity, int32_t *d_keys,
                   double *const *d_sums, int64_t *d_counts, float *const *d_mins, float *const *d_maxs,
                   int64_t *d_n_groups, int64_t *h_n_groups) {
  const JoinNames names = check_join_group_args(left, right, left_key_expr, right_key_col, join_type, val_exprs,
                                                n_vals, group_key_expr, cond);
  int smask = 0, qmask = 0;
  masks_of(n_vals, d_sums, d_mins, d_maxs, smask, qmask);
  check_group_multi_masks(n_vals, smask, qmask);
  const wx_launch L = launch_of(Lp);
  if (L.flags & WX_F_ROW_ORDER) fail(WX_ERR_UNSUPPORTED, "row-order sums are not available for joins");
  if (capacity < 0 || (capacity > 0 && (!d_keys || !d_counts)))
    fail(WX_ERR_INVALID, "group outputs must hold `capacity` entries");
  if ((int64_t)key_lo + WX_GROUP_WINDOW - 1 > INT32_MAX) fail(WX_ERR_INVALID, "key window out of range");
  const int64_t n_right = right->n_rows;
  const int *d_rkeys = static_cast<const int *>(right->cols[names.right_key].d_ptr);

  Op op(L, join_table_spec());  // held over the whole call: the table and the accumulators are the workspace's
  Workspace &w = op.w;
  int64_t *ng = count_slot(w, w.g_ngroups, d_n_groups);
  if (n_right == 0 || left->n_rows == 0) {  // no row is kept: no group, and the accumulators stay idle
    WX_HIP(hipMemsetAsync(ng, 0, 8, op.s));
    if (h_n_groups) {
      WX_HIP(hipStreamSynchronize(op.s));
      *h_n_groups = 0;
    } else if (L.flags & WX_F_SYNC) {
      WX_HIP(hipStreamSynchronize(op.s));
    }
    return;
  }
  const JoinTable jt = build_join_table(op, d_rkeys, n_right);
  const Spec spec = join_group_spec(left, right, val_exprs, n_vals, smask, qmask, jt.plan.form, left_key_expr,
                                    group_key_expr, cond, L);
  const std::shared_ptr<Module> mod = get_module(L.device, spec, true);
  const int ns = popcount4(smask), nq = popcount4(qmask);
  WxJoinGroupArgs a{};
  fill_cols(left, spec.cols, a.g.col);
  a.g.n_rows = left->n_rows;
  a.g.acc = group_planes(w, op.s, ns, nq, capacity, key_lo);
  a.c.ctrs = static_cast<wx_u64 *>(w.ctrs.p);
  fill_cols(right, spec.rcols, a.rcol);
  a.rows = static_cast<const int *>(w.jn_rows.p);
  a.slots = static_cast<const wx_u64 *>(w.jn_slots.p);
  a.key_lo = jt.key_lo;
  a.span = jt.span;
  a.mask = jt.mask;
  a.shift = jt.shift;
  WxGroupMultiFinArgs f{};
  f.acc = a.g.acc;
  f.out_keys = d_keys;
  f.out_counts = reinterpret_cast<wx_i64 *>(d_counts);
  for (int32_t j = 0; j < n_vals; ++j) {
    f.out_sums[j] = d_sums ? d_sums[j] : nullptr;
    f.out_mins[j] = d_mins ? d_mins[j] : nullptr;
    f.out_maxs[j] = d_maxs ? d_maxs[j] : nullptr;
  }
  f.n_groups_out = reinterpret_cast<wx_i64 *>(ng);
  f.capacity = capacity;
  {
    // 16 waves per CU (WX_JG_PER_CU workgroups of WX_JG_BLOCK threads), one row quad per thread
    const GroupWindowPlan P =
        group_window_plan(left->n_rows, ns, nq, WX_GW_JOIN_GROUP, jt.plan.form, op.d.cus, spec.extra);
    launch(mod->fn("wx_join_group"), P.grid, &a, op.s, op.timed, (unsigned)P.block);
  }
  f.sorted = sort_general_keys(op, nullptr, a.g.acc.ctrs, a.g.acc.h_used, a.g.acc.h_tag, capacity, true);
  finish_group(op, mod->fn("wx_group_multi_finalize"), &f, ng, h_n_groups);
}

}  // namespace wx
