// warpexec.cpp -- host runtime behind include/warpexec.h.
//
// Replaces the reference's NVRTC path (src/jit.cpp:48-307): instead of a new
// CUcontext + NVRTC compile + module load per call, generated programs are
// built once per (device arch, query shape) with hiprtc for gfx950, cached in
// memory and on disk, and launched on the caller's stream into per-(device,
// stream) workspaces.  Kernels: warpdb_amd/csrc/kernels/wx_*.hip (one source per family).
//
// This file is the C ABI alone: argument checks that belong to an entry point
// and the call into the family's host code (DESIGN.md 2 has the file table).
#include "wx_host.hpp"

using namespace wx;

// ======================================================================= ABI
extern "C" {

wx_status wx_project_filter(const wx_table *table, const char *expr, const char *cond, const wx_launch *launch_,
                            int32_t mode, float *d_out_vals, void *d_out_idx, int32_t idx_bytes, int64_t row_base,
                            int64_t *d_count, int64_t *h_count, char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    do_project_filter(table, expr, cond, launch_, mode, d_out_vals, d_out_idx, idx_bytes, row_base, d_count,
                      h_count);
  });
}

wx_status wx_project_filter_multi(const wx_table *table, const char *const *exprs, int32_t n_exprs, const char *cond,
                                  const wx_launch *launch_, int32_t mode, float *const *d_out_vals, void *d_out_idx,
                                  int32_t idx_bytes, int64_t row_base, int64_t *d_count, int64_t *h_count, char *err,
                                  size_t errlen) {
  return guarded(err, errlen, [&] {
    do_project_filter_multi(table, exprs, n_exprs, cond, launch_, mode, d_out_vals, d_out_idx, idx_bytes, row_base,
                            d_count, h_count);
  });
}

wx_status wx_prepare_multi(const wx_table *table, const char *const *exprs, int32_t n_exprs, const char *cond,
                           const wx_launch *launch_, char *err, size_t errlen) {
  if (n_exprs == 1 && exprs && !blank(exprs[0]))
    return wx_prepare(table, WX_OP_COMPACT, exprs[0], cond, nullptr, 0, launch_, nullptr, 0, err, errlen);
  return guarded(err, errlen, [&] {
    check_table(table);
    check_select_exprs(exprs, n_exprs);
    const wx_launch L = launch_of(launch_);
    prepare_module(L, select_spec(table, exprs, n_exprs, cond, L));
  });
}

int32_t wx_select_tile_rows(int32_t n_exprs) {
  if (n_exprs < 1 || n_exprs > WX_MAX_OUTPUTS) return 0;
  try {
    Spec spec;
    if (n_exprs == 1) compact_geometry(spec);
    else select_geometry(spec, n_exprs);
    return (int32_t)(spec.dwaves * 64 * 4 * spec.groups);
  } catch (const WxError &) {
    return 0;
  }
}

wx_status wx_compact_last_launch(const wx_launch *launch_, wx_compact_geom *out, char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    if (!out) fail(WX_ERR_INVALID, "null geometry output");
    const wx_launch L = launch_of(launch_);
    *out = {0, 0, 0, 0};
    // (no workspace yet: nothing was launched there, and none is made for the question)
    if (Workspace *w = find_workspace(L.device, static_cast<hipStream_t>(L.stream))) {
      OpLock lock(w->op_mu);
      *out = w->cs_last;
    }
  });
}

wx_status wx_gather_multi(const wx_table *table, const char *const *exprs, int32_t n_exprs, const void *d_rows,
                          int32_t idx_bytes, int64_t row_base, int64_t count, const int64_t *d_count,
                          const wx_launch *launch_, float *const *d_out_vals, int64_t *d_out_rows, int64_t out_row_base,
                          char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    do_gather_multi(table, exprs, n_exprs, d_rows, idx_bytes, row_base, count, d_count, launch_, d_out_vals,
                    d_out_rows, out_row_base);
  });
}

wx_status wx_prepare_gather(const wx_table *table, const char *const *exprs, int32_t n_exprs, const wx_launch *launch_,
                            char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    check_gather_args(table, exprs, n_exprs, 8, 0);
    const wx_launch L = launch_of(launch_);
    prepare_module(L, gather_spec(table, exprs, n_exprs, L));
  });
}

int32_t wx_gather_tile_rows(int32_t n_exprs) {
  if (n_exprs < 1 || n_exprs > WX_MAX_OUTPUTS) return 0;
  try {
    Spec spec;
    gather_geometry(spec, n_exprs);
    return (int32_t)(spec.gblock * 4 * spec.gunroll);
  } catch (const WxError &) {
    return 0;
  }
}

wx_status wx_select_ordered(const wx_table *table, const char *const *exprs, int32_t n_exprs, const char *cond,
                            const char *order_expr, int32_t descending, int64_t limit, const wx_launch *launch_,
                            int64_t row_base, float *const *d_out_vals, float *d_out_keys, int64_t *d_out_rows,
                            int64_t capacity, int64_t *d_count, int64_t *h_count, char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    do_select_ordered(table, exprs, n_exprs, cond, order_expr, descending, limit, launch_, row_base, d_out_vals,
                      d_out_keys, d_out_rows, capacity, d_count, h_count);
  });
}

wx_status wx_reduce_sum(const wx_table *table, const char *expr, const char *cond, const wx_launch *launch_,
                        void *d_out, double *h_sum, int64_t *h_count, char *err, size_t errlen) {
  return guarded(err, errlen, [&] { do_reduce_sum(table, expr, cond, launch_, d_out, h_sum, h_count); });
}

wx_status wx_reduce_stats(const wx_table *table, const char *expr, const char *cond, const wx_launch *launch_,
                          void *d_out, wx_stats *h_out, char *err, size_t errlen) {
  return guarded(err, errlen,
                 [&] { do_reduce_sum(table, expr, cond, launch_, d_out, nullptr, nullptr, true, h_out); });
}

wx_status wx_group_agg(const wx_table *table, const char *val_expr, const char *key_expr, const char *cond,
                       const wx_launch *launch_, int32_t key_window_lo, int64_t capacity, int32_t *d_keys,
                       double *d_sums, int64_t *d_counts, float *d_mins, float *d_maxs, int64_t *d_n_groups,
                       int64_t *h_n_groups, char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    do_group_sum(table, val_expr, key_expr, cond, launch_, key_window_lo, capacity, d_keys, d_sums, d_counts,
                 d_n_groups, h_n_groups, d_mins, d_maxs);
  });
}

wx_status wx_group_sum(const wx_table *table, const char *val_expr, const char *key_expr, const char *cond,
                       const wx_launch *launch_, int32_t key_window_lo, int64_t capacity, int32_t *d_keys,
                       double *d_sums, int64_t *d_counts, int64_t *d_n_groups, int64_t *h_n_groups, char *err,
                       size_t errlen) {
  return guarded(err, errlen, [&] {
    do_group_sum(table, val_expr, key_expr, cond, launch_, key_window_lo, capacity, d_keys, d_sums, d_counts,
                 d_n_groups, h_n_groups);
  });
}

wx_status wx_group_agg_multi(const wx_table *table, const char *const *val_exprs, int32_t n_vals,
                             const char *key_expr, const char *cond, const wx_launch *launch_, int32_t key_window_lo,
                             int64_t capacity, int32_t *d_keys, double *const *d_sums, int64_t *d_counts,
                             float *const *d_mins, float *const *d_maxs, int64_t *d_n_groups, int64_t *h_n_groups,
                             char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    do_group_multi(table, val_exprs, n_vals, key_expr, cond, launch_, key_window_lo, capacity, d_keys, d_sums,
                   d_counts, d_mins, d_maxs, d_n_groups, h_n_groups);
  });
}

wx_status wx_prepare_group_multi(const wx_table *table, const char *const *val_exprs, int32_t n_vals,
                                 uint32_t sum_mask, uint32_t minmax_mask, const char *key_expr, const char *cond,
                                 const wx_launch *launch_, char *err, size_t errlen) {
  if (n_vals == 1 && val_exprs && !blank(val_exprs[0]) && !blank(key_expr) && ((sum_mask | minmax_mask) == 1u))
    return wx_prepare(table, WX_OP_GROUP, val_exprs[0], cond, key_expr, minmax_mask ? 1 : 0, launch_, nullptr, 0, err,
                      errlen);
  return guarded(err, errlen, [&] {
    check_table(table);
    check_group_multi_exprs(val_exprs, n_vals, key_expr);
    if ((sum_mask | minmax_mask) >> WX_GROUP_MAX_VALUES) fail(WX_ERR_INVALID, "an aggregate mask names a value beyond n_vals");
    check_group_multi_masks(n_vals, (int)sum_mask, (int)minmax_mask);
    const wx_launch L = launch_of(launch_);
    prepare_module(L, group_multi_spec(table, val_exprs, n_vals, (int)sum_mask, (int)minmax_mask, key_expr, cond, L));
  });
}

wx_status wx_window_select(const wx_table *table, const char *const *exprs, int32_t n_exprs,
                           const wx_window_item *items, int32_t n_items, const char *part_expr, const char *cond,
                           const wx_launch *launch_, int32_t key_window_lo, int64_t group_capacity,
                           float *const *d_out_vals, void *d_out_idx, int32_t idx_bytes, int64_t row_base,
                           int64_t *d_count, int64_t *h_count, char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    do_window_select(table, exprs, n_exprs, items, n_items, part_expr, cond, launch_, key_window_lo, group_capacity,
                     d_out_vals, d_out_idx, idx_bytes, row_base, d_count, h_count);
  });
}

wx_status wx_prepare_window(const wx_table *table, const char *const *exprs, int32_t n_exprs,
                            const wx_window_item *items, int32_t n_items, const char *part_expr, const char *cond,
                            const wx_launch *launch_, int32_t search, char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    do_prepare_window(table, exprs, n_exprs, items, n_items, part_expr, cond, launch_, search);
  });
}

int32_t wx_window_tile_rows(int32_t n_outputs, int32_t n_items, int32_t search) {
  if (search != 0 && search != 1) return 0;
  try {
    Spec spec;
    window_geometry(spec, n_outputs, n_items, search != 0);
    return (int32_t)(spec.dwaves * 64 * 4 * spec.groups);
  } catch (const WxError &) {
    return 0;
  }
}

wx_status wx_join_select(const wx_table *left, const wx_table *right, const char *left_key_expr,
                         const char *right_key_col, int32_t join_type, const char *const *exprs, int32_t n_exprs,
                         const char *cond, const wx_launch *launch_, float *const *d_out_vals, void *d_out_idx,
                         int32_t idx_bytes, int64_t row_base, int32_t *d_out_right_row, int64_t *d_count,
                         int64_t *h_count, char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    do_join_select(left, right, left_key_expr, right_key_col, join_type, exprs, n_exprs, cond, launch_, d_out_vals,
                   d_out_idx, idx_bytes, row_base, d_out_right_row, d_count, h_count);
  });
}

wx_status wx_prepare_join(const wx_table *left, const wx_table *right, const char *left_key_expr,
                          const char *right_key_col, int32_t join_type, const char *const *exprs, int32_t n_exprs,
                          const char *cond, const wx_launch *launch_, int32_t with_right_row, int32_t form, char *err,
                          size_t errlen) {
  return guarded(err, errlen, [&] {
    do_prepare_join(left, right, left_key_expr, right_key_col, join_type, exprs, n_exprs, cond, launch_,
                    with_right_row, form);
  });
}

int32_t wx_join_tile_rows(int32_t n_outputs, int32_t form, int32_t with_right_row) {
  if (with_right_row != 0 && with_right_row != 1) return 0;
  try {
    Spec spec;
    join_geometry(spec, n_outputs, form, with_right_row != 0);
    return (int32_t)(spec.dwaves * 64 * 4 * spec.groups);
  } catch (const WxError &) {
    return 0;
  }
}

wx_status wx_join_plan(int64_t n_right, int32_t key_min, int32_t key_max, int32_t *form, int32_t *log2_capacity,
                       char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    const JoinPlan p = join_plan(n_right, key_min, key_max);
    if (form) *form = p.form;
    if (log2_capacity) *log2_capacity = p.log2cap;
  });
}

int32_t wx_join_hash_slot(int32_t key, int32_t log2_capacity) {
  if (log2_capacity < WX_JOIN_MIN_LOG2CAP || log2_capacity > 27) return -1;
  return (int32_t)(((uint32_t)key * WX_JOIN_HASH_MUL) >> (32 - log2_capacity));
}

wx_status wx_join_group_agg(const wx_table *left, const wx_table *right, const char *left_key_expr,
                            const char *right_key_col, int32_t join_type, const char *const *val_exprs, int32_t n_vals,
                            const char *group_key_expr, const char *cond, const wx_launch *launch_,
                            int32_t key_window_lo, int64_t capacity, int32_t *d_keys, double *const *d_sums,
                            int64_t *d_counts, float *const *d_mins, float *const *d_maxs, int64_t *d_n_groups,
                            int64_t *h_n_groups, char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    do_join_group(left, right, left_key_expr, right_key_col, join_type, val_exprs, n_vals, group_key_expr, cond,
                  launch_, key_window_lo, capacity, d_keys, d_sums, d_counts, d_mins, d_maxs, d_n_groups, h_n_groups);
  });
}

wx_status wx_prepare_join_group(const wx_table *left, const wx_table *right, const char *left_key_expr,
                                const char *right_key_col, int32_t join_type, const char *const *val_exprs,
                                int32_t n_vals, uint32_t sum_mask, uint32_t minmax_mask, const char *group_key_expr,
                                const char *cond, const wx_launch *launch_, int32_t form, char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    do_prepare_join_group(left, right, left_key_expr, right_key_col, join_type, val_exprs, n_vals, (int)sum_mask,
                          (int)minmax_mask, group_key_expr, cond, launch_, form);
  });
}

wx_status wx_join_group_geometry(int32_t n_sums, int32_t n_minmax, int32_t form, int32_t *block, int32_t *per_cu,
                                 int32_t *lds_bytes, char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    if (n_sums < 0 || n_sums > WX_GM_MAX || n_minmax < 0 || n_minmax > WX_GM_MAX || n_sums + n_minmax < 1)
      fail(WX_ERR_INVALID, "n_sums and n_minmax must be between 0 and " + std::to_string(WX_GM_MAX) +
                               ", and one of them at least 1");
    if (form != WX_JOIN_FORM_DIRECT && form != WX_JOIN_FORM_HASH)
      fail(WX_ERR_INVALID, "form must be 0 (direct) or 1 (hash)");
    if (block) *block = WX_JG_BLOCK(n_sums, n_minmax, form);
    if (per_cu) *per_cu = WX_JG_PER_CU(n_sums, n_minmax, form);
    if (lds_bytes) *lds_bytes = WX_JG_LDS_BYTES(n_sums, n_minmax, form);
  });
}

wx_status wx_group_partials(const wx_table *table, const char *val_expr, const char *key_expr, const char *cond,
                            const wx_launch *launch_, int32_t key_window_lo, double *d_window, int64_t capacity,
                            int32_t *d_keys, double *d_sums, int64_t *d_counts, int64_t *d_n_extra,
                            int64_t *h_n_extra, char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    if (!d_window) fail(WX_ERR_INVALID, "null exchange window");
    do_group_sum(table, val_expr, key_expr, cond, launch_, key_window_lo, capacity, d_keys, d_sums, d_counts,
                 d_n_extra, h_n_extra, nullptr, nullptr, d_window);
  });
}

wx_status wx_group_combine(const double *d_window, int32_t key_window_lo, const int32_t *d_x_keys,
                           const double *d_x_sums, const int64_t *d_x_counts, int64_t n_extra,
                           const wx_launch *launch_, int64_t capacity, int32_t *d_keys, double *d_sums,
                           int64_t *d_counts, int64_t *d_n_groups, int64_t *h_n_groups, char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    do_group_combine(d_window, key_window_lo, d_x_keys, d_x_sums, d_x_counts, n_extra, launch_, capacity, d_keys,
                     d_sums, d_counts, d_n_groups, h_n_groups);
  });
}

wx_status wx_group_partials_slots(const wx_table *table, const char *val_expr, const char *key_expr, const char *cond,
                                  const wx_launch *launch_, int32_t key_window_lo, double *d_exchange, int32_t n_slots,
                                  int32_t slot, int32_t slot_groups, int64_t capacity, int32_t *d_keys, double *d_sums,
                                  int64_t *d_counts, int64_t *d_n_extra, int64_t *h_n_extra, char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    if (!d_exchange) fail(WX_ERR_INVALID, "null exchange buffer");
    check_slots(n_slots, slot_groups);
    if (slot < 0 || slot >= n_slots) fail(WX_ERR_INVALID, "slot out of range");
    do_group_sum(table, val_expr, key_expr, cond, launch_, key_window_lo, capacity, d_keys, d_sums, d_counts,
                 d_n_extra, h_n_extra, nullptr, nullptr, d_exchange, n_slots, slot, slot_groups);
  });
}

wx_status wx_group_combine_slots(const double *d_exchange, int32_t n_slots, int32_t slot_groups,
                                 int32_t key_window_lo, const wx_launch *launch_, int64_t capacity, int32_t *d_keys,
                                 double *d_sums, int64_t *d_counts, int64_t *d_n_groups, int64_t *h_n_groups,
                                 char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    do_group_combine_slots(d_exchange, n_slots, slot_groups, key_window_lo, launch_, capacity, d_keys, d_sums,
                           d_counts, d_n_groups, h_n_groups);
  });
}

wx_status wx_group_merge_lists(const void *d_lists, int32_t n_lists, int64_t list_capacity, const double *d_window,
                               int32_t key_window_lo, const wx_launch *launch_, int64_t capacity, int32_t *d_keys,
                               double *d_sums, int64_t *d_counts, int64_t *d_n_groups, int64_t *h_n_groups, char *err,
                               size_t errlen) {
  return guarded(err, errlen, [&] {
    do_group_merge_lists(d_lists, n_lists, list_capacity, d_window, key_window_lo, launch_, capacity, d_keys, d_sums,
                         d_counts, d_n_groups, h_n_groups);
  });
}

wx_status wx_topk_merge(const wx_topk_record *d_records, int32_t n_records, int32_t k, int32_t descending,
                        const wx_launch *launch_, float *d_keys, int64_t *d_idx, float *d_vals, int64_t *d_count,
                        int64_t *h_count, char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    do_topk_merge(d_records, n_records, k, descending, launch_, d_keys, d_idx, d_vals, d_count, h_count);
  });
}

wx_status wx_order_head(const wx_table *table, const char *order_expr, const char *cond, const char *select_expr,
                        int64_t limit, int32_t descending, const wx_launch *launch_, int64_t row_base, void *d_record,
                        int64_t cap, char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    do_order_head(table, order_expr, cond, select_expr, limit, descending, launch_, row_base, d_record, cap);
  });
}

wx_status wx_head_merge(const void *d_records, int32_t n_records, int64_t cap, int64_t limit, int32_t descending,
                        const wx_launch *launch_, float *d_keys, int64_t *d_rows, float *d_vals, int64_t *d_count,
                        int64_t *h_count, char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    do_head_merge(d_records, n_records, cap, limit, descending, launch_, d_keys, d_rows, d_vals, d_count, h_count);
  });
}

wx_status wx_cast(const void *d_src, int32_t src_dtype, void *d_dst, int32_t dst_dtype, int64_t n,
                  const wx_launch *launch_, char *err, size_t errlen) {
  return guarded(err, errlen, [&] { do_cast(d_src, src_dtype, d_dst, dst_dtype, n, launch_); });
}

wx_status wx_topk(const wx_table *table, const char *order_expr, const char *cond, const char *select_expr,
                  int32_t k, int32_t descending, const wx_launch *launch_, int64_t row_base, float *d_keys,
                  int64_t *d_idx, float *d_vals, int64_t *d_count, int64_t *h_count, char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    do_topk(table, order_expr, cond, select_expr, k, descending, launch_, row_base, d_keys, d_idx, d_vals, d_count,
            h_count);
  });
}

wx_status wx_topk_plan(int64_t n_rows, int32_t k, int32_t cus, const wx_launch *launch_, wx_topk_geometry *out,
                       char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    if (!out) fail(WX_ERR_INVALID, "null plan output");
    if (n_rows < 0) fail(WX_ERR_INVALID, "negative row count");
    if (k < 1 || k > WX_TOPK_MAX) fail(WX_ERR_UNSUPPORTED, "LIMIT must be between 1 and 32");
    if (cus <= 0) cus = device_state(launch_of(launch_).device, true).cus;
    const TopkPlan P = topk_plan(n_rows, k, cus, env_or("WARPDB_EXTRA_DEFINES", ""));
    out->grid = P.grid;
    out->span_rows = P.span * 4;
    out->max_batches = P.max_batches;
    out->seed_grid = P.seed_grid;
    out->seed_stride_rows = P.seed_stride * 4;
  });
}

wx_status wx_group_part_geometry(int64_t n_rows, int64_t key_span, int32_t cus, const wx_launch *launch_,
                                 wx_group_part_geom *out, char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    if (!out) fail(WX_ERR_INVALID, "null geometry output");
    if (cus <= 0) cus = device_state(launch_of(launch_).device, true).cus;
    const GpPlan P = gp_plan(n_rows, key_span, cus, env_or("WARPDB_EXTRA_DEFINES", ""));
    out->tile_rows = P.tile_rows;
    out->n_tiles = P.n_tiles;
    out->grid = P.grid;
    out->tiles_per_wg = P.tiles_per_wg;
    out->n_part = P.n_part;
    out->part_keys = P.part_keys;
    out->chunk_rows = P.chunk_rows;
    out->target_items = P.target_items;
    out->work_cap = P.work_cap;
    out->dir_chunk = P.dir_chunk;
    out->agg_tiles_per_sweep = P.agg_sweep;
  });
}

wx_status wx_group_part_passes(const wx_launch *launch_, int64_t *passes, char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    if (!passes) fail(WX_ERR_INVALID, "null pass count output");
    Op op(launch_of(launch_));
    *passes = op.w.gp_passes;
  });
}

wx_status wx_group_rows_geometry(wx_group_rows_geom *out, char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    if (!out) fail(WX_ERR_INVALID, "null geometry output");
    const std::string extra = env_or("WARPDB_EXTRA_DEFINES", "");
    out->tile_rows = WX_RO_TILE_ROWS;
    out->span_bins = kRoSpanBins;
    out->count_span_rows = kRoCountRows;
    out->fold_block_values = 64 * (int64_t)define_value(extra, "WX_XF_J", kXfJ);
    out->fold_blocks_ahead = define_value(extra, "WX_XF_AHEAD", kXfAhead);
    out->fold_small = WX_FOLD_SMALL;
    out->starts_chunk = WX_GS_CHUNK;
    out->rle_wave_rows = kRleWaveRows;
    out->xf_chunk = WX_XF_CHUNK;
    out->xf_big = WX_XF_BIG;
    out->sample_rows = (int64_t)kSampleGrid * WX_GP_BLOCK;
  });
}

wx_status wx_group_rows_last_call(const wx_launch *launch_, wx_group_rows_record *out, char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    if (!out) fail(WX_ERR_INVALID, "null record output");
    const wx_launch L = launch_of(launch_);
    *out = {0, 0, 0, 0, 0, 0, 0};
    // (no workspace yet: nothing ran there, and none is made for the question)
    if (Workspace *w = find_workspace(L.device, static_cast<hipStream_t>(L.stream))) {
      OpLock lock(w->op_mu);
      *out = w->ro_last;
    }
  });
}

wx_status wx_group_rows_last_values(const wx_launch *launch_, float *d_out, int64_t capacity, int64_t *n_values,
                                    char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    const wx_launch L = launch_of(launch_);
    if (n_values) *n_values = 0;
    if (capacity < 0 || (capacity > 0 && !d_out)) fail(WX_ERR_INVALID, "the value buffer must hold `capacity` floats");
    Workspace *w = find_workspace(L.device, static_cast<hipStream_t>(L.stream));
    if (!w) fail(WX_ERR_INVALID, "no row-order GROUP BY ran on this (device, stream)");
    OpLock lock(w->op_mu);
    if (w->ro_last.route == WX_RO_ROUTE_NONE) fail(WX_ERR_INVALID, "no row-order GROUP BY ran on this (device, stream)");
    const int64_t m = w->ro_last.n_values;
    if (n_values) *n_values = m;
    if (m > capacity) fail(WX_ERR_CAPACITY, "the row-ordered value array holds more than `capacity` values");
    if (m == 0) return;
    DevGuard guard(L.device);
    hipStream_t s = static_cast<hipStream_t>(L.stream);
    WX_HIP(hipMemcpyAsync(d_out, w->ro_last_vals, (size_t)m * 4, hipMemcpyDeviceToDevice, s));
    if (L.flags & WX_F_SYNC) WX_HIP(hipStreamSynchronize(s));
  });
}

wx_status wx_group_window_geometry(int64_t n_rows, int32_t n_sums, int32_t n_minmax, int32_t family,
                                   int32_t join_form, int32_t cus, const wx_launch *launch_, wx_group_window_geom *out,
                                   char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    if (!out) fail(WX_ERR_INVALID, "null geometry output");
    if (cus <= 0) cus = device_state(launch_of(launch_).device, true).cus;
    const GroupWindowPlan P =
        group_window_plan(n_rows, n_sums, n_minmax, family, join_form, cus, env_or("WARPDB_EXTRA_DEFINES", ""));
    out->block_threads = P.block;
    out->span_rows = P.span_rows;
    out->grid = P.grid;
    out->max_batches = P.max_batches;
    out->window_keys = WX_GROUP_WINDOW;
    out->hsort_max = WX_GROUP_HSORT_MAX;
    out->lead = P.lead;
  });
}

wx_status wx_group_table_slots(const wx_launch *launch_, int64_t *slots, char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    if (!slots) fail(WX_ERR_INVALID, "null slot count output");
    Op op(launch_of(launch_));
    *slots = op.w.g_hcap;
  });
}

int32_t wx_group_hash_slot(int32_t key, int64_t slots) {
  if (slots < 1 || slots > (1ll << 30) || (slots & (slots - 1))) return -1;
  return (int32_t)(((uint32_t)key * 2654435761u) & (uint32_t)(slots - 1));
}

wx_status wx_sort_pairs(int32_t *d_keys, float *d_vals, int64_t count, int32_t ascending, const wx_launch *launch_,
                        char *err, size_t errlen) {
  return guarded(err, errlen, [&] { do_sort(d_keys, d_vals, count, 1, ascending, launch_); });
}

wx_status wx_sort_float(float *d_vals, int64_t count, int32_t ascending, const wx_launch *launch_, char *err,
                        size_t errlen) {
  return guarded(err, errlen, [&] { do_sort(d_vals, nullptr, count, 0, ascending, launch_); });
}

wx_status wx_sort_float_from(const float *d_src, float *d_dst, int64_t count, int32_t ascending,
                             const wx_launch *launch_, char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    if (count > 0 && !d_src) fail(WX_ERR_INVALID, "null source buffer");
    if (d_src && d_dst && d_src != d_dst && d_src < d_dst + count && d_dst < d_src + count)
      fail(WX_ERR_INVALID, "source and destination overlap");
    do_sort(d_dst, nullptr, count, 0, ascending, launch_, -1, d_src);
  });
}

wx_status wx_sort_by_key(float *d_keys, float *d_vals, int64_t count, int32_t ascending, const wx_launch *launch_,
                         char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    if (count > 1 && !d_vals) fail(WX_ERR_INVALID, "null payload buffer");
    do_sort(d_keys, d_vals, count, 0, ascending, launch_);
  });
}

wx_status wx_sort_float_limit(float *d_vals, int64_t count, int64_t limit, int32_t ascending, const wx_launch *launch_,
                              char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    if (limit < 0) fail(WX_ERR_INVALID, "negative limit");
    do_sort(d_vals, nullptr, count, 0, ascending, launch_, limit);
  });
}

wx_status wx_sort_by_key_limit(float *d_keys, float *d_vals, int64_t count, int64_t limit, int32_t ascending,
                               const wx_launch *launch_, char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    if (limit < 0) fail(WX_ERR_INVALID, "negative limit");
    if (count > 1 && !d_vals) fail(WX_ERR_INVALID, "null payload buffer");
    do_sort(d_keys, d_vals, count, 0, ascending, launch_, limit);
  });
}

int32_t wx_sort_tile_keys(int32_t with_payload) {
  try {
    int items = 0, block = 0;
    rs_tile_shape(with_payload != 0, &items, &block);
    return (int32_t)(items * block);
  } catch (const WxError &) {
    return 0;
  }
}

int32_t wx_sort_hist_span_keys(void) {
  const int unroll = define_value(env_or("WARPDB_EXTRA_DEFINES", ""), "WX_RS_HUNROLL", WX_RS_HUNROLL);
  return unroll < 1 || unroll > 64 ? 0 : (int32_t)(WX_RS_HBLOCK * unroll * 4);
}

wx_status wx_fill_synthetic(void *d_ptr, int32_t dtype, int64_t n, uint64_t seed, int32_t kind, double lo, double hi,
                            int64_t row_base, const wx_launch *launch_, char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    if (n < 0 || (n > 0 && !d_ptr)) fail(WX_ERR_INVALID, "bad buffer");
    if (dtype < WX_INT32 || dtype > WX_FLOAT64) fail(WX_ERR_INVALID, "bad dtype");
    if (kind != 0 && kind != 1) fail(WX_ERR_INVALID, "bad kind");
    if (n == 0) return;
    Op op(launch_of(launch_), util_spec());
    WxFillArgs a;
    a.out = d_ptr;
    a.n = n;
    a.seed = seed;
    a.lo = lo;
    a.hi = hi;
    a.row_base = row_base;
    a.dtype = dtype;
    a.kind = kind;
    launch(op.mod->fn("wx_fill_synthetic"), grid_for(n, op.d.cus, 16), &a, op.s);
    if (op.L.flags & WX_F_SYNC) WX_HIP(hipStreamSynchronize(op.s));
  });
}

wx_status wx_prepare(const wx_table *table, int32_t op, const char *expr, const char *cond, const char *aux_expr,
                     int32_t k, const wx_launch *launch_, char *src_out, size_t src_len, char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    const wx_launch L = launch_of(launch_);
    Spec spec;
    std::string more;  // UTIL: + the key/payload radix geometry's module
    if (op == WX_OP_UTIL) {
      spec = util_spec();
      int items = 0, block = 0;
      more = rs_geometry(true, &items, &block, device_visible(L) ? device_state(L.device, true).arch : default_arch());
    } else {
      check_table(table);
      if (op < WX_OP_DENSE || op > WX_OP_TOPK) fail(WX_ERR_INVALID, "bad op");
      if (blank(expr)) fail(WX_ERR_INVALID, "Empty query expression");
      if (op == WX_OP_TOPK && (k < 1 || k > WX_TOPK_MAX)) fail(WX_ERR_UNSUPPORTED, "LIMIT must be between 1 and 32");
      // The run path's builders, with what a prepare cannot know assumed: an
      // aligned dense output, a descending top-K.  k = 1 of SUM / GROUP: the
      // MIN / MAX build.
      switch (op) {
        case WX_OP_SUM: spec = sum_spec(table, expr, cond, L, k != 0, aux_expr); break;
        case WX_OP_GROUP: spec = group_spec(table, expr, aux_expr, cond, L, k != 0); break;
        case WX_OP_TOPK: spec = topk_spec(table, expr, cond, aux_expr, k, 1, L); break;
        default: spec = project_spec(table, op, expr, cond, L, true, aux_expr); break;
      }
    }
    if (src_out && src_len) std::snprintf(src_out, src_len, "%s", spec.source().c_str());
    prepare_module(L, spec);
    if (!more.empty()) prepare_module(L, util_spec(more));
  });
}

wx_status wx_check(const wx_launch *launch_, char *err, size_t errlen) {
  return guarded(err, errlen, [&] {
    Op op(launch_of(launch_));
    check_errors(op.w);
  });
}

wx_status wx_timing_read(double *total_ms, int64_t *launches, char *err, size_t errlen) {
  return guarded(err, errlen, [&] { timing_take(-1, total_ms, launches); });
}

wx_status wx_timing_read_device(int32_t device, double *total_ms, int64_t *launches, char *err, size_t errlen) {
  return guarded(err, errlen, [&] { timing_take(device, total_ms, launches); });
}

void wx_cache_stats(int64_t *compiles, int64_t *hits) { cache_stats(compiles, hits); }

void wx_shutdown(void) { shutdown(); }

int32_t wx_abi_version(void) { return WX_ABI_VERSION; }

}  // extern "C"
