// topk.cpp -- top-K (wx_topk.hip), the merge of shard candidates, and the
// ORDER BY .. LIMIT heads of any length with their merge (wx_util.hip).
#include "wx_host.hpp"

namespace wx {

// The launch plan of a top-K query: the one statement of the scan's and the
// seed pass's geometry (do_topk launches it, wx_topk_plan reports it).
//
// Scan: workgroup b runs the spans b, b + grid, ... of `span` quads each.
// The grid is one workgroup per WX_BLOCK quads up to two per CU
// (profiles/r01/ablate_topk_grid_bound.txt: few waves publish early bounds);
// WX_TOPK_GRID (diagnostic define) caps it further and changes nothing else,
// so that a small table runs many batches per workgroup.
//
// Seed pass (wx_topk_seed): one span per workgroup at evenly spaced
// offsets, ~1M rows, its exact K-th best raised into slot 0 before the
// scan.  WX_TOPK_SEED (diagnostic define) 0 = off, 1 = K >= 5 over tables
// of >= 2^24 rows (the default; WX_TOPK_SEED_MINK moves the K bound), 2 =
// any table of two spans or more.  Per 1e9 rows: K = 5 (C5) scan 0.607-0.612
// -> 0.564 ms, query 0.649-0.656 -> 0.644-0.649; K = 8 query -17..-22 us;
// K = 2 neutral (profiles/r06/topk_seed_k_le8.txt); K = 9 / 16 / 32 0.79 /
// 0.89 / 1.31 ms instead of 0.85 / 1.04 / 1.94 (profiles/r05/topk_seed.txt).
TopkPlan topk_plan(int64_t n_rows, int32_t k, int cus, const std::string &extra) {
  TopkPlan P;
  P.nq = (n_rows + 3) / 4;
  P.grid = grid_for(P.nq, cus, 2);
  const int cap = define_value(extra, "WX_TOPK_GRID", 0);
  if (cap >= 1 && P.grid > (unsigned)cap) P.grid = (unsigned)cap;
  P.span = (int64_t)WX_BLOCK * define_value(extra, "WX_UNROLL", 8);  // quads per batch
  if (P.span < 1) fail(WX_ERR_INVALID, "WX_UNROLL must be at least 1");
  const int seed_mode = define_value(extra, "WX_TOPK_SEED", 1);
  const int seed_min_k = define_value(extra, "WX_TOPK_SEED_MINK", 5);
  const int64_t spans = P.nq / P.span;
  const bool seed =
      spans >= 2 && (seed_mode == 2 || (seed_mode == 1 && k >= seed_min_k && n_rows >= ((int64_t)1 << 24)));
  P.seed_grid = seed ? std::min<int64_t>(spans, WX_TOPK_SEED_SPANS) : 0;
  P.seed_stride = seed ? (spans / P.seed_grid) * P.span : 0;
  // workgroup 0 runs the most batches: every grid-th of the span positions
  const int64_t positions = (P.nq + P.span - 1) / P.span;
  P.max_batches = (positions + P.grid - 1) / P.grid;
  return P;
}

void do_topk(const wx_table *t, const char *order_expr, const char *cond, const char *select_expr, int32_t k,
             int32_t desc, const wx_launch *Lp, int64_t row_base, float *d_keys, int64_t *d_idx, float *d_vals,
             int64_t *d_count, int64_t *h_count) {
  check_table(t);
  const wx_launch L = launch_of(Lp);
  if (blank(order_expr)) fail(WX_ERR_INVALID, "Empty ORDER BY expression");
  if (k < 1 || k > WX_TOPK_MAX) fail(WX_ERR_UNSUPPORTED, "LIMIT must be between 1 and 32");
  const Spec spec = topk_spec(t, order_expr, cond, select_expr, k, desc, L);
  Op op(L, spec);
  const TopkPlan P = topk_plan(t->n_rows, k, op.d.cus, spec.extra);
  const unsigned grid = P.grid;
  const int64_t span = P.span, nq = P.nq, gs = P.seed_grid;
  const bool seed = gs > 0;
  // candidates of the scan's grid, or of the seed's workgroups when a device
  // with few CUs gives the scan the smaller grid
  const size_t n_cand_max = (size_t)std::max<int64_t>(grid, gs) * k;
  ensure(op.w, op.w.cand_k, n_cand_max * 4, false);
  ensure(op.w, op.w.cand_i, n_cand_max * 8, false);
  int64_t *cnt = count_slot(op.w, op.w.count_tmp, d_count, h_count != nullptr);
  WxTopkArgs a;
  fill_cols(t, spec.cols, a.col);
  a.cand_k = static_cast<wx_u32 *>(op.w.cand_k.p);
  a.cand_i = static_cast<wx_i64 *>(op.w.cand_i.p);
  // The bound slots start at 0: zeroed when allocated, then by the previous
  // query's finalize; a query that did not reach its finalize launch leaves
  // them marked dirty and the next one clears them here.
  const size_t thresh_bytes = (size_t)WX_TOPK_SLOTS * WX_TOPK_SLOT_STRIDE * 4;
  void *old_thresh = op.w.topk_thresh.p;
  ensure(op.w, op.w.topk_thresh, thresh_bytes, true);
  if (op.w.topk_thresh.p != old_thresh) op.w.topk_clean = true;
  if (!op.w.topk_clean) WX_HIP(hipMemsetAsync(op.w.topk_thresh.p, 0, thresh_bytes, op.s));
  op.w.topk_clean = false;
  a.g_thresh = static_cast<wx_u32 *>(op.w.topk_thresh.p);
  a.n_rows = t->n_rows;
  if (seed) {
    WxTopkArgs sa = a;
    sa.q_stride = P.seed_stride;
    sa.q_step = nq;  // one batch per workgroup
    launch(op.mod->fn("wx_topk_seed"), (unsigned)gs, &sa, op.s, false);
    WxTopkFinArgs sf;
    fill_cols(t, spec.cols, sf.col);
    sf.cand_k = a.cand_k;
    sf.cand_i = a.cand_i;
    sf.n_cand = gs * k;
    sf.row_base = 0;
    sf.out_keys = nullptr;
    sf.out_idx = nullptr;
    sf.out_vals = nullptr;
    sf.count_out = nullptr;
    sf.g_thresh = a.g_thresh;
    sf.seed = 1;
    void *sparams[] = {&sf};
    WX_HIP(hipModuleLaunchKernel(op.mod->fn("wx_topk_finalize"), 1, 1, 1, 1024, 1, 1, 0, op.s, sparams, nullptr));
  }
  a.q_stride = span;
  a.q_step = (int64_t)grid * span;
  launch(op.mod->fn("wx_topk_scan"), grid, &a, op.s, op.timed);
  WxTopkFinArgs f;
  fill_cols(t, spec.cols, f.col);
  f.cand_k = a.cand_k;
  f.cand_i = a.cand_i;
  f.n_cand = (wx_i64)grid * k;
  f.row_base = row_base;
  f.out_keys = d_keys;
  f.out_idx = reinterpret_cast<wx_i64 *>(d_idx);
  f.out_vals = d_vals;
  f.count_out = reinterpret_cast<wx_i64 *>(cnt);
  f.g_thresh = a.g_thresh;
  f.seed = 0;
  void *params[] = {&f};
  WX_HIP(hipModuleLaunchKernel(op.mod->fn("wx_topk_finalize"), 1, 1, 1, 1024, 1, 1, 0, op.s, params, nullptr));  // WX_FIN_BLOCK
  op.w.topk_clean = true;
  if ((L.flags & WX_F_SYNC) || h_count) check_errors(op.w);
  if (h_count) WX_HIP(hipMemcpy(h_count, cnt, 8, hipMemcpyDeviceToHost));
}

void do_topk_merge(const wx_topk_record *recs, int32_t n_records, int32_t k, int32_t desc, const wx_launch *Lp,
                   float *d_keys, int64_t *d_idx, float *d_vals, int64_t *d_count, int64_t *h_count) {
  const wx_launch L = launch_of(Lp);
  static_assert(sizeof(wx_topk_record) == WX_TOPK_REC_BYTES, "record layout");
  if (k < 1 || k > WX_TOPK_MAX) fail(WX_ERR_UNSUPPORTED, "LIMIT must be between 1 and 32");
  if (n_records < 0 || (n_records > 0 && !recs)) fail(WX_ERR_INVALID, "bad candidate records");
  if ((int64_t)n_records * k > WX_TOPK_MERGE_MAX) fail(WX_ERR_UNSUPPORTED, "n_records * k must be <= 4096");
  Op op(L, util_spec());
  int64_t *cnt = count_slot(op.w, op.w.g_ngroups, d_count, h_count != nullptr);
  WxTopkMergeArgs a;
  a.records = reinterpret_cast<const unsigned char *>(recs);
  a.n_records = n_records;
  a.k = k;
  a.descending = desc ? 1 : 0;
  a.out_keys = d_keys;
  a.out_idx = reinterpret_cast<wx_i64 *>(d_idx);
  a.out_vals = d_vals;
  a.count_out = reinterpret_cast<wx_i64 *>(cnt);
  launch(op.mod->fn("wx_topk_merge"), 1, &a, op.s, op.timed, 1024);
  read_count(op, cnt, h_count);
}

// ORDER BY .. LIMIT head of one shard (any limit): ordered compaction of the
// key (and of the SELECT expression when it differs) with shard-local rows,
// a stable key sort of the positions limited to the head, the head gathered
// into the record.
void do_order_head(const wx_table *t, const char *order_expr, const char *cond, const char *select_expr, int64_t limit,
                   int32_t desc, const wx_launch *Lp, int64_t row_base, void *d_record, int64_t cap) {
  check_table(t);
  const wx_launch L0 = launch_of(Lp);
  if (blank(order_expr)) fail(WX_ERR_INVALID, "Empty ORDER BY expression");
  if (limit < 0 || cap < limit || !d_record) fail(WX_ERR_INVALID, "head record must hold `limit` rows");
  // the passing rows' local ids are compacted as int32 (WxHeadArgs.rows)
  if (t->n_rows > INT32_MAX) fail(WX_ERR_UNSUPPORTED, "ORDER BY .. LIMIT head: a shard holds at most 2^31 - 1 rows");
  wx_launch L = L0;
  L.flags &= ~(int32_t)WX_F_TIME;
  Op op(L, util_spec());
  const size_t n = (size_t)std::max<int64_t>(1, t->n_rows);
  ensure(op.w, op.w.hd_keys, n * 4, false);
  ensure(op.w, op.w.hd_rows, n * 4, false);
  ensure(op.w, op.w.hd_idx, n * 4, false);
  ensure(op.w, op.w.hd_count, 8, false);
  const bool same = blank(select_expr) || one_line(select_expr) == one_line(order_expr);
  int64_t count = 0;
  do_project_filter(t, order_expr, cond, &L, WX_MODE_COMPACT, static_cast<float *>(op.w.hd_keys.p), op.w.hd_rows.p, 4, 0,
                    static_cast<int64_t *>(op.w.hd_count.p), &count);
  if (!same) {
    ensure(op.w, op.w.hd_vals, n * 4, false);
    int64_t c2 = 0;
    do_project_filter(t, select_expr, cond, &L, WX_MODE_COMPACT, static_cast<float *>(op.w.hd_vals.p), nullptr, 0, 0,
                      nullptr, &c2);
    if (c2 != count) fail(WX_ERR_INTERNAL, "ORDER BY rows differ from SELECT rows");
  }
  WxHeadArgs a{};
  a.n = count;
  a.idx = static_cast<wx_u32 *>(op.w.hd_idx.p);
  if (count > 0) launch(op.mod->fn("wx_iota"), grid_for(count, op.d.cus, 8), &a, op.s);
  const int64_t m = std::min(count, limit);
  if (m > 0) do_sort(op.w.hd_keys.p, static_cast<float *>(op.w.hd_idx.p), count, 0, desc ? 0 : 1, &L, m);
  a.keys = static_cast<const float *>(op.w.hd_keys.p);
  a.vals = same ? nullptr : static_cast<const float *>(op.w.hd_vals.p);
  a.rows = static_cast<const int *>(op.w.hd_rows.p);
  a.row_base = row_base;
  a.count = static_cast<const wx_i64 *>(op.w.hd_count.p);
  a.limit = limit;
  a.record = static_cast<unsigned char *>(d_record);
  a.cap = cap;
  launch(op.mod->fn("wx_head_gather"), grid_for(std::max<int64_t>(1, m), op.d.cus, 8), &a, op.s);
  WX_HIP(hipStreamSynchronize(op.s));  // synchronous (the workspace's scratch is reused by the next call)
  if (L.flags & WX_F_SYNC) check_errors(op.w);
}

void do_head_merge(const void *recs, int32_t n_records, int64_t cap, int64_t limit, int32_t desc, const wx_launch *Lp,
                   float *d_keys, int64_t *d_rows, float *d_vals, int64_t *d_count, int64_t *h_count) {
  const wx_launch L0 = launch_of(Lp);
  if (n_records < 0 || n_records > 1024 || (n_records > 0 && !recs)) fail(WX_ERR_INVALID, "bad head records");
  if (cap < 0 || limit < 0 || (int64_t)n_records * cap >= (1ll << 32)) fail(WX_ERR_INVALID, "bad head capacity");
  wx_launch L = L0;
  L.flags &= ~(int32_t)WX_F_TIME;
  Op op(L, util_spec());
  const size_t nc = (size_t)std::max<int64_t>(1, (int64_t)n_records * cap);
  ensure(op.w, op.w.hm_keys, nc * 4, false);
  ensure(op.w, op.w.hm_idx, nc * 4, false);
  ensure(op.w, op.w.hm_count, 8, false);
  WxHeadArgs a{};
  a.records = static_cast<const unsigned char *>(recs);
  a.n_records = n_records;
  a.cap = cap;
  a.cat_keys = static_cast<float *>(op.w.hm_keys.p);
  a.cat_idx = static_cast<wx_u32 *>(op.w.hm_idx.p);
  a.cat_count = static_cast<wx_i64 *>(op.w.hm_count.p);
  launch(op.mod->fn("wx_head_concat"), 1, &a, op.s, false, 1024);
  int64_t total = 0;
  WX_HIP(hipMemcpyAsync(&op.w.host_word, a.cat_count, 8, hipMemcpyDeviceToHost, op.s));
  WX_HIP(hipStreamSynchronize(op.s));
  total = (int64_t)op.w.host_word;
  const int64_t m = std::min(total, limit);
  if (m > 0) do_sort(op.w.hm_keys.p, static_cast<float *>(op.w.hm_idx.p), total, 0, desc ? 0 : 1, &L, m);
  int64_t *cnt = count_slot(op.w, op.w.count_tmp, d_count);
  a.idx = a.cat_idx;
  a.keys = a.cat_keys;
  a.count = a.cat_count;
  a.limit = limit;
  a.out_keys = d_keys;
  a.out_rows = reinterpret_cast<wx_i64 *>(d_rows);
  a.out_vals = d_vals;
  a.count_out = reinterpret_cast<wx_i64 *>(cnt);
  launch(op.mod->fn("wx_head_emit"), grid_for(std::max<int64_t>(1, m), op.d.cus, 8), &a, op.s);
  if (h_count) *h_count = m;
  WX_HIP(hipStreamSynchronize(op.s));
  if (L.flags & WX_F_SYNC) check_errors(op.w);
}

}  // namespace wx
