// select_ordered.cpp -- the multi-output row gather (wx_gather.hip) and the
// ordered multi-column SELECT built on it.
#include "wx_host.hpp"

namespace wx {

// n_exprs expressions at `count` row ids (wx_gather.hip), bounded on the
// device by *d_count when given.
void do_gather_multi(const wx_table *t, const char *const *exprs, int32_t n_exprs, const void *d_rows,
                     int32_t idx_bytes, int64_t row_base, int64_t count, const int64_t *d_count, const wx_launch *Lp,
                     float *const *d_out_vals, int64_t *d_out_rows, int64_t out_row_base) {
  check_gather_args(t, exprs, n_exprs, idx_bytes, count);
  if (count > 0 && !d_rows) fail(WX_ERR_INVALID, "null row id buffer");
  const wx_launch L = launch_of(Lp);
  if (count == 0) return;
  const Spec spec = gather_spec(t, exprs, n_exprs, L);
  Op op(L, spec);
  WxGatherArgs a;
  fill_cols(t, spec.cols, a.col);
  a.rows = d_rows;
  a.d_count = reinterpret_cast<const wx_i64 *>(d_count);
  for (int j = 0; j < WX_GATHER_MAX_OUT; ++j) a.out_val[j] = j < n_exprs && d_out_vals ? d_out_vals[j] : nullptr;
  a.out_rows = reinterpret_cast<wx_i64 *>(d_out_rows);
  a.count = count;
  a.n_rows = t->n_rows;
  a.row_base = row_base;
  a.out_row_base = out_row_base;
  a.idx64 = idx_bytes == 8;
  // every CU full of waves (2048 threads): a random gather lives on the
  // number of independent misses in flight
  const int64_t tile = (int64_t)spec.gblock * 4 * spec.gunroll;
  const int64_t tiles = (count + tile - 1) / tile;
  const unsigned grid = (unsigned)std::min<int64_t>(tiles, (int64_t)op.d.cus * std::max(1, 2048 / spec.gblock));
  launch(op.mod->fn("wx_select_gather"), grid, &a, op.s, op.timed, (unsigned)spec.gblock);
  if (L.flags & WX_F_SYNC) check_errors(op.w);
}

// ORDER BY order_expr [DESC] [LIMIT] over a multi-column SELECT: the sorted
// row ids once (top-K scan, or key compaction + stable pair sort with the
// row ids as the payload), then the expressions gathered at those rows in
// chunks of WX_MAX_OUTPUTS.
void do_select_ordered(const wx_table *t, const char *const *exprs, int32_t n_exprs, const char *cond,
                       const char *order_expr, int32_t desc, int64_t limit, const wx_launch *Lp, int64_t row_base,
                       float *const *d_out_vals, float *d_out_keys, int64_t *d_out_rows, int64_t capacity,
                       int64_t *d_count, int64_t *h_count) {
  check_table(t);
  if (n_exprs < 0 || n_exprs > WX_ORDERED_MAX_EXPRS || (n_exprs > 0 && !exprs))
    fail(WX_ERR_INVALID, "n_exprs must be between 0 and " + std::to_string(WX_ORDERED_MAX_EXPRS));
  for (int32_t j = 0; j < n_exprs; ++j)
    if (blank(exprs[j])) fail(WX_ERR_INVALID, "Empty query expression");
  if (blank(order_expr)) fail(WX_ERR_INVALID, "Empty ORDER BY expression");
  if (capacity < 0) fail(WX_ERR_INVALID, "negative output capacity");
  if (limit < 0) limit = INT64_MAX;
  const wx_launch L0 = launch_of(Lp);
  if (limit == 0 || t->n_rows == 0) {  // nothing to order: no launch, no workspace
    DevGuard g(L0.device);
    if (d_count) WX_HIP(hipMemsetAsync(d_count, 0, 8, static_cast<hipStream_t>(L0.stream)));
    if (h_count) *h_count = 0;
    return;
  }
  Op op(L0);
  wx_launch L = L0;  // the inner calls: no per-call sync, no timing of a part
  L.flags &= ~(uint32_t)(WX_F_TIME | WX_F_SYNC);
  // the expressions at the rows, four at a time (chunks with no output wanted are skipped)
  auto gather = [&](const void *rows, int32_t idx_bytes, int64_t rows_base, int64_t count, const int64_t *dc,
                    int64_t *out_rows) {
    bool rows_done = out_rows == nullptr;
    for (int32_t c = 0; c < n_exprs; c += WX_MAX_OUTPUTS) {
      const int32_t m = std::min<int32_t>(WX_MAX_OUTPUTS, n_exprs - c);
      bool any = false;
      for (int32_t j = 0; j < m; ++j) any = any || (d_out_vals && d_out_vals[c + j]);
      if (!any) continue;
      do_gather_multi(t, exprs + c, m, rows, idx_bytes, rows_base, count, dc, &L, d_out_vals + c,
                      rows_done ? nullptr : out_rows, row_base);
      rows_done = true;
    }
    if (!rows_done) {  // rows only: a constant expression reads no column
      const char *none[1] = {"0.0f"};
      do_gather_multi(t, none, 1, rows, idx_bytes, rows_base, count, dc, &L, nullptr, out_rows, row_base);
    }
  };
  const bool topk_route = limit <= WX_TOPK_MAX && env_or("WARPDB_ORDERED_ROUTE", "auto") != "sort";
  if (topk_route) {
    // keys, global rows and the device count from one scan; a caller whose
    // buffers could be too short gets them through the workspace, after a
    // host read of the count
    const bool direct = capacity >= limit;
    ensure(op.w, op.w.so_keys, WX_TOPK_MAX * 4, false);
    ensure(op.w, op.w.so_rows, WX_TOPK_MAX * 8, false);
    ensure(op.w, op.w.so_cnt, 8, false);
    float *keys = direct ? d_out_keys : static_cast<float *>(op.w.so_keys.p);
    int64_t *rows = direct && d_out_rows ? d_out_rows : static_cast<int64_t *>(op.w.so_rows.p);
    int64_t *cnt = d_count ? d_count : static_cast<int64_t *>(op.w.so_cnt.p);
    int64_t count = 0;
    do_topk(t, order_expr, cond, nullptr, (int32_t)limit, desc, &L, row_base, keys, rows, nullptr, cnt,
            direct ? nullptr : &count);
    if (!direct) {
      if (count > capacity) {
        if (h_count) *h_count = count;
        fail(WX_ERR_CAPACITY, "ordered SELECT: the result holds " + std::to_string(count) + " rows, capacity is " +
                                  std::to_string(capacity));
      }
      if (d_out_keys && count) WX_HIP(hipMemcpyAsync(d_out_keys, keys, (size_t)count * 4, hipMemcpyDeviceToDevice, op.s));
      if (d_out_rows && count) WX_HIP(hipMemcpyAsync(d_out_rows, rows, (size_t)count * 8, hipMemcpyDeviceToDevice, op.s));
    }
    gather(rows, 8, row_base, direct ? limit : count, cnt, nullptr);
    if ((L0.flags & WX_F_SYNC) || h_count) check_errors(op.w);
    if (h_count) WX_HIP(hipMemcpy(h_count, cnt, 8, hipMemcpyDeviceToHost));
    return;
  }
  // the passing rows' local ids are compacted as int32 and sorted as the key's 4-byte payload
  if (t->n_rows > INT32_MAX) fail(WX_ERR_UNSUPPORTED, "ordered SELECT: a table holds at most 2^31 - 1 rows");
  const size_t n = (size_t)std::max<int64_t>(1, t->n_rows);
  ensure(op.w, op.w.hd_keys, n * 4, false);
  ensure(op.w, op.w.hd_rows, n * 4, false);
  ensure(op.w, op.w.hd_count, 8, false);
  int64_t count = 0;
  do_project_filter(t, order_expr, cond, &L, WX_MODE_COMPACT, static_cast<float *>(op.w.hd_keys.p), op.w.hd_rows.p, 4, 0,
                    static_cast<int64_t *>(op.w.hd_count.p), &count);
  const int64_t m = std::min(count, limit);
  if (m > capacity) {
    if (h_count) *h_count = m;
    fail(WX_ERR_CAPACITY, "ordered SELECT: the result holds " + std::to_string(m) + " rows, capacity is " +
                              std::to_string(capacity));
  }
  if (m > 0) {
    do_sort(op.w.hd_keys.p, static_cast<float *>(op.w.hd_rows.p), count, 0, desc ? 0 : 1, &L, m);
    if (d_out_keys) WX_HIP(hipMemcpyAsync(d_out_keys, op.w.hd_keys.p, (size_t)m * 4, hipMemcpyDeviceToDevice, op.s));
    gather(op.w.hd_rows.p, 4, 0, m, nullptr, d_out_rows);
  }
  if (d_count) WX_HIP(hipMemcpyAsync(d_count, &m, 8, hipMemcpyHostToDevice, op.s));
  WX_HIP(hipStreamSynchronize(op.s));  // synchronous (the workspace's scratch is reused by the next call; &m)
  if (L0.flags & WX_F_SYNC) check_errors(op.w);
  if (h_count) *h_count = m;
}

}  // namespace wx
