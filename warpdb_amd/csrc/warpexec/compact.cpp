// compact.cpp -- dense and compacting projection (wx_dense.hip,
// wx_compact.hip), the multi-output compaction (wx_select.hip,
// wx_compact_multi.hip), SUM
// (wx_sum.hip) and the type cast.
#include "wx_host.hpp"

namespace wx {

// WX_DIAG_TIMELINE builds: per-workgroup entry / first tile / first
// evaluation / end, 10 ns ticks -> us
static void print_timeline(Op &op, unsigned grid, int64_t n_tiles) {
  std::vector<wx_u64> h((size_t)grid * 16);
  WX_HIP(hipMemcpyAsync(h.data(), op.w.diag.p, h.size() * 8, hipMemcpyDeviceToHost, op.s));
  WX_HIP(hipStreamSynchronize(op.s));
  wx_u64 t0 = ~0ull;
  for (unsigned b = 0; b < grid; ++b) t0 = std::min(t0, h[(size_t)b * 16]);
  const char *names[4] = {"entry", "tickets", "eval0", "end"};
  std::fprintf(stderr, "[warpexec] timeline grid %u tiles %lld:", grid, (long long)n_tiles);
  for (int i = 0; i < 4; ++i) {
    std::vector<double> v;
    for (unsigned b = 0; b < grid; ++b) v.push_back((double)(h[(size_t)b * 16 + i] - t0) / 100.0);
    std::sort(v.begin(), v.end());
    std::fprintf(stderr, " %s min %.1f p50 %.1f max %.1f |", names[i], v.front(), v[v.size() / 2], v.back());
  }
  int64_t tmin = INT64_MAX, tmax = 0;
  for (unsigned b = 0; b < grid; ++b) {
    tmin = std::min<int64_t>(tmin, (int64_t)h[(size_t)b * 16 + 4]);
    tmax = std::max<int64_t>(tmax, (int64_t)h[(size_t)b * 16 + 4]);
  }
  std::fprintf(stderr, " tiles/wg %lld..%lld (us)\n", (long long)tmin, (long long)tmax);
}

// The launch the single- and the multi-output compaction and the window
// broadcast (window.cpp) share.  `c` is the
// WxCompactArgs inside `args`, the struct the kernels `deep_fn` / `ticket_fn`
// take; the caller has set its columns and value outputs, the rest is filled
// here.  Ends with the error check and the host count of a synchronous call.
void compact_launch(Op &op, const Spec &spec, const wx_table *t, WxCompactArgs &c, void *args, const char *deep_fn,
                    const char *ticket_fn, void *d_out_idx, int32_t idx_bytes, int64_t row_base, int64_t *d_count,
                    int64_t *h_count) {
  Workspace &w = op.w;
  // (read before anything is enqueued: a bad $WARPDB_COMPACT_GRID leaves the workspace as it was)
  const bool ticket = compact_ticket_sched();
  const int64_t grid_cap = ticket ? 0 : compact_grid_cap();
  int64_t *count_dst = count_slot(w, w.count_tmp, d_count, h_count != nullptr);
  const int64_t tile_rows = (int64_t)spec.dwaves * 64 * 4 * spec.groups;
  const int64_t n_tiles = (t->n_rows + tile_rows - 1) / tile_rows;
  w.cs_last = {0, 0, 0, 0};
  if (n_tiles == 0) {
    if (count_dst) WX_HIP(hipMemsetAsync(count_dst, 0, 8, op.s));
  } else {
    if (n_tiles > 0xffffffffll) fail(WX_ERR_INVALID, "table too large for one launch");
    // No per-query clearing: the status words carry the launch's epoch
    // (a fresh array starts at epoch 0 = all zero; one memset every 63
    // launches), and the last workgroup to retire returns the ticket to 0.
    void *old_status = w.status.p;
    ensure(w, w.status, (size_t)(n_tiles + 1) * 8, true);
    if (w.status.p != old_status) w.cs_epoch = 0;
    if (++w.cs_epoch > WX_CS_EPOCHS) {
      WX_HIP(hipMemsetAsync(w.status.p, 0, w.status.bytes, op.s));
      w.cs_epoch = 1;
    }
    c.out_idx = d_out_idx;
    c.status = static_cast<wx_u64 *>(w.status.p);
    c.ctrs = static_cast<wx_u64 *>(w.ctrs.p);
    c.count_out = reinterpret_cast<wx_i64 *>(count_dst);
    c.n_rows = t->n_rows;
    c.n_tiles = n_tiles;
    c.row_base = row_base;
    c.idx64 = idx_bytes == 8;
    c.epoch = w.cs_epoch;
    c.diag = nullptr;
    // diagnostics only, and only the single-output kernel records them
    const bool timeline = spec.more.empty() && spec.extra.find("WX_DIAG_TIMELINE") != std::string::npos;
    if (!ticket) {
      // Persistent pipelined kernel, tiles from a ticket counter: any grid
      // size is correct (a workgroup that starts late finds the tickets
      // taken and exits); one workgroup per CU at the occupancy the
      // kernel's LDS allows is what keeps every CU streaming.
      // $WARPDB_COMPACT_GRID caps the grid (diagnostic: fewer workgroups,
      // all resident, each running more tiles).
      hipFunction_t fn = op.mod->fn(deep_fn);
      int per_cu = 0, lds = 0;
      const unsigned cblock = (unsigned)(spec.dwaves + 1) * 64;
      WX_HIP(hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, cblock, 0));
      WX_HIP(hipFuncGetAttribute(&lds, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, fn));
      const int lds_limit = lds > 0 ? (160 * 1024) / lds : 64;
      const int bpc = std::max(1, std::min(per_cu, lds_limit));
      int64_t full = std::min<int64_t>(n_tiles, (int64_t)op.d.cus * bpc);
      if (grid_cap) full = std::min(full, grid_cap);
      const unsigned grid = (unsigned)full;
      w.cs_last = {tile_rows, n_tiles, (int64_t)grid, 1};
      if (std::getenv("WARPDB_DEBUG"))
        std::fprintf(stderr, "[warpexec] %s: occupancy %d/CU, lds %d B, lds_limit %d, bpc %d, grid %u, tiles %lld\n",
                     deep_fn, per_cu, lds, lds_limit, bpc, grid, (long long)n_tiles);
      if (timeline) {
        ensure(w, w.diag, (size_t)grid * 16 * 8, false);
        WX_HIP(hipMemsetAsync(w.diag.p, 0, (size_t)grid * 16 * 8, op.s));
        c.diag = static_cast<wx_u64 *>(w.diag.p);
      }
      launch(fn, grid, args, op.s, op.timed, cblock);
      if (timeline) print_timeline(op, grid, n_tiles);
    } else {
      w.cs_last = {tile_rows, n_tiles, n_tiles, 0};
      launch(op.mod->fn(ticket_fn), (unsigned)n_tiles, args, op.s, op.timed, (unsigned)spec.dwaves * 64);
    }
  }
  if ((op.L.flags & WX_F_SYNC) || h_count) check_errors(w);
  if (h_count) WX_HIP(hipMemcpy(h_count, count_dst, 8, hipMemcpyDeviceToHost));
}

void do_project_filter(const wx_table *t, const char *expr, const char *cond, const wx_launch *Lp, int32_t mode,
                       float *d_out_vals, void *d_out_idx, int32_t idx_bytes, int64_t row_base,
                       int64_t *d_count, int64_t *h_count) {
  check_table(t);
  const wx_launch L = launch_of(Lp);
  if (blank(expr)) fail(WX_ERR_INVALID, "Empty query expression");
  if (mode < WX_MODE_DENSE || mode > WX_MODE_COMPACT) fail(WX_ERR_INVALID, "unknown mode");
  if (mode == WX_MODE_COMPACT) check_row_ids(t, d_out_idx, idx_bytes, row_base);
  if (mode != WX_MODE_COMPACT && !d_out_vals && t->n_rows) fail(WX_ERR_INVALID, "null output buffer");
  // No WHERE and no row indices wanted: every row passes in order, so the
  // compacted values are the dense projection (no ballots, no look-back)
  const bool every_row = mode == WX_MODE_COMPACT && blank(cond) && !d_out_idx;
  const int kop = mode == WX_MODE_COMPACT && !every_row ? WX_OP_COMPACT : WX_OP_DENSE;
  const Spec spec = project_spec(t, kop, expr, cond, L, aligned16(d_out_vals));
  Op op(L, spec);
  if (kop == WX_OP_COMPACT) {
    WxCompactArgs a;
    fill_cols(t, spec.cols, a.col);
    a.out_val = d_out_vals;
    compact_launch(op, spec, t, a, &a, "wx_project_compact_deep", "wx_project_compact_ticket", d_out_idx, idx_bytes,
                   row_base, d_count, h_count);
    return;
  }
  if (t->n_rows > 0 && d_out_vals) {  // (no values buffer: a count-only every_row call)
    WxDenseArgs a;
    fill_cols(t, spec.cols, a.col);
    a.out = d_out_vals;
    a.n_rows = t->n_rows;
    a.fill = mode == WX_MODE_DENSE_FILL;
    // 4 quads per thread per span (WX_UNROLL), contiguous spans, 3 per CU
    const int64_t spans = ((t->n_rows + 3) / 4 + 4 * WX_BLOCK - 1) / (4 * WX_BLOCK);
    launch(op.mod->fn("wx_project_dense"), grid_for(spans * WX_BLOCK, op.d.cus, 3), &a, op.s, op.timed);
  }
  // the reference's dense contract has no count; report the row count
  // (every_row: all rows passed).  Two 32-bit fills, so nothing on the
  // stream reads from this call's (pageable) stack after it returns.
  if (d_count) {
    const uint64_t n = (uint64_t)t->n_rows;
    WX_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_count), (int)(uint32_t)n, 1, op.s));
    WX_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(reinterpret_cast<uint32_t *>(d_count) + 1),
                             (int)(uint32_t)(n >> 32), 1, op.s));
  }
  if (h_count) *h_count = t->n_rows;
  if ((L.flags & WX_F_SYNC) || h_count) check_errors(op.w);
}

// n_exprs outputs of one filtered result in one pass (wx_select.hip's hooks
// over wx_compact_multi.hip's kernels); one
// expression is the single-output call itself.  With no WHERE every row
// passes through the same kernel.
void do_project_filter_multi(const wx_table *t, const char *const *exprs, int32_t n_exprs, const char *cond,
                             const wx_launch *Lp, int32_t mode, float *const *d_out_vals, void *d_out_idx,
                             int32_t idx_bytes, int64_t row_base, int64_t *d_count, int64_t *h_count) {
  check_table(t);
  check_select_exprs(exprs, n_exprs);
  if (n_exprs == 1) {
    do_project_filter(t, exprs[0], cond, Lp, mode, d_out_vals ? d_out_vals[0] : nullptr, d_out_idx, idx_bytes,
                      row_base, d_count, h_count);
    return;
  }
  const wx_launch L = launch_of(Lp);
  if (mode < WX_MODE_DENSE || mode > WX_MODE_COMPACT) fail(WX_ERR_INVALID, "unknown mode");
  if (mode != WX_MODE_COMPACT) fail(WX_ERR_UNSUPPORTED, "more than one output needs WX_MODE_COMPACT");
  check_row_ids(t, d_out_idx, idx_bytes, row_base);
  const Spec spec = select_spec(t, exprs, n_exprs, cond, L);
  Op op(L, spec);
  // the status words and the ticket are the single-output kernel's
  WxSelectArgs a;
  fill_cols(t, spec.cols, a.c.col);
  a.c.out_val = nullptr;
  for (int j = 0; j < WX_SELECT_MAX_OUT; ++j) a.out_val[j] = j < n_exprs && d_out_vals ? d_out_vals[j] : nullptr;
  compact_launch(op, spec, t, a.c, &a, "wx_select_compact_deep", "wx_select_compact_ticket", d_out_idx, idx_bytes,
                 row_base, d_count, h_count);
}

void do_reduce_sum(const wx_table *t, const char *expr, const char *cond, const wx_launch *Lp, void *d_out,
                   double *h_sum, int64_t *h_count, bool minmax, wx_stats *h_stats) {
  check_table(t);
  const wx_launch L = launch_of(Lp);
  if (blank(expr)) fail(WX_ERR_INVALID, "Empty query expression");
  const Spec spec = sum_spec(t, expr, cond, L, minmax);
  Op op(L, spec);
  const unsigned grid = grid_for((t->n_rows + 3) / 4, op.d.cus, 8);  // profiles/r01/ablate_stream.txt
  ensure(op.w, op.w.part_sum, grid * 8, false);
  ensure(op.w, op.w.part_cnt, grid * 8, false);
  if (minmax) {
    ensure(op.w, op.w.part_min, grid * 4, false);
    ensure(op.w, op.w.part_max, grid * 4, false);
  }
  void *out = d_out;
  if (!out) {
    ensure(op.w, op.w.sum_out, sizeof(wx_stats), false);
    out = op.w.sum_out.p;
  }
  WxSumArgs a;
  fill_cols(t, spec.cols, a.col);
  a.part_sum = static_cast<double *>(op.w.part_sum.p);
  a.part_cnt = static_cast<wx_i64 *>(op.w.part_cnt.p);
  a.part_min = static_cast<wx_u32 *>(op.w.part_min.p);
  a.part_max = static_cast<wx_u32 *>(op.w.part_max.p);
  a.n_rows = t->n_rows;
  launch(op.mod->fn("wx_reduce_sum"), grid, &a, op.s, op.timed);
  WxSumFinArgs f;
  f.part_sum = a.part_sum;
  f.part_cnt = a.part_cnt;
  f.part_min = a.part_min;
  f.part_max = a.part_max;
  f.out = static_cast<double *>(out);
  f.n_parts = (int)grid;
  f.count_f64 = (L.flags & WX_F_F64_COUNTS) && d_out && !minmax ? 1 : 0;
  void *params[] = {&f};
  WX_HIP(hipModuleLaunchKernel(op.mod->fn("wx_sum_finalize"), 1, 1, 1, 1024, 1, 1, 0, op.s, params, nullptr));  // WX_SFIN_BLOCK
  if ((L.flags & WX_F_SYNC) || h_sum || h_count || h_stats) check_errors(op.w);
  if (h_sum || h_count || h_stats) {
    wx_stats host;
    WX_HIP(hipMemcpy(&host, out, minmax ? sizeof(wx_stats) : 16, hipMemcpyDeviceToHost));
    if (h_sum) *h_sum = host.sum;
    if (f.count_f64) {
      double c;
      std::memcpy(&c, &host.count, 8);
      host.count = (int64_t)c;
    }
    if (h_count) *h_count = host.count;
    if (h_stats) *h_stats = host;
  }
}

void do_cast(const void *src, int32_t sdt, void *dst, int32_t ddt, int64_t n, const wx_launch *Lp) {
  const wx_launch L = launch_of(Lp);
  if (n < 0 || (n > 0 && (!src || !dst))) fail(WX_ERR_INVALID, "bad buffer");
  if (sdt < WX_INT32 || sdt > WX_FLOAT64 || ddt < WX_INT32 || ddt > WX_FLOAT64) fail(WX_ERR_INVALID, "bad dtype");
  if (n == 0) return;
  Op op(L, util_spec());
  WxCastArgs a;
  a.src = src;
  a.dst = dst;
  a.n = n;
  a.src_dtype = sdt;
  a.dst_dtype = ddt;
  launch(op.mod->fn("wx_cast"), grid_for(n, op.d.cus, 8), &a, op.s);
  if (L.flags & WX_F_SYNC) WX_HIP(hipStreamSynchronize(op.s));
}

}  // namespace wx
