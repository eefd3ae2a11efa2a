// join.cpp -- the PK-FK equi-join (wx_join.hip): the right table's key range
// (wx_join_range), its direct or hash table (wx_join_build), then one
// probing compaction per chunk of WX_MAX_OUTPUTS outputs.
#include "wx_host.hpp"

namespace wx {

namespace {
// Every launch of a call: outputs [first, first + n); the first launch alone
// writes the row ids, the right rows and the count.
struct Chunk {
  int32_t first = 0, n = 0;
};
std::vector<Chunk> join_chunks(int32_t n_exprs) {
  std::vector<Chunk> c;
  for (int32_t first = 0; first < n_exprs; first += WX_MAX_OUTPUTS)
    c.push_back({first, std::min<int32_t>(WX_MAX_OUTPUTS, n_exprs - first)});
  return c;
}

// The build's record after everything enqueued so far: one copy, and the
// synchronisation that also reads the error words.
void read_record(Workspace &w, hipStream_t s) {
  WX_HIP(hipMemcpyAsync(w.jn_host, w.jn_rec.p, sizeof(w.jn_host), hipMemcpyDeviceToHost, s));
  check_errors(w);
}
}  // namespace

// Phases 1 and 2 of every join call, in the workspace of `op`.
JoinTable build_join_table(Op &op, const int *d_rkeys, int64_t n_right) {
  Workspace &w = op.w;
  // ---- phase 1: the key range, read with one synchronisation; the span decides the form
  ensure(w, w.jn_rec, WX_JOIN_REC_WORDS * 4, false);
  wx_u32 *d_rec = static_cast<wx_u32 *>(w.jn_rec.p);
  JoinPlan plan = join_plan(0, 0, 0);
  int32_t key_lo = 0;
  int64_t span = 0;
  if (n_right > 0) {
    // every fill is ordered on the workspace's stream, like the kernels that read it
    WX_HIP(hipMemsetAsync(d_rec, 0xff, 8, op.s));
    WX_HIP(hipMemsetAsync(d_rec + 2, 0, (WX_JOIN_REC_WORDS - 2) * 4, op.s));
    WxJoinRangeArgs ra;
    ra.keys = d_rkeys;
    ra.n_right = n_right;
    ra.rec = d_rec;
    launch(op.mod->fn("wx_join_range"), grid_for((n_right + 3) / 4, op.d.cus, 4), &ra, op.s, false, WX_JOIN_BLOCK);
    read_record(w, op.s);
    const int64_t seen = (int64_t)(((uint64_t)w.jn_host[5] << 32) | w.jn_host[4]);
    if (seen != n_right) fail(WX_ERR_INTERNAL, "JOIN: the key range record was not written");
    key_lo = (int32_t)(w.jn_host[0] ^ 0x80000000u);
    const int32_t key_hi = (int32_t)(~w.jn_host[1] ^ 0x80000000u);
    if (key_lo > key_hi) fail(WX_ERR_INTERNAL, "JOIN: bad key range");
    span = (int64_t)key_hi - key_lo + 1;
    plan = join_plan(n_right, key_lo, key_hi);
  }
  const bool direct = plan.form == WX_JOIN_FORM_DIRECT;
  // ---- phase 2: the table (rows of -1, or slots of all-ones), built by vector atomics
  const size_t slots = direct ? 0 : (size_t)1 << plan.log2cap;
  if (direct) {
    ensure(w, w.jn_rows, WX_JOIN_TABLE_BYTES, false);
    WX_HIP(hipMemsetAsync(w.jn_rows.p, 0xff, WX_JOIN_TABLE_BYTES, op.s));
  } else {
    ensure(w, w.jn_slots, slots * 8, false);
    WX_HIP(hipMemsetAsync(w.jn_slots.p, 0xff, slots * 8, op.s));
  }
  if (n_right > 0) {
    WxJoinBuildArgs ba{};
    ba.keys = d_rkeys;
    ba.n_right = n_right;
    ba.rows = static_cast<int *>(w.jn_rows.p);
    ba.slots = static_cast<wx_u64 *>(w.jn_slots.p);
    ba.rec = d_rec;
    ba.ctrs = static_cast<wx_u64 *>(w.ctrs.p);
    ba.key_lo = key_lo;
    ba.span = direct ? (wx_u32)span : 0u;
    ba.log2cap = direct ? WX_JOIN_MIN_LOG2CAP : plan.log2cap;
    ba.form = plan.form;
    launch(op.mod->fn("wx_join_build"), grid_for((n_right + 3) / 4, op.d.cus, 4), &ba, op.s, false, WX_JOIN_BLOCK);
    read_record(w, op.s);
    if (w.jn_host[2])
      fail(WX_ERR_UNSUPPORTED,
           "JOIN: the right key is not unique (key " + std::to_string((int32_t)w.jn_host[3]) + ")");
  }
  JoinTable jt;
  jt.plan = plan;
  jt.key_lo = key_lo;
  jt.span = direct ? (wx_u32)span : 0u;
  jt.mask = direct ? 0u : (wx_u32)(slots - 1);
  jt.shift = direct ? 0 : 32 - plan.log2cap;
  return jt;
}

void do_prepare_join(const wx_table *left, const wx_table *right, const char *left_key_expr, const char *right_key_col,
                     int32_t join_type, const char *const *exprs, int32_t n_exprs, const char *cond,
                     const wx_launch *Lp, int32_t with_right_row, int32_t form) {
  (void)check_join_args(left, right, left_key_expr, right_key_col, join_type, exprs, n_exprs, cond);
  if (form != WX_JOIN_FORM_DIRECT && form != WX_JOIN_FORM_HASH)
    fail(WX_ERR_INVALID, "form must be 0 (direct) or 1 (hash)");
  const wx_launch L = launch_of(Lp);
  prepare_module(L, join_table_spec());
  for (const Chunk &k : join_chunks(n_exprs))
    prepare_module(L, join_spec(left, right, exprs + k.first, k.n, form, join_type == WX_JOIN_LEFT,
                                with_right_row && k.first == 0, left_key_expr, cond, L));
}

void do_join_select(const wx_table *left, const wx_table *right, const char *left_key_expr, const char *right_key_col,
                    int32_t join_type, const char *const *exprs, int32_t n_exprs, const char *cond,
                    const wx_launch *Lp, float *const *d_out_vals, void *d_out_idx, int32_t idx_bytes,
                    int64_t row_base, int32_t *d_out_right_row, int64_t *d_count, int64_t *h_count) {
  const JoinNames names = check_join_args(left, right, left_key_expr, right_key_col, join_type, exprs, n_exprs, cond);
  const wx_launch L = launch_of(Lp);
  if (L.flags & WX_F_ROW_ORDER) fail(WX_ERR_UNSUPPORTED, "row-order sums are not available for joins");
  check_row_ids(left, d_out_idx, idx_bytes, row_base);
  const int64_t n_right = right->n_rows;
  const int *d_rkeys = static_cast<const int *>(right->cols[names.right_key].d_ptr);

  Op op(L, join_table_spec());  // held over the phases: the record and the table are the workspace's
  Workspace &w = op.w;
  const JoinTable jt = build_join_table(op, d_rkeys, n_right);  // phases 1 and 2
  const JoinPlan &plan = jt.plan;
  // ---- phase 3: the probing compactions
  bool first = true;
  for (const Chunk &k : join_chunks(n_exprs)) {
    const bool rrow = first && d_out_right_row != nullptr;
    const Spec spec = join_spec(left, right, exprs + k.first, k.n, plan.form, join_type == WX_JOIN_LEFT, rrow,
                                left_key_expr, cond, L);
    Op cop(L, spec);
    WxJoinArgs a{};
    fill_cols(left, spec.cols, a.c.col);
    a.c.out_val = nullptr;
    for (int32_t j = 0; j < k.n; ++j) a.out_val[j] = d_out_vals ? d_out_vals[k.first + j] : nullptr;
    if (rrow) a.out_val[k.n] = reinterpret_cast<float *>(d_out_right_row);
    fill_cols(right, spec.rcols, a.rcol);
    if (n_right == 0)  // nothing ever hits, so nothing is read: any valid address
      for (size_t i = 0; i < spec.rcols.size(); ++i) a.rcol[i] = w.jn_slots.p;
    a.rows = static_cast<const int *>(w.jn_rows.p);
    a.slots = static_cast<const wx_u64 *>(w.jn_slots.p);
    a.key_lo = jt.key_lo;
    a.span = jt.span;
    a.mask = jt.mask;
    a.shift = jt.shift;
    compact_launch(cop, spec, left, a.c, &a, "wx_join_compact_deep", "wx_join_compact_ticket",
                   first ? d_out_idx : nullptr, idx_bytes, row_base, first ? d_count : nullptr,
                   first ? h_count : nullptr);
    first = false;
  }
  // (compact_launch ends a synchronous launch with the check; a later launch of a call that only asked for
  // the host count has not been checked yet)
  if (n_exprs > WX_MAX_OUTPUTS && h_count && !(L.flags & WX_F_SYNC)) check_errors(w);
}

}  // namespace wx
