// window.cpp -- window aggregates, AGG(x) OVER (PARTITION BY k) beside plain
// expressions (wx_window.hip): one grouped pass over the distinct values
// (wx_group_agg_multi into workspace scratch), the per-item f32 planes
// (wx_window_table), then one broadcast compaction per chunk of
// WX_MAX_OUTPUTS outputs.
#include "wx_host.hpp"

namespace wx {

namespace {
// The distinct value expressions of the items (by their one-line text), which
// of them need a sum and which a MIN / MAX, and each item's value.  A COUNT
// counts the partition's rows whatever it names: it takes no value of its
// own unless nothing else is aggregated (the group pass needs one).
struct WindowValues {
  std::vector<std::string> text;
  int sum_mask = 0, mm_mask = 0;
  int of_item[WX_WIN_MAX_ITEMS] = {};
};

WindowValues window_values(const wx_window_item *items, int32_t n_items) {
  WindowValues v;
  for (int32_t j = 0; j < n_items; ++j) {
    if (items[j].agg == WX_WIN_COUNT) continue;
    const std::string e = one_line(items[j].val_expr);
    size_t s = std::find(v.text.begin(), v.text.end(), e) - v.text.begin();
    if (s == v.text.size()) v.text.push_back(e);
    v.of_item[j] = (int)s;
    if (items[j].agg == WX_WIN_MIN || items[j].agg == WX_WIN_MAX) v.mm_mask |= 1 << s;
    else v.sum_mask |= 1 << s;
  }
  if (v.text.size() > WX_GROUP_MAX_VALUES)
    fail(WX_ERR_INVALID, "window items name " + std::to_string(v.text.size()) +
                             " distinct value expressions, at most " + std::to_string(WX_GROUP_MAX_VALUES) +
                             " are supported");
  if (v.text.empty()) {  // COUNTs only
    v.text.push_back(one_line(items[0].val_expr));
    v.sum_mask = 1;
  }
  return v;
}

// The launches of a call: outputs [first, first + n) of (plain expressions,
// then window items), at most WX_MAX_OUTPUTS each.
struct Chunk {
  int32_t first = 0, n = 0;
  int mask = 0;  // bit j: output first + j is a window item
};
std::vector<Chunk> window_chunks(int32_t n_exprs, int32_t n_items) {
  std::vector<Chunk> c;
  for (int32_t first = 0; first < n_exprs + n_items; first += WX_MAX_OUTPUTS) {
    Chunk k;
    k.first = first;
    k.n = std::min<int32_t>(WX_MAX_OUTPUTS, n_exprs + n_items - first);
    for (int32_t j = 0; j < k.n; ++j)
      if (first + j >= n_exprs) k.mask |= 1 << j;
    c.push_back(k);
  }
  return c;
}

Spec chunk_spec(const wx_table *t, const Chunk &k, const char *const *exprs, bool search, const char *part_expr,
                const char *cond, const wx_launch &L) {
  const char *ex[WX_MAX_OUTPUTS] = {};
  for (int32_t j = 0; j < k.n; ++j)
    if (!((k.mask >> j) & 1)) ex[j] = exprs[k.first + j];
  return window_spec(t, ex, k.n, k.mask, search, part_expr, cond, L);
}
}  // namespace

void do_prepare_window(const wx_table *t, const char *const *exprs, int32_t n_exprs, const wx_window_item *items,
                       int32_t n_items, const char *part_expr, const char *cond, const wx_launch *Lp, int32_t search) {
  check_window_args(t, exprs, n_exprs, items, n_items, part_expr, cond);
  const WindowValues v = window_values(items, n_items);
  const wx_launch L = launch_of(Lp);
  // the group pass's module, the table module, then every launch of the broadcast
  prepare_module(L, window_table_spec());
  std::vector<const char *> vals;
  for (const auto &e : v.text) vals.push_back(e.c_str());
  if (vals.size() == 1) prepare_module(L, group_spec(t, vals[0], part_expr, cond, L, v.mm_mask != 0));
  else prepare_module(L, group_multi_spec(t, vals.data(), (int32_t)vals.size(), v.sum_mask, v.mm_mask, part_expr, cond, L));
  for (const Chunk &k : window_chunks(n_exprs, n_items)) {
    if (k.mask) prepare_module(L, chunk_spec(t, k, exprs, search != 0, part_expr, cond, L));
    else if (k.n == 1) prepare_module(L, project_spec(t, WX_OP_COMPACT, exprs[k.first], cond, L, true));
    else prepare_module(L, select_spec(t, exprs + k.first, k.n, cond, L));
  }
}

void do_window_select(const wx_table *t, const char *const *exprs, int32_t n_exprs, const wx_window_item *items,
                      int32_t n_items, const char *part_expr, const char *cond, const wx_launch *Lp, int32_t key_lo,
                      int64_t group_capacity, float *const *d_out_vals, void *d_out_idx, int32_t idx_bytes,
                      int64_t row_base, int64_t *d_count, int64_t *h_count) {
  check_window_args(t, exprs, n_exprs, items, n_items, part_expr, cond);
  const WindowValues v = window_values(items, n_items);
  const wx_launch L = launch_of(Lp);
  if (L.flags & WX_F_ROW_ORDER)
    fail(WX_ERR_UNSUPPORTED, "row-order sums are not available for window aggregates");
  check_row_ids(t, d_out_idx, idx_bytes, row_base);
  if (group_capacity < 1) fail(WX_ERR_INVALID, "group_capacity must be at least 1");
  if (group_capacity > INT32_MAX) fail(WX_ERR_INVALID, "group_capacity exceeds the int32 key space");
  if ((int64_t)key_lo + WX_GROUP_WINDOW - 1 > INT32_MAX) fail(WX_ERR_INVALID, "key window out of range");
  const int n_vals = (int)v.text.size();
  const size_t cap = (size_t)group_capacity;

  const Spec tspec = window_table_spec();
  Op op(L, tspec);  // held over the phases: the scratch groups and planes are the workspace's
  Workspace &w = op.w;
  // ---- phase 1: the partitions' aggregates, in workspace scratch
  ensure(w, w.wn_keys, cap * 4, false);
  ensure(w, w.wn_cnts, cap * 8, false);
  ensure(w, w.wn_ng, 32, false);  // [0] the group pass's count, [1..2] wx_window_range's record
  const char *vals[WX_GROUP_MAX_VALUES] = {};
  double *sums[WX_GROUP_MAX_VALUES] = {};
  float *mins[WX_GROUP_MAX_VALUES] = {}, *maxs[WX_GROUP_MAX_VALUES] = {};
  for (int s = 0; s < n_vals; ++s) {
    vals[s] = v.text[(size_t)s].c_str();
    if ((v.sum_mask >> s) & 1) {
      ensure(w, w.wn_sums[s], cap * 8, false);
      sums[s] = static_cast<double *>(w.wn_sums[s].p);
    }
    if ((v.mm_mask >> s) & 1) {
      ensure(w, w.wn_mins[s], cap * 4, false);
      ensure(w, w.wn_maxs[s], cap * 4, false);
      mins[s] = static_cast<float *>(w.wn_mins[s].p);
      maxs[s] = static_cast<float *>(w.wn_maxs[s].p);
    }
  }
  int32_t *d_keys = static_cast<int32_t *>(w.wn_keys.p);
  int64_t *d_cnts = static_cast<int64_t *>(w.wn_cnts.p);
  wx_launch GL = L;  // asynchronous; WX_F_TIME times the broadcast pass alone
  GL.flags &= ~(WX_F_TIME | WX_F_SYNC);
  int64_t *d_ng = static_cast<int64_t *>(w.wn_ng.p);
  do_group_multi(t, vals, n_vals, part_expr, cond, &GL, key_lo, group_capacity, d_keys, sums, d_cnts, mins, maxs, d_ng,
                 nullptr);
  // ---- the one host read between the phases: {group count, first key, last
  // key}, gathered on the device and fetched by the synchronisation that
  // also reads the error words.  The span decides the form (at most
  // WX_WIN_BINS keys: the dense table).
  WxWindowRangeArgs ra;
  ra.n_groups = reinterpret_cast<const wx_i64 *>(d_ng);
  ra.keys = d_keys;
  ra.capacity = group_capacity;
  ra.out = reinterpret_cast<wx_i64 *>(d_ng + 1);
  launch(op.mod->fn("wx_window_range"), 1, &ra, op.s, false, 64);
  WX_HIP(hipMemcpyAsync(w.wn_range, d_ng + 1, 16, hipMemcpyDeviceToHost, op.s));
  try {
    check_errors(w);  // one stream synchronisation: the record has landed when it returns or throws
  } catch (const WxError &e) {
    if (e.st == WX_ERR_CAPACITY)
      fail(WX_ERR_CAPACITY, "window partitions: " + std::to_string(w.wn_range[0]) + " found, group_capacity is " +
                                std::to_string(group_capacity));
    throw;
  }
  const int64_t n_groups = w.wn_range[0];
  if (n_groups < 0 || n_groups > group_capacity) fail(WX_ERR_INTERNAL, "window partitions: bad group count");
  int64_t lo = 0, span = 0;
  if (n_groups > 0) {
    int32_t ends[2];
    std::memcpy(ends, &w.wn_range[1], 8);
    lo = ends[0];
    span = (int64_t)ends[1] - lo + 1;
    if (span < n_groups) fail(WX_ERR_INTERNAL, "window partitions: keys are not ascending");
  }
  const std::string form = env_or("WARPDB_WINDOW_FORM", "auto");  // test hook: "search" forces the search form
  const bool search = span > WX_WIN_BINS || form == "search";
  // ---- phase 2: the planes
  const int64_t stride = search ? std::max<int64_t>(n_groups, 1) : WX_WIN_BINS;
  ensure(w, w.wn_planes, (size_t)n_items * (size_t)stride * 4, false);
  float *planes = static_cast<float *>(w.wn_planes.p);
  const std::vector<Chunk> chunks = window_chunks(n_exprs, n_items);
  bool table_done = false;
  bool first = true;
  for (const Chunk &k : chunks) {
    float *out[WX_MAX_OUTPUTS] = {};
    for (int32_t j = 0; j < k.n; ++j) out[j] = d_out_vals ? d_out_vals[k.first + j] : nullptr;
    void *idx = first ? d_out_idx : nullptr;
    int64_t *dc = first ? d_count : nullptr, *hc = first ? h_count : nullptr;
    first = false;
    if (!k.mask) {  // plain expressions only: the select module
      do_project_filter_multi(t, exprs + k.first, k.n, cond, &L, WX_MODE_COMPACT, out, idx, idx_bytes, row_base, dc,
                              hc);
      continue;
    }
    const Spec spec = chunk_spec(t, k, exprs, search, part_expr, cond, L);
    Op cop(L, spec);
    if (!table_done) {
      WxWindowTableArgs ta{};
      ta.keys = d_keys;
      ta.counts = reinterpret_cast<const wx_i64 *>(d_cnts);
      for (int s = 0; s < n_vals; ++s) {
        ta.sums[s] = sums[s];
        ta.mins[s] = mins[s];
        ta.maxs[s] = maxs[s];
      }
      ta.planes = planes;
      ta.n_groups = n_groups;
      ta.stride = stride;
      ta.key_lo = (int)lo;
      ta.span = search ? 0u : (wx_u32)span;
      ta.search = search ? 1 : 0;
      ta.n_items = n_items;
      for (int32_t j = 0; j < n_items; ++j) {
        ta.agg[j] = (signed char)items[j].agg;
        ta.val[j] = (signed char)v.of_item[j];
      }
      const unsigned grid = search ? grid_for((n_groups + 3) / 4, cop.d.cus, 4) : 1u;
      launch(op.mod->fn("wx_window_table"), grid, &ta, op.s, false, WX_WIN_TBLOCK);
      table_done = true;
    }
    WxWindowArgs a{};
    fill_cols(t, spec.cols, a.c.col);
    a.c.out_val = nullptr;
    for (int32_t j = 0; j < k.n; ++j) {
      a.out_val[j] = out[j];
      if ((k.mask >> j) & 1) a.plane[j] = planes + (size_t)(k.first + j - n_exprs) * (size_t)stride;
    }
    a.keys = d_keys;
    a.key_lo = (int)lo;
    a.span = search ? 0u : (wx_u32)span;
    a.n_groups = search ? (wx_u32)n_groups : 0u;
    compact_launch(cop, spec, t, a.c, &a, "wx_window_compact_deep", "wx_window_compact_ticket", idx, idx_bytes,
                   row_base, dc, hc);
  }
  if ((L.flags & WX_F_SYNC) || h_count) check_errors(w);
}

}  // namespace wx
