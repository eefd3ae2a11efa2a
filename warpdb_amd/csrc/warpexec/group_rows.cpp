// group_rows.cpp -- GROUP BY with each group's sum folded in row order
// (WX_F_ROW_ORDER): the key-span routes (wx_group_rows.hip) and the general
// sort + fold route (wx_util.hip).
#include "wx_host.hpp"

#include <cerrno>

namespace wx {

// Row-order GROUP BY when the groups' keys span at most 2048 values
// (wx_group_rows.hip): per-range bin counts straight from the table, their
// totals / bases / per-range offsets, one stable counting scatter of the
// passing rows' values into key-major row-ordered segments, one wave per
// group folding its segment.  No compaction, no key bits, no radix pass.
// Groups of more than WX_XF_BIG rows are folded in WX_XF_CHUNK-value chunks
// by wx_xf_big_* (wx_util.hip) instead of one wave each; launches them and
// returns the count the per-group fold skips above (0: no such group).  The
// groups' segments follow each other in group order (key-major values).
int64_t xf_big_groups(Module *umod, const float *svals, const int64_t *d_counts, int64_t ng, int64_t passing,
                      double *d_sums, Workspace &w, hipStream_t s, bool timed) {
  // $WARPDB_XF_BIG: "0" off, unset / "1" the default threshold, else the
  // threshold in rows (at least one chunk)
  const std::string xb = env_or("WARPDB_XF_BIG", "1");
  if (xb == "0") return 0;
  const int64_t big = xb == "1" ? (int64_t)WX_XF_BIG : std::max<int64_t>(std::atoll(xb.c_str()), WX_XF_CHUNK);
  if (passing <= big || ng < 1 || ng > (1 << 20)) return 0;
  std::vector<int64_t> hc((size_t)ng);
  WX_HIP(hipMemcpyAsync(hc.data(), d_counts, (size_t)ng * 8, hipMemcpyDeviceToHost, s));
  WX_HIP(hipStreamSynchronize(s));
  w.xf_host.clear();
  int64_t start = 0, chunks = 0;
  for (int64_t g = 0; g < ng; ++g) {
    if (hc[g] > big) {
      w.xf_host.insert(w.xf_host.end(), {g, start, hc[g], chunks});
      chunks += (hc[g] + WX_XF_CHUNK - 1) / WX_XF_CHUNK;
    }
    start += hc[g];
  }
  if (w.xf_host.empty()) return 0;
  const int n_ent = (int)(w.xf_host.size() / 4);
  w.ro_last.big_groups = n_ent;
  w.ro_last.big_chunks = chunks;
  ensure(w, w.xf_ent, w.xf_host.size() * 8, false);
  ensure(w, w.xf_approx, (size_t)chunks * 8, false);
  ensure(w, w.xf_rec, (size_t)chunks * 64, false);
  WX_HIP(hipMemcpyAsync(w.xf_ent.p, w.xf_host.data(), w.xf_host.size() * 8, hipMemcpyHostToDevice, s));
  WxXfBigArgs x{};
  x.svals = svals;
  x.ent = static_cast<const wx_i64 *>(w.xf_ent.p);
  x.n_ent = n_ent;
  x.n_chunks = chunks;
  x.approx = static_cast<double *>(w.xf_approx.p);
  x.rec = static_cast<double *>(w.xf_rec.p);
  x.out_sums = d_sums;
  const unsigned cg = (unsigned)std::min<int64_t>(chunks, 4096);
  launch(umod->fn("wx_xf_big_approx"), cg, &x, s, timed, 64);
  launch(umod->fn("wx_xf_big_exact"), cg, &x, s, timed, 64);
  launch(umod->fn("wx_xf_big_combine"), (unsigned)n_ent, &x, s, timed, 64);
  return big;
}

// The span path's tail, once the bins' totals are in ro_tot and their
// exclusive prefix in ro_tot + 2048: each range's first slot of every bin,
// the stable counting scatter of the passing values into key-major order,
// and the exact row-order fold of every group's segment.
void ro_scatter_fold(Module *gmod, Module *umod, WxRoArgs &a, int64_t passing, const int64_t *d_counts, int64_t ng,
                     double *d_sums, Workspace &w, hipStream_t s, bool timed) {
  if (passing > 0xffffffffll)  // counts, offsets and scatter positions are 32-bit
    fail(WX_ERR_UNSUPPORTED, "row-order sums over a key span take at most 2^32 - 1 passing rows");
  // the key-major copy (4 B per passing row) stays in the workspace, as the
  // radix sort's ping-pong buffer does (a 4 GB hipMalloc per query cost ms)
  ensure(w, w.ro_vals, (size_t)std::max<int64_t>(1, passing) * 4, false);
  a.out = static_cast<float *>(w.ro_vals.p);
  WxRoScanArgs sc{};
  sc.cnt = a.cnt;
  sc.ranges = a.ranges;
  sc.base = static_cast<wx_u32 *>(w.ro_tot.p) + 2048;
  sc.off = static_cast<wx_u32 *>(w.ro_off.p);
  launch(umod->fn("wx_ro_scan"), 32, &sc, s, timed, 256);
  launch(gmod->fn("wx_ro_scatter"), (unsigned)a.ranges, &a, s, timed, WX_RO_THREADS);
  WxRoFoldArgs f{};
  f.svals = a.out;
  f.gcounts = reinterpret_cast<const wx_i64 *>(d_counts);
  f.n_groups = ng;
  f.out_sums = d_sums;
  f.skip_above = xf_big_groups(umod, a.out, d_counts, ng, passing, d_sums, w, s, timed);
  launch(umod->fn("wx_ro_fold"), (unsigned)std::min<int64_t>(ng, 1 << 20), &f, s, timed, 64);
}

// $WARPDB_RO_RANGES=<n>: a diagnostic cap on the span path's ranges (a test
// hook: few workgroups run many tiles each, so small tables reach the
// scatter's cross-tile state); 0 when unset.
int64_t ro_ranges_cap() {
  const std::string v = env_or("WARPDB_RO_RANGES", "");
  if (v.empty()) return 0;
  char *end = nullptr;
  errno = 0;
  const long long n = std::strtoll(v.c_str(), &end, 10);
  if (errno || end == v.c_str() || *end || n < 1)
    fail(WX_ERR_INVALID, "WARPDB_RO_RANGES must be an integer >= 1, not '" + v + "'");
  return n;
}

// count arguments of the span path over [kmin, kmin + span)
// the call's record, written once its route has finished (a call that fails
// leaves the zeroed record of do_group_sum_rows)
void ro_done(Workspace &w, int route, const float *vals, int64_t n_values) {
  w.ro_last.route = route;
  w.ro_last.n_values = n_values;
  w.ro_last_vals = vals;
}

WxRoArgs ro_args(const wx_table *t, const Spec &spec, DeviceState &d, int32_t kmin, int span, Workspace &w) {
  const int64_t n = t->n_rows;
  const int64_t tiles = (n + WX_RO_TILE_ROWS - 1) / WX_RO_TILE_ROWS;
  // two 512-thread workgroups per CU (72 KB of LDS each), one range each:
  // one workgroup per CU (LDS-padded) 13.6 vs 12.4 ms per query,
  // nontemporal value stores 15.4, 16 384-row tiles at one workgroup per CU
  // 12.9 vs 12.9 (their runs halve the written bytes, 7.56 -> 5.76 GB, and
  // the time stays; profiles/r05/ro_scatter_ab.txt)
  int ranges = (int)std::max<int64_t>(1, std::min<int64_t>(tiles, 2ll * d.cus));
  if (const int64_t cap = ro_ranges_cap()) ranges = (int)std::min<int64_t>(ranges, cap);
  w.ro_last.ranges = ranges;
  w.ro_last.tiles = tiles;
  ensure(w, w.ro_cnt, (size_t)ranges * 2048 * 4, false);
  ensure(w, w.ro_off, (size_t)ranges * 2048 * 4, false);
  ensure(w, w.ro_tot, 2 * 2048 * 4, false);
  ensure(w, w.g_ctrs, 64, true);
  WxRoArgs a{};
  fill_cols(t, spec.cols, a.col);
  a.n_rows = n;
  a.key_lo = kmin;
  a.span = span;
  a.ranges = ranges;
  a.cnt = static_cast<wx_u32 *>(w.ro_cnt.p);
  a.off = static_cast<const wx_u32 *>(w.ro_off.p);
  a.ctrs = static_cast<wx_u64 *>(w.g_ctrs.p);
  a.info = nullptr;
  return a;
}

// Row-order GROUP BY when the groups' keys span at most 2048 values
// (wx_group_rows.hip), after an ordinary call gave the groups and counts:
// per-range bin counts straight from the table, their totals / bases (checked
// against the ordinary call) / per-range offsets, one stable counting scatter
// of the passing rows' values into key-major row-ordered segments, the exact
// fold of each group's segment.  No compaction, no key bits, no radix pass.
void group_rows_span(const wx_table *t, const char *val_expr, const char *key_expr, const char *cond,
                     const wx_launch &L, int32_t kmin, int span, const int32_t *d_keys, double *d_sums,
                     const int64_t *d_counts, int64_t ng, Workspace &w, hipStream_t s, bool minmax) {
  const Spec spec = group_spec(t, val_expr, key_expr, cond, L, minmax);
  auto gmod = get_module(L.device, spec, true);
  auto umod = util_module(L.device, true);
  DeviceState &d = device_state(L.device, true);
  const bool timed = (L.flags & WX_F_TIME) != 0;
  int64_t passing = 0;  // the groups' rows: the key-major array's length
  {
    std::vector<int64_t> hc((size_t)ng);
    WX_HIP(hipMemcpyAsync(hc.data(), d_counts, (size_t)ng * 8, hipMemcpyDeviceToHost, s));
    WX_HIP(hipStreamSynchronize(s));
    for (int64_t c : hc) passing += c;
  }
  if (passing > 0xffffffffll)
    fail(WX_ERR_UNSUPPORTED, "row-order sums over a key span take at most 2^32 - 1 passing rows");
  WxRoArgs a = ro_args(t, spec, d, kmin, span, w);
  wx_u32 *tot = static_cast<wx_u32 *>(w.ro_tot.p);
  launch(gmod->fn("wx_ro_count"), (unsigned)a.ranges, &a, s, timed, WX_RO_THREADS);
  WxRoScanArgs sc{};
  sc.cnt = a.cnt;
  sc.totals = tot;
  sc.ranges = a.ranges;
  launch(umod->fn("wx_ro_scan"), 32, &sc, s, timed, 256);
  WxRoBaseArgs b{};
  b.totals = tot;
  b.base = tot + 2048;
  b.gkeys = d_keys;
  b.gcounts = reinterpret_cast<const wx_i64 *>(d_counts);
  b.n_groups = ng;
  b.key_lo = kmin;
  b.ctrs = a.ctrs;
  launch(umod->fn("wx_ro_base"), 1, &b, s, timed, 1024);
  ro_scatter_fold(gmod.get(), umod.get(), a, passing, d_counts, ng, d_sums, w, s, timed);
  check_errors(w);
  ro_done(w, WX_RO_ROUTE_ORDINARY_SPAN, static_cast<const float *>(w.ro_vals.p), passing);
}

// The span path without the ordinary call (no MIN / MAX asked): a key range
// from the memo of an earlier call or a strided sample picks a 2048-key span
// around it, and the groups come straight from the bins' totals (the keys of
// the non-empty bins, ascending, and their counts).  Returns false, having
// written nothing the caller keeps, when the sample was too wide or a row's
// key fell outside the span (the count kernel flags it): the caller then runs
// the ordinary call first (and does for the next 16 calls over the same
// expressions and table, so a sample that keeps missing costs once per 17).
// 1: done; 0: the ordinary call first (a recent miss, no sampled row, or a
// key outside the guessed span); 2: the keys span more than 2048 (the
// sample or the memo says so), the general path without the ordinary call
int group_rows_direct(const wx_table *t, const char *val_expr, const char *key_expr, const char *cond,
                       const wx_launch &L, int64_t capacity, int32_t *d_keys, double *d_sums, int64_t *d_counts,
                       int64_t *d_n_groups, int64_t *h_n_groups, Workspace &w, hipStream_t s) {
  const Spec spec = group_spec(t, val_expr, key_expr, cond, L, false);
  auto gmod = get_module(L.device, spec, true);
  auto umod = util_module(L.device, true);
  DeviceState &d = device_state(L.device, true);
  const bool timed = (L.flags & WX_F_TIME) != 0;
  const uint64_t mkey = gp_memo_key(spec, t, spec.cols);
  auto miss = w.ro_miss.find(mkey);
  if (miss != w.ro_miss.end() && miss->second-- > 0) {  // missed lately: the ordinary call first
    w.ro_last.why = WX_RO_WHY_RECENT_MISS;
    return 0;
  }
  if (miss != w.ro_miss.end()) w.ro_miss.erase(miss);
  KeyRange r;
  auto it = w.gp_memo.find(mkey);
  if (it != w.gp_memo.end()) {
    r.any = true;
    r.lo = it->second.lo;
    r.hi = it->second.hi;
  } else {
    r = sample_keys(t, spec.cols, gmod.get(), w, s, timed);
  }
  if (!r.any) {
    w.ro_last.why = WX_RO_WHY_NO_SAMPLE;
    return 0;
  }
  if (r.span() > 2048) {
    w.ro_last.why = WX_RO_WHY_WIDE;
    return 2;
  }
  // the sampled keys centred in the span, inside the int32 range
  int64_t lo = r.lo - (2048 - r.span()) / 2;
  lo = std::max<int64_t>(INT32_MIN, std::min<int64_t>(lo, (int64_t)INT32_MAX - 2047));
  WxRoArgs a = ro_args(t, spec, d, (int32_t)lo, 2048, w);
  ensure(w, w.ro_info, 64, false);
  WX_HIP(hipMemsetAsync(w.ro_info.p, 0, 64, s));
  a.info = static_cast<wx_i64 *>(w.ro_info.p);
  wx_u32 *tot = static_cast<wx_u32 *>(w.ro_tot.p);
  launch(gmod->fn("wx_ro_count"), (unsigned)a.ranges, &a, s, timed, WX_RO_THREADS);
  WxRoScanArgs sc{};
  sc.cnt = a.cnt;
  sc.totals = tot;
  sc.ranges = a.ranges;
  launch(umod->fn("wx_ro_scan"), 32, &sc, s, timed, 256);
  WxRoBaseArgs b{};
  b.totals = tot;
  b.base = tot + 2048;
  b.key_lo = (int32_t)lo;
  b.ctrs = a.ctrs;
  b.out_keys = d_keys;
  b.out_counts = reinterpret_cast<wx_i64 *>(d_counts);
  b.capacity = capacity;
  b.n_groups_out = reinterpret_cast<wx_i64 *>(d_n_groups);
  b.info = a.info;
  launch(umod->fn("wx_ro_base"), 1, &b, s, timed, 1024);
  int64_t info[5];
  WX_HIP(hipMemcpyAsync(info, w.ro_info.p, sizeof(info), hipMemcpyDeviceToHost, s));
  WX_HIP(hipStreamSynchronize(s));
  if (info[2]) {  // a key outside the guessed span: the ordinary call first, for the next 16 calls too
    w.gp_memo.erase(mkey);
    if (w.ro_miss.size() > 256) w.ro_miss.clear();
    w.ro_miss[mkey] = 16;
    w.ro_last.why = WX_RO_WHY_OUTSIDE;
    return 0;
  }
  const int64_t ng = info[0];
  if (h_n_groups) *h_n_groups = ng;
  if (ng > 0) {
    if (w.gp_memo.size() > 256) w.gp_memo.clear();  // bounded, as the ordinary path's
    w.gp_memo[mkey] = Workspace::GpMemo{info[3], info[4], info[4] - info[3] + 1 <= WX_GROUP_WINDOW, 0};
  }
  if (ng > capacity) {
    check_errors(w);  // the base kernel raised the capacity bit: the ordinary call's error
    fail(WX_ERR_CAPACITY, "group table / output capacity exceeded");
  }
  if (ng > 0) ro_scatter_fold(gmod.get(), umod.get(), a, info[1], d_counts, ng, d_sums, w, s, timed);
  check_errors(w);
  ro_done(w, WX_RO_ROUTE_DIRECT, ng > 0 ? static_cast<const float *>(w.ro_vals.p) : nullptr, ng > 0 ? info[1] : 0);
  return 1;
}

// The column an expression reads when it is nothing but `name[idx]` (outer
// parentheses and blanks allowed), else null.
const wx_col *bare_column(const wx_table *t, const char *expr) {
  if (!t || !expr) return nullptr;
  std::string e(expr);
  auto trim = [&e]() {
    const size_t b = e.find_first_not_of(" \t\n\r"), x = e.find_last_not_of(" \t\n\r");
    e = b == std::string::npos ? std::string() : e.substr(b, x - b + 1);
  };
  trim();
  while (e.size() >= 2 && e.front() == '(' && e.back() == ')') {
    int depth = 0;
    bool outer = true;  // the first '(' closes at the last character
    for (size_t i = 0; i + 1 < e.size(); ++i) {
      depth += e[i] == '(' ? 1 : e[i] == ')' ? -1 : 0;
      if (depth == 0) {
        outer = false;
        break;
      }
    }
    if (!outer) break;
    e = e.substr(1, e.size() - 2);
    trim();
  }
  const std::string tail = "[idx]";
  if (e.size() <= tail.size() || e.compare(e.size() - tail.size(), tail.size(), tail) != 0) return nullptr;
  const std::string name = e.substr(0, e.size() - tail.size());
  for (int c = 0; c < t->n_cols; ++c)
    if (t->cols[c].name && name == t->cols[c].name) return &t->cols[c];
  return nullptr;
}

// The general row-order path: (1) the passing rows' values and key bits in
// row order (ordered compactions; a bare int32 key column with no WHERE is
// read in place), (2) the stable radix pair sort by key, (3) each group's
// first row -- from the ordinary call's counts (ng >= 0: d_keys / d_counts
// hold its ng groups) or, with no ordinary call (ng < 0), by run-length
// encoding the sorted keys into d_keys / d_counts / d_n_groups -- (4) each
// group's values folded in row order.
void group_rows_general(const wx_table *t, const char *val_expr, const char *key_expr, const char *cond,
                        const wx_launch &L, const wx_launch &L1, int64_t capacity, int32_t *d_keys, double *d_sums,
                        int64_t *d_counts, int64_t *d_n_groups, int64_t &ng, Workspace &w, hipStream_t s) {
  const int64_t n = t->n_rows;
  if (n > 0xffffffffll) fail(WX_ERR_UNSUPPORTED, "row-order sums sort at most 2^32 - 1 rows");
  const bool runs = ng < 0;  // the groups from the sorted keys' runs
  w.ro_last.ranges = w.ro_last.tiles = 0;  // (a direct attempt that missed set them)
  ensure(w, w.ro_vals, (size_t)n * 4, false);
  ensure(w, w.ro_keys, (size_t)n * 4, false);
  float *vals = static_cast<float *>(w.ro_vals.p);
  int32_t *keys = static_cast<int32_t *>(w.ro_keys.p);
  int64_t m = 0, mk = 0;
  // a bare float32 value column and no WHERE: the sort's first pass reads
  // the column itself as its payload, no value projection
  const wx_col *vc = blank(cond) ? bare_column(t, val_expr) : nullptr;
  if (vc && (vc->dtype != WX_FLOAT32 || !vc->d_ptr)) vc = nullptr;
  if (vc)
    m = t->n_rows;
  else
    do_project_filter(t, val_expr, cond, &L1, WX_MODE_COMPACT, vals, nullptr, 8, 0, nullptr, &m);
  // a bare int32 key column and no WHERE: the sort's first pass reads the
  // column itself (its bits are the keys), no key projection
  const wx_col *kc = blank(cond) ? bare_column(t, key_expr) : nullptr;
  if (kc && (kc->dtype != WX_INT32 || !kc->d_ptr)) kc = nullptr;
  if (kc) {
    mk = t->n_rows;
  } else {
    // the key's bits through the float-valued compaction, unchanged
    const std::string kx = "__int_as_float((int)(" + std::string(key_expr) + "))";
    do_project_filter(t, kx.c_str(), cond, &L1, WX_MODE_COMPACT, reinterpret_cast<float *>(keys), nullptr, 8, 0,
                      nullptr, &mk);
  }
  if (m != mk) fail(WX_ERR_INTERNAL, "row-order GROUP BY: value and key compactions disagree");
  // stable: row order kept within a key; the fold reads the sorted arrays
  // where the last pass left them (no copy back)
  const void *ksrc = kc ? kc->d_ptr : nullptr;
  const float *vsrc = vc ? static_cast<const float *>(vc->d_ptr) : nullptr;
  const int32_t *sk = kc ? static_cast<const int32_t *>(ksrc) : keys;
  const float *sv = vc ? vsrc : vals;
  if (m > 1) {
    if (env_or("WARPDB_SORT", "radix") == "bitonic") {
      if (vc) WX_HIP(hipMemcpyAsync(vals, vsrc, (size_t)m * 4, hipMemcpyDeviceToDevice, s));
      do_sort(keys, vals, m, 1, 1, &L1, -1, ksrc);
      sk = keys;
      sv = vals;
    } else {
      void *rk = nullptr;
      float *rv = nullptr;
      radix_sort(keys, vals, m, 1, 1, L1, w, s, -1, ksrc, &rk, &rv, vsrc);
      sk = static_cast<const int32_t *>(rk);
      sv = rv;
    }
  }
  const bool timed = (L.flags & WX_F_TIME) != 0;
  WxGroupFoldArgs a{};
  a.skeys = sk;
  a.svals = sv;
  a.m = m;
  a.gkeys = d_keys;
  a.gcounts = reinterpret_cast<const wx_i64 *>(d_counts);
  a.n_groups = ng;
  a.out_sums = d_sums;
  ensure(w, w.g_ctrs, 64, true);
  a.ctrs = static_cast<wx_u64 *>(w.g_ctrs.p);
  auto mod = util_module(L.device, true);
  if (ng < 0) {
    // no ordinary call ran: the groups are the sorted keys' runs, in
    // ascending key order -- keys, counts and first rows by run-length
    // encoding (the counts then cover the rows by construction)
    // wave ranges: at most 32 768, each a multiple of 64 rows
    const int n_blk = (int)std::min<int64_t>(32768, std::max<int64_t>(1, (m + kRleWaveRows - 1) / kRleWaveRows));
    ensure(w, w.gf_chunks, 64 + (size_t)n_blk * 8, false);
    WxRleArgs r{};
    r.sk = sk;
    r.m = m;
    r.n_blk = n_blk;
    r.span = ((m + n_blk - 1) / n_blk + 63) / 64 * 64;
    const unsigned rle_grid = (unsigned)((n_blk + WX_RLE_BLOCK / 64 - 1) / (WX_RLE_BLOCK / 64));
    r.n_out = static_cast<wx_i64 *>(w.gf_chunks.p);
    r.blk = r.n_out + 8;
    r.n_groups_out = reinterpret_cast<wx_i64 *>(d_n_groups);
    r.capacity = capacity;
    r.out_keys = d_keys;
    r.out_counts = reinterpret_cast<wx_i64 *>(d_counts);
    launch(mod->fn("wx_rle_count"), rle_grid, &r, s, timed, WX_RLE_BLOCK);
    launch(mod->fn("wx_rle_scan"), 1u, &r, s, timed, WX_RLE_BLOCK);
    WX_HIP(hipMemcpyAsync(&w.host_word, r.n_out, 8, hipMemcpyDeviceToHost, s));
    WX_HIP(hipStreamSynchronize(s));
    ng = (int64_t)w.host_word;
    if (ng > capacity) fail(WX_ERR_CAPACITY, "group table / output capacity exceeded");
    ensure(w, w.gf_starts, (size_t)std::max<int64_t>(ng, 1) * 8, false);
    r.starts = static_cast<wx_i64 *>(w.gf_starts.p);
    if (ng > 0) {
      launch(mod->fn("wx_rle_emit"), rle_grid, &r, s, timed, WX_RLE_BLOCK);
      launch(mod->fn("wx_rle_counts"), (unsigned)((ng + WX_GS_BLOCK - 1) / WX_GS_BLOCK), &r, s, timed, WX_GS_BLOCK);
    }
    a.n_groups = ng;
    a.starts = r.starts;
  } else {
    // each group's first sorted row: the counts' exclusive prefix (the
    // groups come in ascending key order and the sorted array holds
    // exactly their rows, which wx_group_starts_scan checks)
    const int64_t n_chunks = (ng + WX_GS_CHUNK - 1) / WX_GS_CHUNK;
    ensure(w, w.gf_starts, (size_t)ng * 8, false);
    ensure(w, w.gf_chunks, (size_t)n_chunks * 8, false);
    a.starts = static_cast<wx_i64 *>(w.gf_starts.p);
    a.chunk_sums = static_cast<wx_i64 *>(w.gf_chunks.p);
    a.n_chunks = n_chunks;
    launch(mod->fn("wx_group_starts_sum"), (unsigned)n_chunks, &a, s, timed, WX_GS_BLOCK);
    launch(mod->fn("wx_group_starts_scan"), 1u, &a, s, timed, 1024);
    launch(mod->fn("wx_group_starts_emit"), (unsigned)n_chunks, &a, s, timed, WX_GS_BLOCK);
  }
  if (ng > 0) {
    ensure(w, w.gf_big, 64 + (size_t)ng * 8, false);
    a.big_n = static_cast<wx_u32 *>(w.gf_big.p);
    a.big_list = reinterpret_cast<wx_i64 *>(static_cast<char *>(w.gf_big.p) + 64);
    // $WARPDB_FOLD_SMALL: the largest group folded by one lane (0: every group one wave, for A/B)
    const std::string fs = env_or("WARPDB_FOLD_SMALL", "");
    a.small_max = fs.empty() ? (int64_t)WX_FOLD_SMALL : std::max<int64_t>(0, std::atoll(fs.c_str()));
    WX_HIP(hipMemsetAsync(a.big_n, 0, 4, s));
    a.skip_above = xf_big_groups(mod.get(), sv, d_counts, ng, m, d_sums, w, s, timed);
    launch(mod->fn("wx_group_fold_small"), (unsigned)((ng + WX_GS_BLOCK - 1) / WX_GS_BLOCK), &a, s, timed,
           WX_GS_BLOCK);
    launch(mod->fn("wx_group_fold"), (unsigned)std::min<int64_t>(ng, 4096), &a, s, timed, 64);
  }
  WX_HIP(hipStreamSynchronize(s));
  // (the sorted arrays -- ro_vals / ro_keys and the sort's ping-pong
  // buffers -- stay in the workspace for the next call, as the span path's do)
  check_errors(w);
  ro_done(w, runs ? WX_RO_ROUTE_GENERAL_RUNS : WX_RO_ROUTE_GENERAL_ORDINARY, sv, m);
}

// GROUP BY with each group's sum folded in ascending row order, one double
// add per row (WX_F_ROW_ORDER): the reference's std::map fold
// (src/warpdb.cpp:373-385) to the bit, the same on every run.  Keys spanning
// at most 2048: the key-span path (counting scatter + fold,
// wx_group_rows.hip), straight from the table or after the ordinary call.
// Wider: the general path (group_rows_general: compactions, stable radix
// pair sort, fold), its groups from the ordinary call or, with no MIN / MAX
// asked, from the sorted keys' runs.  MIN / MAX always come from the
// ordinary call (they do not depend on order).  Synchronous.
static void group_rows_routes(Op &op, const wx_table *t, const char *val_expr, const char *key_expr, const char *cond,
                              const wx_launch &L, int32_t key_lo, int64_t capacity, int32_t *d_keys, double *d_sums,
                              int64_t *d_counts, int64_t *d_n_groups, int64_t *h_n_groups, float *d_mins,
                              float *d_maxs) {
  wx_launch L1 = L;
  L1.flags &= ~(WX_F_ROW_ORDER | WX_F_SYNC);
  const std::string rows_mode = env_or("WARPDB_GROUP_ROWS", "span");
  (void)ro_ranges_cap();  // a bad $WARPDB_RO_RANGES fails before anything is enqueued
  op.w.ro_last.why = WX_RO_WHY_NOT_TRIED;
  // Without MIN / MAX (they come from the ordinary call): the span path
  // straight from the table (under the same lane-order guard as below), or,
  // when the keys are known to span more than 2048 (or the general path is
  // asked for), the general path with its groups from the sorted keys -- no
  // ordinary call either way
  if (!d_mins && !d_maxs && (rows_mode == "span" || rows_mode == "general") && t->n_rows > 0) {
    if (blank(val_expr) || blank(key_expr)) fail(WX_ERR_INVALID, "Empty query expression");
    if (capacity < 0 || (capacity > 0 && (!d_keys || !d_sums || !d_counts)))
      fail(WX_ERR_INVALID, "group outputs must hold `capacity` entries");
    int route = 2;  // (WARPDB_GROUP_ROWS=general: why stays "not tried")
    if (rows_mode == "span" && rs_rank_extra(device_state(L.device, true).arch).empty()) op.w.ro_last.why = WX_RO_WHY_NONE;
    if (rows_mode == "span")
      route = rs_rank_extra(device_state(L.device, true).arch).empty()
                  ? group_rows_direct(t, val_expr, key_expr, cond, L1, capacity, d_keys, d_sums, d_counts,
                                      d_n_groups, h_n_groups, op.w, op.s)
                  : 0;
    if (route == 1) return;
    if (route == 2) {
      int64_t ng = -1;
      group_rows_general(t, val_expr, key_expr, cond, L, L1, capacity, d_keys, d_sums, d_counts, d_n_groups, ng, op.w, op.s);
      if (h_n_groups) *h_n_groups = ng;
      return;
    }
  }
  int64_t ng = 0;
  do_group_sum(t, val_expr, key_expr, cond, &L1, key_lo, capacity, d_keys, d_sums, d_counts, d_n_groups, &ng, d_mins,
               d_maxs);
  if (ng > 0 && rows_mode != "general") {
    // the groups' key span (they come out in ascending key order)
    int32_t kk[2] = {0, 0};
    WX_HIP(hipMemcpyAsync(&kk[0], d_keys, 4, hipMemcpyDeviceToHost, op.s));
    WX_HIP(hipMemcpyAsync(&kk[1], d_keys + (ng - 1), 4, hipMemcpyDeviceToHost, op.s));
    WX_HIP(hipStreamSynchronize(op.s));
    const int64_t span = (int64_t)kk[1] - kk[0] + 1;
    // the span path's stable scatter takes row order from the LDS returning
    // same-address adds in ascending lane order -- the undocumented gfx950
    // property the radix ranking relies on: only where rs_rank_extra allows it
    // (elsewhere the general path's sort ranks by peer masks)
    const bool lane_ordered_adds = rs_rank_extra(device_state(L.device, true).arch).empty();
    if (span <= 2048 && lane_ordered_adds) {
      group_rows_span(t, val_expr, key_expr, cond, L1, kk[0], (int)span, d_keys, d_sums, d_counts, ng, op.w, op.s,
                      d_mins || d_maxs);
      if (h_n_groups) *h_n_groups = ng;
      return;
    }
  }
  if (ng > 0) group_rows_general(t, val_expr, key_expr, cond, L, L1, capacity, d_keys, d_sums, d_counts, d_n_groups,
                                 ng, op.w, op.s);
  if (h_n_groups) *h_n_groups = ng;
}

void do_group_sum_rows(const wx_table *t, const char *val_expr, const char *key_expr, const char *cond,
                       const wx_launch &L, int32_t key_lo, int64_t capacity, int32_t *d_keys, double *d_sums,
                       int64_t *d_counts, int64_t *d_n_groups, int64_t *h_n_groups, float *d_mins, float *d_maxs) {
  Op op(L);  // recursive: the steps below take it again; the buffers stay this call's
  // the call's record (wx_group_rows_last_call): all zero unless a route finishes
  auto forget = [&op] {
    op.w.ro_last = {0, 0, 0, 0, 0, 0, 0};
    op.w.ro_last_vals = nullptr;
  };
  forget();
  try {
    group_rows_routes(op, t, val_expr, key_expr, cond, L, key_lo, capacity, d_keys, d_sums, d_counts, d_n_groups,
                      h_n_groups, d_mins, d_maxs);
  } catch (...) {
    forget();
    throw;
  }
  if (op.w.ro_last.route == WX_RO_ROUTE_NONE) forget();  // the ordinary call found no group
}

}  // namespace wx
