// group.cpp -- GROUP BY: the LDS window + global hash (wx_group.hip), the
// range-partitioned form (wx_group_part.hip), and the merges of shard
// partials (combine, slots, lists).
#include "wx_host.hpp"

namespace wx {

uint32_t next_pow2(uint64_t v) {
  uint64_t p = 1;
  while (p < v) p <<= 1;
  return (uint32_t)std::min<uint64_t>(p, 1u << 30);
}

// Range-partitioned GROUP BY (wx_group_part.hip), for a
// caller expecting many groups (capacity > WX_GROUP_HSORT_MAX) on >= 2^20
// rows.  The key range comes from the previous call over the same table and
// expressions (memo), else from a 65 536-row sample (widened by an eighth on
// each side), else from an exact min / max pass.  A range within the LDS
// window runs the window kernel with the window placed on it (the global hash
// still catches any key outside: no further host read); a range up to
// 2^24 keys runs the partitioned kernels, which count the rows outside the
// planned range: the host reads that summary once at the end (the one host
// synchronisation of the partitioned form) and, when some row was outside,
// re-plans from the exact range the same pass measured.  Anything wider
// keeps the window + global hash.
// below 2^20 rows the window + hash path is as fast; $WARPDB_GP_MIN_ROWS
// lowers the floor (test hook: small reference fixtures through this path)
int64_t gp_min_rows() {
  const char *v = std::getenv("WARPDB_GP_MIN_ROWS");
  return (v && *v) ? std::atoll(v) : (1 << 20);
}
#define WX_GP_STAGE_MAX_PARTS 2048  // the tile scan: two partitions per thread (wx_group_part.hip WX_GP_STAGE_MAXP)
#define WX_GP_AGG_DIR_WORDS 4096    // directory words the aggregation stages in LDS (WX_GP_DIRCH)

// row quads per thread per tile: the kernel's WX_GP_SUNROLL
int gp_sunroll() { return 4; }
// the tile kernel's workgroup (wx_group_part.hip WX_GP_TBLOCK) and rows per tile
#define WX_GP_TBLOCK 1024
int64_t gp_tile_rows() { return (int64_t)WX_GP_TBLOCK * 4 * gp_sunroll(); }

// 8192 keys per partition (96 KB of LDS per aggregating workgroup)
int gp_shift() { return 13; }
int64_t gp_max_span() { return (int64_t)WX_GP_STAGE_MAX_PARTS << gp_shift(); }

// The launch geometry of one partitioned pass over n_rows rows and a key
// span of `span`: the one statement of it (group_partitioned launches it,
// wx_group_part_geometry reports it).  One 1024-thread tile workgroup per CU
// (two of 512) up to the 1024 the plan kernel scans, each running
// tiles_per_wg consecutive tiles.  Two diagnostic defines shrink it so that a
// small table reaches what only ~1e9 rows reach otherwise: WX_GP_GRID=<g>
// caps the grid (before tiles_per_wg is derived) and changes nothing else;
// WX_GP_DIRCH=<w> (1..4096, the kernel's define of the same name) shortens
// the aggregation's directory rounds, the LDS stays sized for 4096 words.
GpPlan gp_plan(int64_t n_rows, int64_t span, int cus, const std::string &extra) {
  if (n_rows < 1) fail(WX_ERR_INVALID, "partitioned GROUP BY: no rows");
  if (cus < 1) fail(WX_ERR_INVALID, "partitioned GROUP BY: no compute units");
  if (span <= WX_GROUP_WINDOW || span > gp_max_span())
    fail(WX_ERR_UNSUPPORTED, "partitioned GROUP BY: key spans of 2049 to 2^24 only");
  const int grid_cap = define_value(extra, "WX_GP_GRID", INT32_MAX);
  if (grid_cap < 1) fail(WX_ERR_INVALID, "WX_GP_GRID must be at least 1");
  GpPlan g;
  g.dir_chunk = define_value(extra, "WX_GP_DIRCH", WX_GP_AGG_DIR_WORDS);
  if (g.dir_chunk < 1 || g.dir_chunk > WX_GP_AGG_DIR_WORDS)
    fail(WX_ERR_INVALID, "WX_GP_DIRCH must be between 1 and 4096");
  const int agg_r = define_value(extra, "WX_GP_AGG_R", 8);
  if (agg_r < 1) fail(WX_ERR_INVALID, "WX_GP_AGG_R must be at least 1");
  g.agg_sweep = WX_GP_BLOCK / 64 * agg_r;
  g.part_keys = 1ll << gp_shift();
  g.n_part = (int)((span + g.part_keys - 1) >> gp_shift());
  g.tile_rows = gp_tile_rows();
  g.n_tiles = (n_rows + g.tile_rows - 1) / g.tile_rows;
  g.grid = std::min<int64_t>(std::min<int64_t>((int64_t)cus * (1024 / WX_GP_TBLOCK), 1024), g.n_tiles);
  g.grid = std::min<int64_t>(g.grid, grid_cap);
  g.tiles_per_wg = (g.n_tiles + g.grid - 1) / g.grid;
  g.grid = (g.n_tiles + g.tiles_per_wg - 1) / g.tiles_per_wg;
  g.chunk_rows = 1 << 16;
  g.target_items = 4ll * cus;
  g.work_cap = g.n_part + g.target_items + 2;
  if (g.work_cap > 4096) fail(WX_ERR_INTERNAL, "partitioned GROUP BY: more than 4096 work items");
  return g;
}

// (min, max, passing) over the per-workgroup words mm[4g .. 4g+2]
KeyRange reduce_mm(const int64_t *h, int64_t groups) {
  KeyRange r;
  int64_t mn = INT32_MAX, mx = INT32_MIN;
  for (int64_t g = 0; g < groups; ++g) {
    if (!h[4 * g + 2]) continue;
    mn = std::min(mn, h[4 * g]);
    mx = std::max(mx, h[4 * g + 1]);
    r.passing += h[4 * g + 2];
  }
  if (r.passing) {
    r.any = true;
    r.lo = mn;
    r.hi = mx;
  }
  return r;
}

KeyRange read_mm(Workspace &w, hipStream_t s, int64_t groups) {
  std::vector<int64_t> h((size_t)groups * 4);
  WX_HIP(hipMemcpyAsync(h.data(), w.gp_mm.p, h.size() * 8, hipMemcpyDeviceToHost, s));
  WX_HIP(hipStreamSynchronize(s));
  return reduce_mm(h.data(), groups);
}

// the range of a strided 65 536-row sample (one host read)
KeyRange sample_keys(const wx_table *t, const std::vector<UsedCol> &cols, Module *mod, Workspace &w, hipStream_t s,
                     bool timed) {
  const unsigned grid = kSampleGrid;
  ensure(w, w.gp_mm, (size_t)grid * 32, false);
  WxGroupPartArgs a{};
  fill_cols(t, cols, a.col);
  a.n_rows = t->n_rows;
  a.mm = static_cast<wx_i64 *>(w.gp_mm.p);
  launch(mod->fn("wx_group_part_sample"), grid, &a, s, timed, WX_GP_BLOCK);
  return read_mm(w, s, grid);
}

// exact (min, max) key and passing rows over the whole table (one host read);
// WX_GP_BLOCK threads over contiguous ranges of >= 4096 rows
KeyRange probe_keys(const wx_table *t, const std::vector<UsedCol> &cols, Module *mod, DeviceState &d, Workspace &w,
                    hipStream_t s, bool timed) {
  int64_t G = std::min<int64_t>((int64_t)d.cus, std::max<int64_t>(1, (t->n_rows + 4095) / 4096));
  int64_t rpw = ((t->n_rows + G - 1) / G + 3) & ~3ll;
  G = (t->n_rows + rpw - 1) / rpw;
  ensure(w, w.gp_mm, (size_t)G * 32, false);
  WxGroupPartArgs a{};
  fill_cols(t, cols, a.col);
  a.n_rows = t->n_rows;
  a.rows_per_wg = rpw;
  a.mm = static_cast<wx_i64 *>(w.gp_mm.p);
  launch(mod->fn("wx_group_part_minmax"), (unsigned)G, &a, s, timed, WX_GP_BLOCK);
  return read_mm(w, s, G);
}

// One partitioned pass for keys [lo, lo + P << shift): tiles -> plan -> agg
// -> count -> scan2 -> emit, then the summary read (passing rows, rows
// outside the range, min key, max key).  Nothing is aggregated or emitted
// when some row was outside (the caller re-plans).
struct GpSummary {
  int64_t passing = 0, outside = 0, mn = 0, mx = -1;
};

GpSummary group_partitioned(const wx_table *t, const std::vector<UsedCol> &cols, Module *mod, DeviceState &d,
                            Workspace &w, hipStream_t s, bool timed, int64_t lo, int64_t span, int64_t capacity,
                            int32_t *d_keys, double *d_sums, int64_t *d_counts, int64_t *ng,
                            const std::string &extra) {
  const GpPlan plan = gp_plan(t->n_rows, span, d.cus, extra);
  const int shift = gp_shift();
  const int64_t B = plan.part_keys;
  const int P = plan.n_part;
  const int64_t tile = plan.tile_rows, n_tiles = plan.n_tiles, G = plan.grid, tpw = plan.tiles_per_wg;
  const int64_t target_items = plan.target_items, work_cap = plan.work_cap;
  ensure(w, w.gp_mm, (size_t)G * 32, false);
  ensure(w, w.gp_pcount, (size_t)G * P * 4, false);
  ensure(w, w.gp_ptotal, (size_t)WX_GP_STAGE_MAX_PARTS * 8, false);
  // cleared on every call (the plan also leaves it clean, but a call that
  // failed between the tiles' adds and the plan would leave stale totals:
  // ADVICE r4); P x 8 bytes
  WX_HIP(hipMemsetAsync(w.gp_ptotal.p, 0, (size_t)P * 8, s));
  ensure(w, w.gp_dir, (size_t)P * n_tiles * 4, false);
  ensure(w, w.gp_vals, (size_t)n_tiles * tile * 4, false);
  ensure(w, w.gp_bins, (size_t)n_tiles * tile * 2, false);
  ensure(w, w.gp_work, (size_t)work_cap * 16, false);
  ensure(w, w.gp_nwork, 8, false);
  ensure(w, w.gp_pitem, (size_t)(P + 1) * 4, false);
  ensure(w, w.gp_order, (size_t)(work_cap + 8) * 4, false);  // + 8: the XCD-dealt order's empty slots
  ensure(w, w.gp_psum, (size_t)work_cap * B * 8, false);
  ensure(w, w.gp_pcnt, (size_t)work_cap * B * 4, false);
  ensure(w, w.gp_summary, 32, false);
  ensure(w, w.gp_pnz, (size_t)P * 4, false);
  ensure(w, w.g_ctrs, 64, true);
  WxGroupPartArgs a{};
  fill_cols(t, cols, a.col);
  a.n_rows = t->n_rows;
  a.n_tiles = n_tiles;
  a.tiles_per_wg = (int)tpw;
  a.n_wg = (int)G;
  a.n_part = P;
  a.key_lo = (int32_t)lo;
  a.shift = shift;
  a.mm = static_cast<wx_i64 *>(w.gp_mm.p);
  a.pcount = static_cast<wx_u32 *>(w.gp_pcount.p);
  a.ptotal = static_cast<wx_u64 *>(w.gp_ptotal.p);
  a.dir = static_cast<wx_u32 *>(w.gp_dir.p);
  a.vals = static_cast<float *>(w.gp_vals.p);
  a.bins = static_cast<unsigned short *>(w.gp_bins.p);
  a.work = static_cast<wx_i64 *>(w.gp_work.p);
  a.n_work = static_cast<wx_i64 *>(w.gp_nwork.p);
  a.pitem = static_cast<wx_u32 *>(w.gp_pitem.p);
  a.order = static_cast<wx_u32 *>(w.gp_order.p);
  a.work_cap = work_cap;
  a.chunk = plan.chunk_rows;
  a.target_items = target_items;
  a.psum = static_cast<double *>(w.gp_psum.p);
  a.pcnt = static_cast<wx_u32 *>(w.gp_pcnt.p);
  a.summary = static_cast<wx_i64 *>(w.gp_summary.p);
  a.pnz = static_cast<wx_u32 *>(w.gp_pnz.p);
  a.out_keys = d_keys;
  a.out_sums = d_sums;
  a.out_counts = reinterpret_cast<wx_i64 *>(d_counts);
  a.capacity = capacity;
  a.n_groups_out = reinterpret_cast<wx_i64 *>(ng);
  a.ctrs = static_cast<wx_u64 *>(w.g_ctrs.p);
  // the tile kernel's LDS: the staged tile (6 B per row) + 12 B per partition (+ its static words), within 160 KB
  const int64_t tile_lds = tile * 6 + (int64_t)P * 12;
  if (tile_lds + 1024 > 160 * 1024 / (1024 / WX_GP_TBLOCK))
    fail(WX_ERR_INTERNAL, "partitioned GROUP BY: tile LDS exceeds the per-CU share");
  // diagnostics only: per-phase times of the tile kernel (WX_GP_DIAG builds)
  const bool diag = env_or("WARPDB_EXTRA_DEFINES", "").find("WX_GP_DIAG") != std::string::npos;
  a.diag = nullptr;
  if (diag) {
    ensure(w, w.diag, (size_t)G * 16 * 8, false);
    WX_HIP(hipMemsetAsync(w.diag.p, 0, (size_t)G * 16 * 8, s));
    a.diag = static_cast<wx_u64 *>(w.diag.p);
  }
  launch(mod->fn("wx_group_part_tiles"), (unsigned)G, &a, s, timed, WX_GP_TBLOCK, (unsigned)tile_lds);
  if (diag) {  // mean per-workgroup phase time per tile, 10 ns ticks -> us
    std::vector<wx_u64> h((size_t)G * 16);
    WX_HIP(hipMemcpyAsync(h.data(), w.diag.p, h.size() * 8, hipMemcpyDeviceToHost, s));
    WX_HIP(hipStreamSynchronize(s));
    const char *names[8] = {"write-out", "eval", "next-loads", "barrier1", "scan", "barrier2", "place", "barrier3"};
    for (int role = 0; role < 2; ++role) {
      std::fprintf(stderr, "[warpexec] tiles %s:", role ? "wave 15" : "wave 0 ");
      double tot = 0;
      for (int i = 0; i < 8; ++i) {
        double m = 0;
        for (int64_t b = 0; b < G; ++b) m += (double)h[(size_t)b * 16 + role * 8 + i];
        m = m / (double)G / (double)tpw / 100.0;
        tot += m;
        std::fprintf(stderr, " %s %.2f", names[i], m);
      }
      std::fprintf(stderr, " | %.2f us per tile\n", tot);
    }
  }
  launch(mod->fn("wx_group_part_plan"), 1, &a, s, timed, 1024);
  // one workgroup per possible item; those past the plan's count return at once
  launch(mod->fn("wx_group_part_agg"), (unsigned)((work_cap + 7) / 8 * 8), &a, s, timed, WX_GP_BLOCK,
         (unsigned)(B * 12 + WX_GP_AGG_DIR_WORDS * 4));
  launch(mod->fn("wx_group_part_count"), (unsigned)P, &a, s, timed, WX_GP_BLOCK);
  launch(mod->fn("wx_group_part_scan2"), 1, &a, s, timed, 1024);
  launch(mod->fn("wx_group_part_emit"), (unsigned)P, &a, s, timed, WX_GP_BLOCK);
  int64_t h[4];
  WX_HIP(hipMemcpyAsync(h, a.summary, sizeof h, hipMemcpyDeviceToHost, s));
  WX_HIP(hipStreamSynchronize(s));
  GpSummary r;
  r.passing = h[0];
  r.outside = h[1];
  r.mn = h[2];
  r.mx = h[3];
  ++w.gp_passes;
  return r;
}

// memo of the last key range per (expressions, columns, rows): the next
// call's first guess (never trusted for correctness: the window path's hash
// and the partitioned pass's outside count both catch a stale range)
uint64_t gp_memo_key(const Spec &spec, const wx_table *t, const std::vector<UsedCol> &cols) {
  std::string k = spec.expr + '\x01' + spec.key + '\x01' + spec.cond + '\x01' + spec.custom + '\x01' +
                  std::to_string(t->n_rows);
  for (auto &c : cols) k += '\x01' + std::to_string(reinterpret_cast<uintptr_t>(t->cols[c.table_index].d_ptr));
  return fnv1a(k);
}

// The general-key table of at least hcap slots (a power of two), zeroed when
// it grows; shared by wx_group_sum and wx_group_multi.
void ensure_group_table(Workspace &w, hipStream_t s, uint32_t hcap) {
  if (w.g_hcap >= hcap) return;
  ensure(w, w.g_tag, (size_t)hcap * 8, true);
  ensure(w, w.g_sum, (size_t)hcap * 8, true);
  ensure(w, w.g_cnt, (size_t)hcap * 8, true);
  ensure(w, w.g_used, (size_t)hcap * 4, true);
  WX_HIP(hipMemsetAsync(w.g_tag.p, 0, w.g_tag.bytes, s));
  WX_HIP(hipMemsetAsync(w.g_sum.p, 0, w.g_sum.bytes, s));
  WX_HIP(hipMemsetAsync(w.g_cnt.p, 0, w.g_cnt.bytes, s));
  w.g_hcap = hcap;
}

void do_group_sum(const wx_table *t, const char *val_expr, const char *key_expr, const char *cond,
                  const wx_launch *Lp, int32_t key_lo, int64_t capacity, int32_t *d_keys, double *d_sums,
                  int64_t *d_counts, int64_t *d_n_groups, int64_t *h_n_groups, float *d_mins, float *d_maxs,
                  double *d_window, int32_t n_slots, int32_t slot_rank, int32_t slot_groups) {
  const bool minmax = d_mins || d_maxs;
  if (minmax && d_window) fail(WX_ERR_UNSUPPORTED, "GROUP BY partials carry SUM and COUNT only");
  check_table(t);
  const wx_launch L = launch_of(Lp);
  if (L.flags & WX_F_ROW_ORDER) {
    if (d_window) fail(WX_ERR_UNSUPPORTED, "row-order sums are not available for shard partials");
    do_group_sum_rows(t, val_expr, key_expr, cond, L, key_lo, capacity, d_keys, d_sums, d_counts, d_n_groups,
                      h_n_groups, d_mins, d_maxs);
    return;
  }
  if (blank(val_expr) || blank(key_expr)) fail(WX_ERR_INVALID, "Empty query expression");
  if (capacity < 0 || (capacity > 0 && (!d_keys || !d_sums || !d_counts)))
    fail(WX_ERR_INVALID, "group outputs must hold `capacity` entries");
  if ((int64_t)key_lo + WX_GROUP_WINDOW - 1 > INT32_MAX) fail(WX_ERR_INVALID, "key window out of range");
  const Spec spec = group_spec(t, val_expr, key_expr, cond, L, minmax);
  Op op(L, spec);
  // the general-key table must hold every distinct key outside the window
  ensure_group_table(op.w, op.s, next_pow2(std::max<int64_t>(4096, 2 * capacity)));
  ensure(op.w, op.w.g_win_sum, WX_GROUP_WINDOW * 8, true);
  ensure(op.w, op.w.g_win_cnt, WX_GROUP_WINDOW * 8, true);
  if (minmax && op.w.g_mm_cap < op.w.g_hcap) {
    ensure(op.w, op.w.g_win_min, WX_GROUP_WINDOW * 4, false);
    ensure(op.w, op.w.g_win_max, WX_GROUP_WINDOW * 4, true);
    ensure(op.w, op.w.g_min, (size_t)op.w.g_hcap * 4, false);
    ensure(op.w, op.w.g_max, (size_t)op.w.g_hcap * 4, false);
    WX_HIP(hipMemsetAsync(op.w.g_win_min.p, 0xff, op.w.g_win_min.bytes, op.s));
    WX_HIP(hipMemsetAsync(op.w.g_min.p, 0xff, op.w.g_min.bytes, op.s));
    WX_HIP(hipMemsetAsync(op.w.g_max.p, 0, op.w.g_max.bytes, op.s));
    op.w.g_mm_cap = op.w.g_hcap;
  }
  ensure(op.w, op.w.g_ctrs, 64, true);
  int64_t *ng = count_slot(op.w, op.w.g_ngroups, d_n_groups);
  if (capacity > WX_GROUP_HSORT_MAX && !minmax && !d_window && t->n_rows >= gp_min_rows() && t->n_rows > 0 &&
      env_or("WARPDB_GROUP_PARTITION", "1") != "0") {
    // the key range: the memo of the previous call, else a sample (widened),
    // else an exact pass (see gp_min_rows above)
    const uint64_t mkey = gp_memo_key(spec, t, spec.cols);
    if (op.w.gp_memo.size() > 256) op.w.gp_memo.clear();
    KeyRange r;
    bool from_memo = false;
    auto it = op.w.gp_memo.find(mkey);
    // a window-kind memo is re-checked every 16th call (nothing else would
    // notice a table rewritten in place with many more keys)
    if (it != op.w.gp_memo.end() && (!it->second.window || it->second.uses < 16)) {
      r.any = true;
      r.lo = it->second.lo;
      r.hi = it->second.hi;
      ++it->second.uses;
      from_memo = true;
    } else {
      if (env_or("WARPDB_GP_GUESS", "1") != "0") {
        r = sample_keys(t, spec.cols, op.mod.get(), op.w, op.s, op.timed);
        if (r.any) {
          const int64_t margin = std::max<int64_t>(r.span() / 8, 64);
          r.lo = std::max<int64_t>(INT32_MIN, r.lo - margin);
          r.hi = std::min<int64_t>(INT32_MAX, r.hi + margin);
        }
      }
      if (!r.any || r.span() > gp_max_span()) r = probe_keys(t, spec.cols, op.mod.get(), op.d, op.w, op.s, op.timed);
    }
    if (r.any && r.span() > WX_GROUP_WINDOW && r.span() <= gp_max_span()) {
      GpSummary g = group_partitioned(t, spec.cols, op.mod.get(), op.d, op.w, op.s, op.timed, r.lo, r.span(), capacity, d_keys,
                                      d_sums, d_counts, ng, spec.extra);
      bool done = g.outside == 0;
      if (!done && g.mx - g.mn + 1 > WX_GROUP_WINDOW && g.mx - g.mn + 1 <= gp_max_span()) {
        // some key was outside the planned range: again over the exact one
        g = group_partitioned(t, spec.cols, op.mod.get(), op.d, op.w, op.s, op.timed, g.mn, g.mx - g.mn + 1, capacity, d_keys,
                              d_sums, d_counts, ng, spec.extra);
        if (g.outside) fail(WX_ERR_INTERNAL, "partitioned GROUP BY: rows outside the exact key range");
        done = true;
      }
      if (g.passing) {
        Workspace::GpMemo m;
        m.lo = g.mn;
        m.hi = g.mx;
        m.window = g.mx - g.mn + 1 <= WX_GROUP_WINDOW;
        op.w.gp_memo[mkey] = m;
      } else {
        op.w.gp_memo.erase(mkey);
      }
      if (done) {
        if (h_n_groups) WX_HIP(hipMemcpy(h_n_groups, ng, 8, hipMemcpyDeviceToHost));
        if ((L.flags & WX_F_SYNC) || h_n_groups) check_errors(op.w);
        return;
      }
      // the exact range fits the window (or is too wide): the window path below
      r.any = true;
      r.lo = g.mn;
      r.hi = g.mx;
    }
    if (r.any && r.span() <= WX_GROUP_WINDOW) {  // every (sampled) key inside the window: move it there
      key_lo = (int32_t)std::min<int64_t>(r.lo, INT32_MAX - (WX_GROUP_WINDOW - 1));
      if (!from_memo) op.w.gp_memo[mkey] = Workspace::GpMemo{r.lo, r.hi, true, 0};
    }
  }
  WxGroupArgs a;
  fill_cols(t, spec.cols, a.col);
  a.n_rows = t->n_rows;
  a.win_sum = static_cast<double *>(op.w.g_win_sum.p);
  a.win_cnt = static_cast<wx_u64 *>(op.w.g_win_cnt.p);
  a.h_tag = static_cast<wx_u64 *>(op.w.g_tag.p);
  a.h_sum = static_cast<double *>(op.w.g_sum.p);
  a.h_cnt = static_cast<wx_u64 *>(op.w.g_cnt.p);
  a.h_used = static_cast<wx_u32 *>(op.w.g_used.p);
  a.ctrs = static_cast<wx_u64 *>(op.w.g_ctrs.p);
  a.win_min = static_cast<wx_u32 *>(op.w.g_win_min.p);
  a.win_max = static_cast<wx_u32 *>(op.w.g_win_max.p);
  a.h_min = static_cast<wx_u32 *>(op.w.g_min.p);
  a.h_max = static_cast<wx_u32 *>(op.w.g_max.p);
  a.hmask = op.w.g_hcap - 1;
  a.key_lo = key_lo;
  // The finalize: its own one-workgroup launch after the (possible) key
  // sort (fusing it into wx_group_sum's last workgroup measured slower,
  // DESIGN.md 5.2).
  WxGroupFinArgs f;
  f.win_sum = a.win_sum;
  f.win_cnt = a.win_cnt;
  f.h_tag = a.h_tag;
  f.h_sum = a.h_sum;
  f.h_cnt = a.h_cnt;
  f.h_used = a.h_used;
  f.ctrs = a.ctrs;
  f.win_min = a.win_min;
  f.win_max = a.win_max;
  f.h_min = a.h_min;
  f.h_max = a.h_max;
  f.out_keys = d_keys;
  f.out_sums = d_sums;
  f.out_counts = reinterpret_cast<wx_i64 *>(d_counts);
  f.out_mins = d_mins;
  f.out_maxs = d_maxs;
  f.n_groups_out = reinterpret_cast<wx_i64 *>(ng);
  f.capacity = capacity;
  f.key_lo = key_lo;
  f.win_out = d_window;
  f.slots = (d_window && n_slots > 0) ? d_window + WX_GROUP_EXCHANGE : nullptr;
  f.n_slots = n_slots;
  f.slot_rank = slot_rank;
  f.slot_groups = slot_groups;
  if (t->n_rows > 0) {
    const GroupWindowPlan P = group_window_plan(t->n_rows, 1, minmax ? 1 : 0, WX_GW_GROUP_SUM, 0, op.d.cus, spec.extra);
    launch(op.mod->fn("wx_group_sum"), P.grid, &a, op.s, op.timed, (unsigned)P.block);
  }
  f.sorted = sort_general_keys(op, op.mod.get(), a.ctrs, a.h_used, a.h_tag, capacity, t->n_rows > 0);
  finish_group(op, op.mod->fn("wx_group_finalize"), &f, ng, h_n_groups);
}

void do_group_combine(const double *d_window, int32_t key_lo, const int32_t *xk, const double *xs, const int64_t *xc,
                      int64_t n_extra, const wx_launch *Lp, int64_t capacity, int32_t *d_keys, double *d_sums,
                      int64_t *d_counts, int64_t *d_n_groups, int64_t *h_n_groups) {
  const wx_launch L = launch_of(Lp);
  if (!d_window) fail(WX_ERR_INVALID, "null exchange window");
  if (n_extra < 0 || (n_extra > 0 && (!xk || !xs || !xc))) fail(WX_ERR_INVALID, "bad out-of-window groups");
  if (capacity < 0 || (capacity > 0 && (!d_keys || !d_sums || !d_counts)))
    fail(WX_ERR_INVALID, "group outputs must hold `capacity` entries");
  if ((int64_t)key_lo + WX_GROUP_WINDOW - 1 > INT32_MAX) fail(WX_ERR_INVALID, "key window out of range");
  Op op(L, util_spec());
  int64_t *ng = count_slot(op.w, op.w.g_ngroups, d_n_groups);
  WxGroupCombineArgs a;
  a.window = d_window;
  a.x_keys = xk;
  a.x_sums = xs;
  a.x_counts = reinterpret_cast<const wx_i64 *>(xc);
  a.n_extra = n_extra;
  a.key_lo = key_lo;
  a.out_keys = d_keys;
  a.out_sums = d_sums;
  a.out_counts = reinterpret_cast<wx_i64 *>(d_counts);
  a.capacity = capacity;
  a.n_groups_out = reinterpret_cast<wx_i64 *>(ng);
  launch(op.mod->fn("wx_group_combine"), 1, &a, op.s, op.timed, 1024);  // WX_GCOMB_BLOCK
  if (read_count(op, ng, h_n_groups) && *h_n_groups > capacity)
    fail(WX_ERR_CAPACITY, "group table / output capacity exceeded");
}

void check_slots(int32_t n_slots, int32_t slot_groups) {
  if (n_slots < 1 || n_slots > WX_GROUP_EXCHANGE_MAX_SLOTS || slot_groups < 1 ||
      (int64_t)n_slots * slot_groups > WX_GROUP_SLOT_MAX)
    fail(WX_ERR_INVALID, "exchange slots: 1 <= n_slots <= 1024, slot_groups >= 1, n_slots * slot_groups <= 4096");
}

void do_group_combine_slots(const double *d_exchange, int32_t n_slots, int32_t slot_groups, int32_t key_lo,
                            const wx_launch *Lp, int64_t capacity, int32_t *d_keys, double *d_sums, int64_t *d_counts,
                            int64_t *d_n_groups, int64_t *h_n_groups) {
  const wx_launch L = launch_of(Lp);
  if (!d_exchange) fail(WX_ERR_INVALID, "null exchange buffer");
  check_slots(n_slots, slot_groups);
  if (capacity < 0 || (capacity > 0 && (!d_keys || !d_sums || !d_counts)))
    fail(WX_ERR_INVALID, "group outputs must hold `capacity` entries");
  if ((int64_t)key_lo + WX_GROUP_WINDOW - 1 > INT32_MAX) fail(WX_ERR_INVALID, "key window out of range");
  Op op(L, util_spec());
  int64_t *ng = count_slot(op.w, op.w.g_ngroups, d_n_groups);
  WxGroupSlotsArgs a;
  a.exchange = d_exchange;
  a.n_slots = n_slots;
  a.slot_groups = slot_groups;
  a.key_lo = key_lo;
  a.out_keys = d_keys;
  a.out_sums = d_sums;
  a.out_counts = reinterpret_cast<wx_i64 *>(d_counts);
  a.capacity = capacity;
  a.n_groups_out = reinterpret_cast<wx_i64 *>(ng);
  launch(op.mod->fn("wx_group_combine_slots"), 1, &a, op.s, op.timed, 1024);  // WX_GCOMB_BLOCK
  if (read_count(op, ng, h_n_groups) && *h_n_groups > capacity)
    fail(WX_ERR_CAPACITY, "group table / output capacity exceeded");
}

void do_group_merge_lists(const void *d_lists, int32_t n_lists, int64_t list_cap, const double *d_window,
                          int32_t key_lo, const wx_launch *Lp, int64_t capacity, int32_t *d_keys, double *d_sums,
                          int64_t *d_counts, int64_t *d_n_groups, int64_t *h_n_groups) {
  const wx_launch L = launch_of(Lp);
  if (n_lists < 1 || n_lists > WX_GROUP_EXCHANGE_MAX_SLOTS) fail(WX_ERR_INVALID, "1 <= n_lists <= 1024");
  if (list_cap < 1 || list_cap > (1ll << 31)) fail(WX_ERR_INVALID, "1 <= list_capacity <= 2^31");
  if (!d_lists) fail(WX_ERR_INVALID, "null list records");
  if (capacity < 0 || (capacity > 0 && (!d_keys || !d_sums || !d_counts)))
    fail(WX_ERR_INVALID, "group outputs must hold `capacity` entries");
  if (d_window && (int64_t)key_lo + WX_GROUP_WINDOW - 1 > INT32_MAX) fail(WX_ERR_INVALID, "key window out of range");
  Op op(L, util_spec());
  const int64_t total = (int64_t)n_lists * list_cap;
  const int64_t n_blk = std::max<int64_t>(1, (total + WX_GLIST_SPAN - 1) / WX_GLIST_SPAN);
  ensure(op.w, op.w.gl_keys, (size_t)total * 4, false);
  ensure(op.w, op.w.gl_sums, (size_t)total * 8, false);
  ensure(op.w, op.w.gl_cnts, (size_t)total * 8, false);
  ensure(op.w, op.w.gl_head, (size_t)total * 4, false);
  ensure(op.w, op.w.gl_blk, (size_t)n_blk * 8, false);
  ensure(op.w, op.w.gl_meta, 64, false);
  int64_t *ng = count_slot(op.w, op.w.g_ngroups, d_n_groups);
  WxGroupListsArgs a;
  a.lists = static_cast<const unsigned char *>(d_lists);
  a.list_bytes = WX_GROUP_LIST_BYTES(list_cap);
  a.list_cap = list_cap;
  a.sums_off = WX_GROUP_LIST_SUMS_OFF(list_cap);
  a.counts_off = WX_GROUP_LIST_COUNTS_OFF(list_cap);
  a.n_lists = n_lists;
  a.key_lo = key_lo;
  a.window = d_window;
  a.m_keys = static_cast<int *>(op.w.gl_keys.p);
  a.m_sums = static_cast<double *>(op.w.gl_sums.p);
  a.m_cnts = static_cast<wx_i64 *>(op.w.gl_cnts.p);
  a.m_head = static_cast<wx_u32 *>(op.w.gl_head.p);
  a.blk = static_cast<wx_i64 *>(op.w.gl_blk.p);
  a.n_blk = n_blk;
  a.meta = static_cast<wx_i64 *>(op.w.gl_meta.p);
  a.out_keys = d_keys;
  a.out_sums = d_sums;
  a.out_counts = reinterpret_cast<wx_i64 *>(d_counts);
  a.capacity = capacity;
  a.n_groups_out = reinterpret_cast<wx_i64 *>(ng);
  launch(op.mod->fn("wx_glist_place"), grid_for(total, op.d.cus, 8), &a, op.s, op.timed);
  launch(op.mod->fn("wx_glist_count"), (unsigned)n_blk, &a, op.s, op.timed, WX_GLIST_BLOCK);
  launch(op.mod->fn("wx_glist_scan"), 1, &a, op.s, op.timed, WX_GLIST_BLOCK);
  launch(op.mod->fn("wx_glist_emit"), (unsigned)n_blk, &a, op.s, op.timed, WX_GLIST_BLOCK);
  if (read_count(op, ng, h_n_groups)) {
    if (*h_n_groups < 0) fail(WX_ERR_CAPACITY, "a shard's group list overflowed its capacity");
    if (*h_n_groups > capacity) fail(WX_ERR_CAPACITY, "group table / output capacity exceeded");
  }
}

}  // namespace wx
