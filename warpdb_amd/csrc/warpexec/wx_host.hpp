// wx_host.hpp -- the one internal header of the host runtime behind
// include/warpexec.h: the types every family's host code shares and, per
// file, the declarations of what the others use from it (DESIGN.md 2 has the
// file table).  Everything here is built with hidden visibility; only the ABI
// is exported.
#pragma once

#pragma GCC visibility push(default)
#include "warpexec.h"
#pragma GCC visibility pop

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../kernels/wx_args.h"
#include "../kernels/wx_select_args.h"
#include "../kernels/wx_window_args.h"
#include "../kernels/wx_join_args.h"
#include "../kernels/wx_gather_args.h"
#include "../kernels/wx_radix_args.h"
#include "../kernels/wx_group_multi_args.h"
#include "../kernels/wx_join_group_args.h"

namespace wx {

struct WxError {
  wx_status st;
  std::string msg;
};

[[noreturn]] inline void fail(wx_status st, const std::string &m) { throw WxError{st, m}; }

#define WX_HIP(call)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess) fail(WX_ERR_DEVICE, std::string("HIP error: ") + #call + ": " +     \
                                                  hipGetErrorString(e_));                     \
  } while (0)

inline std::string env_or(const char *k, const char *dflt) {
  const char *v = std::getenv(k);
  return (v && *v) ? std::string(v) : std::string(dflt);
}

// ------------------------------------------------------------------ modules
struct Module {
  hipModule_t mod = nullptr;
  std::mutex mu;
  std::unordered_map<std::string, hipFunction_t> fns;
  hipFunction_t fn(const char *name) {
    std::lock_guard<std::mutex> lk(mu);
    auto it = fns.find(name);
    if (it != fns.end()) return it->second;
    hipFunction_t f;
    WX_HIP(hipModuleGetFunction(&f, mod, name));
    fns.emplace(name, f);
    return f;
  }
};

// One workspace per (device, stream): look-back tile status, counters,
// reduction partials, group tables, top-K candidates, sort scratch.
struct Buf {
  void *p = nullptr;
  size_t bytes = 0;
};

struct Workspace {
  int device = 0;
  hipStream_t stream = nullptr;
  // Held for a whole operation (enqueue, internal syncs, host reads): two
  // host threads on one (device, stream) -- e.g. pywarpdb calls with the GIL
  // released, all on the null stream -- take turns instead of interleaving
  // epochs, memsets and buffer growth.
  std::recursive_mutex op_mu;
  Buf ctrs;        // u64[8]: [0] ticket, [1] error bits, [2] retired workgroups (compaction)
  Buf status;      // u64[n_tiles + 1] compaction look-back words {epoch | flag | value}
  uint32_t cs_epoch = 0;  // epoch of the last compaction launch (0: words all zero)
  wx_compact_geom cs_last = {0, 0, 0, 0};  // what the last compaction launched (wx_compact_last_launch)
  uint64_t host_word = 0;  // landing slot of small synchronous D2H reads (outlives the copy)
  uint64_t *h_err = nullptr;  // pinned: the error words of ctrs / g_ctrs, read with one stream sync
  bool topk_clean = false;    // topk_thresh is zero (see do_topk)
  Buf part_sum, part_cnt, part_min, part_max;
  Buf sum_out;     // 24 bytes (wx_stats)
  Buf count_tmp;   // i64 scratch for host-count requests
  // group state (kept clean between calls by wx_group_finalize)
  Buf g_win_sum, g_win_cnt, g_tag, g_sum, g_cnt, g_used, g_ctrs, g_ngroups;
  uint32_t g_hcap = 0;
  // MIN / MAX group state: ~0 / 0 when unused (restored by wx_group_finalize)
  Buf g_win_min, g_win_max, g_min, g_max;
  uint32_t g_mm_cap = 0;
  Buf g_sorted;  // large GROUP BY: sorted general-key entries
  // multi-value GROUP BY (wx_group_multi.hip): the value planes of the window
  // and of the general-key table (the counts, tags and used list are the
  // buffers above); idle between calls (sums 0, minima ~0, maxima 0), so only
  // a fresh allocation is filled.  gm_scratch: sums nobody asked for (n_vals == 1)
  Buf gm_win_sum, gm_win_min, gm_win_max, gm_sum, gm_min, gm_max, gm_scratch;
  // many-key list merge (wx_group_merge_lists): merged groups, head flags,
  // per-span head counts, totals
  Buf gl_keys, gl_sums, gl_cnts, gl_head, gl_blk, gl_meta;
  // range-partitioned GROUP BY (many keys): per-workgroup range words,
  // per-(workgroup, partition) rows, the run directory, the tiles' sorted
  // values and bins, work items and their partial windows, the range
  // summary, per-partition key counts; nothing needs zeroing between calls
  Buf gp_order, gp_mm, gp_pcount, gp_ptotal, gp_dir, gp_vals, gp_bins, gp_work, gp_nwork, gp_pitem, gp_psum, gp_pcnt, gp_summary, gp_pnz;
  struct GpMemo {
    int64_t lo = 0, hi = -1;
    bool window = false;  // the range fit the LDS window (taken without a read-back)
    int uses = 0;
  };
  std::unordered_map<uint64_t, GpMemo> gp_memo;  // last key range per (expressions, columns, rows)
  int64_t gp_passes = 0;  // completed partitioned passes (wx_group_part_passes: which route a query took)
  Buf cand_k, cand_i, topk_thresh;
  // ORDER BY .. LIMIT heads of any length: keys, SELECT values, local rows,
  // positions and the passing count of one shard; the merge's candidates
  Buf hd_keys, hd_vals, hd_rows, hd_idx, hd_count, hm_keys, hm_idx, hm_count;
  Buf so_keys, so_rows, so_cnt;  // ordered multi-column SELECT, top-K route: keys, global rows, count
  Buf sort_keys, sort_copy_a, sort_copy_v;
  Buf ro_vals, ro_keys;  // row-order GROUP BY: passing values and keys, sorted by key
  // the general row-order fold: group starts, chunk prefixes, the big groups' count + list
  Buf gf_starts, gf_chunks, gf_big;
  // radix sort: histograms + digit bases, look-back words, per-pass
  // ticket / abort words, ping-pong buffers
  Buf rs_hist, rs_status, rs_ctl, rs_tmp_k, rs_tmp_v;
  uint32_t rs_epoch = 0;
  // row-order GROUP BY over a key span <= 2048 (wx_group_rows.hip):
  // per-range bin counts, per-range output offsets, bin totals and bases
  Buf ro_cnt, ro_off, ro_tot;
  Buf ro_info;  // the direct span path: groups, passing rows, outside flag, min / max key
  // the direct span path's recent misses (a key outside the guessed span):
  // calls left before it is tried again for the same expressions / table
  std::unordered_map<uint64_t, int> ro_miss;
  // what the last row-order GROUP BY did (wx_group_rows_last_call) and where
  // it left its row-ordered values (wx_group_rows_last_values; null: none)
  wx_group_rows_record ro_last = {0, 0, 0, 0, 0, 0, 0};
  const float *ro_last_vals = nullptr;
  // row-order folds of big groups (wx_xf_big_*): entries, chunk sums, chunk records
  Buf xf_ent, xf_approx, xf_rec;
  std::vector<int64_t> xf_host;  // the entries' host copy (outlives its asynchronous upload)
  // window aggregates (wx_window.hip): the group pass's scratch results
  // (keys, counts, group count; sums, minima and maxima per distinct value)
  // and the per-item f32 planes the broadcast reads
  Buf wn_keys, wn_cnts, wn_ng, wn_planes;
  Buf wn_sums[WX_WIN_MAX_VALUES], wn_mins[WX_WIN_MAX_VALUES], wn_maxs[WX_WIN_MAX_VALUES];
  int64_t wn_range[2] = {0, 0};  // landing slot of {group count, first | last key} (outlives the copy)
  // join (wx_join.hip): the build's record, the direct table, the hash table
  Buf jn_rec, jn_rows, jn_slots;
  uint32_t jn_host[WX_JOIN_REC_WORDS] = {};  // landing slot of the record (outlives the copy)
  Buf diag;  // WX_DIAG_TIMELINE per-workgroup times
  std::vector<Buf *> bufs;  // every buffer ensure() has allocated: wx_shutdown frees them all
};

struct DeviceState {
  std::string arch;
  int cus = 256;
  std::unordered_map<std::string, std::shared_ptr<Module>> modules;  // key: query spec
};

class DevGuard {
 public:
  explicit DevGuard(int dev) {
    if (hipGetDevice(&prev_) != hipSuccess) prev_ = -1;
    if (prev_ != dev) WX_HIP(hipSetDevice(dev));
    dev_ = dev;
  }
  ~DevGuard() {
    if (prev_ >= 0 && prev_ != dev_) (void)hipSetDevice(prev_);
  }

 private:
  int prev_ = -1, dev_ = 0;
};

using OpLock = std::lock_guard<std::recursive_mutex>;

// --------------------------------------------------------------- codegen
struct UsedCol {
  std::string name;
  const char *ctype;
  int table_index;
};

struct Spec {
  int op = 0;
  std::vector<UsedCol> cols;
  std::string expr, cond, key, select;
  std::vector<std::string> more;  // multi-output compaction: expressions 1.. (expr is expression 0)
  int topk_k = 0, topk_desc = 1;
  bool aligned = false;
  int groups = 0;  // compaction tile depth (row quads per thread), 0 = n/a
  int dwaves = 0;  // compaction data waves per workgroup
  int gblock = 0, gunroll = 0;  // row gather: threads per workgroup, quads per thread (0 = n/a)
  int minmax = 0;        // SUM / GROUP BY builds that also track MIN / MAX
  int gm_sums = 0, gm_mms = 0;  // multi-value GROUP BY: the values that carry a SUM / a MIN / MAX (bit j: value j)
  // window broadcast (wx_window.hip): outputs of the launch (0 = n/a), which
  // of them are window items, dense (0) or search (1) form; win_exprs[j] is
  // output j's plain expression (empty for a window item), `key` the partition
  int win_nout = 0, win_mask = 0, win_search = 0;
  std::vector<std::string> win_exprs;
  // join probe (wx_join.hip): outputs of the launch (0 = n/a), direct (0) or
  // hash (1) form, inner (0) or left outer (1), which outputs name a right
  // column, whether the WHERE does, whether the matched right row is staged;
  // join_exprs[j] is output j's expression, `key` the left key, rcols the
  // referenced columns of the right table (table_index: into the right table)
  int join_nout = 0, join_form = 0, join_left = 0, join_rmask = 0, join_condr = 0, join_rrow = 0;
  std::vector<std::string> join_exprs;
  std::string join_cond;  // the WHERE (`cond` stays empty: see Spec::source)
  std::vector<UsedCol> rcols;
  // JOIN under GROUP BY (wx_join_group.hip, op WX_OP_JOIN_GROUP): `expr` and
  // `more` are the values, gm_sums / gm_mms their masks, `key` the left join
  // key, `cond` the WHERE, gkey the group key; join_form, join_condr and rcols
  // as for the probe
  std::string gkey;
  std::string custom;
  std::string extra;  // diagnostic -D list from $WARPDB_EXTRA_DEFINES

  std::string key_string() const;
  std::string source() const;
};

// codegen.cpp (no HIP call: it also links into tests/cpp/sanitize_test)
void scan_identifiers(const char *s, std::vector<std::string> &out);
std::vector<UsedCol> used_columns(const wx_table *t, const std::vector<const char *> &exprs);
bool blank(const char *s);
std::string one_line(const char *s);
int define_value(const std::string &extra, const std::string &name, int dflt);
void compact_geometry(Spec &spec);
bool compact_ticket_sched();
int64_t compact_grid_cap();
void select_geometry(Spec &spec, int nout);
void window_geometry(Spec &spec, int nout, int n_items, bool search);
void join_geometry(Spec &spec, int nout, int form, bool right_row);
void gather_geometry(Spec &spec, int nout);
std::string default_arch();
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
void fill_cols(const wx_table *t, const std::vector<UsedCol> &cols, const void **dst);
void check_table(const wx_table *t);
void check_select_exprs(const char *const *exprs, int32_t n_exprs);
void check_row_ids(const wx_table *t, const void *d_out_idx, int32_t idx_bytes, int64_t row_base);
void check_gather_args(const wx_table *t, const char *const *exprs, int32_t n_exprs, int32_t idx_bytes, int64_t count);
wx_launch default_launch();
inline wx_launch launch_of(const wx_launch *Lp) { return Lp ? *Lp : default_launch(); }
// One builder per module family, shared by the run path and the prepare
// entry points, so the two cannot name different programs.
Spec project_spec(const wx_table *t, int op, const char *expr, const char *cond, const wx_launch &L, bool out_aligned,
                  const char *also = nullptr);
Spec sum_spec(const wx_table *t, const char *expr, const char *cond, const wx_launch &L, bool minmax,
              const char *also = nullptr);
Spec topk_spec(const wx_table *t, const char *order_expr, const char *cond, const char *select_expr, int32_t k,
               int32_t desc, const wx_launch &L);
Spec group_spec(const wx_table *t, const char *val_expr, const char *key_expr, const char *cond, const wx_launch &L,
                bool minmax);
Spec group_multi_spec(const wx_table *t, const char *const *val_exprs, int32_t n_vals, int sum_mask, int mm_mask,
                      const char *key_expr, const char *cond, const wx_launch &L);
void check_group_multi_exprs(const char *const *val_exprs, int32_t n_vals, const char *key_expr);
void check_group_multi_masks(int32_t n_vals, int sum_mask, int mm_mask);
Spec select_spec(const wx_table *t, const char *const *exprs, int32_t n_exprs, const char *cond, const wx_launch &L);
Spec gather_spec(const wx_table *t, const char *const *exprs, int32_t n_exprs, const wx_launch &L);
// One launch of the window broadcast: n_out outputs, exprs[j] null for a
// window item (bit j of win_mask).  The call's column limit is
// check_window_args's.
Spec window_spec(const wx_table *t, const char *const *exprs, int32_t n_out, int win_mask, bool search,
                 const char *part_expr, const char *cond, const wx_launch &L);
Spec window_table_spec();
void check_window_args(const wx_table *t, const char *const *exprs, int32_t n_exprs, const wx_window_item *items,
                       int32_t n_items, const char *part_expr, const char *cond);
// The join family.  JoinNames: what a call's expressions reference in each
// table, checked without a device (check_join_args); join_spec: one launch of
// the probe over outputs [first, first + n_out) of the call.
struct JoinNames {
  std::vector<UsedCol> left, right;  // over the whole call
  int right_key = -1;                // index of right_key_col in the right table
};
JoinNames check_join_args(const wx_table *left, const wx_table *right, const char *left_key_expr,
                          const char *right_key_col, int32_t join_type, const char *const *exprs, int32_t n_exprs,
                          const char *cond);
Spec join_spec(const wx_table *left, const wx_table *right, const char *const *exprs, int32_t n_out, int form,
               bool left_outer, bool right_row, const char *left_key_expr, const char *cond, const wx_launch &L);
Spec join_table_spec();
// One launch of the grouped pass over a join: 1 .. WX_GM_MAX values.  The
// call's checks are check_join_group_args's (n_vals, blank expressions, then
// check_join_args over the values, the group key and the WHERE, then INNER).
JoinNames check_join_group_args(const wx_table *left, const wx_table *right, const char *left_key_expr,
                                const char *right_key_col, int32_t join_type, const char *const *val_exprs,
                                int32_t n_vals, const char *group_key_expr, const char *cond);
Spec join_group_spec(const wx_table *left, const wx_table *right, const char *const *val_exprs, int32_t n_vals,
                     int sum_mask, int mm_mask, int form, const char *left_key_expr, const char *group_key_expr,
                     const char *cond, const wx_launch &L);
struct JoinPlan {
  int form = WX_JOIN_FORM_HASH;
  int log2cap = WX_JOIN_MIN_LOG2CAP;  // hash form: log2 of the slots (0 in the direct form)
};
JoinPlan join_plan(int64_t n_right, int32_t key_min, int32_t key_max);
Spec util_spec(const std::string &more = "");

// runtime.cpp
uint64_t fnv1a(const std::string &s);
void ensure(Workspace &w, Buf &b, size_t bytes, bool zero);
DeviceState &device_state(int dev, bool need_device);
Workspace &workspace(int dev, hipStream_t s);
Workspace *find_workspace(int dev, hipStream_t s);
std::shared_ptr<Module> get_module(int dev, const Spec &spec, bool load);
void prepare_module(const wx_launch &L, const Spec &spec);
bool device_visible(const wx_launch &L);
void launch(hipFunction_t f, unsigned grid, void *args, hipStream_t s, bool timed = false,
            unsigned block = WX_BLOCK, unsigned shmem = 0);
void check_errors(Workspace &w);
unsigned grid_for(int64_t work_items, int cus, int per_cu);
void timing_take(int32_t device, double *total_ms, int64_t *launches);
void cache_stats(int64_t *compiles, int64_t *hits);
void shutdown();

// What every operation opens with, acquired in the order the calls rely on:
// the device guard before any device call, then the module (so a compile
// never runs under the operation lock), then the workspace, then its lock.
// Nested operations (do_order_head -> do_project_filter / do_sort,
// do_select_ordered -> do_topk / do_gather_multi) open their own on the same
// workspace: the lock is recursive.
struct Op {
  const wx_launch L;
  DevGuard guard;
  hipStream_t s;
  std::shared_ptr<Module> mod;  // null for an operation that only calls others
  DeviceState &d;
  Workspace &w;
  OpLock lock;
  const bool timed;
  explicit Op(const wx_launch &l) : Op(l, nullptr) {}
  Op(const wx_launch &l, const Spec &spec) : Op(l, &spec) {}

 private:
  Op(const wx_launch &l, const Spec *spec)
      : L(l),
        guard(l.device),
        s(static_cast<hipStream_t>(l.stream)),
        mod(spec ? get_module(l.device, *spec, true) : nullptr),
        d(device_state(l.device, true)),
        w(workspace(l.device, s)),
        lock(w.op_mu),
        timed((l.flags & WX_F_TIME) != 0) {}
};

int64_t *count_slot(Workspace &w, Buf &b, int64_t *d_dst, bool need = true);
bool read_count(Op &op, const int64_t *d_src, int64_t *h_dst);

template <typename F>
wx_status guarded(char *err, size_t errlen, F &&body) {
  if (err && errlen) err[0] = 0;
  try {
    body();
    return WX_OK;
  } catch (const WxError &e) {
    if (err && errlen) std::snprintf(err, errlen, "%s", e.msg.c_str());
    return e.st;
  } catch (const std::bad_alloc &) {
    if (err && errlen) std::snprintf(err, errlen, "out of host memory");
    return WX_ERR_INTERNAL;
  } catch (const std::exception &e) {
    if (err && errlen) std::snprintf(err, errlen, "%s", e.what());
    return WX_ERR_INTERNAL;
  }
}

// ----------------------------------------------------------- operations
// compact.cpp
void do_project_filter(const wx_table *t, const char *expr, const char *cond, const wx_launch *Lp, int32_t mode,
                       float *d_out_vals, void *d_out_idx, int32_t idx_bytes, int64_t row_base,
                       int64_t *d_count, int64_t *h_count);
void do_project_filter_multi(const wx_table *t, const char *const *exprs, int32_t n_exprs, const char *cond,
                             const wx_launch *Lp, int32_t mode, float *const *d_out_vals, void *d_out_idx,
                             int32_t idx_bytes, int64_t row_base, int64_t *d_count, int64_t *h_count);
void do_reduce_sum(const wx_table *t, const char *expr, const char *cond, const wx_launch *Lp, void *d_out,
                   double *h_sum, int64_t *h_count, bool minmax = false, wx_stats *h_stats = nullptr);
void do_cast(const void *src, int32_t sdt, void *dst, int32_t ddt, int64_t n, const wx_launch *Lp);
void compact_launch(Op &op, const Spec &spec, const wx_table *t, WxCompactArgs &c, void *args, const char *deep_fn,
                    const char *ticket_fn, void *d_out_idx, int32_t idx_bytes, int64_t row_base, int64_t *d_count,
                    int64_t *h_count);

// window.cpp
void do_window_select(const wx_table *t, const char *const *exprs, int32_t n_exprs, const wx_window_item *items,
                      int32_t n_items, const char *part_expr, const char *cond, const wx_launch *Lp, int32_t key_lo,
                      int64_t group_capacity, float *const *d_out_vals, void *d_out_idx, int32_t idx_bytes,
                      int64_t row_base, int64_t *d_count, int64_t *h_count);
void do_prepare_window(const wx_table *t, const char *const *exprs, int32_t n_exprs, const wx_window_item *items,
                       int32_t n_items, const char *part_expr, const char *cond, const wx_launch *Lp, int32_t search);

// join.cpp
void do_join_select(const wx_table *left, const wx_table *right, const char *left_key_expr, const char *right_key_col,
                    int32_t join_type, const char *const *exprs, int32_t n_exprs, const char *cond,
                    const wx_launch *Lp, float *const *d_out_vals, void *d_out_idx, int32_t idx_bytes,
                    int64_t row_base, int32_t *d_out_right_row, int64_t *d_count, int64_t *h_count);
void do_prepare_join(const wx_table *left, const wx_table *right, const char *left_key_expr, const char *right_key_col,
                     int32_t join_type, const char *const *exprs, int32_t n_exprs, const char *cond,
                     const wx_launch *Lp, int32_t with_right_row, int32_t form);
// The right table's key range and its direct or hash table in the workspace
// of `op` (opened on join_table_spec()): two synchronisations, the second for
// the duplicate report.  What a probe needs of the result.
struct JoinTable {
  JoinPlan plan;
  int32_t key_lo = 0;
  wx_u32 span = 0;   // direct form: keys lie in [key_lo, key_lo + span)
  wx_u32 mask = 0;   // hash form: slots - 1
  int shift = 0;     // hash form: 32 - log2cap
};
JoinTable build_join_table(Op &op, const int *d_rkeys, int64_t n_right);

// join_group.cpp
void do_join_group(const wx_table *left, const wx_table *right, const char *left_key_expr, const char *right_key_col,
                   int32_t join_type, const char *const *val_exprs, int32_t n_vals, const char *group_key_expr,
                   const char *cond, const wx_launch *Lp, int32_t key_lo, int64_t capacity, int32_t *d_keys,
                   double *const *d_sums, int64_t *d_counts, float *const *d_mins, float *const *d_maxs,
                   int64_t *d_n_groups, int64_t *h_n_groups);
void do_prepare_join_group(const wx_table *left, const wx_table *right, const char *left_key_expr,
                           const char *right_key_col, int32_t join_type, const char *const *val_exprs, int32_t n_vals,
                           int sum_mask, int mm_mask, const char *group_key_expr, const char *cond,
                           const wx_launch *Lp, int32_t form);

// group.cpp
struct KeyRange {
  bool any = false;
  int64_t lo = 0, hi = -1, passing = 0;
  int64_t span() const { return hi - lo + 1; }
};
uint32_t next_pow2(uint64_t v);
int64_t gp_min_rows();
struct GpPlan {
  int64_t tile_rows = 0;     // rows of one tile
  int64_t n_tiles = 0;       // tiles of the table
  int64_t grid = 0;          // tile workgroups
  int64_t tiles_per_wg = 0;  // tiles of every workgroup but (possibly) the last
  int n_part = 0;            // partitions
  int64_t part_keys = 0;     // keys per partition
  int64_t chunk_rows = 0;    // the floor of a work item's rows
  int64_t target_items = 0;  // work items the plan aims at over all passing rows
  int64_t work_cap = 0;      // most work items
  int dir_chunk = 0;         // directory words the aggregation stages per round
  int agg_sweep = 0;         // tiles all waves of an aggregating workgroup take per sweep
};
GpPlan gp_plan(int64_t n_rows, int64_t span, int cus, const std::string &extra);
void ensure_group_table(Workspace &w, hipStream_t s, uint32_t hcap);
KeyRange sample_keys(const wx_table *t, const std::vector<UsedCol> &cols, Module *mod, Workspace &w, hipStream_t s,
                     bool timed);
uint64_t gp_memo_key(const Spec &spec, const wx_table *t, const std::vector<UsedCol> &cols);
void check_slots(int32_t n_slots, int32_t slot_groups);
void do_group_sum(const wx_table *t, const char *val_expr, const char *key_expr, const char *cond,
                  const wx_launch *Lp, int32_t key_lo, int64_t capacity, int32_t *d_keys, double *d_sums,
                  int64_t *d_counts, int64_t *d_n_groups, int64_t *h_n_groups, float *d_mins = nullptr,
                  float *d_maxs = nullptr, double *d_window = nullptr, int32_t n_slots = 0, int32_t slot_rank = 0,
                  int32_t slot_groups = 0);
void do_group_combine(const double *d_window, int32_t key_lo, const int32_t *xk, const double *xs, const int64_t *xc,
                      int64_t n_extra, const wx_launch *Lp, int64_t capacity, int32_t *d_keys, double *d_sums,
                      int64_t *d_counts, int64_t *d_n_groups, int64_t *h_n_groups);
void do_group_combine_slots(const double *d_exchange, int32_t n_slots, int32_t slot_groups, int32_t key_lo,
                            const wx_launch *Lp, int64_t capacity, int32_t *d_keys, double *d_sums, int64_t *d_counts,
                            int64_t *d_n_groups, int64_t *h_n_groups);
void do_group_merge_lists(const void *d_lists, int32_t n_lists, int64_t list_cap, const double *d_window,
                          int32_t key_lo, const wx_launch *Lp, int64_t capacity, int32_t *d_keys, double *d_sums,
                          int64_t *d_counts, int64_t *d_n_groups, int64_t *h_n_groups);

// group_multi.cpp
void do_group_multi(const wx_table *t, const char *const *val_exprs, int32_t n_vals, const char *key_expr,
                    const char *cond, const wx_launch *Lp, int32_t key_lo, int64_t capacity, int32_t *d_keys,
                    double *const *d_sums, int64_t *d_counts, float *const *d_mins, float *const *d_maxs,
                    int64_t *d_n_groups, int64_t *h_n_groups);

// group_window.cpp: shared by the LDS-window GROUP BY families
int popcount4(int m);
struct GroupWindowPlan {
  int block = 0;            // threads per workgroup
  int64_t span_rows = 0;    // rows of one batch span (block * WX_UNROLL quads)
  unsigned grid = 1;        // workgroups of the streaming kernel
  int64_t max_batches = 0;  // batches of the workgroup that runs the most
  int lead = 0;             // WX_GROUP_LEAD of the build (0: no wave-combined add)
};
GroupWindowPlan group_window_plan(int64_t n_rows, int ns, int nq, int family, int form, int cus,
                                  const std::string &extra);
void ensure_planes(Workspace &w, hipStream_t s, Buf &b, size_t bytes, int fill);
WxGroupPlanes group_planes(Workspace &w, hipStream_t s, int ns, int nq, int64_t capacity, int key_lo);
const wx_u64 *sort_general_keys(Op &op, Module *own, wx_u64 *ctrs, wx_u32 *h_used, wx_u64 *h_tag, int64_t capacity,
                                bool any_rows);
void finish_group(Op &op, hipFunction_t finalize, void *fin_args, int64_t *ng, int64_t *h_n_groups);

// group_rows.cpp
// Sizes of the row-order kernels that only their sources name (the kernel
// sources stay as they are: their text keys the code-object cache); the host
// uses them and wx_group_rows_geometry reports them, and
// tests/test_ro_layouts.py reads the sources and checks each against them.
constexpr int kRoSpanBins = 2048;                  // WX_RO_BINS (wx_group_rows.hip)
constexpr int kRoCountRows = WX_RO_THREADS * 8;    // one span of wx_ro_count's loop: eight rows per thread
constexpr int kRleWaveRows = 16384;                // sorted rows per wave of wx_rle_* until 32 768 ranges are reached
constexpr int kXfJ = 8, kXfAhead = 4;              // WX_XF_J / WX_XF_AHEAD defaults (wx_util.hip)
constexpr int kSampleGrid = 64;                    // workgroups of wx_group_part_sample (sample_keys)
void do_group_sum_rows(const wx_table *t, const char *val_expr, const char *key_expr, const char *cond,
                       const wx_launch &L, int32_t key_lo, int64_t capacity, int32_t *d_keys, double *d_sums,
                       int64_t *d_counts, int64_t *d_n_groups, int64_t *h_n_groups, float *d_mins, float *d_maxs);

// sort.cpp
std::shared_ptr<Module> util_module(int dev, bool load, const std::string &more = "");
std::string rs_rank_extra(const std::string &arch);
void rs_tile_shape(bool pairs, int *items, int *block);
std::string rs_geometry(bool pairs, int *items, int *block, const std::string &arch);
void bitonic_u64(int dev, wx_u64 *keys, int64_t npad, hipStream_t s);
// the LSD radix sort; with res_k the sorted keys and payload are left
// wherever the last pass wrote them (*res_k / *res_v) instead of being
// copied back into d_a / d_v
void radix_sort(void *d_a, float *d_v, int64_t count, int kind, int32_t ascending, const wx_launch &L, Workspace &w,
                hipStream_t s, int64_t limit = -1, const void *src0 = nullptr, void **res_k = nullptr,
                float **res_v = nullptr, const float *src_v = nullptr);
void do_sort(void *d_a, float *d_v, int64_t count, int kind, int32_t ascending, const wx_launch *Lp,
             int64_t limit = -1, const void *src = nullptr);

// topk.cpp
struct TopkPlan {
  unsigned grid = 1;        // scan workgroups
  int64_t nq = 0;           // row quads of the table
  int64_t span = 0;         // quads per batch span
  int64_t max_batches = 0;  // batches of the workgroup that runs the most
  int64_t seed_grid = 0;    // seed workgroups (0: no seed pass)
  int64_t seed_stride = 0;  // quads between the seed workgroups' spans
};
TopkPlan topk_plan(int64_t n_rows, int32_t k, int cus, const std::string &extra);
void do_topk(const wx_table *t, const char *order_expr, const char *cond, const char *select_expr, int32_t k,
             int32_t desc, const wx_launch *Lp, int64_t row_base, float *d_keys, int64_t *d_idx, float *d_vals,
             int64_t *d_count, int64_t *h_count);
void do_topk_merge(const wx_topk_record *recs, int32_t n_records, int32_t k, int32_t desc, const wx_launch *Lp,
                   float *d_keys, int64_t *d_idx, float *d_vals, int64_t *d_count, int64_t *h_count);
void do_order_head(const wx_table *t, const char *order_expr, const char *cond, const char *select_expr, int64_t limit,
                   int32_t desc, const wx_launch *Lp, int64_t row_base, void *d_record, int64_t cap);
void do_head_merge(const void *recs, int32_t n_records, int64_t cap, int64_t limit, int32_t desc, const wx_launch *Lp,
                   float *d_keys, int64_t *d_rows, float *d_vals, int64_t *d_count, int64_t *h_count);

// select_ordered.cpp
void do_gather_multi(const wx_table *t, const char *const *exprs, int32_t n_exprs, const void *d_rows,
                     int32_t idx_bytes, int64_t row_base, int64_t count, const int64_t *d_count, const wx_launch *Lp,
                     float *const *d_out_vals, int64_t *d_out_rows, int64_t out_row_base);
void do_select_ordered(const wx_table *t, const char *const *exprs, int32_t n_exprs, const char *cond,
                       const char *order_expr, int32_t desc, int64_t limit, const wx_launch *Lp, int64_t row_base,
                       float *const *d_out_vals, float *d_out_keys, int64_t *d_out_rows, int64_t capacity,
                       int64_t *d_count, int64_t *h_count);

}  // namespace wx
