/*
 * warpexec.h -- C ABI of the MI355X (gfx950) query execution layer.
 *
 * This is the drop-in boundary for WarpDB's execution path.  Every entry
 * point takes plain pointers and sizes, returns a wx_status and reports
 * failures through an (err, errlen) buffer; no C++ exception and no torch
 * type crosses it.  Device buffers are caller-owned (hipMalloc / torch);
 * warpexec owns only its compiled kernel cache and a per-(device, stream)
 * workspace.
 *
 * Reference interfaces replaced (paths relative to the WarpDB snapshot):
 *   wx_project_filter   jit_compile_and_launch   include/jit.hpp:7-10, src/jit.cpp:48-174
 *                       + the launch/D2H part of WarpDB::query src/warpdb.cpp:243-256
 *   wx_group_sum        jit_group_sum            include/jit.hpp:15-18, src/jit.cpp:179-246
 *   wx_sort_pairs       jit_sort_pairs           include/jit.hpp:22-23, src/jit.cpp:248-281
 *   wx_sort_float       jit_sort_float           include/jit.hpp:26-27, src/jit.cpp:283-307
 *   wx_sort_float_from  projection + jit_sort_float of ORDER BY <column>  src/warpdb.cpp:450-455
 *   wx_sort_by_key      ORDER BY <expr> keyed sort  src/warpdb.cpp:470-476
 *   wx_topk             jit_sort_float + LIMIT   src/warpdb.cpp:453-455,483-495
 *   wx_reduce_sum       per-shard SUM of query_multi_gpu (new; the reference
 *                       gathers dense results on the host, src/multi_gpu_utils.cpp:5-63)
 *   wx_reduce_stats     ungrouped SUM / COUNT / AVG / MIN / MAX of query_sql
 *                       (src/warpdb.cpp:297-498, AggData :383-384) and the column
 *                       statistics of the optimizer (include/csv_loader.hpp:22-37,
 *                       src/optimizer.cpp:13-17)
 *   wx_group_agg        jit_group_sum + the per-group MIN / MAX of query_sql's
 *                       AggData (src/warpdb.cpp:375-385)
 *   wx_group_agg_multi  the same for 2 .. 4 value expressions of one GROUP BY in
 *                       one pass (new; query_sql aggregates one expression,
 *                       src/warpdb.cpp:375-385)
 *   wx_group_partials,  GROUP BY over row shards: per-shard
 *   wx_group_combine    partials in an all-reduce layout and the final merge;
 *                       the reference's multi-GPU path gathers dense results
 *                       on the host instead (src/multi_gpu_utils.cpp:5-63)
 *   wx_group_partials_slots,  the same in ONE collective: window + per-shard
 *   wx_group_combine_slots    slots of out-of-window groups (src/multi_gpu_utils.cpp:23-60)
 *   wx_group_merge_lists  GROUP BY over row shards with many groups: the
 *                       device merge of the shards' gathered group lists (the
 *                       reference gathers on the host, src/multi_gpu_utils.cpp:23-60)
 *   wx_topk_merge       ORDER BY .. LIMIT over row shards: the merge of the
 *                       shards' candidate records (src/warpdb.cpp:453-455,
 *                       483-495 sort the gathered dense results instead)
 *   wx_cast             device-side type conversion (jit_group_sum's float
 *                       outputs, include/jit.hpp:15-18)
 *
 * Expression inputs are the reference's lowered C expressions over
 * identifiers `<column>[idx]` (include/expression.hpp:32-78), e.g.
 * "(price[idx] * quantity[idx])".  An empty / NULL condition means no filter
 * (src/jit.cpp:56).  The text of custom.cu (or custom_src) is prepended to
 * every generated kernel exactly as src/jit.cpp:65-73 does.
 *
 * All work is enqueued on `stream` (a hipStream_t; NULL = the null stream)
 * and is asynchronous unless WX_F_SYNC is set or a host output pointer is
 * passed, in which case the call returns with results complete.
 */
#ifndef WARPEXEC_H
#define WARPEXEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WX_ABI_VERSION 1

typedef enum wx_status {
  WX_OK = 0,
  WX_ERR_INVALID = 1,     /* bad argument / unknown column type / overflow */
  WX_ERR_COMPILE = 2,     /* hiprtc failed; err holds the compiler log */
  WX_ERR_DEVICE = 3,      /* a HIP runtime call failed */
  WX_ERR_CAPACITY = 4,    /* an output or group table was too small */
  WX_ERR_UNSUPPORTED = 5, /* request outside what the engine implements */
  WX_ERR_INTERNAL = 6     /* a device-side check failed (e.g. look-back timeout) */
} wx_status;

/* Same numbering as WarpDB's DataType (include/csv_loader.hpp:13). */
typedef enum wx_dtype {
  WX_INT32 = 0,
  WX_INT64 = 1,
  WX_FLOAT32 = 2,
  WX_FLOAT64 = 3,
  WX_STRING = 4 /* accepted in a table, cannot be referenced by an expression */
} wx_dtype;

/* One device column: mirrors ColumnDesc (include/csv_loader.hpp:15-20);
 * the length is the table's n_rows. */
typedef struct wx_col {
  const char *name;
  int32_t dtype;
  const void *d_ptr;
} wx_col;

/* Mirrors Table (include/csv_loader.hpp:39-51) with 64-bit row counts. */
typedef struct wx_table {
  int64_t n_rows;
  int32_t n_cols;
  const wx_col *cols;
} wx_table;

/* Where and how to run. */
typedef struct wx_launch {
  int32_t device;         /* HIP device ordinal */
  void *stream;           /* hipStream_t (NULL = null stream) */
  const char *custom_src; /* NULL: read $WARPDB_CUSTOM_PATH or ./custom.cu per call */
  uint32_t flags;         /* WX_F_* */
} wx_launch;

#define WX_F_SYNC 1u      /* synchronise the stream and check device errors before returning */
#define WX_F_NO_CUSTOM 2u /* do not prepend custom.cu */
#define WX_F_TIME 4u      /* record HIP events around the main kernel (wx_timing_read) */
#define WX_F_F64_COUNTS 8u /* wx_reduce_sum: d_out's count is written as a double (exact below
                            * 2^53), so ONE all-reduce of two doubles combines shards */
#define WX_F_ROW_ORDER 16u /* wx_group_sum / wx_group_agg: each group's sum folded in ascending row
                            * order, one double add per row -- the reference's std::map fold
                            * (src/warpdb.cpp:373-385) to the bit, the same on every run.
                            * Synchronous; two ordered compactions, a stable pair sort and a
                            * per-group fold whose time grows with the largest group's rows */

/* wx_project_filter modes */
#define WX_MODE_DENSE 0      /* out_vals[row] = expr where cond holds, other rows untouched (src/jit.cpp:55-61) */
#define WX_MODE_DENSE_FILL 1 /* as DENSE, other rows set to 0.0f */
#define WX_MODE_COMPACT 2    /* ordered stream compaction: k-th passing row -> out_vals[k], out_idx[k] */

/* Project + filter.  DENSE modes write n_rows floats to d_out_vals.
 * COMPACT writes the passing rows in ascending row order: d_out_vals[k] (nullable)
 * and d_out_idx[k] = row_base + row (nullable; idx_bytes 4 -> int32, 8 -> int64);
 * both must hold n_rows entries.  d_count (device int64, nullable) receives the
 * passing count; h_count (host, nullable) too, which synchronises. */
wx_status wx_project_filter(const wx_table *table, const char *expr, const char *cond,
                            const wx_launch *launch, int32_t mode, float *d_out_vals,
                            void *d_out_idx, int32_t idx_bytes, int64_t row_base,
                            int64_t *d_count, int64_t *h_count, char *err, size_t errlen);

/* Project + filter with several outputs (a multi-column SELECT): n_exprs
 * expressions of the same filtered rows in ONE pass -- the columns are read,
 * the condition evaluated and the rows ranked once.  d_out_vals[j][k]
 * (each pointer nullable, n_rows entries) = (float)exprs[j] of the k-th
 * passing row; d_out_idx / idx_bytes / row_base / d_count / h_count as in
 * wx_project_filter.  n_exprs == 1 is wx_project_filter itself (same module,
 * any mode); 2 .. WX_MAX_OUTPUTS need WX_MODE_COMPACT (a DENSE mode returns
 * WX_ERR_UNSUPPORTED).  n_exprs outside 1 .. WX_MAX_OUTPUTS or a blank
 * expression returns WX_ERR_INVALID.  The expressions and the condition
 * together may reference at most 16 columns. */
#define WX_MAX_OUTPUTS 4
wx_status wx_project_filter_multi(const wx_table *table, const char *const *exprs, int32_t n_exprs,
                                  const char *cond, const wx_launch *launch, int32_t mode,
                                  float *const *d_out_vals, void *d_out_idx, int32_t idx_bytes,
                                  int64_t row_base, int64_t *d_count, int64_t *h_count,
                                  char *err, size_t errlen);
/* Build (and cache) the module wx_project_filter_multi would use in
 * WX_MODE_COMPACT, without launching (works without a GPU, like wx_prepare). */
wx_status wx_prepare_multi(const wx_table *table, const char *const *exprs, int32_t n_exprs,
                           const char *cond, const wx_launch *launch, char *err, size_t errlen);
/* Rows per compaction tile of an n_exprs-output call (it shrinks as the
 * outputs grow; the diagnostic define list may override it); 0 when n_exprs
 * is out of range or the geometry is invalid. */
int32_t wx_select_tile_rows(int32_t n_exprs);
/* What the last ordered compaction on the launch's (device, stream) launched
 * -- wx_project_filter in WX_MODE_COMPACT, wx_project_filter_multi, a
 * broadcast launch of wx_window_select, a probe launch of wx_join_select:
 * plain host numbers (no device read, no synchronisation).  All zero before
 * any such launch and after a call over an empty table.  The pipelined
 * kernel runs min(n_tiles, resident workgroups) workgroups that take tiles
 * from a ticket counter; the diagnostic variable WARPDB_COMPACT_GRID=<n>
 * (an integer >= 1, else WX_ERR_INVALID from the compacting call) caps that
 * grid, so that few workgroups run many tiles each.  The one-tile-per-
 * workgroup schedule (WARPDB_COMPACT_SCHED=ticket) ignores the cap. */
typedef struct wx_compact_geom {
  int64_t tile_rows; /* rows of one tile */
  int64_t n_tiles;   /* tiles of the table */
  int64_t grid;      /* workgroups launched (n_tiles under the ticket schedule) */
  int64_t deep;      /* 1: the pipelined kernel, 0: one tile per workgroup */
} wx_compact_geom;
wx_status wx_compact_last_launch(const wx_launch *launch, wx_compact_geom *out, char *err, size_t errlen);

/* Row gather with several outputs (late materialisation): n_exprs
 * expressions (1 .. WX_MAX_OUTPUTS) at a list of row ids.  For k < count,
 * row = d_rows[k] - row_base (ids of idx_bytes 4 -> int32 or 8 -> int64,
 * e.g. the row ids of wx_project_filter or wx_topk); d_out_vals[j][k] (each
 * pointer nullable) = (float)exprs[j] at that row and d_out_rows[k]
 * (nullable) = out_row_base + row.  Each referenced column is read once per
 * row.  d_count (device int64, nullable) bounds the count further on the
 * device (min(count, *d_count)), so the ids of an asynchronous call can be
 * consumed without a host read.  A row outside [0, n_rows) reads no memory
 * and every output holds NaN there; nothing is written at k >= count.
 * Asynchronous unless WX_F_SYNC is set.  n_exprs out of range, a blank
 * expression, idx_bytes other than 4 / 8 or a negative count return
 * WX_ERR_INVALID. */
wx_status wx_gather_multi(const wx_table *table, const char *const *exprs, int32_t n_exprs,
                          const void *d_rows, int32_t idx_bytes, int64_t row_base, int64_t count,
                          const int64_t *d_count, const wx_launch *launch, float *const *d_out_vals,
                          int64_t *d_out_rows, int64_t out_row_base, char *err, size_t errlen);
/* Build (and cache) the module wx_gather_multi would use, without launching
 * (works without a GPU, like wx_prepare). */
wx_status wx_prepare_gather(const wx_table *table, const char *const *exprs, int32_t n_exprs,
                            const wx_launch *launch, char *err, size_t errlen);
/* Output positions per workgroup iteration of an n_exprs-output gather (the
 * diagnostic define list may override the geometry); 0 when n_exprs is out
 * of range or the geometry is invalid. */
int32_t wx_gather_tile_rows(int32_t n_exprs);

/* ORDER BY order_expr [DESC] [LIMIT limit] over a multi-column SELECT:
 * n_exprs expressions (0 .. WX_ORDERED_MAX_EXPRS; 0 = keys and rows only) of
 * the rows passing cond, in the order of wx_sort_by_key and wx_topk (NaN keys
 * last in both directions, -0.0 == +0.0, ties by ascending row).  The first
 * min(limit, passing) positions (limit < 0: all) of d_out_keys (the order
 * keys), d_out_rows (row_base + row) and d_out_vals[j] are written; every
 * output pointer is nullable and holds `capacity` entries.  The count goes
 * to d_count / h_count; a result longer than capacity returns
 * WX_ERR_CAPACITY with the needed count in *h_count.  The sorted row ids are
 * computed once, whatever n_exprs: limit <= 32 takes one wx_topk scan and
 * stays asynchronous (unless h_count is given, or capacity < limit, which
 * needs a host read of the count); otherwise one ordered compaction of the
 * key with int32 row ids, a stable pair sort with the row ids as payload
 * (limited to the head) and the gather, synchronous (scratch: 8 bytes per
 * table row; at most 2^31 - 1 rows, WX_ERR_UNSUPPORTED beyond).  The
 * expressions are gathered at the sorted rows in chunks of WX_MAX_OUTPUTS.
 * $WARPDB_ORDERED_ROUTE=sort forces the second route for small limits. */
#define WX_ORDERED_MAX_EXPRS 16
wx_status wx_select_ordered(const wx_table *table, const char *const *exprs, int32_t n_exprs,
                            const char *cond, const char *order_expr, int32_t descending, int64_t limit,
                            const wx_launch *launch, int64_t row_base, float *const *d_out_vals,
                            float *d_out_keys, int64_t *d_out_rows, int64_t capacity, int64_t *d_count,
                            int64_t *h_count, char *err, size_t errlen);

/* SUM((float)expr) over rows where cond holds, accumulated in double.
 * d_out (device, nullable) receives {sum as double, count as int64 bits};
 * h_sum / h_count (host, nullable) synchronise. */
wx_status wx_reduce_sum(const wx_table *table, const char *expr, const char *cond,
                        const wx_launch *launch, void *d_out, double *h_sum, int64_t *h_count,
                        char *err, size_t errlen);

/* SUM / COUNT / MIN / MAX of (float)expr over rows where cond holds.  MIN and
 * MAX skip NaN values and read NaN when no value qualifies (SQL NULL); -0.0
 * and +0.0 compare equal and come back as +0.0. */
typedef struct wx_stats {
  double sum;
  int64_t count;
  float min;
  float max;
} wx_stats;

/* d_out (device, nullable): a wx_stats; h_out (host, nullable) synchronises. */
wx_status wx_reduce_stats(const wx_table *table, const char *expr, const char *cond,
                          const wx_launch *launch, void *d_out, wx_stats *h_out, char *err,
                          size_t errlen);

/* SUM((float)val_expr) GROUP BY (int)key_expr WHERE cond.  Sums in double,
 * counts in int64, groups in ascending key order.  capacity = entries of the
 * device outputs (and the distinct-key bound of the general-key table).
 * Keys in [key_window_lo, key_window_lo + 2048) take the LDS fast path; at
 * most 4096 distinct keys may fall outside it unless capacity is larger.
 * With capacity > 4096 on >= 2^20 rows (a caller expecting many groups) the
 * call first takes a key-range guess: the previous call's over the same
 * expressions, columns and row count (no host read), else a 65 536-row sample
 * (one host synchronisation), else an exact min / max pass (one more).  A
 * range of at most 2048 keys moves the window onto it and the call stays
 * asynchronous after that; a range of up to 2^24 keys runs the
 * range-partitioned kernels, which end with one host read
 * of their range summary (the call returns with the result complete, and
 * runs again over the exact range when a row fell outside the guess); a
 * wider one the window + hash path.  Results are the same either way. */
wx_status wx_group_sum(const wx_table *table, const char *val_expr, const char *key_expr,
                       const char *cond, const wx_launch *launch, int32_t key_window_lo,
                       int64_t capacity, int32_t *d_keys, double *d_sums, int64_t *d_counts,
                       int64_t *d_n_groups, int64_t *h_n_groups, char *err, size_t errlen);

/* On WX_ERR_CAPACITY from wx_group_sum / wx_group_agg, *h_n_groups (when
 * given) holds the number of groups found, a lower bound of the capacity
 * needed (exact unless the general-key table itself overflowed). */

/* Row-sharded GROUP BY, step 1 (per shard): SUM((float)val_expr) GROUP BY
 * (int)key_expr WHERE cond in the exchange layout.  d_window (device,
 * WX_GROUP_EXCHANGE_DOUBLES doubles) receives the dense key window
 * [key_window_lo, key_window_lo + WX_GROUP_WINDOW_BINS): the sums at
 * [0, W), the counts as doubles at [W, 2W) (exact below 2^53), and at [2W]
 * the number of groups outside the window.  Summing the shards' buffers
 * element-wise -- one ncclAllReduce(SUM, ncclFloat64) -- yields the global
 * window.  Groups outside the window go to d_keys / d_sums / d_counts
 * (ascending keys, `capacity` entries) and their count to d_n_extra /
 * h_n_extra. */
#define WX_GROUP_WINDOW_BINS 2048
#define WX_GROUP_EXCHANGE_DOUBLES (2 * WX_GROUP_WINDOW_BINS + 1)
wx_status wx_group_partials(const wx_table *table, const char *val_expr, const char *key_expr,
                            const char *cond, const wx_launch *launch, int32_t key_window_lo,
                            double *d_window, int64_t capacity, int32_t *d_keys, double *d_sums,
                            int64_t *d_counts, int64_t *d_n_extra, int64_t *h_n_extra, char *err,
                            size_t errlen);

/* Row-sharded GROUP BY, step 2: the final groups in ascending key order from
 * a combined window (wx_group_partials layout) and the combined
 * out-of-window groups (n_extra entries, ascending keys, none inside the
 * window; device arrays, nullable when n_extra is 0).  Writes at most
 * `capacity` groups; the total goes to d_n_groups / h_n_groups (a host
 * request that exceeds capacity returns WX_ERR_CAPACITY). */
wx_status wx_group_combine(const double *d_window, int32_t key_window_lo, const int32_t *d_x_keys,
                           const double *d_x_sums, const int64_t *d_x_counts, int64_t n_extra,
                           const wx_launch *launch, int64_t capacity, int32_t *d_keys, double *d_sums,
                           int64_t *d_counts, int64_t *d_n_groups, int64_t *h_n_groups, char *err,
                           size_t errlen);

/* Row-sharded GROUP BY in ONE collective (replaces the
 * reference's host gather of dense shard results, src/multi_gpu_utils.cpp:23-60).
 * The exchange buffer holds WX_GROUP_SLOTS_DOUBLES(n_slots, slot_groups)
 * doubles: the dense window exactly as wx_group_partials writes it, then one
 * slot per shard of 1 + 3 * slot_groups doubles -- the shard's out-of-window
 * group count (-1: its general-key table overflowed), then up to slot_groups
 * (key, sum, count) triples in ascending key order.  wx_group_partials_slots
 * writes the window, shard `slot`'s slot and zeros in every other slot, so an
 * element-wise SUM all-reduce of the shards' buffers (one ncclAllReduce,
 * ncclFloat64) both reduces the window and gathers the slots.  It also writes
 * ALL of the shard's out-of-window groups to d_keys / d_sums / d_counts
 * (`capacity` entries) and their count to d_n_extra / h_n_extra, for the
 * fallback below.  1 <= n_slots <= WX_GROUP_EXCHANGE_MAX_SLOTS, slot_groups >= 1,
 * n_slots * slot_groups <= 4096. */
#define WX_GROUP_EXCHANGE_MAX_SLOTS 1024
#define WX_GROUP_SLOTS_DOUBLES(n_slots, slot_groups) \
  (WX_GROUP_EXCHANGE_DOUBLES + (int64_t)(n_slots) * (1 + 3 * (int64_t)(slot_groups)))
#define WX_GROUP_NEEDS_MERGE (-2)
wx_status wx_group_partials_slots(const wx_table *table, const char *val_expr, const char *key_expr,
                                  const char *cond, const wx_launch *launch, int32_t key_window_lo,
                                  double *d_exchange, int32_t n_slots, int32_t slot, int32_t slot_groups,
                                  int64_t capacity, int32_t *d_keys, double *d_sums, int64_t *d_counts,
                                  int64_t *d_n_extra, int64_t *h_n_extra, char *err, size_t errlen);

/* The final groups (ascending keys) from a combined exchange buffer
 * (wx_group_partials_slots layout, summed over the shards): the slots' groups
 * of equal key are added in slot order, then merged with the window.  The
 * group count goes to d_n_groups / h_n_groups; it is -1 when a shard's
 * general-key table overflowed and WX_GROUP_NEEDS_MERGE when some shard had
 * more than slot_groups out-of-window groups -- every rank reads the same
 * combined buffer, so every rank sees the same value and can take the
 * fallback together: a variable-size exchange of the d_keys / d_sums /
 * d_counts lists of wx_group_partials_slots, then wx_group_combine.  The
 * kernel never reads the host; a host request over capacity returns
 * WX_ERR_CAPACITY. */
wx_status wx_group_combine_slots(const double *d_exchange, int32_t n_slots, int32_t slot_groups,
                                 int32_t key_window_lo, const wx_launch *launch, int64_t capacity,
                                 int32_t *d_keys, double *d_sums, int64_t *d_counts, int64_t *d_n_groups,
                                 int64_t *h_n_groups, char *err, size_t errlen);

/* Row-sharded GROUP BY with many groups per shard, in ONE collective and no
 * host read (replaces the host-side gather and merge of shard results,
 * src/multi_gpu_utils.cpp:23-60 / src/warpdb.cpp:508-542, for results that
 * outgrow the exchange slots).  Each shard writes its groups -- keys
 * ascending and unique, e.g. straight from wx_group_sum, or the out-of-window
 * groups of wx_group_partials_slots -- into one fixed-size list record of
 * WX_GROUP_LIST_BYTES(list_capacity) bytes: int64 count at offset 0, then
 * list_capacity int32 keys, doubles sums at WX_GROUP_LIST_SUMS_OFF, int64
 * counts at WX_GROUP_LIST_COUNTS_OFF.  One all-gather of the records
 * (ncclAllGather, bytes) hands every rank the n_lists records back to back;
 * this call merges them on the device: groups of equal key summed in list
 * order (so every rank computes the same bits), then, with d_window (the
 * combined wx_group_partials window, nullable), merged with the window's
 * non-empty bins, none of whose keys may appear in a list.  Ascending keys,
 * at most `capacity` written; the count goes to d_n_groups / h_n_groups.
 * It is -1 when a list's count is negative or above list_capacity (a shard
 * whose table or list overflowed): every rank sees the same records, so
 * every rank gets the same -1.  1 <= n_lists <= 1024, 1 <= list_capacity
 * <= 2^31; the merge keeps 24 bytes of workspace per gathered list entry. */
#define WX_GROUP_LIST_SUMS_OFF(cap) (8 + 8 * (((int64_t)(cap) + 1) / 2))
#define WX_GROUP_LIST_COUNTS_OFF(cap) (WX_GROUP_LIST_SUMS_OFF(cap) + 8 * (int64_t)(cap))
#define WX_GROUP_LIST_BYTES(cap) (WX_GROUP_LIST_COUNTS_OFF(cap) + 8 * (int64_t)(cap))
wx_status wx_group_merge_lists(const void *d_lists, int32_t n_lists, int64_t list_capacity,
                               const double *d_window, int32_t key_window_lo, const wx_launch *launch,
                               int64_t capacity, int32_t *d_keys, double *d_sums, int64_t *d_counts,
                               int64_t *d_n_groups, int64_t *h_n_groups, char *err, size_t errlen);

/* dst[i] = (dst type) src[i] for i < n, types in wx_dtype numbering (not
 * WX_STRING); C conversion semantics. */
wx_status wx_cast(const void *d_src, int32_t src_dtype, void *d_dst, int32_t dst_dtype, int64_t n,
                  const wx_launch *launch, char *err, size_t errlen);

/* wx_group_sum plus per-group MIN / MAX of (float)val_expr (d_mins / d_maxs,
 * nullable, `capacity` entries; NaN skipped as in wx_reduce_stats). */
wx_status wx_group_agg(const wx_table *table, const char *val_expr, const char *key_expr,
                       const char *cond, const wx_launch *launch, int32_t key_window_lo,
                       int64_t capacity, int32_t *d_keys, double *d_sums, int64_t *d_counts,
                       float *d_mins, float *d_maxs, int64_t *d_n_groups, int64_t *h_n_groups,
                       char *err, size_t errlen);

/* wx_group_agg over several value expressions of the same GROUP BY in ONE
 * pass: the key column is read, the condition evaluated, the window flushed
 * and the groups ranked once for all n_vals values.  d_sums / d_mins / d_maxs
 * are arrays of n_vals device pointers (`capacity` entries each); every
 * pointer, and each array itself, is nullable, and what is non-null decides
 * what the kernel carries: value j is summed when d_sums[j] is given and has
 * its MIN / MAX tracked when d_mins[j] or d_maxs[j] is.  A value with nothing
 * requested returns WX_ERR_INVALID.  d_keys and d_counts (the one count per
 * group serves every value: there are no NULLs) are as in wx_group_agg, and
 * so are the groups, the capacity rule, WX_ERR_CAPACITY with the found count
 * in *h_n_groups, asynchrony, and the MIN / MAX semantics (NaN skipped, NaN
 * when none qualifies, -0.0 == +0.0 -> +0.0).
 * n_vals == 1 is wx_group_agg itself (same module, same cache entry); n_vals
 * outside 1 .. WX_GROUP_MAX_VALUES or a blank expression returns
 * WX_ERR_INVALID; WX_F_ROW_ORDER with n_vals >= 2 returns WX_ERR_UNSUPPORTED
 * (one wx_group_agg call per value gives row-order sums).  The value
 * expressions, the key and the condition together may reference at most 16
 * columns.
 * Routes: the LDS window + general-key hash at any capacity, as wx_group_agg's
 * MIN / MAX builds.  With capacity > 4096 on >= 2^20 rows the call takes
 * wx_group_sum's key-range memo for (val_exprs[0], key_expr, cond), else its
 * 65 536-row sample (one host synchronisation), only to move the window onto
 * a range of at most 2048 keys.  The range-partitioned kernels are not
 * extended to several values: a wider range keeps the window + hash.
 * Window LDS: 2048 x (4 + 8 S + 8 Q) bytes for S summed and Q MIN / MAX
 * values; S + Q <= 4 runs two 512-thread workgroups per CU, more runs one of
 * 1024 threads. */
#define WX_GROUP_MAX_VALUES 4
wx_status wx_group_agg_multi(const wx_table *table, const char *const *val_exprs, int32_t n_vals,
                             const char *key_expr, const char *cond, const wx_launch *launch,
                             int32_t key_window_lo, int64_t capacity, int32_t *d_keys,
                             double *const *d_sums, int64_t *d_counts, float *const *d_mins,
                             float *const *d_maxs, int64_t *d_n_groups, int64_t *h_n_groups,
                             char *err, size_t errlen);
/* Build (and cache) the module wx_group_agg_multi would use for the values
 * whose bit is set in sum_mask (a SUM) and minmax_mask (a MIN / MAX), without
 * launching (works without a GPU, like wx_prepare).  Every value needs a bit
 * in one of the masks and no bit may lie at or above n_vals. */
wx_status wx_prepare_group_multi(const wx_table *table, const char *const *val_exprs, int32_t n_vals,
                                 uint32_t sum_mask, uint32_t minmax_mask, const char *key_expr,
                                 const char *cond, const wx_launch *launch, char *err, size_t errlen);

/* Window aggregates: n_exprs plain expressions and n_items window items
 * AGG(val_expr) OVER (PARTITION BY part_expr) of the rows cond keeps, in
 * ascending row order -- wx_project_filter_multi's result with, for a window
 * item, the aggregate of the row's partition (over the rows cond keeps) in
 * place of a per-row value.  d_out_vals holds n_exprs + n_items device
 * pointers, plain expressions first, each nullable; row ids, d_count /
 * h_count, idx_bytes and row_base behave as in wx_project_filter_multi.
 * A window item is (float)sum for WX_WIN_SUM, (float)(sum / (double)count)
 * for WX_WIN_AVG, (float)count for WX_WIN_COUNT and the f32 minimum / maximum
 * of wx_group_agg for WX_WIN_MIN / WX_WIN_MAX (a COUNT counts the partition's
 * rows whatever its val_expr names).  The partition key is (int)part_expr;
 * "0" makes the whole result one partition.
 * Arguments: n_items in 1 .. 16 (0 returns WX_ERR_INVALID: that call is
 * wx_project_filter_multi); n_exprs + n_items <= WX_ORDERED_MAX_EXPRS; the
 * items other than COUNTs name at most WX_GROUP_MAX_VALUES distinct value
 * expressions; a blank expression or an unknown agg returns WX_ERR_INVALID;
 * everything referenced together may name at most 16 columns;
 * WX_F_ROW_ORDER returns WX_ERR_UNSUPPORTED.
 * Run: one wx_group_agg_multi call over the distinct values into workspace
 * scratch (key_window_lo and group_capacity are its key_window_lo and
 * capacity; more partitions than group_capacity return WX_ERR_CAPACITY with
 * the found count in the message), one small launch that turns the groups
 * into an f32 plane per item, then one broadcast compaction per chunk of
 * WX_MAX_OUTPUTS outputs: the first writes the row ids and the count, later
 * ones repeat the compaction for their outputs.  Between the grouped pass
 * and the broadcast the call synchronises the stream once, to read the group
 * count, the first and the last key (gathered into one record on the device)
 * and the error words: a key span of at
 * most WX_GROUP_WINDOW_BINS takes the dense form (the planes indexed by key
 * - first key, copied into LDS per workgroup), a wider one the search form
 * (a binary search over the sorted keys per row).  A key that belongs to no
 * partition (a row cond drops) yields NaN internally and is never written.
 * With WX_F_TIME only the broadcast compactions are timed. */
#define WX_WIN_SUM 0 /* numbering of AggregationType */
#define WX_WIN_AVG 1
#define WX_WIN_COUNT 2
#define WX_WIN_MIN 3
#define WX_WIN_MAX 4
typedef struct wx_window_item {
  const char *val_expr;
  int32_t agg;
} wx_window_item;
wx_status wx_window_select(const wx_table *table, const char *const *exprs, int32_t n_exprs,
                           const wx_window_item *items, int32_t n_items, const char *part_expr,
                           const char *cond, const wx_launch *launch, int32_t key_window_lo,
                           int64_t group_capacity, float *const *d_out_vals, void *d_out_idx,
                           int32_t idx_bytes, int64_t row_base, int64_t *d_count, int64_t *h_count,
                           char *err, size_t errlen);
/* Build (and cache) the modules wx_window_select would use -- the grouped
 * pass and every broadcast launch, in the dense (search == 0) or the search
 * form -- without launching (works without a GPU, like wx_prepare). */
wx_status wx_prepare_window(const wx_table *table, const char *const *exprs, int32_t n_exprs,
                            const wx_window_item *items, int32_t n_items, const char *part_expr,
                            const char *cond, const wx_launch *launch, int32_t search, char *err,
                            size_t errlen);
/* Rows per tile of one broadcast launch of n_outputs outputs (1 ..
 * WX_MAX_OUTPUTS), n_items of them window items (1 .. n_outputs), in the
 * dense (search == 0) or the search form; 0 when an argument is out of
 * range.  The dense form's LDS table takes n_items x 8 KiB from the stage
 * buffers, so its tile shrinks with n_items.  Follows WX_COMPACT_GROUPS /
 * WX_COMPACT_DWAVES of WARPDB_EXTRA_DEFINES like wx_select_tile_rows. */
int32_t wx_window_tile_rows(int32_t n_outputs, int32_t n_items, int32_t search);

/* PK-FK equi-join: the rows of `left` that cond keeps, each looked up in
 * `right` by (int)left_key_expr == right_key_col, in ascending left row order
 * -- wx_project_filter_multi's result over the columns of both tables.  Every
 * left row matches at most one right row: right_key_col is a bare INT32
 * column of `right` whose values are unique (a key that occurs twice returns
 * WX_ERR_UNSUPPORTED, "JOIN: the right key is not unique (key <k>)").
 * exprs (1 .. WX_ORDERED_MAX_EXPRS) and cond are lowered C text over the
 * columns of both tables and may mix them; an identifier that names a column
 * in both tables returns WX_ERR_INVALID ("column <x> is in both tables");
 * left_key_expr may name left columns only.  At most 16 columns of each table
 * may be referenced; `right` holds at most 2^26 rows; WX_F_ROW_ORDER returns
 * WX_ERR_UNSUPPORTED.
 * WX_JOIN_INNER keeps the rows that cond keeps and that match.  WX_JOIN_LEFT
 * keeps the rows that cond keeps (a cond that names a right column is false
 * for an unmatched row); an output that names a right column is NaN for an
 * unmatched row.  With no right rows an INNER join is empty and a LEFT join
 * is the filtered left table.
 * d_out_vals holds n_exprs device pointers, each nullable; d_out_right_row
 * (device int32, nullable, n_rows entries) receives the matched right row of
 * every kept row, -1 for an unmatched one; row ids, d_count / h_count,
 * idx_bytes and row_base behave as in wx_project_filter_multi, and nothing is
 * written at positions >= count.
 * Run: one reduction finds the smallest and the largest right key and the
 * call synchronises the stream once to read them: a span of at most 4096 keys
 * takes the direct form (rows[key - min], copied into LDS per workgroup), a
 * wider one the hash form (open addressing, linear probing, the smallest
 * power of two >= 2 * n_right and >= 64 slots of {key, row}).  The table is
 * built, a second synchronisation reads the duplicate report, then one
 * probing compaction runs per chunk of WX_MAX_OUTPUTS outputs: the first
 * writes the row ids, the right rows and the count, later ones repeat the
 * probe for their outputs.  With WX_F_TIME only the probing compactions are
 * timed.  $WARPDB_JOIN_FORM=hash forces the hash form (a test hook). */
#define WX_JOIN_INNER 0
#define WX_JOIN_LEFT 1
wx_status wx_join_select(const wx_table *left, const wx_table *right, const char *left_key_expr,
                         const char *right_key_col, int32_t join_type, const char *const *exprs, int32_t n_exprs,
                         const char *cond, const wx_launch *launch, float *const *d_out_vals, void *d_out_idx,
                         int32_t idx_bytes, int64_t row_base, int32_t *d_out_right_row, int64_t *d_count,
                         int64_t *h_count, char *err, size_t errlen);
/* Build (and cache) the modules wx_join_select would use -- the build module
 * and every probe launch, in the direct (form == 0) or the hash (form == 1)
 * form, with or without the right-row output -- without launching (works
 * without a GPU, like wx_prepare). */
wx_status wx_prepare_join(const wx_table *left, const wx_table *right, const char *left_key_expr,
                          const char *right_key_col, int32_t join_type, const char *const *exprs, int32_t n_exprs,
                          const char *cond, const wx_launch *launch, int32_t with_right_row, int32_t form, char *err,
                          size_t errlen);
/* Rows per tile of one probe launch of n_outputs outputs (1 ..
 * WX_MAX_OUTPUTS) in the direct (0) or the hash (1) form, with or without
 * the right-row output; 0 when an argument is out of range.  Follows
 * WX_COMPACT_GROUPS / WX_COMPACT_DWAVES of WARPDB_EXTRA_DEFINES. */
int32_t wx_join_tile_rows(int32_t n_outputs, int32_t form, int32_t with_right_row);
/* The form wx_join_select takes for a right table of n_right rows whose keys
 * lie in [key_min, key_max] (*form: 0 direct, 1 hash) and the hash table's
 * log2 capacity (0 in the direct form); n_right above 2^26 returns
 * WX_ERR_UNSUPPORTED.  Needs no device. */
wx_status wx_join_plan(int64_t n_right, int32_t key_min, int32_t key_max, int32_t *form, int32_t *log2_capacity,
                       char *err, size_t errlen);
/* The home slot of a key in a hash table of 1 << log2_capacity slots, as the
 * kernels compute it; -1 when log2_capacity is outside 6 .. 27. */
int32_t wx_join_hash_slot(int32_t key, int32_t log2_capacity);

/* JOIN under GROUP BY: wx_group_agg_multi over exactly the rows
 * wx_join_select(left, right, .., WX_JOIN_INNER, .., cond) keeps, in one pass
 * that probes the right table and adds into the group accumulators, so no
 * joined row is written.  Groups of (int)group_key_expr, ascending, one count
 * per group; val_exprs (1 .. WX_GROUP_MAX_VALUES), group_key_expr and cond are
 * lowered C text over the columns of both tables and may mix them.  Sums are
 * of (float) values in double; MIN / MAX follow wx_group_agg (NaN skipped, NaN
 * when none qualifies, -0.0 returned as +0.0).  The nullable output pointers
 * say what is computed, as in wx_group_agg_multi: a value with neither a sum,
 * a minimum nor a maximum requested returns WX_ERR_INVALID.  key_window_lo,
 * capacity, d_n_groups / h_n_groups and WX_ERR_CAPACITY (h_n_groups still
 * holds the number of groups found) behave as in wx_group_agg_multi; the
 * window stays at key_window_lo.
 * The tables, left_key_expr, right_key_col and the column rules are
 * wx_join_select's (16 columns per table, "column <x> is in both tables",
 * left_key_expr over left columns only, a bare unique INT32 right key, at
 * most 2^26 right rows; a duplicate key fails before the grouped pass runs).
 * WX_JOIN_LEFT returns WX_ERR_UNSUPPORTED ("LEFT JOIN under GROUP BY is not
 * supported (an unmatched row needs NULL-aware aggregates)"): the engine has
 * no NULLs and keeps one count per group.  WX_F_ROW_ORDER returns
 * WX_ERR_UNSUPPORTED.  With no right rows or no left rows the result is zero
 * groups.
 * Run: the table build of wx_join_select (two synchronisations), then one
 * launch of wx_join_group and the finalize; with WX_F_TIME the grouped pass
 * alone is timed. */
wx_status wx_join_group_agg(const wx_table *left, const wx_table *right, const char *left_key_expr,
                            const char *right_key_col, int32_t join_type, const char *const *val_exprs, int32_t n_vals,
                            const char *group_key_expr, const char *cond, const wx_launch *launch,
                            int32_t key_window_lo, int64_t capacity, int32_t *d_keys, double *const *d_sums,
                            int64_t *d_counts, float *const *d_mins, float *const *d_maxs, int64_t *d_n_groups,
                            int64_t *h_n_groups, char *err, size_t errlen);
/* Build (and cache) the modules wx_join_group_agg would use -- the build
 * module and the grouped pass for these masks (bit j: value j carries a SUM /
 * a MIN or MAX) in the direct (form == 0) or the hash (form == 1) form --
 * without launching (works without a GPU, like wx_prepare). */
wx_status wx_prepare_join_group(const wx_table *left, const wx_table *right, const char *left_key_expr,
                                const char *right_key_col, int32_t join_type, const char *const *val_exprs,
                                int32_t n_vals, uint32_t sum_mask, uint32_t minmax_mask, const char *group_key_expr,
                                const char *cond, const wx_launch *launch, int32_t form, char *err, size_t errlen);
/* Threads per workgroup, workgroups per CU and LDS bytes per workgroup of the
 * grouped pass for n_sums summed and n_minmax MIN / MAX values (0 .. 4 each,
 * at least one in all) in the direct (0) or the hash (1) form; each output
 * nullable.  per_cu * lds_bytes never exceeds the 160 KiB of a CU.  Needs no
 * device. */
wx_status wx_join_group_geometry(int32_t n_sums, int32_t n_minmax, int32_t form, int32_t *block, int32_t *per_cu,
                                 int32_t *lds_bytes, char *err, size_t errlen);

/* ORDER BY order_expr [DESC] LIMIT k (1 <= k <= 32) over rows where cond
 * holds; ties broken by ascending row index.  Outputs (device, nullable):
 * order keys, row_base + row indices, and (float)select_expr at those rows
 * (select_expr NULL = the order key).  The count (<= k) goes to d_count / h_count. */
wx_status wx_topk(const wx_table *table, const char *order_expr, const char *cond,
                  const char *select_expr, int32_t k, int32_t descending,
                  const wx_launch *launch, int64_t row_base, float *d_keys, int64_t *d_idx,
                  float *d_vals, int64_t *d_count, int64_t *h_count, char *err, size_t errlen);
/* The launch plan wx_topk follows for a table of n_rows rows and LIMIT k
 * under the current diagnostic define list (WX_UNROLL, WX_TOPK_GRID,
 * WX_TOPK_SEED, WX_TOPK_SEED_MINK of WARPDB_EXTRA_DEFINES): the same
 * arithmetic as the run path's.  cus > 0: a device of that many compute
 * units (needs no device); cus <= 0: the launch's device.  Workgroup b of the
 * scan runs the spans b, b + grid, ... of span_rows rows each, one batch per
 * span. */
typedef struct wx_topk_geometry {
  int64_t grid;             /* workgroups of the scan */
  int64_t span_rows;        /* rows of one batch span */
  int64_t max_batches;      /* the most batches any workgroup runs */
  int64_t seed_grid;        /* workgroups of the seed pass, 0 = no seed pass */
  int64_t seed_stride_rows; /* rows between the seed workgroups' spans */
} wx_topk_geometry;
wx_status wx_topk_plan(int64_t n_rows, int32_t k, int32_t cus, const wx_launch *launch, wx_topk_geometry *out,
                       char *err, size_t errlen);

/* The launch geometry of one pass of the range-partitioned GROUP BY (the form
 * wx_group_sum takes for capacity > 4096 over a key span of 2049 .. 2^24)
 * over n_rows rows and a span of key_span keys, under the current diagnostic
 * define list (WX_GP_GRID=<g> caps the tile grid, WX_GP_DIRCH=<w> shortens
 * the aggregation's directory rounds; WARPDB_EXTRA_DEFINES): the same
 * arithmetic as the run path's.  cus > 0: a device of that many compute
 * units (needs no device); cus <= 0: the launch's device.  Tile workgroup g
 * runs the tiles [g * tiles_per_wg, (g + 1) * tiles_per_wg) of tile_rows rows
 * each; a work item of the aggregation covers whole workgroups' tiles of one
 * partition.  A span outside 2049 .. 2^24 is WX_ERR_UNSUPPORTED, a define
 * out of range (WX_GP_GRID < 1, WX_GP_DIRCH outside 1..4096) WX_ERR_INVALID. */
typedef struct wx_group_part_geom {
  int64_t tile_rows;           /* rows of one tile */
  int64_t n_tiles;             /* tiles of the table */
  int64_t grid;                /* tile workgroups */
  int64_t tiles_per_wg;        /* tiles of every workgroup (the last may own fewer) */
  int64_t n_part;              /* key partitions */
  int64_t part_keys;           /* keys per partition */
  int64_t chunk_rows;          /* the floor of the rows one work item aims at */
  int64_t target_items;        /* work items aimed at over all passing rows */
  int64_t work_cap;            /* most work items */
  int64_t dir_chunk;           /* directory words (tiles) an item stages per round */
  int64_t agg_tiles_per_sweep; /* tiles the waves of an aggregating workgroup take per sweep */
} wx_group_part_geom;
wx_status wx_group_part_geometry(int64_t n_rows, int64_t key_span, int32_t cus, const wx_launch *launch,
                                 wx_group_part_geom *out, char *err, size_t errlen);
/* Partitioned passes completed so far on the launch's (device, stream): a
 * plain host counter (no device read, no synchronisation).  The difference
 * around a wx_group_sum call says which route it took: 0 the LDS window +
 * global hash, 1 one partitioned pass, 2 a pass re-planned over the exact
 * range (an aborted pass followed by the window + hash also counts 1). */
wx_status wx_group_part_passes(const wx_launch *launch, int64_t *passes, char *err, size_t errlen);

/* The sizes the row-order GROUP BY (WX_F_ROW_ORDER) works in, from which its
 * tests size their tables.  Needs no device.  fold_block_values and
 * fold_blocks_ahead follow the diagnostic define list (WX_XF_J, WX_XF_AHEAD of
 * WARPDB_EXTRA_DEFINES); the rest are fixed. */
typedef struct wx_group_rows_geom {
  int64_t tile_rows;          /* rows of one tile of the span path's scatter */
  int64_t span_bins;          /* bins of the span path: the widest key span it takes */
  int64_t count_span_rows;    /* rows of one span of the count kernel's loop */
  int64_t fold_block_values;  /* values of one block of the exact fold */
  int64_t fold_blocks_ahead;  /* blocks the exact fold keeps in flight */
  int64_t fold_small;         /* general path: largest group folded by one lane (WARPDB_FOLD_SMALL overrides) */
  int64_t starts_chunk;       /* general path after the ordinary call: groups per chunk of the start scan */
  int64_t rle_wave_rows;      /* general path without it: sorted rows one wave run-length encodes */
  int64_t xf_chunk;           /* values of one chunk of a group folded in chunks */
  int64_t xf_big;             /* groups of more rows are folded in chunks (WARPDB_XF_BIG overrides) */
  int64_t sample_rows;        /* rows the direct span path samples (thread i: row i * n_rows / sample_rows) */
} wx_group_rows_geom;
wx_status wx_group_rows_geometry(wx_group_rows_geom *out, char *err, size_t errlen);

/* What the last WX_F_ROW_ORDER call on the launch's (device, stream) did:
 * plain host numbers (no device read, no synchronisation).  All zero before
 * any such call, after one that failed, and after one whose ordinary call
 * found no group.  The span path runs `ranges` workgroups over static ranges
 * of whole tiles, min(tiles, 2 * compute units) of them; the diagnostic
 * variable WARPDB_RO_RANGES=<n> (an integer >= 1, else WX_ERR_INVALID from
 * the grouping call) caps that number, so that one workgroup runs many tiles
 * in order.  It changes no result. */
#define WX_RO_ROUTE_NONE 0
#define WX_RO_ROUTE_DIRECT 1           /* the span path straight from the table */
#define WX_RO_ROUTE_ORDINARY_SPAN 2    /* the ordinary call, then the span path over its exact key range */
#define WX_RO_ROUTE_GENERAL_RUNS 3     /* sort + fold, the groups from the sorted keys' runs */
#define WX_RO_ROUTE_GENERAL_ORDINARY 4 /* the ordinary call, then sort + fold over its groups */
#define WX_RO_WHY_NONE 0       /* the direct span path was taken */
#define WX_RO_WHY_RECENT_MISS 1 /* it missed within the last 16 calls over these expressions and table */
#define WX_RO_WHY_NO_SAMPLE 2  /* no sampled row passed the WHERE */
#define WX_RO_WHY_OUTSIDE 3    /* a passing row's key lay outside the guessed span */
#define WX_RO_WHY_WIDE 4       /* the sampled (or remembered) keys span more than span_bins */
#define WX_RO_WHY_NOT_TRIED 5  /* MIN / MAX asked, WARPDB_GROUP_ROWS, or a device without lane-ordered LDS adds */
typedef struct wx_group_rows_record {
  int64_t route;      /* WX_RO_ROUTE_* */
  int64_t why;        /* WX_RO_WHY_*: why the direct span path was not taken */
  int64_t ranges;     /* span routes: workgroups (ranges of tiles) launched; else 0 */
  int64_t tiles;      /* span routes: tiles of the table; else 0 */
  int64_t n_values;   /* length of the row-ordered value array (the passing rows) */
  int64_t big_groups; /* groups folded in chunks */
  int64_t big_chunks; /* their chunks */
} wx_group_rows_record;
wx_status wx_group_rows_last_call(const wx_launch *launch, wx_group_rows_record *out, char *err, size_t errlen);
/* Copies the last WX_F_ROW_ORDER call's row-ordered value array -- the
 * passing rows' values, key-major, ascending row order within a key: the
 * span routes' scatter output, the general routes' sorted payload where the
 * last sort pass left it -- into d_out (device, `capacity` floats), device to
 * device on the launch's stream (synchronous with WX_F_SYNC), and gives its
 * length in n_values (nullable).  The array lives in the workspace and is
 * valid until the next call on that (device, stream).  WX_ERR_INVALID when
 * no such call ran (route WX_RO_ROUTE_NONE), WX_ERR_CAPACITY when it holds
 * more than `capacity` values (n_values is still given). */
wx_status wx_group_rows_last_values(const wx_launch *launch, float *d_out, int64_t capacity, int64_t *n_values,
                                    char *err, size_t errlen);

/* The launch geometry of the streaming kernel of an LDS-window GROUP BY over
 * n_rows rows with n_sums summed and n_minmax MIN / MAX values, under the
 * current diagnostic define list (WX_GROUP_GRID=<g> caps the grid and changes
 * nothing else, WX_UNROLL, WX_GROUP_LEAD; WARPDB_EXTRA_DEFINES): the same
 * arithmetic as the run path's.  family: wx_group_sum / wx_group_agg (one
 * sum, n_minmax 0 or 1), wx_group_agg_multi, or wx_join_group_agg in the
 * join form join_form (0 direct, 1 hash; ignored otherwise).  cus > 0: a
 * device of that many compute units (needs no device); cus <= 0: the
 * launch's device.  With q = row >> 2 and span = span_rows / 4 quads, row
 * `row` is element row & 3 of thread q % block_threads in round (q % span) /
 * block_threads of batch (q / span) / grid of workgroup (q / span) % grid.
 * An argument or define out of range (WX_GROUP_GRID < 1) is WX_ERR_INVALID. */
#define WX_GW_GROUP_SUM 0
#define WX_GW_GROUP_MULTI 1
#define WX_GW_JOIN_GROUP 2
typedef struct wx_group_window_geom {
  int64_t block_threads; /* threads per workgroup */
  int64_t span_rows;     /* rows of one batch span */
  int64_t grid;          /* workgroups */
  int64_t max_batches;   /* the most batches any workgroup runs */
  int64_t window_keys;   /* keys of the LDS window (WX_GROUP_WINDOW_BINS) */
  int64_t hsort_max;     /* most general keys the finalize sorts in LDS; more are sorted on the device */
  int64_t lead;          /* lanes of a wave on one window bin from which they add once (0: the build has no such add) */
} wx_group_window_geom;
wx_status wx_group_window_geometry(int64_t n_rows, int32_t n_sums, int32_t n_minmax, int32_t family,
                                   int32_t join_form, int32_t cus, const wx_launch *launch, wx_group_window_geom *out,
                                   char *err, size_t errlen);
/* Slots of the general-key table (keys outside the window) of the launch's
 * (device, stream) as it stands: a power of two that only grows, 0 before the
 * first GROUP BY there.  A plain host number (no device read). */
wx_status wx_group_table_slots(const wx_launch *launch, int64_t *slots, char *err, size_t errlen);
/* The home slot of a key in a general-key table of `slots` slots (a power of
 * two up to 2^30), as the kernels compute it; probing goes on to the next
 * slot, wrapping.  -1 when `slots` is not such a number. */
int32_t wx_group_hash_slot(int32_t key, int64_t slots);

/* One shard's ORDER BY .. LIMIT candidates in the exchange layout (520 bytes):
 * wx_topk's d_keys / d_vals / d_idx / d_count pointed at keys, vals, rows and
 * count fill it, so the records of all shards are one all-gather of bytes. */
typedef struct wx_topk_record {
  float keys[32];
  float vals[32];
  int64_t rows[32]; /* global row numbers (wx_topk's row_base + row) */
  int64_t count;    /* valid candidates, <= k */
} wx_topk_record;

/* Global ORDER BY .. LIMIT k of a row-sharded query (the
 * reference gathers dense shard results on the host, src/multi_gpu_utils.cpp:
 * 23-60, then sorts them, src/warpdb.cpp:453-455,483-495) from the records
 * of every shard (device memory, n_records * k <= 4096): better key first (NaN
 * last, -0.0 == +0.0), ties by the smaller row.  Outputs as wx_topk; the
 * count (<= k) goes to d_count / h_count.  Runs on the device, no host read. */
wx_status wx_topk_merge(const wx_topk_record *d_records, int32_t n_records, int32_t k, int32_t descending,
                        const wx_launch *launch, float *d_keys, int64_t *d_idx, float *d_vals,
                        int64_t *d_count, int64_t *h_count, char *err, size_t errlen);

/* ORDER BY .. LIMIT of any length over row shards (the k > 32 form of
 * wx_topk / wx_topk_merge; single-GPU query_sql sorts the whole projection
 * with wx_sort_*_limit, src/warpdb.cpp:453-455,483-495).  A head record of
 * capacity cap holds: count (int64) | keys (float x cap) | vals (float x cap)
 * | rows (int64 x cap); WX_HEAD_RECORD_BYTES(cap) bytes, so the records of all
 * shards are one all-gather of bytes.
 *
 * wx_order_head: this shard's first min(limit, passing) rows in ORDER BY
 * order -- the rows passing cond, keyed by order_expr, stably sorted (the
 * order of wx_sort_by_key: NaN keys last, -0.0 == +0.0, ties by ascending
 * row), with select_expr's value (null: the key) and the global row
 * (row_base + row) -- written to d_record (limit <= cap).  Synchronous (the
 * sort needs the passing count).  Scratch: 16 bytes per table row.  A shard
 * holds at most 2^31 - 1 rows (WX_ERR_UNSUPPORTED beyond).
 *
 * wx_head_merge: the global head of n_records shard records (record order =
 * row order): the first min(limit, total) of their candidates in the same
 * order, keys / rows / vals to the (nullable) outputs, the count to d_count /
 * h_count.  n_records * cap < 2^32. */
#define WX_HEAD_RECORD_BYTES(cap) (8 + 16 * (int64_t)(cap))
wx_status wx_order_head(const wx_table *table, const char *order_expr, const char *cond, const char *select_expr,
                        int64_t limit, int32_t descending, const wx_launch *launch, int64_t row_base, void *d_record,
                        int64_t cap, char *err, size_t errlen);
wx_status wx_head_merge(const void *d_records, int32_t n_records, int64_t cap, int64_t limit, int32_t descending,
                        const wx_launch *launch, float *d_keys, int64_t *d_rows, float *d_vals, int64_t *d_count,
                        int64_t *h_count, char *err, size_t errlen);

/* In-place sorts used by the legacy jit_sort_* entry points.  Stable. */
wx_status wx_sort_pairs(int32_t *d_keys, float *d_vals, int64_t count, int32_t ascending,
                        const wx_launch *launch, char *err, size_t errlen);
wx_status wx_sort_float(float *d_vals, int64_t count, int32_t ascending, const wx_launch *launch,
                        char *err, size_t errlen);
/* As wx_sort_float, reading the keys from d_src (not written) and leaving
 * the sorted keys in d_dst: ORDER BY a bare float column with no WHERE sorts
 * straight out of the column instead of projecting a copy first
 * (query_sql's projection + jit_sort_float, src/warpdb.cpp:450-455,
 * src/jit.cpp:283-307).  d_src == d_dst sorts in place; partial overlap is
 * refused. */
wx_status wx_sort_float_from(const float *d_src, float *d_dst, int64_t count, int32_t ascending,
                             const wx_launch *launch, char *err, size_t errlen);
/* Stable sort of float keys carrying a 4-byte payload (the ORDER BY key of
 * each selected row and its SELECT value: the keyed sort query_sql intends,
 * src/warpdb.cpp:470-476).  Same order as wx_sort_float: NaN keys last,
 * -0.0 == +0.0, ties keep their input order. */
wx_status wx_sort_by_key(float *d_keys, float *d_vals, int64_t count, int32_t ascending,
                         const wx_launch *launch, char *err, size_t errlen);

/* ORDER BY .. LIMIT: as wx_sort_float / wx_sort_by_key, but only the first
 * min(limit, count) positions are required to hold the sorted order (the
 * rest of the buffers is left unspecified). */
wx_status wx_sort_float_limit(float *d_vals, int64_t count, int64_t limit, int32_t ascending,
                              const wx_launch *launch, char *err, size_t errlen);
wx_status wx_sort_by_key_limit(float *d_keys, float *d_vals, int64_t count, int64_t limit,
                               int32_t ascending, const wx_launch *launch, char *err, size_t errlen);
/* Keys per radix sort tile: of the key sorts (wx_sort_float*, with_payload
 * 0) or of the key + payload sorts (wx_sort_by_key*, wx_sort_pairs; nonzero).
 * The diagnostic define list may override the geometry; 0 when it is
 * invalid.  Needs no device. */
int32_t wx_sort_tile_keys(int32_t with_payload);
/* Keys one workgroup of the sort's histogram pass reads per iteration (its
 * software-pipelined loop runs where a workgroup owns two or more whole
 * spans); 0 when the define list's override is invalid.  Needs no device. */
int32_t wx_sort_hist_span_keys(void);

/* Seeded synthetic column generator (counter-based, so every shard can
 * generate its own rows on the device):  h = splitmix64(row + seed * 0xD1B54A32D192ED03)
 *   kind 0: uniform float  lo + ((h >> 40) * 2^-24) * (hi - lo)   (float arithmetic)
 *   kind 1: uniform int    lo + (h >> 32) % (hi - lo + 1)
 * row = row_base + i; the value is converted to `dtype`. */
wx_status wx_fill_synthetic(void *d_ptr, int32_t dtype, int64_t n, uint64_t seed,
                            int32_t kind, double lo, double hi, int64_t row_base,
                            const wx_launch *launch, char *err, size_t errlen);

/* Build (and cache) the kernels a call would use, without launching.  Works
 * without a GPU (arch taken from $WARPDB_ARCH, default gfx950).  op: 0 project
 * dense, 1 project compact, 2 sum, 3 group, 4 topk (k = LIMIT; for sum and
 * group, k = 1 selects the MIN / MAX build).  src_out (nullable)
 * receives the generated HIP source. */
wx_status wx_prepare(const wx_table *table, int32_t op, const char *expr, const char *cond,
                     const char *aux_expr, int32_t k, const wx_launch *launch, char *src_out,
                     size_t src_len, char *err, size_t errlen);

/* Synchronise `stream` and report any device-side failure flagged since the
 * last check (look-back timeout, table capacity). */
wx_status wx_check(const wx_launch *launch, char *err, size_t errlen);

/* Sum of the HIP-event durations of the main kernels launched with WX_F_TIME
 * (by any thread of the process) since the last read, and their number
 * (synchronises on the recorded events).  _device: only those launched on
 * `device`; the others stay for a later read. */
wx_status wx_timing_read(double *total_ms, int64_t *launches, char *err, size_t errlen);
wx_status wx_timing_read_device(int32_t device, double *total_ms, int64_t *launches, char *err, size_t errlen);

/* Kernel-cache statistics: compiled modules and hits since load. */
void wx_cache_stats(int64_t *compiles, int64_t *hits);

/* Release cached modules and workspaces of every device. */
void wx_shutdown(void);

int32_t wx_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* WARPEXEC_H */
