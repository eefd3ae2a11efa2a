// warpdb.hpp -- the WarpDB facade (drop-in for the reference's
// include/warpdb.hpp:11-48) running on the MI355X execution layer.
#pragma once
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "arrow_utils.hpp"
#include "csv_loader.hpp"
#include "expression.hpp"
#include "jit.hpp"
#include "json_loader.hpp"
#include "multi_gpu_utils.hpp"

namespace warpdb {
// A result with several columns (query_select, query_sql_table): column j of
// result row i is columns[j][i].  `rows` holds the source row id of each
// result row; it is empty for grouped results.
struct ResultTable {
  std::vector<std::string> names;
  std::vector<std::vector<float>> columns;
  std::vector<int64_t> rows;
  // joined results (query_join, query_sql_joined): the matched row of the
  // attached table for each result row, -1 for an unmatched row of a LEFT
  // join; empty everywhere else
  std::vector<int64_t> right_rows;
};
// Result column names of a SELECT list, without running anything: a bare
// column keeps its name, an aggregate is agg_kernel() + "_" + its position
// in the list (from 0: "sum_1"), anything else is "expr" + its position.
std::vector<std::string> result_column_names(const std::string &sql);
}  // namespace warpdb

class WarpDB {
 public:
  using ResultTable = warpdb::ResultTable;
  // most expressions of one query_select / plain query_sql_table select list
  static constexpr size_t kMaxSelectExprs = 16;
  // Loads .csv (optional schema; default all Float32) or .json into HBM of
  // `device` and keeps the host copy for query_multi_gpu.
  explicit WarpDB(const std::string &filepath, const std::vector<DataType> &schema = {}, int device = 0);
  ~WarpDB();
  WarpDB(const WarpDB &) = delete;
  WarpDB &operator=(const WarpDB &) = delete;

  // "expr [WHERE cond]": dense vector of num_rows floats in row order; rows
  // where cond is false are 0.0f (the reference leaves them uninitialised).
  std::vector<float> query(const std::string &expr);

  // SELECT ... [WHERE] [GROUP BY k [HAVING]] [ORDER BY [ASC|DESC]] [LIMIT] [OFFSET]
  // with SUM/AVG/COUNT aggregates, DISTINCT, ORDER BY .. LIMIT (top-K).
  std::vector<float> query_sql(const std::string &sql);

  // Every visible GPU, rows sharded; same result contract as query().
  std::vector<float> query_multi_gpu(const std::string &expr);

  // Stream a CSV file in chunks of rows_per_chunk through query_multi_gpu.
  static std::vector<float> query_multi_gpu_csv(const std::string &csv_path, const std::string &expr,
                                                int rows_per_chunk = 1000000);

  // query() exported as an Arrow float32 array (malloc or POSIX shm).
  void query_arrow(const std::string &expr, ArrowArray *out_array, ArrowSchema *out_schema,
                   bool use_shared_memory = false);

  // --- extensions on the same execution path -------------------------------
  // Ordered compaction: values and ascending row indices of passing rows.
  std::pair<std::vector<float>, std::vector<int64_t>> query_compact(const std::string &expr);
  // SUM(expr) WHERE cond on the device, and its row count.
  std::pair<double, int64_t> query_sum(const std::string &expr);
  // SUM(expr) WHERE cond over every GPU with an RCCL all-reduce.
  std::pair<double, int64_t> query_multi_gpu_sum(const std::string &expr);
  // "SELECT SUM(v) FROM t [WHERE c] GROUP BY k" over every GPU: per-GPU dense
  // key-window partials and per-GPU slots of keys outside [key_window_lo,
  // key_window_lo + 2048) combined by ONE RCCL all-reduce (more than 64 such
  // keys on a GPU: merged on the host).  Groups in ascending key order with
  // double sums and counts: SUM / COUNT / AVG (MIN / MAX are refused).
  warpdb::GroupResult query_multi_gpu_group(const std::string &sql, int32_t key_window_lo = 0);
  // "SELECT e FROM t [WHERE c] ORDER BY o [ASC|DESC] LIMIT k [OFFSET n]" over
  // every GPU: per GPU its best OFFSET + LIMIT rows (top-K candidates up to 32,
  // beyond that the sorted head), one RCCL all-gather, the (key, row) merge on
  // the device.  The winning ORDER BY keys, global row numbers and SELECT
  // values, best first.
  warpdb::TopkResult query_multi_gpu_topk(const std::string &sql);
  // Zero-copy result: dense device buffer as an ArrowDeviceArray (ROCm).
  void query_arrow_device(const std::string &expr, ArrowDeviceArray *out_array, ArrowSchema *out_schema);
  // The compacted result (passing rows only) as struct<value: float32, row: int64>:
  // host copy, and zero-copy in HBM (ARROW_DEVICE_ROCM; buffers sized for n_rows).
  void query_arrow_compact(const std::string &expr, ArrowArray *out_array, ArrowSchema *out_schema);
  void query_arrow_device_compact(const std::string &expr, ArrowDeviceArray *out_array, ArrowSchema *out_schema);

  // Multi-column results.  query_select: the expressions' values at the rows
  // WHERE keeps, in ascending row order, with those rows' ids -- up to four
  // expressions per pass over the table (one fused ordered compaction: the
  // columns are read and the WHERE evaluated once), longer lists in
  // ceil(n / 4) passes; at most kMaxSelectExprs expressions.
  ResultTable query_select(const std::vector<std::string> &exprs, const std::string &where = "");
  // SELECT a, b, ... FROM t [WHERE c] [LIMIT n] [OFFSET m]: every select item
  // as a column, in row order (ORDER BY / DISTINCT over more than one item
  // are not supported; one item runs as query_sql).  With GROUP BY k: every
  // item is the key expression or SUM / AVG / COUNT / MIN / MAX of ONE common
  // value expression, from one grouped pass; HAVING, ORDER BY, LIMIT and
  // OFFSET as in query_sql; `rows` stays empty.
  ResultTable query_sql_table(const std::string &sql);
  // SELECT items FROM t [WHERE c] GROUP BY k [HAVING h] [ORDER BY o [ASC|DESC]]
  // [LIMIT n] [OFFSET m]: each item is the key expression or SUM / AVG / COUNT
  // / MIN / MAX of ANY value expression (at most kMaxSelectExprs items).  The
  // distinct value expressions -- those HAVING and ORDER BY aggregate
  // included, selected or not -- run four per pass over the table (one fused
  // grouped pass: the key is read and the WHERE evaluated once for all four).
  // HAVING, ORDER BY, LIMIT and OFFSET apply on the host over the groups;
  // `rows` stays empty.  query_sql_table keeps refusing a select list that
  // aggregates two different expressions.
  ResultTable query_sql_grouped(const std::string &sql);
  // SELECT items FROM t [WHERE c] [LIMIT n] [OFFSET m], each item a plain
  // expression or SUM / AVG / COUNT / MIN / MAX (x) OVER (PARTITION BY k), at
  // least one of them a window item: one row per row WHERE keeps, in row
  // order with the row ids, a window item holding the aggregate of the row's
  // partition (over the rows WHERE keeps, with query_sql_grouped's float
  // conversions).  One grouped pass, then fused compaction passes of up to
  // four items that look the partition's aggregate up per row.  All window
  // items share one partition key (OVER () is one partition) and aggregate at
  // most kMaxWindowValues different expressions; ORDER BY or a frame inside
  // OVER, GROUP BY, HAVING, DISTINCT, an outer ORDER BY and JOIN are refused.
  static constexpr size_t kMaxWindowValues = 4;
  ResultTable query_sql_windowed(const std::string &sql);
  // query_sql_windowed as struct<one float32 child per item, row: int64>.
  void query_arrow_sql_windowed(const std::string &sql, ArrowArray *out_array, ArrowSchema *out_schema);
  // query_select as struct<one float32 child per expression, row: int64>.
  void query_arrow_select(const std::vector<std::string> &exprs, const std::string &where, ArrowArray *out_array,
                          ArrowSchema *out_schema);

  // Ordered multi-column results: the expressions' values at the rows WHERE
  // keeps, ordered by one key expression (NaN keys last in both directions,
  // ties by ascending row), with those rows' ids.  The sorted row ids are
  // computed once (a top-K scan for OFFSET + LIMIT <= 32, else a key
  // compaction and a pair sort), then the expressions are gathered at them,
  // four per pass; only OFFSET + LIMIT rows are computed and downloaded.
  // limit < 0: no limit.  At most kMaxSelectExprs expressions, validated and
  // named as in query_select.
  ResultTable query_select_ordered(const std::vector<std::string> &exprs, const std::string &where,
                                   const std::string &order_by, bool descending = false, int64_t limit = -1,
                                   int64_t offset = 0);
  // Late materialisation: the expressions' values at the given row ids (e.g.
  // those of query_compact), in the given order; `rows` of the result is the
  // input.  An id outside the table throws "Row id out of range: <id>".
  ResultTable query_rows(const std::vector<std::string> &exprs, const std::vector<int64_t> &rows);
  // SELECT a, b, ... FROM t [WHERE c] ORDER BY o [ASC|DESC] [LIMIT n] [OFFSET m]
  // through query_select_ordered's path (one item is allowed; ORDER BY is
  // required; GROUP BY, DISTINCT, aggregates, window functions and JOIN are
  // refused).  query_sql_table keeps refusing ORDER BY over several items.
  ResultTable query_sql_ordered(const std::string &sql);
  // query_select_ordered as struct<one float32 child per expression, row: int64>.
  void query_arrow_select_ordered(const std::vector<std::string> &exprs, const std::string &where,
                                  const std::string &order_by, bool descending, int64_t limit, int64_t offset,
                                  ArrowArray *out_array, ArrowSchema *out_schema);

  // Joins.  attach loads a second table (.csv with an optional schema, or
  // .json) into HBM of the same device under `name`; attaching again under
  // the same name replaces it.  query_join / query_sql_joined run a PK-FK
  // equi-join of this table (the left, fact side) with an attached one (the
  // right, dimension side): every left row matches at most one right row,
  // the right key is an INT32 column whose values are unique, and the result
  // is one row per left row the join keeps, in left row order, with the left
  // row ids in `rows` and the matched right rows in `right_rows`.
  enum class JoinType { Inner, Left };
  void attach(const std::string &name, const std::string &filepath, const std::vector<DataType> &schema = {});
  // exprs and where are expressions over the columns of both tables (a name
  // in both must be qualified: t.x with this table's FROM name `left_name`,
  // or <name>.x); left_key is an expression over this table's columns,
  // right_key a column of the attached table.  INNER keeps the rows WHERE
  // keeps and that match; LEFT keeps the rows WHERE keeps, an expression
  // that names a right column being NaN for an unmatched row.
  ResultTable query_join(const std::string &name, const std::string &left_key, const std::string &right_key,
                         const std::vector<std::string> &exprs, const std::string &where = "",
                         JoinType join_type = JoinType::Inner);
  // SELECT items FROM t [INNER] JOIN u ON <expression over t> = <column of u>
  // [WHERE c] [LIMIT n] [OFFSET m], or LEFT [OUTER] JOIN; u is an attached
  // table.  GROUP BY, HAVING, DISTINCT, ORDER BY, aggregates, window items
  // and a second JOIN are refused.
  ResultTable query_sql_joined(const std::string &sql);
  // SELECT items FROM t [INNER] JOIN u ON <expression over t> = <column of u>
  // [WHERE c] GROUP BY k [HAVING h] [ORDER BY o [ASC|DESC]] [LIMIT n]
  // [OFFSET m]: query_sql_grouped over the rows the inner join keeps, in one
  // pass per four value expressions that probes u and aggregates without
  // writing a joined row.  Items are the key or SUM / AVG / COUNT / MIN / MAX of
  // any expression; expressions, the key and WHERE are over the columns of
  // both tables.  LEFT JOIN is refused (an unmatched row would need NULL-aware
  // aggregates), as are a second JOIN, DISTINCT and window items.
  ResultTable query_sql_joined_grouped(const std::string &sql);

  const Table &table() const { return table_; }
  const HostTable &host_table() const { return host_table_; }

 private:
  warpdb::ResidentShards &shards();
  Table table_;
  HostTable host_table_;
  // attach()'s tables live beside the object, keyed by it (warpdb.cpp), not
  // in a member: programs built against this header's earlier versions and not
  // rebuilt (the prebuilt reference tests among them) allocate a WarpDB of
  // the size it had, and the constructor must not write past it.  A query
  // holds its table by a shared pointer, so attach() may replace a table
  // while another thread's join still reads the old one.
  std::shared_ptr<const Table> attached(const std::string &name) const;  // null: none under that name
  std::unique_ptr<warpdb::ResidentShards> shards_;  // query_multi_gpu*: built on first use
  std::once_flag shards_once_;                      // the bindings release the GIL: one builder
};
