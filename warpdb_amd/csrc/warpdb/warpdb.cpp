// warpdb.cpp -- the WarpDB facade on the MI355X execution layer.
// Reference: src/warpdb.cpp:159-590.  query() keeps the reference's result
// contract (dense vector of num_rows floats); the work runs through the C
// ABI (include/warpexec.h) on the table resident in HBM.
#include "warpdb/warpdb.hpp"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdlib>
#include <cctype>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <exception>
#include <fstream>
#include <functional>
#include <map>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <thread>
#include <unordered_set>

#include "warpdb/internal.hpp"
#include "warpdb/multi_gpu_utils.hpp"

using warpdb::DeviceBuffer;
using warpdb::DevGuard;
using warpdb::hip_ok;
using warpdb::sync_launch;
using warpdb::throw_on;
using warpdb::WxTableView;

namespace {

// Every column reference must name a table column (src/warpdb.cpp:19-44).
void validate_ast(const ASTNode *node, const std::unordered_set<std::string> &cols) {
  if (!node) return;
  if (auto v = dynamic_cast<const VariableNode *>(node)) {
    if (!cols.count(v->name)) throw std::runtime_error("Unknown column: " + v->name);
  } else if (auto b = dynamic_cast<const BinaryOpNode *>(node)) {
    validate_ast(b->left.get(), cols);
    validate_ast(b->right.get(), cols);
  } else if (auto f = dynamic_cast<const FunctionCallNode *>(node)) {
    for (const auto &a : f->args) validate_ast(a.get(), cols);
  } else if (auto a = dynamic_cast<const AggregationNode *>(node)) {
    validate_ast(a->expr.get(), cols);
  } else if (auto w = dynamic_cast<const WindowFunctionNode *>(node)) {
    validate_ast(w->expr.get(), cols);
    for (const auto &p : w->partition_by) validate_ast(p.get(), cols);
    if (w->order_by) validate_ast(w->order_by->expr.get(), cols);
  }
}

std::unordered_set<std::string> names_of(const Table &t) {
  std::unordered_set<std::string> s;
  for (const auto &c : t.columns) s.insert(c.name);
  return s;
}

std::unordered_set<std::string> names_of(const HostTable &t) {
  std::unordered_set<std::string> s;
  for (const auto &c : t.columns) s.insert(c.name);
  return s;
}

bool blank(const std::string &s) {
  return std::all_of(s.begin(), s.end(), [](char c) { return std::isspace(static_cast<unsigned char>(c)); });
}

// split + parse + validate + lower, with the reference's error prefixes
void lower_query(const std::string &query, const std::unordered_set<std::string> &cols, std::string &expr_c,
                 std::string &cond_c) {
  if (query.empty()) throw std::runtime_error("Empty query expression");
  std::string e, c;
  warpdb::split_where(query, e, c);
  ASTNodePtr ex;
  try {
    ex = parse_expression(tokenize(e));
  } catch (const std::exception &err) {
    throw std::runtime_error(std::string("Failed to parse expression: ") + err.what());
  }
  validate_ast(ex.get(), cols);
  expr_c = ex->to_cuda_expr();
  cond_c.clear();
  if (!blank(c)) {
    try {
      auto cx = parse_expression(tokenize(c));
      validate_ast(cx.get(), cols);
      cond_c = cx->to_cuda_expr();
    } catch (const std::exception &err) {
      throw std::runtime_error(std::string("Failed to parse WHERE clause: ") + err.what());
    }
  }
}

std::string lower_ext(const std::string &path) {
  const auto dot = path.find_last_of('.');
  std::string ext = dot == std::string::npos ? "" : path.substr(dot + 1);
  for (char &ch : ext) ch = static_cast<char>(std::tolower(static_cast<unsigned char>(ch)));
  return ext;
}

std::vector<float> download(const void *d, int64_t n, int device) {
  std::vector<float> h = warpdb::host_result(static_cast<size_t>(n));
  DevGuard g(device);
  if (n) warpdb::copy_d2h(device, nullptr, h.data(), d, sizeof(float) * static_cast<size_t>(n));
  return h;
}

bool same_expr(const ASTNode *a, const ASTNode *b) { return a && b && a->to_cuda_expr() == b->to_cuda_expr(); }

}  // namespace

WarpDB::WarpDB(const std::string &filepath, const std::vector<DataType> &schema, int device) {
  const std::string ext = lower_ext(filepath);
  if (ext == "csv") {
    host_table_ = load_csv_to_host(filepath, schema);
  } else if (ext == "json") {
    host_table_ = load_json_to_host(filepath);
  } else if (ext == "parquet" || ext == "arrow" || ext == "feather" || ext == "orc") {
    throw std::runtime_error("Arrow support is not compiled into WarpDB");
  } else {
    throw std::runtime_error("Unsupported file format: " + filepath);
  }
  table_ = upload_to_gpu(host_table_, device);
}

WarpDB::~WarpDB() { free_table(table_); }

void WarpDB::lower(const std::string &query, std::string &expr_c, std::string &cond_c) const {
  lower_query(query, names_of(table_), expr_c, cond_c);
}

std::vector<float> WarpDB::query(const std::string &expr) {
  std::string e, c;
  lower(expr, e, c);
  const int64_t n = table_.num_rows;
  DeviceBuffer out(table_.device, sizeof(float) * static_cast<size_t>(n ? n : 1));
  WxTableView v(table_);
  wx_launch L = sync_launch(table_.device);
  char err[8192];
  throw_on(wx_project_filter(&v.table, e.c_str(), c.c_str(), &L, WX_MODE_DENSE_FILL, static_cast<float *>(out.ptr),
                             nullptr, 0, 0, nullptr, nullptr, err, sizeof(err)),
           err);
  return download(out.ptr, n, table_.device);
}

std::pair<std::vector<float>, std::vector<int64_t>> WarpDB::query_compact(const std::string &expr) {
  std::string e, c;
  lower(expr, e, c);
  const int64_t n = table_.num_rows;
  DeviceBuffer vals(table_.device, sizeof(float) * static_cast<size_t>(n ? n : 1));
  DeviceBuffer idx(table_.device, sizeof(int64_t) * static_cast<size_t>(n ? n : 1));
  WxTableView v(table_);
  wx_launch L = sync_launch(table_.device);
  int64_t count = 0;
  char err[8192];
  throw_on(wx_project_filter(&v.table, e.c_str(), c.c_str(), &L, WX_MODE_COMPACT, static_cast<float *>(vals.ptr),
                             idx.ptr, 8, 0, nullptr, &count, err, sizeof(err)),
           err);
  std::vector<float> hv = download(vals.ptr, count, table_.device);
  std::vector<int64_t> hi(static_cast<size_t>(count));
  DevGuard g(table_.device);
  if (count) hip_ok(hipMemcpy(hi.data(), idx.ptr, sizeof(int64_t) * count, hipMemcpyDeviceToHost), "hipMemcpy");
  return {std::move(hv), std::move(hi)};
}

std::pair<double, int64_t> WarpDB::query_sum(const std::string &expr) {
  std::string e, c;
  lower(expr, e, c);
  WxTableView v(table_);
  wx_launch L = sync_launch(table_.device);
  double s = 0;
  int64_t n = 0;
  char err[8192];
  throw_on(wx_reduce_sum(&v.table, e.c_str(), c.c_str(), &L, nullptr, &s, &n, err, sizeof(err)), err);
  return {s, n};
}

void WarpDB::query_arrow(const std::string &expr, ArrowArray *out_array, ArrowSchema *out_schema,
                         bool use_shared_memory) {
  auto r = query(expr);
  export_to_arrow(r.data(), static_cast<int64_t>(r.size()), use_shared_memory, out_array, out_schema);
}

void WarpDB::query_arrow_device(const std::string &expr, ArrowDeviceArray *out_array, ArrowSchema *out_schema) {
  std::string e, c;
  lower(expr, e, c);
  const int64_t n = table_.num_rows;
  DeviceBuffer out(table_.device, sizeof(float) * static_cast<size_t>(n ? n : 1));
  WxTableView v(table_);
  wx_launch L = sync_launch(table_.device);
  char err[8192];
  throw_on(wx_project_filter(&v.table, e.c_str(), c.c_str(), &L, WX_MODE_DENSE_FILL, static_cast<float *>(out.ptr),
                             nullptr, 0, 0, nullptr, nullptr, err, sizeof(err)),
           err);
  const int dev = table_.device;
  export_device_to_arrow(static_cast<float *>(out.release()), n, dev, out_array, out_schema);
}

// The row shards of query_multi_gpu*, built on first use.  With one visible
// GPU holding table_ the shard IS table_ (borrowed, no second HBM copy).
warpdb::ResidentShards &WarpDB::shards() {
  if (host_table_.num_rows() == 0) throw std::runtime_error("Host table not available for multi-GPU query");
  // call_once: two threads' first multi-GPU calls (GIL released) build one set
  // of shards; a throwing build leaves the flag unset, so the next call retries
  std::call_once(shards_once_, [this] {
    int ndev = 0;
    hip_ok(hipGetDeviceCount(&ndev), "hipGetDeviceCount");
    if (ndev == 1 && table_.device == 0 && !std::getenv("WARPDB_VIRTUAL_SHARDS"))  // (test hook: multi_gpu.cpp)
      shards_ = warpdb::ResidentShards::borrow(table_);
    else
      shards_ = std::make_unique<warpdb::ResidentShards>(host_table_);
  });
  return *shards_;
}

void WarpDB::query_arrow_compact(const std::string &expr, ArrowArray *out_array, ArrowSchema *out_schema) {
  auto r = query_compact(expr);
  export_compact_to_arrow(r.first.data(), r.second.data(), static_cast<int64_t>(r.first.size()), out_array,
                          out_schema);
}

void WarpDB::query_arrow_device_compact(const std::string &expr, ArrowDeviceArray *out_array,
                                        ArrowSchema *out_schema) {
  std::string e, c;
  lower(expr, e, c);
  const int64_t n = table_.num_rows;
  // sized for every row passing; the array's length is the passing count
  DeviceBuffer vals(table_.device, sizeof(float) * static_cast<size_t>(n ? n : 1));
  DeviceBuffer rows(table_.device, sizeof(int64_t) * static_cast<size_t>(n ? n : 1));
  WxTableView v(table_);
  wx_launch L = sync_launch(table_.device);
  int64_t count = 0;
  char err[8192];
  throw_on(wx_project_filter(&v.table, e.c_str(), c.c_str(), &L, WX_MODE_COMPACT, static_cast<float *>(vals.ptr),
                             rows.ptr, 8, 0, nullptr, &count, err, sizeof(err)),
           err);
  const int dev = table_.device;
  export_device_compact_to_arrow(static_cast<float *>(vals.release()), static_cast<int64_t *>(rows.release()), count,
                                 dev, out_array, out_schema);
}

std::vector<float> WarpDB::query_multi_gpu(const std::string &expr) {
  std::string e, c;
  lower_query(expr, names_of(host_table_), e, c);
  return shards().dense(e, c);
}

std::pair<double, int64_t> WarpDB::query_multi_gpu_sum(const std::string &expr) {
  std::string e, c;
  lower_query(expr, names_of(host_table_), e, c);
  return shards().sum(e, c);
}

warpdb::GroupResult WarpDB::query_multi_gpu_group(const std::string &sql, int32_t key_window_lo) {
  QueryAST ast;
  try {
    ast = parse_query(tokenize(sql));
  } catch (const std::exception &e) {
    throw std::runtime_error(std::string("Failed to parse SQL: ") + e.what());
  }
  const auto cols = names_of(host_table_);
  auto *agg = ast.select_list.empty() ? nullptr : dynamic_cast<const AggregationNode *>(ast.select_list[0].get());
  if (!ast.group_by || !agg) throw std::runtime_error("query_multi_gpu_group expects SELECT <agg>(expr) ... GROUP BY key");
  if (ast.group_by->keys.size() != 1) throw std::runtime_error("GROUP BY supports one key expression");
  if (!ast.joins.empty()) throw std::runtime_error("JOIN is not supported by the execution engine");
  const std::string kind = agg->agg_kernel();
  if (kind != "sum" && kind != "count" && kind != "avg")  // the shards exchange (sum, count) only
    throw std::runtime_error("query_multi_gpu_group supports SUM / COUNT / AVG, not " + kind);
  validate_ast(agg->expr.get(), cols);
  validate_ast(ast.group_by->keys[0].get(), cols);
  std::string cond;
  if (ast.where) {
    validate_ast(ast.where->get(), cols);
    cond = (*ast.where)->to_cuda_expr();
  }
  // SUM / COUNT / AVG all derive from the (sum, count) the shards exchange
  return shards().group_sum(agg->expr->to_cuda_expr(), ast.group_by->keys[0]->to_cuda_expr(), cond, key_window_lo);
}

warpdb::TopkResult WarpDB::query_multi_gpu_topk(const std::string &sql) {
  QueryAST ast;
  try {
    ast = parse_query(tokenize(sql));
  } catch (const std::exception &e) {
    throw std::runtime_error(std::string("Failed to parse SQL: ") + e.what());
  }
  if (ast.select_list.size() != 1 || ast.group_by || ast.distinct || !ast.order_by || !ast.limit)
    throw std::runtime_error("query_multi_gpu_topk expects SELECT expr FROM t [WHERE c] ORDER BY o [DESC] LIMIT k");
  if (dynamic_cast<const AggregationNode *>(ast.select_list[0].get()))
    throw std::runtime_error("query_multi_gpu_topk takes a plain SELECT expression");
  if (!ast.joins.empty()) throw std::runtime_error("JOIN is not supported by the execution engine");
  const int64_t off = ast.offset ? ast.offset->count : 0;
  int64_t lim = ast.limit->count;
  if (off < 0 || lim < 0) throw std::runtime_error("query_multi_gpu_topk needs OFFSET, LIMIT >= 0");
  const int64_t n_rows = static_cast<int64_t>(host_table_.num_rows());
  // nothing beyond the table: LIMIT 0 or OFFSET >= rows is an empty result
  // (no head is gathered); otherwise off + lim <= rows, computed without
  // overflow, so each shard's head record holds at most the table's rows
  lim = off >= n_rows ? 0 : std::min(lim, n_rows - off);
  const auto cols = names_of(host_table_);
  validate_ast(ast.select_list[0].get(), cols);
  validate_ast(ast.order_by->expr.get(), cols);
  std::string cond;
  if (ast.where) {
    validate_ast(ast.where->get(), cols);
    cond = (*ast.where)->to_cuda_expr();
  }
  warpdb::TopkResult r;
  if (lim == 0) return r;
  r = shards().topk(ast.order_by->expr->to_cuda_expr(), cond, ast.select_list[0]->to_cuda_expr(), off + lim,
                    !ast.order_by->ascending);
  const size_t drop = std::min(r.keys.size(), static_cast<size_t>(off));  // OFFSET
  r.keys.erase(r.keys.begin(), r.keys.begin() + drop);
  r.rows.erase(r.rows.begin(), r.rows.begin() + drop);
  r.values.erase(r.values.begin(), r.values.begin() + drop);
  return r;
}

std::vector<float> WarpDB::query_multi_gpu_csv(const std::string &csv_path, const std::string &expr,
                                               int rows_per_chunk) {
  if (rows_per_chunk <= 0) throw std::runtime_error("rows_per_chunk must be positive");
  std::ifstream file(csv_path);
  if (!file.is_open()) throw std::runtime_error("Failed to open file: " + csv_path);
  std::string header;
  if (!std::getline(file, header)) throw std::runtime_error("Empty CSV file");
  if (!header.empty() && header.back() == '\r') header.pop_back();
  std::vector<std::string> names;
  {
    std::stringstream ss(header);
    std::string n;
    while (std::getline(ss, n, ',')) names.push_back(n);
  }
  std::unordered_set<std::string> cols(names.begin(), names.end());
  std::string e, c;
  lower_query(expr, cols, e, c);
  // Two-stage pipeline: a parser thread reads chunk i+1 while the GPUs run
  // chunk i (the reference parses, uploads and runs each chunk in turn,
  // src/warpdb.cpp:544-590).  At most two parsed chunks wait in the queue.
  std::mutex mu;
  std::condition_variable cv;
  std::deque<HostTable> ready;
  bool done = false;
  std::exception_ptr parse_err;
  // The parser reads the file in large blocks and cuts each chunk after its
  // rows_per_chunk-th non-empty line with memchr (line-by-line std::getline
  // capped the whole pipeline at ≈29-41 M rows/s); the chunk's rows are
  // parsed on parse_threads() threads.  Rows keep the default Float32 schema
  // of the reference's chunk loader (src/csv_loader.cpp:186-223).
  std::thread parser([&] {
    try {
      const size_t block = size_t(64) << 20;
      std::string buf;
      size_t start = 0;
      bool eof = false;
      while (true) {
        // position just past the rows_per_chunk-th non-empty line of buf[start..)
        size_t pos = start, cut = std::string::npos;
        int64_t rows = 0;
        while (true) {
          const char *b = buf.data();
          while (rows < rows_per_chunk && pos < buf.size()) {
            const char *nl = static_cast<const char *>(std::memchr(b + pos, '\n', buf.size() - pos));
            if (!nl) break;
            const size_t len = static_cast<size_t>(nl - (b + pos));
            if (len > 1 || (len == 1 && b[pos] != '\r')) ++rows;
            pos = static_cast<size_t>(nl - b) + 1;
          }
          if (rows == rows_per_chunk) {
            cut = pos;
            break;
          }
          if (eof) {
            cut = buf.size();  // the rest, a last line without '\n' included
            break;
          }
          buf.erase(0, start);  // keep only the unconsumed text, then read on
          pos -= start;
          start = 0;
          const size_t old = buf.size();
          buf.resize(old + block);
          file.read(&buf[old], static_cast<std::streamsize>(block));
          buf.resize(old + static_cast<size_t>(file.gcount()));
          eof = !file;
        }
        HostTable chunk;
        for (const auto &nm : names) chunk.columns.push_back({nm, DataType::Float32, std::vector<float>()});
        warpdb::parse_csv_rows(buf.data() + start, buf.data() + cut, chunk, warpdb::parse_threads());
        start = cut;
        const bool last = eof && start >= buf.size();
        if (chunk.num_rows() > 0) {
          std::unique_lock<std::mutex> lk(mu);
          cv.wait(lk, [&] { return ready.size() < 2 || done; });
          if (done) break;  // consumer gave up
          ready.push_back(std::move(chunk));
          cv.notify_all();
        }
        if (last) break;
      }
    } catch (...) {
      std::lock_guard<std::mutex> lk(mu);
      parse_err = std::current_exception();
    }
    std::lock_guard<std::mutex> lk(mu);
    done = true;
    cv.notify_all();
  });
  std::vector<float> all;
  try {
    while (true) {
      HostTable chunk;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !ready.empty() || done; });
        if (ready.empty()) break;
        chunk = std::move(ready.front());
        ready.pop_front();
        cv.notify_all();
      }
      auto part = run_multi_gpu_jit_host(chunk, e, c);
      all.insert(all.end(), part.begin(), part.end());
    }
  } catch (...) {
    {
      std::lock_guard<std::mutex> lk(mu);
      done = true;
      cv.notify_all();
    }
    parser.join();
    throw;
  }
  parser.join();
  if (parse_err) std::rethrow_exception(parse_err);
  return all;
}

// ------------------------------------------------------------------ SQL
namespace {
bool uses_minmax(const ASTNode *n) {
  if (!n) return false;
  if (auto a = dynamic_cast<const AggregationNode *>(n))
    return a->agg == AggregationType::Min || a->agg == AggregationType::Max;
  if (auto b = dynamic_cast<const BinaryOpNode *>(n)) return uses_minmax(b->left.get()) || uses_minmax(b->right.get());
  return false;
}

// One grouped query's wx_group_agg call and the host-side ordering of its
// groups (HAVING, then ORDER BY; they arrive in ascending key order), shared
// by query_sql and query_sql_table.  `val` is the aggregated expression.
struct GroupRun {
  std::vector<int32_t> keys;
  std::vector<double> sums;
  std::vector<int64_t> cnts;
  std::vector<float> mins, maxs;  // MIN / MAX builds only
  std::vector<size_t> order;      // the groups HAVING keeps, in result order
  // per-group aggregate value (AggData, src/warpdb.cpp:375-385)
  double value_of(AggregationType t, size_t i) const {
    switch (t) {
      case AggregationType::Sum: return sums[i];
      case AggregationType::Avg: return sums[i] / static_cast<double>(cnts[i]);
      case AggregationType::Count: return static_cast<double>(cnts[i]);
      case AggregationType::Min: return mins[i];
      case AggregationType::Max: return maxs[i];
    }
    return NAN;
  }
};

GroupRun run_grouped(const Table &table, const QueryAST &ast, const ASTNode *val, bool select_minmax,
                     const std::string &cond) {
  WxTableView v(table);
  wx_launch L = sync_launch(table.device);
  char err[8192];
  if (ast.group_by->keys.size() != 1) throw std::runtime_error("GROUP BY supports one key expression");
  const ASTNode *key = ast.group_by->keys[0].get();
  const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(table.num_rows, 1 << 22));
  // MIN / MAX anywhere (SELECT, HAVING, ORDER BY) selects the MIN / MAX build
  const bool mm = select_minmax || (ast.having && uses_minmax(ast.having->get())) ||
                  (ast.order_by && uses_minmax(ast.order_by->expr.get()));
  DeviceBuffer dk(table.device, cap * 4), ds(table.device, cap * 8), dc(table.device, cap * 8);
  DeviceBuffer dmn(table.device, mm ? cap * 4 : 4), dmx(table.device, mm ? cap * 4 : 4);
  int64_t g = 0;
  // WARPDB_GROUP_ROW_ORDER=1: each group's sum folded in row order, the
  // reference's own fold (src/warpdb.cpp:373-385) to the bit (WX_F_ROW_ORDER)
  const char *ro = std::getenv("WARPDB_GROUP_ROW_ORDER");
  if (ro && std::string(ro) == "1") L.flags |= WX_F_ROW_ORDER;
  throw_on(wx_group_agg(&v.table, val->to_cuda_expr().c_str(), key->to_cuda_expr().c_str(), cond.c_str(), &L,
                        0, cap, static_cast<int32_t *>(dk.ptr), static_cast<double *>(ds.ptr),
                        static_cast<int64_t *>(dc.ptr), mm ? static_cast<float *>(dmn.ptr) : nullptr,
                        mm ? static_cast<float *>(dmx.ptr) : nullptr, nullptr, &g, err, sizeof(err)),
           err);
  GroupRun run;
  std::vector<int32_t> &keys = run.keys;
  std::vector<double> &sums = run.sums;
  std::vector<int64_t> &cnts = run.cnts;
  std::vector<float> &mins = run.mins, &maxs = run.maxs;
  keys.resize(g);
  sums.resize(g);
  cnts.resize(g);
  mins.resize(mm ? g : 0);
  maxs.resize(mm ? g : 0);
  {
    DevGuard dg(table.device);
    if (g) {
      hip_ok(hipMemcpy(keys.data(), dk.ptr, g * 4, hipMemcpyDeviceToHost), "hipMemcpy");
      hip_ok(hipMemcpy(sums.data(), ds.ptr, g * 8, hipMemcpyDeviceToHost), "hipMemcpy");
      hip_ok(hipMemcpy(cnts.data(), dc.ptr, g * 8, hipMemcpyDeviceToHost), "hipMemcpy");
      if (mm) {
        hip_ok(hipMemcpy(mins.data(), dmn.ptr, g * 4, hipMemcpyDeviceToHost), "hipMemcpy");
        hip_ok(hipMemcpy(maxs.data(), dmx.ptr, g * 4, hipMemcpyDeviceToHost), "hipMemcpy");
      }
    }
  }
  auto value_of = [&](AggregationType t, size_t i) { return run.value_of(t, i); };
  // HAVING over the (few) aggregated groups, with the reference's
  // comparison semantics (src/warpdb.cpp:387-423)
  std::function<double(const ASTNode *, size_t)> having = [&](const ASTNode *n, size_t i) -> double {
    if (auto c = dynamic_cast<const ConstantNode *>(n)) return std::stod(c->value);
    if (auto a = dynamic_cast<const AggregationNode *>(n)) {
      if (!same_expr(a->expr.get(), val) && a->agg != AggregationType::Count)
        throw std::runtime_error("HAVING may only aggregate the selected expression");
      return value_of(a->agg, i);
    }
    if (auto b = dynamic_cast<const BinaryOpNode *>(n)) {
      const double l = having(b->left.get(), i), r = having(b->right.get(), i);
      const std::string &op = b->op;
      if (op == "+") return l + r;
      if (op == "-") return l - r;
      if (op == "*") return l * r;
      if (op == "/") return l / r;
      if (op == ">") return l > r;
      if (op == "<") return l < r;
      if (op == ">=") return l >= r;
      if (op == "<=") return l <= r;
      if (op == "==") return l == r;
      if (op == "!=") return l != r;
      if (op == "&&") return l != 0 && r != 0;
      if (op == "||") return l != 0 || r != 0;
    }
    if (same_expr(n, key)) return keys[i];
    throw std::runtime_error("unsupported HAVING term");
  };
  std::vector<size_t> &order = run.order;
  for (size_t i = 0; i < static_cast<size_t>(g); ++i)
    if (!ast.having || having(ast.having->get(), i) != 0.0) order.push_back(i);
  if (ast.order_by) {  // groups arrive in ascending key order
    const ASTNode *ob = ast.order_by->expr.get();
    auto *oagg = dynamic_cast<const AggregationNode *>(ob);
    if (oagg) {
      std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
        const double x = value_of(oagg->agg, a), y = value_of(oagg->agg, b);
        return ast.order_by->ascending ? x < y : x > y;
      });
    } else if (same_expr(ob, key)) {
      if (!ast.order_by->ascending) std::reverse(order.begin(), order.end());
    } else {
      throw std::runtime_error("ORDER BY with GROUP BY must name the key or an aggregate");
    }
  }
  return run;
}
}  // namespace

std::vector<float> WarpDB::query_sql(const std::string &sql) {
  QueryAST ast;
  try {
    ast = parse_query(tokenize(sql));
  } catch (const std::exception &e) {
    throw std::runtime_error(std::string("Failed to parse SQL: ") + e.what());
  }
  const auto cols = names_of(table_);
  auto validate_ctx = [&](const ASTNode *n, const std::string &ctx) {
    try {
      validate_ast(n, cols);
    } catch (const std::exception &e) {
      throw std::runtime_error(ctx + ": " + e.what());
    }
  };
  if (ast.select_list.empty()) throw std::runtime_error("Empty SELECT list");
  for (const auto &e : ast.select_list) validate_ctx(e.get(), "SELECT clause");
  for (const auto &j : ast.joins) validate_ctx(j.condition.get(), "JOIN condition");
  if (ast.where) validate_ctx(ast.where->get(), "WHERE clause");
  if (ast.group_by)
    for (const auto &k : ast.group_by->keys) validate_ctx(k.get(), "GROUP BY");
  if (ast.order_by) validate_ctx(ast.order_by->expr.get(), "ORDER BY");
  if (!ast.joins.empty()) throw std::runtime_error("JOIN is not supported by the execution engine");

  const std::string cond = ast.where ? (*ast.where)->to_cuda_expr() : std::string();
  WxTableView v(table_);
  wx_launch L = sync_launch(table_.device);
  char err[8192];
  std::vector<float> result;
  const size_t off = ast.offset ? static_cast<size_t>(std::max(0, ast.offset->count)) : 0;
  const size_t lim = ast.limit ? static_cast<size_t>(std::max(0, ast.limit->count)) : SIZE_MAX;
  auto slice = [&](std::vector<float> r) {
    if (off >= r.size()) return std::vector<float>();
    r.erase(r.begin(), r.begin() + static_cast<long>(off));
    if (r.size() > lim) r.resize(lim);
    return r;
  };
  auto *agg = dynamic_cast<const AggregationNode *>(ast.select_list[0].get());

  if (ast.group_by) {
    if (!agg) throw std::runtime_error("Only aggregation queries supported with GROUP BY");
    const GroupRun r = run_grouped(table_, ast, agg->expr.get(), uses_minmax(agg), cond);
    for (size_t i : r.order) result.push_back(static_cast<float>(r.value_of(agg->agg, i)));
    if (ast.distinct) {
      std::sort(result.begin(), result.end());
      result.erase(std::unique(result.begin(), result.end()), result.end());
    }
    return slice(std::move(result));
  }

  if (agg) {  // ungrouped aggregate over the WHERE rows
    wx_stats st{};
    if (uses_minmax(agg)) {
      throw_on(wx_reduce_stats(&v.table, agg->expr->to_cuda_expr().c_str(), cond.c_str(), &L, nullptr, &st, err,
                               sizeof(err)),
               err);
    } else {
      throw_on(wx_reduce_sum(&v.table, agg->expr->to_cuda_expr().c_str(), cond.c_str(), &L, nullptr, &st.sum,
                             &st.count, err, sizeof(err)),
               err);
    }
    double val = NAN;
    switch (agg->agg) {
      case AggregationType::Sum: val = st.sum; break;
      case AggregationType::Avg: val = st.count ? st.sum / static_cast<double>(st.count) : NAN; break;
      case AggregationType::Count: val = static_cast<double>(st.count); break;
      case AggregationType::Min: val = st.min; break;
      case AggregationType::Max: val = st.max; break;
    }
    return slice({static_cast<float>(val)});
  }

  const ASTNode *sel = ast.select_list[0].get();
  const std::string sel_c = sel->to_cuda_expr();
  const ASTNode *ob = ast.order_by ? ast.order_by->expr.get() : nullptr;
  // ORDER BY .. LIMIT k: device top-K (ties by ascending row index)
  if (ob && !ast.distinct && ast.limit && off + lim <= 32) {
    const int k = static_cast<int>(off + lim);
    if (k == 0) return {};
    DeviceBuffer dv(table_.device, sizeof(float) * k);
    int64_t m = 0;
    throw_on(wx_topk(&v.table, ob->to_cuda_expr().c_str(), cond.c_str(), sel_c.c_str(), k,
                     ast.order_by->ascending ? 0 : 1, &L, 0, nullptr, nullptr, static_cast<float *>(dv.ptr), nullptr,
                     &m, err, sizeof(err)),
             err);
    return slice(download(dv.ptr, m, table_.device));
  }
  const int64_t n = table_.num_rows;
  DeviceBuffer dv(table_.device, sizeof(float) * static_cast<size_t>(n ? n : 1));
  // ORDER BY a bare float column, no WHERE, no LIMIT: the projection would be
  // a copy of the column, so the sort reads the column itself
  // (src/warpdb.cpp:450-455 projects, then jit_sort_float sorts the copy)
  if (ob && !ast.distinct && !ast.limit && cond.empty() && same_expr(ob, sel)) {
    if (auto var = dynamic_cast<const VariableNode *>(sel)) {
      for (const auto &c : table_.columns) {
        if (c.name != var->name || c.type != DataType::Float32) continue;
        throw_on(wx_sort_float_from(static_cast<const float *>(c.device_ptr), static_cast<float *>(dv.ptr), n,
                                    ast.order_by->ascending ? 1 : 0, &L, err, sizeof(err)),
                 err);
        return slice(download(dv.ptr, n, table_.device));
      }
    }
  }
  // projection of the WHERE rows in row order (ordered compaction)
  int64_t count = 0;
  throw_on(wx_project_filter(&v.table, sel_c.c_str(), cond.c_str(), &L, WX_MODE_COMPACT, static_cast<float *>(dv.ptr),
                             nullptr, 0, 0, nullptr, &count, err, sizeof(err)),
           err);
  if (ob && !same_expr(ob, sel)) {
    // ORDER BY another expression: its values at the same rows (same WHERE,
    // same ascending row order) are the keys of a keyed sort that carries the
    // SELECT values along (the pairs the reference builds, src/warpdb.cpp:470-476)
    if (ast.distinct) throw std::runtime_error("DISTINCT with ORDER BY a different expression is not supported");
    DeviceBuffer dk(table_.device, sizeof(float) * static_cast<size_t>(n ? n : 1));
    int64_t kcount = 0;
    throw_on(wx_project_filter(&v.table, ob->to_cuda_expr().c_str(), cond.c_str(), &L, WX_MODE_COMPACT,
                               static_cast<float *>(dk.ptr), nullptr, 0, 0, nullptr, &kcount, err, sizeof(err)),
             err);
    if (kcount != count) throw std::runtime_error("ORDER BY rows differ from SELECT rows");
    // with a LIMIT only the first OFFSET + LIMIT rows of the order are needed
    throw_on(wx_sort_by_key_limit(static_cast<float *>(dk.ptr), static_cast<float *>(dv.ptr), count,
                                  ast.limit ? std::min<int64_t>(count, off + lim) : count,
                                  ast.order_by->ascending ? 1 : 0, &L, err, sizeof(err)),
             err);
    if (ast.limit) count = std::min<int64_t>(count, off + lim);
  } else if (ob || ast.distinct) {
    const bool asc = ob ? ast.order_by->ascending : true;
    const bool head_only = ob && !ast.distinct && ast.limit;  // DISTINCT needs every value
    throw_on(wx_sort_float_limit(static_cast<float *>(dv.ptr), count,
                                 head_only ? std::min<int64_t>(count, off + lim) : count, asc ? 1 : 0, &L, err,
                                 sizeof(err)),
             err);
    if (head_only) count = std::min<int64_t>(count, off + lim);
  }
  result = download(dv.ptr, count, table_.device);
  if (ast.distinct) result.erase(std::unique(result.begin(), result.end()), result.end());
  return slice(std::move(result));
}

// ------------------------------------------------- multi-column results
namespace {
std::string column_name(const ASTNode *n, size_t pos) {
  if (auto v = dynamic_cast<const VariableNode *>(n)) return v->name;
  if (auto a = dynamic_cast<const AggregationNode *>(n)) return a->agg_kernel() + "_" + std::to_string(pos);
  return "expr" + std::to_string(pos);
}

// The lowered expressions' values at the rows `cond` keeps, in row order,
// and those rows' ids: up to WX_MAX_OUTPUTS expressions per fused pass, the
// same WHERE in every pass; only the first pass writes the row ids, and the
// passes' counts must agree.  At most max_rows rows are downloaded.
void select_run(const Table &table, const std::vector<std::string> &exprs_c, const std::string &cond_c,
                int64_t max_rows, warpdb::ResultTable &out) {
  const int64_t n = table.num_rows;
  const size_t m = exprs_c.size();
  const size_t width = std::min<size_t>(m, WX_MAX_OUTPUTS);
  std::vector<std::unique_ptr<DeviceBuffer>> vals;
  for (size_t j = 0; j < width; ++j)
    vals.push_back(std::make_unique<DeviceBuffer>(table.device, sizeof(float) * static_cast<size_t>(n ? n : 1)));
  DeviceBuffer idx(table.device, sizeof(int64_t) * static_cast<size_t>(n ? n : 1));
  WxTableView v(table);
  wx_launch L = sync_launch(table.device);
  char err[8192];
  int64_t count = 0, keep = 0;
  out.columns.clear();
  for (size_t first = 0; first < m; first += WX_MAX_OUTPUTS) {
    const size_t k = std::min<size_t>(WX_MAX_OUTPUTS, m - first);
    const char *ex[WX_MAX_OUTPUTS] = {nullptr, nullptr, nullptr, nullptr};
    float *dst[WX_MAX_OUTPUTS] = {nullptr, nullptr, nullptr, nullptr};
    for (size_t j = 0; j < k; ++j) {
      ex[j] = exprs_c[first + j].c_str();
      dst[j] = static_cast<float *>(vals[j]->ptr);
    }
    int64_t c = 0;
    throw_on(wx_project_filter_multi(&v.table, ex, static_cast<int32_t>(k), cond_c.c_str(), &L, WX_MODE_COMPACT, dst,
                                     first == 0 ? idx.ptr : nullptr, 8, 0, nullptr, &c, err, sizeof(err)),
             err);
    if (first == 0) {
      count = c;
      keep = std::min(count, max_rows);
      out.rows.assign(static_cast<size_t>(keep), 0);
      DevGuard g(table.device);
      if (keep) hip_ok(hipMemcpy(out.rows.data(), idx.ptr, sizeof(int64_t) * keep, hipMemcpyDeviceToHost), "hipMemcpy");
    } else if (c != count) {
      throw std::runtime_error("multi-column SELECT: the passes' row counts disagree");
    }
    for (size_t j = 0; j < k; ++j) out.columns.push_back(download(vals[j]->ptr, keep, table.device));
  }
}
}  // namespace

std::vector<std::string> warpdb::result_column_names(const std::string &sql) {
  QueryAST ast;
  try {
    ast = parse_query(tokenize(sql));
  } catch (const std::exception &e) {
    throw std::runtime_error(std::string("Failed to parse SQL: ") + e.what());
  }
  std::vector<std::string> names;
  for (size_t i = 0; i < ast.select_list.size(); ++i) names.push_back(column_name(ast.select_list[i].get(), i));
  return names;
}

WarpDB::ResultTable WarpDB::query_select(const std::vector<std::string> &exprs, const std::string &where) {
  if (exprs.empty()) throw std::runtime_error("Empty SELECT list");
  if (exprs.size() > kMaxSelectExprs)
    throw std::runtime_error("query_select takes at most " + std::to_string(kMaxSelectExprs) + " expressions");
  const auto cols = names_of(table_);
  ResultTable out;
  std::vector<std::string> lowered;
  for (size_t i = 0; i < exprs.size(); ++i) {
    if (blank(exprs[i])) throw std::runtime_error("Empty query expression");
    ASTNodePtr ex;
    try {
      ex = parse_expression(tokenize(exprs[i]));
    } catch (const std::exception &err) {
      throw std::runtime_error(std::string("Failed to parse expression: ") + err.what());
    }
    validate_ast(ex.get(), cols);
    if (dynamic_cast<const AggregationNode *>(ex.get()))
      throw std::runtime_error("query_select takes plain expressions, not aggregates");
    lowered.push_back(ex->to_cuda_expr());
    out.names.push_back(column_name(ex.get(), i));
  }
  std::string cond_c;
  if (!blank(where)) {
    try {
      auto cx = parse_expression(tokenize(where));
      validate_ast(cx.get(), cols);
      cond_c = cx->to_cuda_expr();
    } catch (const std::exception &err) {
      throw std::runtime_error(std::string("Failed to parse WHERE clause: ") + err.what());
    }
  }
  select_run(table_, lowered, cond_c, table_.num_rows, out);
  return out;
}

void WarpDB::query_arrow_select(const std::vector<std::string> &exprs, const std::string &where,
                                ArrowArray *out_array, ArrowSchema *out_schema) {
  const ResultTable r = query_select(exprs, where);
  std::vector<const float *> columns;
  for (const auto &c : r.columns) columns.push_back(c.data());
  export_select_to_arrow(r.names, columns, r.rows.data(), static_cast<int64_t>(r.rows.size()), out_array, out_schema);
}

// ------------------------------------- ordered multi-column results, row gather
namespace {
// Parse, validate and lower a list of plain expressions as query_select
// does; `who` names the entry point in the messages.
void lower_select_list(const std::vector<std::string> &exprs, const std::unordered_set<std::string> &cols,
                       const char *who, std::vector<std::string> &lowered, std::vector<std::string> &names) {
  if (exprs.empty()) throw std::runtime_error("Empty SELECT list");
  if (exprs.size() > WarpDB::kMaxSelectExprs)
    throw std::runtime_error(std::string(who) + " takes at most " + std::to_string(WarpDB::kMaxSelectExprs) +
                             " expressions");
  for (size_t i = 0; i < exprs.size(); ++i) {
    if (blank(exprs[i])) throw std::runtime_error("Empty query expression");
    ASTNodePtr ex;
    try {
      ex = parse_expression(tokenize(exprs[i]));
    } catch (const std::exception &err) {
      throw std::runtime_error(std::string("Failed to parse expression: ") + err.what());
    }
    validate_ast(ex.get(), cols);
    if (dynamic_cast<const AggregationNode *>(ex.get()))
      throw std::runtime_error(std::string(who) + " takes plain expressions, not aggregates");
    lowered.push_back(ex->to_cuda_expr());
    names.push_back(column_name(ex.get(), i));
  }
}

std::vector<int64_t> download_rows(const void *d, int64_t n, int device) {
  std::vector<int64_t> h(static_cast<size_t>(n), 0);
  DevGuard g(device);
  if (n) hip_ok(hipMemcpy(h.data(), d, sizeof(int64_t) * static_cast<size_t>(n), hipMemcpyDeviceToHost), "hipMemcpy");
  return h;
}

// The lowered expressions of the rows `cond` keeps, ordered by order_c:
// positions [offset, offset + limit) of the ordered result (limit < 0: to
// the end).  One wx_select_ordered call; only offset + limit rows are
// computed and downloaded.
void ordered_run(const Table &table, const std::vector<std::string> &exprs_c, const std::string &cond_c,
                 const std::string &order_c, bool descending, int64_t limit, int64_t offset,
                 warpdb::ResultTable &out) {
  const int64_t n = table.num_rows;
  offset = std::max<int64_t>(0, offset);
  const int64_t want = limit < 0 ? -1 : (limit > INT64_MAX - offset ? INT64_MAX : offset + limit);
  const int64_t cap = want < 0 ? n : std::min(n, want);
  const size_t m = exprs_c.size();
  std::vector<std::unique_ptr<DeviceBuffer>> vals;
  std::vector<const char *> ex;
  std::vector<float *> dst;
  for (size_t j = 0; j < m; ++j) {
    vals.push_back(std::make_unique<DeviceBuffer>(table.device, sizeof(float) * static_cast<size_t>(cap ? cap : 1)));
    ex.push_back(exprs_c[j].c_str());
    dst.push_back(static_cast<float *>(vals[j]->ptr));
  }
  DeviceBuffer rows(table.device, sizeof(int64_t) * static_cast<size_t>(cap ? cap : 1));
  WxTableView v(table);
  wx_launch L = sync_launch(table.device);
  char err[8192];
  int64_t count = 0;
  throw_on(wx_select_ordered(&v.table, ex.data(), static_cast<int32_t>(m), cond_c.c_str(), order_c.c_str(),
                             descending ? 1 : 0, want, &L, 0, dst.data(), nullptr, static_cast<int64_t *>(rows.ptr),
                             cap, nullptr, &count, err, sizeof(err)),
           err);
  const int64_t first = std::min(offset, count), keep = count - first;
  out.columns.clear();
  for (size_t j = 0; j < m; ++j) out.columns.push_back(download(dst[j] + first, keep, table.device));
  out.rows = download_rows(static_cast<int64_t *>(rows.ptr) + first, keep, table.device);
}
}  // namespace

WarpDB::ResultTable WarpDB::query_select_ordered(const std::vector<std::string> &exprs, const std::string &where,
                                                 const std::string &order_by, bool descending, int64_t limit,
                                                 int64_t offset) {
  const auto cols = names_of(table_);
  ResultTable out;
  std::vector<std::string> lowered;
  lower_select_list(exprs, cols, "query_select_ordered", lowered, out.names);
  std::string cond_c, order_c;
  if (!blank(where)) {
    try {
      auto cx = parse_expression(tokenize(where));
      validate_ast(cx.get(), cols);
      cond_c = cx->to_cuda_expr();
    } catch (const std::exception &err) {
      throw std::runtime_error(std::string("Failed to parse WHERE clause: ") + err.what());
    }
  }
  if (blank(order_by)) throw std::runtime_error("Empty ORDER BY expression");
  try {
    auto ox = parse_expression(tokenize(order_by));
    validate_ast(ox.get(), cols);
    if (dynamic_cast<const AggregationNode *>(ox.get())) throw std::runtime_error("aggregates are not supported here");
    order_c = ox->to_cuda_expr();
  } catch (const std::exception &err) {
    throw std::runtime_error(std::string("Failed to parse ORDER BY expression: ") + err.what());
  }
  ordered_run(table_, lowered, cond_c, order_c, descending, limit, offset, out);
  return out;
}

WarpDB::ResultTable WarpDB::query_rows(const std::vector<std::string> &exprs, const std::vector<int64_t> &rows) {
  ResultTable out;
  std::vector<std::string> lowered;
  lower_select_list(exprs, names_of(table_), "query_rows", lowered, out.names);
  for (int64_t r : rows)
    if (r < 0 || r >= table_.num_rows) throw std::runtime_error("Row id out of range: " + std::to_string(r));
  const int64_t count = static_cast<int64_t>(rows.size());
  const size_t m = lowered.size();
  const size_t width = std::min<size_t>(m, WX_MAX_OUTPUTS);
  DeviceBuffer ids(table_.device, sizeof(int64_t) * static_cast<size_t>(count ? count : 1));
  {
    DevGuard g(table_.device);
    if (count)
      hip_ok(hipMemcpy(ids.ptr, rows.data(), sizeof(int64_t) * static_cast<size_t>(count), hipMemcpyHostToDevice),
             "hipMemcpy");
  }
  std::vector<std::unique_ptr<DeviceBuffer>> vals;
  for (size_t j = 0; j < width; ++j)
    vals.push_back(std::make_unique<DeviceBuffer>(table_.device, sizeof(float) * static_cast<size_t>(count ? count : 1)));
  WxTableView v(table_);
  wx_launch L = sync_launch(table_.device);
  char err[8192];
  for (size_t first = 0; first < m; first += WX_MAX_OUTPUTS) {
    const size_t k = std::min<size_t>(WX_MAX_OUTPUTS, m - first);
    const char *ex[WX_MAX_OUTPUTS] = {nullptr, nullptr, nullptr, nullptr};
    float *dst[WX_MAX_OUTPUTS] = {nullptr, nullptr, nullptr, nullptr};
    for (size_t j = 0; j < k; ++j) {
      ex[j] = lowered[first + j].c_str();
      dst[j] = static_cast<float *>(vals[j]->ptr);
    }
    throw_on(wx_gather_multi(&v.table, ex, static_cast<int32_t>(k), ids.ptr, 8, 0, count, nullptr, &L, dst, nullptr, 0,
                             err, sizeof(err)),
             err);
    for (size_t j = 0; j < k; ++j) out.columns.push_back(download(vals[j]->ptr, count, table_.device));
  }
  out.rows = rows;
  return out;
}

WarpDB::ResultTable WarpDB::query_sql_ordered(const std::string &sql) {
  QueryAST ast;
  try {
    ast = parse_query(tokenize(sql));
  } catch (const std::exception &e) {
    throw std::runtime_error(std::string("Failed to parse SQL: ") + e.what());
  }
  const auto cols = names_of(table_);
  auto validate_ctx = [&](const ASTNode *n, const std::string &ctx) {
    try {
      validate_ast(n, cols);
    } catch (const std::exception &e) {
      throw std::runtime_error(ctx + ": " + e.what());
    }
  };
  if (ast.select_list.empty()) throw std::runtime_error("Empty SELECT list");
  if (!ast.joins.empty()) throw std::runtime_error("JOIN is not supported by query_sql_ordered");
  if (ast.group_by) throw std::runtime_error("GROUP BY is not supported by query_sql_ordered (use query_sql_table)");
  if (ast.distinct) throw std::runtime_error("DISTINCT is not supported by query_sql_ordered");
  for (const auto &e : ast.select_list) {
    if (dynamic_cast<const WindowFunctionNode *>(e.get()))
      throw std::runtime_error("window functions are not supported by query_sql_ordered");
    if (dynamic_cast<const AggregationNode *>(e.get()))
      throw std::runtime_error("aggregates are not supported by query_sql_ordered (plain expressions only)");
  }
  if (!ast.order_by) throw std::runtime_error("query_sql_ordered needs an ORDER BY clause");
  if (dynamic_cast<const AggregationNode *>(ast.order_by->expr.get()))
    throw std::runtime_error("aggregates are not supported by query_sql_ordered (plain expressions only)");
  for (const auto &e : ast.select_list) validate_ctx(e.get(), "SELECT clause");
  if (ast.where) validate_ctx(ast.where->get(), "WHERE clause");
  validate_ctx(ast.order_by->expr.get(), "ORDER BY");
  const size_t m = ast.select_list.size();
  if (m > kMaxSelectExprs)
    throw std::runtime_error("a select list takes at most " + std::to_string(kMaxSelectExprs) + " expressions");
  ResultTable out;
  std::vector<std::string> lowered;
  for (size_t i = 0; i < m; ++i) {
    out.names.push_back(column_name(ast.select_list[i].get(), i));
    lowered.push_back(ast.select_list[i]->to_cuda_expr());
  }
  const std::string cond = ast.where ? (*ast.where)->to_cuda_expr() : std::string();
  const int64_t off = ast.offset ? std::max(0, ast.offset->count) : 0;
  const int64_t lim = ast.limit ? std::max(0, ast.limit->count) : -1;
  ordered_run(table_, lowered, cond, ast.order_by->expr->to_cuda_expr(), !ast.order_by->ascending, lim, off, out);
  return out;
}

void WarpDB::query_arrow_select_ordered(const std::vector<std::string> &exprs, const std::string &where,
                                        const std::string &order_by, bool descending, int64_t limit, int64_t offset,
                                        ArrowArray *out_array, ArrowSchema *out_schema) {
  const ResultTable r = query_select_ordered(exprs, where, order_by, descending, limit, offset);
  std::vector<const float *> columns;
  for (const auto &c : r.columns) columns.push_back(c.data());
  export_select_to_arrow(r.names, columns, r.rows.data(), static_cast<int64_t>(r.rows.size()), out_array, out_schema);
}

WarpDB::ResultTable WarpDB::query_sql_table(const std::string &sql) {
  QueryAST ast;
  try {
    ast = parse_query(tokenize(sql));
  } catch (const std::exception &e) {
    throw std::runtime_error(std::string("Failed to parse SQL: ") + e.what());
  }
  const auto cols = names_of(table_);
  auto validate_ctx = [&](const ASTNode *n, const std::string &ctx) {
    try {
      validate_ast(n, cols);
    } catch (const std::exception &e) {
      throw std::runtime_error(ctx + ": " + e.what());
    }
  };
  if (ast.select_list.empty()) throw std::runtime_error("Empty SELECT list");
  for (const auto &e : ast.select_list) validate_ctx(e.get(), "SELECT clause");
  for (const auto &j : ast.joins) validate_ctx(j.condition.get(), "JOIN condition");
  if (ast.where) validate_ctx(ast.where->get(), "WHERE clause");
  if (ast.group_by)
    for (const auto &k : ast.group_by->keys) validate_ctx(k.get(), "GROUP BY");
  if (ast.order_by) validate_ctx(ast.order_by->expr.get(), "ORDER BY");
  if (!ast.joins.empty()) throw std::runtime_error("JOIN is not supported by the execution engine");

  const size_t m = ast.select_list.size();
  ResultTable out;
  for (size_t i = 0; i < m; ++i) out.names.push_back(column_name(ast.select_list[i].get(), i));
  const std::string cond = ast.where ? (*ast.where)->to_cuda_expr() : std::string();
  const size_t off = ast.offset ? static_cast<size_t>(std::max(0, ast.offset->count)) : 0;
  const size_t lim = ast.limit ? static_cast<size_t>(std::max(0, ast.limit->count)) : SIZE_MAX;
  auto slice = [&](auto &r) {
    if (off >= r.size()) {
      r.clear();
      return;
    }
    r.erase(r.begin(), r.begin() + static_cast<long>(off));
    if (r.size() > lim) r.resize(lim);
  };
  auto is_agg = [](const ASTNode *n) { return dynamic_cast<const AggregationNode *>(n) != nullptr; };
  for (const auto &e : ast.select_list)
    if (dynamic_cast<const WindowFunctionNode *>(e.get()))
      throw std::runtime_error("window functions are not supported by the execution engine");

  // one item that query_sql answers whole: an aggregate, or an ordered /
  // distinct projection (no row ids: the rows are aggregated or permuted)
  if (m == 1 && (is_agg(ast.select_list[0].get()) || (!ast.group_by && (ast.order_by || ast.distinct)))) {
    out.columns.push_back(query_sql(sql));
    return out;
  }

  if (ast.group_by) {
    if (ast.group_by->keys.size() != 1) throw std::runtime_error("GROUP BY supports one key expression");
    if (ast.distinct) throw std::runtime_error("DISTINCT over a multi-column result is not supported");
    const ASTNode *key = ast.group_by->keys[0].get();
    // every item: the key, or an aggregate of the one common value expression
    // (COUNT counts the group's rows whatever it names)
    const ASTNode *val = nullptr, *counted = nullptr;
    bool mm = false;
    for (size_t i = 0; i < m; ++i) {
      const ASTNode *item = ast.select_list[i].get();
      if (auto a = dynamic_cast<const AggregationNode *>(item)) {
        mm = mm || uses_minmax(a);
        if (a->agg == AggregationType::Count) {
          if (!counted) counted = a->expr.get();
        } else if (!val) {
          val = a->expr.get();
        } else if (!same_expr(val, a->expr.get())) {
          throw std::runtime_error("GROUP BY select list aggregates two different expressions (" +
                                   val->to_cuda_expr() + " and " + a->expr->to_cuda_expr() + "): one is supported");
        }
      } else if (!same_expr(item, key)) {
        throw std::runtime_error("select item " + std::to_string(i) +
                                 " must be the GROUP BY key or an aggregate (SUM / AVG / COUNT / MIN / MAX)");
      }
    }
    if (!val) val = counted ? counted : key;
    const GroupRun r = run_grouped(table_, ast, val, mm, cond);
    out.columns.assign(m, std::vector<float>());
    for (size_t j = 0; j < m; ++j) {
      auto a = dynamic_cast<const AggregationNode *>(ast.select_list[j].get());
      for (size_t i : r.order)
        out.columns[j].push_back(a ? static_cast<float>(r.value_of(a->agg, i)) : static_cast<float>(r.keys[i]));
      slice(out.columns[j]);
    }
    return out;
  }

  for (const auto &e : ast.select_list)
    if (is_agg(e.get()))
      throw std::runtime_error("aggregates beside other select items need GROUP BY: not supported");
  if (ast.order_by || ast.distinct)
    throw std::runtime_error("ORDER BY / DISTINCT over a multi-column result is not supported (row order only)");
  if (m > kMaxSelectExprs)
    throw std::runtime_error("a select list takes at most " + std::to_string(kMaxSelectExprs) + " expressions");
  std::vector<std::string> lowered;
  for (const auto &e : ast.select_list) lowered.push_back(e->to_cuda_expr());
  // row order: only the first OFFSET + LIMIT rows are downloaded
  const int64_t want = !ast.limit ? table_.num_rows
                                  : static_cast<int64_t>(std::min<size_t>(static_cast<size_t>(table_.num_rows),
                                                                          off + std::min(lim, SIZE_MAX - off)));
  select_run(table_, lowered, cond, want, out);
  for (auto &c : out.columns) slice(c);
  slice(out.rows);
  return out;
}
