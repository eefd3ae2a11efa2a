// warpdb.cpp -- the WarpDB facade on the MI355X execution layer.
// Reference: src/warpdb.cpp:159-590.  query() keeps the reference's result
// contract (dense vector of num_rows floats); the work runs through the C
// ABI (include/warpexec.h) on the table resident in HBM.
//
// This file is the executor: every entry point plans (plan.hpp: what it
// refuses and what it lowers to, decided without the device), runs the plan
// through the wx_* calls, and downloads the result.
#include "warpdb/warpdb.hpp"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cctype>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <deque>
#include <exception>
#include <fstream>
#include <map>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <thread>
#include <unordered_map>

#include "warpdb/internal.hpp"
#include "warpdb/multi_gpu_utils.hpp"
#include "warpdb/plan.hpp"

using warpdb::DeviceBuffer;
using warpdb::DevGuard;
using warpdb::GroupRun;
using warpdb::hip_ok;
using warpdb::Lowered;
using warpdb::names_of;
using warpdb::same_expr;
using warpdb::sync_launch;
using warpdb::Window;
using warpdb::wx_call;
using warpdb::WxTableView;

namespace {

std::string lower_ext(const std::string &path) {
  const auto dot = path.find_last_of('.');
  std::string ext = dot == std::string::npos ? "" : path.substr(dot + 1);
  for (char &ch : ext) ch = static_cast<char>(std::tolower(static_cast<unsigned char>(ch)));
  return ext;
}

// n values of device memory in a fresh host vector: row ids, counts, the
// (few) groups of a GROUP BY.
template <typename T>
std::vector<T> download(const T *d, int64_t n, int device) {
  std::vector<T> h(static_cast<size_t>(n));
  DevGuard g(device);
  if (n) hip_ok(hipMemcpy(h.data(), d, sizeof(T) * static_cast<size_t>(n), hipMemcpyDeviceToHost), "hipMemcpy");
  return h;
}
// A float result column, as large as the table: host_result's pages, filled
// through copy_d2h.
std::vector<float> download_result(const float *d, int64_t n, int device) {
  std::vector<float> h = warpdb::host_result(static_cast<size_t>(n));
  DevGuard g(device);
  if (n) warpdb::copy_d2h(device, nullptr, h.data(), d, sizeof(float) * static_cast<size_t>(n));
  return h;
}

template <typename T>
T *ptr(const DeviceBuffer &b) {
  return static_cast<T *>(b.ptr);
}

// The dense projection: num_rows floats, 0.0f where cond is false.
DeviceBuffer project_dense(const Table &t, const Lowered &q) {
  DeviceBuffer out(t.device, sizeof(float) * static_cast<size_t>(t.num_rows));
  WxTableView v(t);
  wx_launch L = sync_launch(t.device);
  wx_call(wx_project_filter, &v.table, q.expr.c_str(), q.cond.c_str(), &L, WX_MODE_DENSE_FILL, ptr<float>(out), nullptr,
          0, 0, nullptr, nullptr);
  return out;
}

// The ordered compaction with row ids: the first `count` entries of buffers
// sized for every row passing.
struct Compacted {
  DeviceBuffer vals, rows;
  int64_t count = 0;
};
Compacted project_compact(const Table &t, const Lowered &q) {
  const size_t n = static_cast<size_t>(t.num_rows);
  Compacted c;
  c.vals = DeviceBuffer(t.device, sizeof(float) * n);
  c.rows = DeviceBuffer(t.device, sizeof(int64_t) * n);
  WxTableView v(t);
  wx_launch L = sync_launch(t.device);
  wx_call(wx_project_filter, &v.table, q.expr.c_str(), q.cond.c_str(), &L, WX_MODE_COMPACT, ptr<float>(c.vals),
          c.rows.ptr, 8, 0, nullptr, &c.count);
  return c;
}

// One fused pass per chunk of up to WX_MAX_OUTPUTS lowered expressions, the
// chunks sharing min(m, WX_MAX_OUTPUTS) buffers of `rows` floats:
// pass(first, k, ex, dst) runs expressions [first, first + k) into dst[0..k).
template <typename Pass>
void for_each_chunk(int device, const std::vector<std::string> &exprs_c, int64_t rows, Pass &&pass) {
  const size_t m = exprs_c.size();
  std::vector<DeviceBuffer> vals;
  for (size_t j = 0; j < std::min<size_t>(m, WX_MAX_OUTPUTS); ++j)
    vals.emplace_back(device, sizeof(float) * static_cast<size_t>(rows));
  for (size_t first = 0; first < m; first += WX_MAX_OUTPUTS) {
    const size_t k = std::min<size_t>(WX_MAX_OUTPUTS, m - first);
    const char *ex[WX_MAX_OUTPUTS] = {};
    float *dst[WX_MAX_OUTPUTS] = {};
    for (size_t j = 0; j < k; ++j) {
      ex[j] = exprs_c[first + j].c_str();
      dst[j] = ptr<float>(vals[j]);
    }
    pass(first, static_cast<int32_t>(k), ex, dst);
  }
}

void export_result_table(const warpdb::ResultTable &r, ArrowArray *out_array, ArrowSchema *out_schema) {
  std::vector<const float *> columns;
  for (const auto &c : r.columns) columns.push_back(c.data());
  export_select_to_arrow(r.names, columns, r.rows.data(), static_cast<int64_t>(r.rows.size()), out_array, out_schema);
}

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

// The attached tables of every WarpDB (attach()), by name.  Kept outside the
// object (warpdb.hpp says why).  Each table is held by shared pointers whose
// deleter frees its device memory: a running join keeps the table it started
// with, whatever attach() or the destructor do meanwhile.
namespace {
using Attached = std::map<std::string, std::shared_ptr<const Table>>;
std::mutex g_attached_mu;
std::unordered_map<const WarpDB *, Attached> g_attached;
}  // namespace

WarpDB::~WarpDB() {
  Attached mine;
  {
    std::lock_guard<std::mutex> lk(g_attached_mu);
    auto it = g_attached.find(this);
    if (it != g_attached.end()) {
      mine = std::move(it->second);
      g_attached.erase(it);
    }
  }
  mine.clear();  // frees the tables no query still holds
  free_table(table_);
}

std::vector<float> WarpDB::query(const std::string &expr) {
  const DeviceBuffer out = project_dense(table_, warpdb::lower_query(expr, names_of(table_)));
  return download_result(ptr<float>(out), table_.num_rows, table_.device);
}

std::pair<std::vector<float>, std::vector<int64_t>> WarpDB::query_compact(const std::string &expr) {
  const Compacted c = project_compact(table_, warpdb::lower_query(expr, names_of(table_)));
  std::vector<float> vals = download_result(ptr<float>(c.vals), c.count, table_.device);
  return {std::move(vals), download(ptr<int64_t>(c.rows), c.count, table_.device)};
}

std::pair<double, int64_t> WarpDB::query_sum(const std::string &expr) {
  const Lowered q = warpdb::lower_query(expr, names_of(table_));
  WxTableView v(table_);
  wx_launch L = sync_launch(table_.device);
  double s = 0;
  int64_t n = 0;
  wx_call(wx_reduce_sum, &v.table, q.expr.c_str(), q.cond.c_str(), &L, nullptr, &s, &n);
  return {s, n};
}

void WarpDB::query_arrow(const std::string &expr, ArrowArray *out_array, ArrowSchema *out_schema,
                         bool use_shared_memory) {
  auto r = query(expr);
  export_to_arrow(r.data(), static_cast<int64_t>(r.size()), use_shared_memory, out_array, out_schema);
}

void WarpDB::query_arrow_device(const std::string &expr, ArrowDeviceArray *out_array, ArrowSchema *out_schema) {
  DeviceBuffer out = project_dense(table_, warpdb::lower_query(expr, names_of(table_)));
  export_device_to_arrow(static_cast<float *>(out.release()), table_.num_rows, table_.device, out_array, out_schema);
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
  // buffers sized for every row passing; the array's length is the passing count
  Compacted c = project_compact(table_, warpdb::lower_query(expr, names_of(table_)));
  export_device_compact_to_arrow(static_cast<float *>(c.vals.release()), static_cast<int64_t *>(c.rows.release()),
                                 c.count, table_.device, out_array, out_schema);
}

std::vector<float> WarpDB::query_multi_gpu(const std::string &expr) {
  const Lowered q = warpdb::lower_query(expr, names_of(host_table_));
  return shards().dense(q.expr, q.cond);
}

std::pair<double, int64_t> WarpDB::query_multi_gpu_sum(const std::string &expr) {
  const Lowered q = warpdb::lower_query(expr, names_of(host_table_));
  return shards().sum(q.expr, q.cond);
}

warpdb::GroupResult WarpDB::query_multi_gpu_group(const std::string &sql, int32_t key_window_lo) {
  const warpdb::GroupPlan p = warpdb::plan_multi_gpu_group(sql, names_of(host_table_));
  return shards().group_sum(p.value, p.key, p.cond, key_window_lo);
}

warpdb::TopkResult WarpDB::query_multi_gpu_topk(const std::string &sql) {
  const warpdb::TopkPlan p =
      warpdb::plan_multi_gpu_topk(sql, names_of(host_table_), static_cast<int64_t>(host_table_.num_rows()));
  warpdb::TopkResult r;
  if (p.limit == 0) return r;
  r = shards().topk(p.order, p.cond, p.select, p.offset + p.limit, p.descending);
  const size_t drop = std::min(r.keys.size(), static_cast<size_t>(p.offset));  // OFFSET
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
  const Lowered q = warpdb::lower_query(expr, warpdb::NameSet(names.begin(), names.end()));
  // Two-stage pipeline: a parser thread reads chunk i+1 (CsvChunkReader)
  // while the GPUs run chunk i (the reference parses, uploads and runs each
  // chunk in turn, src/warpdb.cpp:544-590).  At most two parsed chunks wait
  // in the queue.
  std::mutex mu;
  std::condition_variable cv;
  std::deque<HostTable> ready;
  bool done = false;
  std::exception_ptr parse_err;
  std::thread parser([&] {
    try {
      warpdb::CsvChunkReader reader(file, names, rows_per_chunk);
      HostTable chunk;
      while (reader.next(chunk)) {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return ready.size() < 2 || done; });
        if (done) break;  // consumer gave up
        ready.push_back(std::move(chunk));
        cv.notify_all();
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
      auto part = run_multi_gpu_jit_host(chunk, q.expr, q.cond);
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
// One grouped query: the wx_group_agg call, its groups downloaded, then
// HAVING and ORDER BY over them on the host (GroupRun::finish), shared by
// query_sql and query_sql_table.  `val` is the aggregated expression, `mm`
// selects the MIN / MAX build.
GroupRun run_grouped(const Table &table, const QueryAST &ast, const ASTNode *val, bool mm, const std::string &cond) {
  const ASTNode *key = ast.group_by->keys[0].get();
  const int dev = table.device;
  const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(table.num_rows, 1 << 22));
  DeviceBuffer dk(dev, cap * 4), ds(dev, cap * 8), dc(dev, cap * 8);
  DeviceBuffer dmn(dev, mm ? cap * 4 : 4), dmx(dev, mm ? cap * 4 : 4);
  WxTableView v(table);
  wx_launch L = sync_launch(dev);
  // WARPDB_GROUP_ROW_ORDER=1: each group's sum folded in row order, the
  // reference's own fold (src/warpdb.cpp:373-385) to the bit (WX_F_ROW_ORDER)
  const char *ro = std::getenv("WARPDB_GROUP_ROW_ORDER");
  if (ro && std::string(ro) == "1") L.flags |= WX_F_ROW_ORDER;
  int64_t g = 0;
  wx_call(wx_group_agg, &v.table, val->to_cuda_expr().c_str(), key->to_cuda_expr().c_str(), cond.c_str(), &L, 0, cap,
          ptr<int32_t>(dk), ptr<double>(ds), ptr<int64_t>(dc), mm ? ptr<float>(dmn) : nullptr,
          mm ? ptr<float>(dmx) : nullptr, nullptr, &g);
  GroupRun run;
  run.keys = download(ptr<int32_t>(dk), g, dev);
  run.sums = download(ptr<double>(ds), g, dev);
  run.cnts = download(ptr<int64_t>(dc), g, dev);
  if (mm) {
    run.mins = download(ptr<float>(dmn), g, dev);
    run.maxs = download(ptr<float>(dmx), g, dev);
  }
  run.finish(ast, val, key);
  return run;
}

// The groups of a GroupedPlan: its slots in chunks of WX_GROUP_MAX_VALUES
// through wx_group_agg_multi (every chunk returns the same keys and counts),
// downloaded, then HAVING and ORDER BY on the host.  WARPDB_GROUP_ROW_ORDER=1:
// one wx_group_agg call with WX_F_ROW_ORDER per slot instead, so that mode
// keeps its bit-exact sums.  `joined` (query_sql_joined_grouped) makes a
// chunk's call instead of wx_group_agg_multi; that route has no row-order mode.
using GroupChunkCall = std::function<void(const char *const *ex, int32_t k, const char *key, const char *cond,
                                          wx_launch *L, int64_t cap, int32_t *d_keys, double *const *d_sums,
                                          int64_t *d_counts, float *const *d_mins, float *const *d_maxs, int64_t *g)>;
warpdb::GroupedRun run_grouped_slots(const Table &table, const warpdb::GroupedPlan &p,
                                     const GroupChunkCall *joined = nullptr) {
  const int dev = table.device;
  const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(table.num_rows, 1 << 22));
  const char *ro = std::getenv("WARPDB_GROUP_ROW_ORDER");
  const bool row_order = !joined && ro && std::string(ro) == "1";
  const std::string key_c = p.key->to_cuda_expr();
  WxTableView v(table);
  wx_launch L = sync_launch(dev);
  if (row_order) L.flags |= WX_F_ROW_ORDER;
  warpdb::GroupedRun r;
  r.slots.resize(p.slots.size());
  DeviceBuffer dk(dev, cap * 4), dc(dev, cap * 8);
  std::vector<DeviceBuffer> ds, dmn, dmx;
  for (int j = 0; j < WX_GROUP_MAX_VALUES; ++j) {
    ds.emplace_back(dev, cap * 8);
    dmn.emplace_back(dev, cap * 4);
    dmx.emplace_back(dev, cap * 4);
  }
  bool first_call = true;
  // what a call returned for slots [first, first + k): the keys and counts of
  // the first call are the result's, every later call's must be the same
  auto collect = [&](size_t first, size_t k, int64_t g) {
    std::vector<int32_t> keys = download(ptr<int32_t>(dk), g, dev);
    std::vector<int64_t> cnts = download(ptr<int64_t>(dc), g, dev);
    if (first_call) {
      r.run.keys = std::move(keys);
      r.run.cnts = std::move(cnts);
      first_call = false;
    } else if (keys != r.run.keys || cnts != r.run.cnts) {
      throw std::runtime_error("grouped query: the passes' groups disagree");
    }
    for (size_t j = 0; j < k; ++j) {
      const auto &slot = p.slots[first + j];
      auto &out = r.slots[first + j];
      if (slot.sum || row_order) out.sums = download(ptr<double>(ds[j]), g, dev);
      if (slot.minmax) {
        out.mins = download(ptr<float>(dmn[j]), g, dev);
        out.maxs = download(ptr<float>(dmx[j]), g, dev);
      }
    }
  };
  const size_t width = row_order ? 1 : WX_GROUP_MAX_VALUES;
  for (const auto &[first, k] : p.chunks(width)) {
    int64_t g = 0;
    if (row_order) {
      const bool mm = p.slots[first].minmax;
      wx_call(wx_group_agg, &v.table, p.slots[first].lowered.c_str(), key_c.c_str(), p.cond.c_str(), &L, 0, cap,
              ptr<int32_t>(dk), ptr<double>(ds[0]), ptr<int64_t>(dc), mm ? ptr<float>(dmn[0]) : nullptr,
              mm ? ptr<float>(dmx[0]) : nullptr, nullptr, &g);
    } else {
      const char *ex[WX_GROUP_MAX_VALUES] = {};
      double *sums[WX_GROUP_MAX_VALUES] = {};
      float *mins[WX_GROUP_MAX_VALUES] = {}, *maxs[WX_GROUP_MAX_VALUES] = {};
      for (size_t j = 0; j < k; ++j) {
        const auto &slot = p.slots[first + j];
        ex[j] = slot.lowered.c_str();
        if (slot.sum) sums[j] = ptr<double>(ds[j]);
        if (slot.minmax) {
          mins[j] = ptr<float>(dmn[j]);
          maxs[j] = ptr<float>(dmx[j]);
        }
      }
      if (joined)
        (*joined)(ex, static_cast<int32_t>(k), key_c.c_str(), p.cond.c_str(), &L, cap, ptr<int32_t>(dk), sums,
                  ptr<int64_t>(dc), mins, maxs, &g);
      else
        wx_call(wx_group_agg_multi, &v.table, ex, static_cast<int32_t>(k), key_c.c_str(), p.cond.c_str(), &L, 0, cap,
                ptr<int32_t>(dk), sums, ptr<int64_t>(dc), mins, maxs, nullptr, &g);
    }
    collect(first, k, g);
  }
  r.finish(p);
  return r;
}

std::vector<float> run_sql(const Table &table, const warpdb::SqlPlan &p) {
  const QueryAST &ast = p.ast;
  const std::string &cond = p.cond;
  const Window &w = p.window;
  const auto *agg = p.agg;
  const int dev = table.device;
  std::vector<float> result;

  if (ast.group_by) {
    const bool mm = warpdb::grouped_minmax(ast, warpdb::uses_minmax(agg));
    const GroupRun r = run_grouped(table, ast, agg->expr.get(), mm, cond);
    for (size_t i : r.order) result.push_back(static_cast<float>(r.value_of(agg->agg, i)));
    if (ast.distinct) {
      std::sort(result.begin(), result.end());
      result.erase(std::unique(result.begin(), result.end()), result.end());
    }
    return w.sliced(std::move(result));
  }

  WxTableView v(table);
  wx_launch L = sync_launch(dev);
  if (agg) {  // ungrouped aggregate over the WHERE rows
    wx_stats st{};
    if (warpdb::uses_minmax(agg))
      wx_call(wx_reduce_stats, &v.table, agg->expr->to_cuda_expr().c_str(), cond.c_str(), &L, nullptr, &st);
    else
      wx_call(wx_reduce_sum, &v.table, agg->expr->to_cuda_expr().c_str(), cond.c_str(), &L, nullptr, &st.sum,
              &st.count);
    double val = NAN;
    switch (agg->agg) {
      case AggregationType::Sum: val = st.sum; break;
      case AggregationType::Avg: val = st.count ? st.sum / static_cast<double>(st.count) : NAN; break;
      case AggregationType::Count: val = static_cast<double>(st.count); break;
      case AggregationType::Min: val = st.min; break;
      case AggregationType::Max: val = st.max; break;
    }
    return w.sliced(std::vector<float>{static_cast<float>(val)});
  }

  const ASTNode *sel = ast.select_list[0].get();
  const std::string sel_c = sel->to_cuda_expr();
  const ASTNode *ob = ast.order_by ? ast.order_by->expr.get() : nullptr;
  // ORDER BY .. LIMIT k: device top-K (ties by ascending row index)
  if (ob && !ast.distinct && w.limited() && w.end() <= 32) {
    const int k = static_cast<int>(w.end());
    if (k == 0) return {};
    DeviceBuffer dv(dev, sizeof(float) * k);
    int64_t m = 0;
    wx_call(wx_topk, &v.table, ob->to_cuda_expr().c_str(), cond.c_str(), sel_c.c_str(), k,
            ast.order_by->ascending ? 0 : 1, &L, 0, nullptr, nullptr, ptr<float>(dv), nullptr, &m);
    return w.sliced(download_result(ptr<float>(dv), m, dev));
  }
  const int64_t n = table.num_rows;
  DeviceBuffer dv(dev, sizeof(float) * static_cast<size_t>(n));
  // ORDER BY a bare float column, no WHERE, no LIMIT: the projection would be
  // a copy of the column, so the sort reads the column itself
  // (src/warpdb.cpp:450-455 projects, then jit_sort_float sorts the copy)
  if (ob && !ast.distinct && !w.limited() && cond.empty() && same_expr(ob, sel)) {
    if (auto var = dynamic_cast<const VariableNode *>(sel)) {
      for (const auto &c : table.columns) {
        if (c.name != var->name || c.type != DataType::Float32) continue;
        wx_call(wx_sort_float_from, static_cast<const float *>(c.device_ptr), ptr<float>(dv), n,
                ast.order_by->ascending ? 1 : 0, &L);
        return w.sliced(download_result(ptr<float>(dv), n, dev));
      }
    }
  }
  // projection of the WHERE rows in row order (ordered compaction)
  int64_t count = 0;
  wx_call(wx_project_filter, &v.table, sel_c.c_str(), cond.c_str(), &L, WX_MODE_COMPACT, ptr<float>(dv), nullptr, 0, 0,
          nullptr, &count);
  if (ob && !same_expr(ob, sel)) {
    // ORDER BY another expression: its values at the same rows (same WHERE,
    // same ascending row order) are the keys of a keyed sort that carries the
    // SELECT values along (the pairs the reference builds, src/warpdb.cpp:470-476)
    if (ast.distinct) throw std::runtime_error("DISTINCT with ORDER BY a different expression is not supported");
    DeviceBuffer dk(dev, sizeof(float) * static_cast<size_t>(n));
    int64_t kcount = 0;
    wx_call(wx_project_filter, &v.table, ob->to_cuda_expr().c_str(), cond.c_str(), &L, WX_MODE_COMPACT, ptr<float>(dk),
            nullptr, 0, 0, nullptr, &kcount);
    if (kcount != count) throw std::runtime_error("ORDER BY rows differ from SELECT rows");
    // with a LIMIT only the first OFFSET + LIMIT rows of the order are needed
    wx_call(wx_sort_by_key_limit, ptr<float>(dk), ptr<float>(dv), count, w.rows_needed(count),
            ast.order_by->ascending ? 1 : 0, &L);
    count = w.rows_needed(count);
  } else if (ob || ast.distinct) {
    const bool asc = ob ? ast.order_by->ascending : true;
    const bool head_only = ob && !ast.distinct && w.limited();  // DISTINCT needs every value
    const int64_t head = head_only ? w.rows_needed(count) : count;
    wx_call(wx_sort_float_limit, ptr<float>(dv), count, head, asc ? 1 : 0, &L);
    count = head;
  }
  result = download_result(ptr<float>(dv), count, dev);
  if (ast.distinct) result.erase(std::unique(result.begin(), result.end()), result.end());
  return w.sliced(std::move(result));
}

// ------------------------------------------------- multi-column results
// The lowered expressions' values at the rows `cond` keeps, in row order,
// and those rows' ids: up to WX_MAX_OUTPUTS expressions per fused pass, the
// same WHERE in every pass; only the first pass writes the row ids, and the
// passes' counts must agree.  At most max_rows rows are downloaded.
void select_run(const Table &table, const std::vector<std::string> &exprs_c, const std::string &cond_c,
                int64_t max_rows, warpdb::ResultTable &out) {
  const int64_t n = table.num_rows;
  DeviceBuffer idx(table.device, sizeof(int64_t) * static_cast<size_t>(n));
  WxTableView v(table);
  wx_launch L = sync_launch(table.device);
  int64_t count = 0, keep = 0;
  out.columns.clear();
  for_each_chunk(table.device, exprs_c, n, [&](size_t first, int32_t k, const char *const *ex, float *const *dst) {
    int64_t c = 0;
    wx_call(wx_project_filter_multi, &v.table, ex, k, cond_c.c_str(), &L, WX_MODE_COMPACT, dst,
            first == 0 ? idx.ptr : nullptr, 8, 0, nullptr, &c);
    if (first == 0) {
      count = c;
      keep = std::min(count, max_rows);
      out.rows = download(ptr<int64_t>(idx), keep, table.device);
    } else if (c != count) {
      throw std::runtime_error("multi-column SELECT: the passes' row counts disagree");
    }
    for (int32_t j = 0; j < k; ++j) out.columns.push_back(download_result(dst[j], keep, table.device));
  });
}

// The lowered expressions of the rows `cond` keeps, ordered by order_c:
// the window `w` of the ordered result.  One wx_select_ordered call; only
// offset + limit rows are computed and downloaded.
void ordered_run(const Table &table, const std::vector<std::string> &exprs_c, const std::string &cond_c,
                 const std::string &order_c, bool descending, const Window &w, warpdb::ResultTable &out) {
  const int64_t want = w.end(), cap = w.rows_needed(table.num_rows);
  const size_t m = exprs_c.size();
  std::vector<DeviceBuffer> vals;
  std::vector<const char *> ex;
  std::vector<float *> dst;
  for (size_t j = 0; j < m; ++j) {
    vals.emplace_back(table.device, sizeof(float) * static_cast<size_t>(cap));
    ex.push_back(exprs_c[j].c_str());
    dst.push_back(ptr<float>(vals[j]));
  }
  DeviceBuffer rows(table.device, sizeof(int64_t) * static_cast<size_t>(cap));
  WxTableView v(table);
  wx_launch L = sync_launch(table.device);
  int64_t count = 0;
  wx_call(wx_select_ordered, &v.table, ex.data(), static_cast<int32_t>(m), cond_c.c_str(), order_c.c_str(),
          descending ? 1 : 0, want, &L, 0, dst.data(), nullptr, ptr<int64_t>(rows), cap, nullptr, &count);
  const int64_t first = std::min(w.offset, count), keep = count - first;
  out.columns.clear();
  for (size_t j = 0; j < m; ++j) out.columns.push_back(download_result(dst[j] + first, keep, table.device));
  out.rows = download(ptr<int64_t>(rows) + first, keep, table.device);
}
}  // namespace

std::vector<float> WarpDB::query_sql(const std::string &sql) {
  return run_sql(table_, warpdb::plan_sql(sql, names_of(table_)));
}

WarpDB::ResultTable WarpDB::query_select(const std::vector<std::string> &exprs, const std::string &where) {
  const auto cols = names_of(table_);
  warpdb::SelectList list = warpdb::lower_select_list(exprs, cols, "query_select");
  const std::string cond_c = warpdb::lower_where(where, cols);
  ResultTable out;
  out.names = std::move(list.names);
  select_run(table_, list.lowered, cond_c, table_.num_rows, out);
  return out;
}

void WarpDB::query_arrow_select(const std::vector<std::string> &exprs, const std::string &where,
                                ArrowArray *out_array, ArrowSchema *out_schema) {
  export_result_table(query_select(exprs, where), out_array, out_schema);
}

WarpDB::ResultTable WarpDB::query_select_ordered(const std::vector<std::string> &exprs, const std::string &where,
                                                 const std::string &order_by, bool descending, int64_t limit,
                                                 int64_t offset) {
  const auto cols = names_of(table_);
  warpdb::SelectList list = warpdb::lower_select_list(exprs, cols, "query_select_ordered");
  const std::string cond_c = warpdb::lower_where(where, cols);
  const std::string order_c = warpdb::lower_order_by(order_by, cols);
  ResultTable out;
  out.names = std::move(list.names);
  ordered_run(table_, list.lowered, cond_c, order_c, descending, Window(offset, limit), out);
  return out;
}

WarpDB::ResultTable WarpDB::query_rows(const std::vector<std::string> &exprs, const std::vector<int64_t> &rows) {
  warpdb::SelectList list = warpdb::lower_select_list(exprs, names_of(table_), "query_rows");
  for (int64_t r : rows)
    if (r < 0 || r >= table_.num_rows) throw std::runtime_error("Row id out of range: " + std::to_string(r));
  const int64_t count = static_cast<int64_t>(rows.size());
  DeviceBuffer ids(table_.device, sizeof(int64_t) * rows.size());
  {
    DevGuard g(table_.device);
    if (count)
      hip_ok(hipMemcpy(ids.ptr, rows.data(), sizeof(int64_t) * rows.size(), hipMemcpyHostToDevice), "hipMemcpy");
  }
  WxTableView v(table_);
  wx_launch L = sync_launch(table_.device);
  ResultTable out;
  out.names = std::move(list.names);
  for_each_chunk(table_.device, list.lowered, count, [&](size_t, int32_t k, const char *const *ex, float *const *dst) {
    wx_call(wx_gather_multi, &v.table, ex, k, ids.ptr, 8, 0, count, nullptr, &L, dst, nullptr, 0);
    for (int32_t j = 0; j < k; ++j) out.columns.push_back(download_result(dst[j], count, table_.device));
  });
  out.rows = rows;
  return out;
}

WarpDB::ResultTable WarpDB::query_sql_ordered(const std::string &sql) {
  warpdb::OrderedPlan p = warpdb::plan_sql_ordered(sql, names_of(table_));
  ResultTable out;
  out.names = std::move(p.names);
  ordered_run(table_, p.lowered, p.cond, p.order, p.descending, p.window, out);
  return out;
}

// A grouped run as the result table of its plan: one column per select item
// over the groups HAVING keeps, in result order, then OFFSET / LIMIT.
static warpdb::ResultTable grouped_result(const warpdb::GroupedPlan &p, const warpdb::GroupedRun &r) {
  warpdb::ResultTable out;
  out.names = p.names;
  for (const auto &item : p.items) {
    std::vector<float> col;
    for (size_t i : r.run.order)
      col.push_back(item.agg ? static_cast<float>(r.value_of(p, *item.agg, item.slot, i))
                             : static_cast<float>(r.run.keys[i]));
    p.window.apply(col);
    out.columns.push_back(std::move(col));
  }
  return out;
}

WarpDB::ResultTable WarpDB::query_sql_grouped(const std::string &sql) {
  const warpdb::GroupedPlan p = warpdb::plan_sql_grouped(sql, names_of(table_));
  return grouped_result(p, run_grouped_slots(table_, p));
}

WarpDB::ResultTable WarpDB::query_sql_windowed(const std::string &sql) {
  const warpdb::WindowedPlan p = warpdb::plan_sql_windowed(sql, names_of(table_));
  const int dev = table_.device;
  const int64_t n = table_.num_rows;
  const size_t n_plain = p.plain.size(), n_out = n_plain + p.items.size();
  // as many partitions as the grouped queries allow groups
  const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(n, 1 << 22));
  std::vector<DeviceBuffer> vals;
  std::vector<float *> dst;
  for (size_t j = 0; j < n_out; ++j) {
    vals.emplace_back(dev, sizeof(float) * static_cast<size_t>(n));
    dst.push_back(ptr<float>(vals[j]));
  }
  std::vector<const char *> ex;
  for (const auto &e : p.plain) ex.push_back(e.c_str());
  std::vector<wx_window_item> items;
  for (const auto &it : p.items) items.push_back({it.value.c_str(), static_cast<int32_t>(it.agg)});
  DeviceBuffer idx(dev, sizeof(int64_t) * static_cast<size_t>(n));
  WxTableView v(table_);
  wx_launch L = sync_launch(dev);
  int64_t count = 0;
  wx_call(wx_window_select, &v.table, ex.data(), static_cast<int32_t>(n_plain), items.data(),
          static_cast<int32_t>(items.size()), p.partition.c_str(), p.cond.c_str(), &L, 0, cap, dst.data(), idx.ptr, 8,
          static_cast<int64_t>(0), nullptr, &count);
  // row order: only the first OFFSET + LIMIT rows are downloaded
  const int64_t keep = std::min(count, p.window.rows_needed(n));
  ResultTable out;
  out.names = p.names;
  for (size_t i = 0; i < n_out; ++i) {
    out.columns.push_back(download_result(dst[p.output[i]], keep, dev));
    p.window.apply(out.columns.back());
  }
  out.rows = download(ptr<int64_t>(idx), keep, dev);
  p.window.apply(out.rows);
  return out;
}

// ------------------------------------------------------------------- joins
// One planned join of `left` with the attached table `right`.
static warpdb::ResultTable join_run(const Table &table_, const Table *right, const warpdb::JoinedPlan &p) {
  if (!right) throw std::runtime_error("Unknown table: " + p.right_table + " (attach it first)");
  const int dev = table_.device;
  const int64_t n = table_.num_rows;
  const size_t m = p.lowered.size();
  // the right table under the planner's prefix, so equal names in the two tables never collide
  WxTableView lv(table_), rv(*right);
  for (size_t c = 0; c < rv.names.size(); ++c) rv.names[c] = warpdb::kJoinRightPrefix + rv.names[c];
  for (size_t c = 0; c < rv.cols.size(); ++c) rv.cols[c].name = rv.names[c].c_str();
  const std::string rkey = warpdb::kJoinRightPrefix + p.right_key;
  std::vector<DeviceBuffer> vals;
  std::vector<float *> dst;
  std::vector<const char *> ex;
  for (size_t j = 0; j < m; ++j) {
    vals.emplace_back(dev, sizeof(float) * static_cast<size_t>(n));
    dst.push_back(ptr<float>(vals[j]));
    ex.push_back(p.lowered[j].c_str());
  }
  DeviceBuffer idx(dev, sizeof(int64_t) * static_cast<size_t>(n)), rrow(dev, sizeof(int32_t) * static_cast<size_t>(n));
  wx_launch L = sync_launch(dev);
  int64_t count = 0;
  wx_call(wx_join_select, &lv.table, &rv.table, p.left_key.c_str(), rkey.c_str(),
          static_cast<int32_t>(p.left_outer ? WX_JOIN_LEFT : WX_JOIN_INNER), ex.data(), static_cast<int32_t>(m),
          p.cond.c_str(), &L, dst.data(), idx.ptr, 8, static_cast<int64_t>(0), ptr<int32_t>(rrow), nullptr, &count);
  // row order: only the first OFFSET + LIMIT rows are downloaded
  const int64_t keep = std::min(count, p.window.rows_needed(n));
  warpdb::ResultTable out;
  out.names = p.names;
  for (size_t j = 0; j < m; ++j) {
    out.columns.push_back(download_result(dst[j], keep, dev));
    p.window.apply(out.columns.back());
  }
  out.rows = download(ptr<int64_t>(idx), keep, dev);
  p.window.apply(out.rows);
  for (int32_t r : download(ptr<int32_t>(rrow), keep, dev)) out.right_rows.push_back(r);
  p.window.apply(out.right_rows);
  return out;
}

std::shared_ptr<const Table> WarpDB::attached(const std::string &name) const {
  std::lock_guard<std::mutex> lk(g_attached_mu);
  auto it = g_attached.find(this);
  if (it == g_attached.end()) return nullptr;
  auto t = it->second.find(name);
  return t == it->second.end() ? nullptr : t->second;
}

void WarpDB::attach(const std::string &name, const std::string &filepath, const std::vector<DataType> &schema) {
  if (warpdb::blank(name)) throw std::runtime_error("attach needs a table name");
  const std::string ext = lower_ext(filepath);
  HostTable host;
  if (ext == "csv") host = load_csv_to_host(filepath, schema);
  else if (ext == "json") host = load_json_to_host(filepath);
  else throw std::runtime_error("Unsupported file format: " + filepath);
  std::shared_ptr<const Table> t(new Table(upload_to_gpu(host, table_.device)), [](const Table *p) {
    free_table(const_cast<Table &>(*p));  // created non-const above
    delete p;
  });
  std::lock_guard<std::mutex> lk(g_attached_mu);
  g_attached[this][name] = std::move(t);  // a table attached earlier under the name goes when its last query ends
}

WarpDB::ResultTable WarpDB::query_join(const std::string &name, const std::string &left_key,
                                       const std::string &right_key, const std::vector<std::string> &exprs,
                                       const std::string &where, JoinType join_type) {
  const std::shared_ptr<const Table> right = attached(name);
  if (!right) throw std::runtime_error("Unknown table: " + name + " (attach it first)");
  // this table has no name of its own outside SQL: only the attached one qualifies
  const warpdb::JoinedPlan p = warpdb::plan_join("", names_of(table_), name, names_of(*right), left_key, right_key,
                                                 exprs, where, join_type == JoinType::Left);
  return join_run(table_, right.get(), p);
}

WarpDB::ResultTable WarpDB::query_sql_joined(const std::string &sql) {
  // the JOIN's table picks the attached table while the planner parses the query (once)
  std::shared_ptr<const Table> right;
  warpdb::NameSet right_cols;
  const warpdb::JoinedPlan p = warpdb::plan_sql_joined(sql, names_of(table_), [&](const std::string &name) {
    right = attached(name);
    if (!right) return static_cast<const warpdb::NameSet *>(nullptr);
    right_cols = names_of(*right);
    return static_cast<const warpdb::NameSet *>(&right_cols);
  });
  return join_run(table_, right.get(), p);
}

WarpDB::ResultTable WarpDB::query_sql_joined_grouped(const std::string &sql) {
  std::shared_ptr<const Table> right;
  warpdb::NameSet right_cols;
  const warpdb::JoinedGroupedPlan p =
      warpdb::plan_sql_joined_grouped(sql, names_of(table_), [&](const std::string &name) {
        right = attached(name);
        if (!right) return static_cast<const warpdb::NameSet *>(nullptr);
        right_cols = names_of(*right);
        return static_cast<const warpdb::NameSet *>(&right_cols);
      });
  // the right table under the planner's prefix, as join_run presents it
  WxTableView lv(table_), rv(*right);
  for (size_t c = 0; c < rv.names.size(); ++c) rv.names[c] = warpdb::kJoinRightPrefix + rv.names[c];
  for (size_t c = 0; c < rv.cols.size(); ++c) rv.cols[c].name = rv.names[c].c_str();
  const std::string rkey = warpdb::kJoinRightPrefix + p.right_key;
  const GroupChunkCall call = [&](const char *const *ex, int32_t k, const char *key, const char *cond, wx_launch *L,
                                  int64_t cap, int32_t *d_keys, double *const *d_sums, int64_t *d_counts,
                                  float *const *d_mins, float *const *d_maxs, int64_t *g) {
    wx_call(wx_join_group_agg, &lv.table, &rv.table, p.left_key.c_str(), rkey.c_str(),
            static_cast<int32_t>(WX_JOIN_INNER), ex, k, key, cond, L, 0, cap, d_keys, d_sums, d_counts, d_mins, d_maxs,
            nullptr, g);
  };
  return grouped_result(p.g, run_grouped_slots(table_, p.g, &call));
}

void WarpDB::query_arrow_sql_windowed(const std::string &sql, ArrowArray *out_array, ArrowSchema *out_schema) {
  export_result_table(query_sql_windowed(sql), out_array, out_schema);
}

void WarpDB::query_arrow_select_ordered(const std::vector<std::string> &exprs, const std::string &where,
                                        const std::string &order_by, bool descending, int64_t limit, int64_t offset,
                                        ArrowArray *out_array, ArrowSchema *out_schema) {
  export_result_table(query_select_ordered(exprs, where, order_by, descending, limit, offset), out_array, out_schema);
}

WarpDB::ResultTable WarpDB::query_sql_table(const std::string &sql) {
  using Route = warpdb::TablePlan::Route;
  warpdb::TablePlan p = warpdb::plan_sql_table(sql, names_of(table_));
  const Window &w = p.sql.window;
  ResultTable out;
  out.names = std::move(p.names);
  switch (p.route) {
    case Route::Single:
      out.columns.push_back(run_sql(table_, p.sql));
      break;
    case Route::Grouped: {
      const GroupRun r = run_grouped(table_, p.sql.ast, p.value, p.minmax, p.sql.cond);
      for (const auto &agg : p.items) {
        std::vector<float> col;
        for (size_t i : r.order)
          col.push_back(agg ? static_cast<float>(r.value_of(*agg, i)) : static_cast<float>(r.keys[i]));
        w.apply(col);
        out.columns.push_back(std::move(col));
      }
      break;
    }
    case Route::Rows:
      // row order: only the first OFFSET + LIMIT rows are downloaded
      select_run(table_, p.lowered, p.sql.cond, w.rows_needed(table_.num_rows), out);
      for (auto &c : out.columns) w.apply(c);
      w.apply(out.rows);
      break;
  }
  return out;
}
