// pywarpdb.cpp -- Python module with the reference's binding surface
// (bindings/python/pywarpdb.cpp:7-38): WarpDB(path), query, query_multi_gpu,
// query_multi_gpu_csv (static), query_arrow -> (array capsule, schema
// capsule); plus query_sql / query_compact / query_sum and the front end.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "warpdb/multi_gpu_utils.hpp"
#include "warpdb/optimizer.hpp"
#include "warpdb/warpdb.hpp"

namespace py = pybind11;

namespace {
py::dict stats_to_dict(const warpdb::StatsMap &m) {
  py::dict d;
  for (const auto &kv : m) {
    const auto &r = kv.second;
    d[py::str(kv.first)] = py::make_tuple(r.known ? py::cast(r.min) : py::none(),
                                          r.known ? py::cast(r.max) : py::none(), r.null_count, r.is_int);
  }
  return d;
}

// {name: (min, max, null_count, is_int)}; min/max None = unbounded
warpdb::StatsMap stats_from_dict(const py::dict &d) {
  warpdb::StatsMap m;
  for (auto item : d) {
    auto t = item.second.cast<py::tuple>();
    warpdb::ColumnRange r;
    r.known = !t[0].is_none() && !t[1].is_none();
    if (r.known) {
      r.min = t[0].cast<double>();
      r.max = t[1].cast<double>();
    }
    r.null_count = t.size() > 2 ? t[2].cast<int64_t>() : 0;
    r.is_int = t.size() > 3 ? t[3].cast<bool>() : false;
    m[item.first.cast<std::string>()] = r;
  }
  return m;
}
// (keys int32, sums float64, counts int64) as numpy arrays
py::tuple group_arrays(const warpdb::GroupResult &g) {
  return py::make_tuple(py::array_t<int32_t>(static_cast<py::ssize_t>(g.keys.size()), g.keys.data()),
                        py::array_t<double>(static_cast<py::ssize_t>(g.sums.size()), g.sums.data()),
                        py::array_t<int64_t>(static_cast<py::ssize_t>(g.counts.size()), g.counts.data()));
}

py::tuple topk_arrays(const warpdb::TopkResult &t) {
  return py::make_tuple(py::array_t<float>(static_cast<py::ssize_t>(t.keys.size()), t.keys.data()),
                        py::array_t<int64_t>(static_cast<py::ssize_t>(t.rows.size()), t.rows.data()),
                        py::array_t<float>(static_cast<py::ssize_t>(t.values.size()), t.values.data()));
}

// (names, [float32 array per column], int64 source rows)
py::tuple table_arrays(const warpdb::ResultTable &t) {
  py::list cols;
  for (const auto &c : t.columns) cols.append(py::array_t<float>(static_cast<py::ssize_t>(c.size()), c.data()));
  return py::make_tuple(t.names, cols, py::array_t<int64_t>(static_cast<py::ssize_t>(t.rows.size()), t.rows.data()));
}
// a joined result: table_arrays' three and the matched right rows
py::tuple joined_arrays(const warpdb::ResultTable &t) {
  py::tuple base = table_arrays(t);
  return py::make_tuple(base[0], base[1], base[2],
                        py::array_t<int64_t>(static_cast<py::ssize_t>(t.right_rows.size()), t.right_rows.data()));
}

py::tuple device_capsules(ArrowDeviceArray *arr, ArrowSchema *schema) {
  // named as the Arrow PyCapsule interface names device arrays
  py::capsule a(arr, "arrow_device_array", [](PyObject *o) {
    auto *x = static_cast<ArrowDeviceArray *>(PyCapsule_GetPointer(o, "arrow_device_array"));
    if (x) {
      if (x->array.release) x->array.release(&x->array);
      delete x;
    }
  });
  py::capsule s(schema, "arrow_schema", [](PyObject *o) {
    auto *x = static_cast<ArrowSchema *>(PyCapsule_GetPointer(o, "arrow_schema"));
    if (x) {
      if (x->release) x->release(x);
      delete x;
    }
  });
  return py::make_tuple(a, s);
}

template <typename Arr, typename F>
py::tuple export_with(F &&fn, py::tuple (*wrap)(Arr *, ArrowSchema *)) {
  auto *arr = new Arr();
  auto *schema = new ArrowSchema();
  try {
    py::gil_scoped_release nogil;
    fn(arr, schema);
  } catch (...) {
    delete arr;
    delete schema;
    throw;
  }
  return wrap(arr, schema);
}

py::tuple arrow_capsules(ArrowArray *arr, ArrowSchema *schema) {
  py::capsule a(arr, [](void *p) {
    auto *x = static_cast<ArrowArray *>(p);
    if (x->release) x->release(x);
    delete x;
  });
  py::capsule s(schema, [](void *p) {
    auto *x = static_cast<ArrowSchema *>(p);
    if (x->release) x->release(x);
    delete x;
  });
  return py::make_tuple(a, s);
}
}  // namespace

PYBIND11_MODULE(pywarpdb, m) {
  m.doc() = "WarpDB query engine on AMD Instinct MI355X (hiprtc + gfx950 kernels)";
  py::enum_<DataType>(m, "DataType")
      .value("Int32", DataType::Int32)
      .value("Int64", DataType::Int64)
      .value("Float32", DataType::Float32)
      .value("Float64", DataType::Float64)
      .value("String", DataType::String);

  py::class_<WarpDB>(m, "WarpDB")
      .def(py::init<const std::string &>())
      .def(py::init<const std::string &, const std::vector<DataType> &, int>(), py::arg("path"), py::arg("schema"),
           py::arg("device") = 0)
      .def("query", &WarpDB::query, py::call_guard<py::gil_scoped_release>())
      .def("query_sql", &WarpDB::query_sql, py::call_guard<py::gil_scoped_release>())
      .def("query_multi_gpu", &WarpDB::query_multi_gpu, py::arg("expr"), py::call_guard<py::gil_scoped_release>(),
           "Execute expression using all available GPUs on the current table.")
      .def_static("query_multi_gpu_csv", &WarpDB::query_multi_gpu_csv, py::arg("csv_path"), py::arg("expr"),
                  py::arg("rows_per_chunk") = 1000000, py::call_guard<py::gil_scoped_release>(),
                  "Stream a CSV file in chunks across all GPUs and return results.")
      .def(
          "query_arrow",
          [](WarpDB &db, const std::string &expr, bool shared_memory) {
            auto *arr = new ArrowArray();
            auto *schema = new ArrowSchema();
            try {
              db.query_arrow(expr, arr, schema, shared_memory);
            } catch (...) {
              delete arr;
              delete schema;
              throw;
            }
            return arrow_capsules(arr, schema);
          },
          py::arg("expr"), py::arg("shared_memory") = false,
          "Return result as Arrow C Data Interface capsules (ArrowArray, ArrowSchema).")
      .def(
          "query_arrow_device",
          [](WarpDB &db, const std::string &expr) {
            return export_with<ArrowDeviceArray>(
                [&](ArrowDeviceArray *a, ArrowSchema *s) { db.query_arrow_device(expr, a, s); }, device_capsules);
          },
          py::arg("expr"),
          "Dense result left in HBM: (ArrowDeviceArray capsule, ArrowSchema capsule), device_type ARROW_DEVICE_ROCM.")
      .def(
          "query_arrow_compact",
          [](WarpDB &db, const std::string &expr) {
            return export_with<ArrowArray>([&](ArrowArray *a, ArrowSchema *s) { db.query_arrow_compact(expr, a, s); },
                                           arrow_capsules);
          },
          py::arg("expr"), "Passing rows as struct<value: float32, row: int64> (Arrow C Data Interface capsules).")
      .def(
          "query_arrow_device_compact",
          [](WarpDB &db, const std::string &expr) {
            return export_with<ArrowDeviceArray>(
                [&](ArrowDeviceArray *a, ArrowSchema *s) { db.query_arrow_device_compact(expr, a, s); },
                device_capsules);
          },
          py::arg("expr"), "Passing rows as struct<value, row> in HBM (ArrowDeviceArray capsule, ROCm).")
      .def("query_compact", &WarpDB::query_compact, py::call_guard<py::gil_scoped_release>())
      .def(
          "query_select",
          [](WarpDB &db, const std::vector<std::string> &exprs, const std::string &where) {
            warpdb::ResultTable t;
            {
              py::gil_scoped_release nogil;
              t = db.query_select(exprs, where);
            }
            return table_arrays(t);
          },
          py::arg("exprs"), py::arg("where") = "",
          "Several expressions of the rows WHERE keeps, in row order (fused passes of up to four) -> "
          "(names, [float32 arrays], int64 rows).")
      .def(
          "query_sql_table",
          [](WarpDB &db, const std::string &sql) {
            warpdb::ResultTable t;
            {
              py::gil_scoped_release nogil;
              t = db.query_sql_table(sql);
            }
            return table_arrays(t);
          },
          py::arg("sql"),
          "SELECT with several items (plain, or GROUP BY key + aggregates of one expression) -> "
          "(names, [float32 arrays], int64 rows; rows empty for grouped results).")
      .def(
          "query_sql_grouped",
          [](WarpDB &db, const std::string &sql) {
            warpdb::ResultTable t;
            {
              py::gil_scoped_release nogil;
              t = db.query_sql_grouped(sql);
            }
            py::list cols;
            for (const auto &c : t.columns)
              cols.append(py::array_t<float>(static_cast<py::ssize_t>(c.size()), c.data()));
            return py::make_tuple(t.names, cols);
          },
          py::arg("sql"),
          "SELECT key / aggregates of any value expressions ... GROUP BY key [HAVING] [ORDER BY] [LIMIT] [OFFSET] "
          "(fused grouped passes of up to four value expressions) -> (names, [float32 arrays]).")
      .def(
          "attach",
          [](WarpDB &db, const std::string &name, const std::string &path, const std::vector<DataType> &schema) {
            py::gil_scoped_release nogil;
            db.attach(name, path, schema);
          },
          py::arg("name"), py::arg("path"), py::arg("schema") = std::vector<DataType>{},
          "Load a second table (.csv / .json) into HBM of the same device under `name`, for query_join / "
          "query_sql_joined.")
      .def(
          "query_join",
          [](WarpDB &db, const std::string &name, const std::string &left_key, const std::string &right_key,
             const std::vector<std::string> &exprs, const std::string &where, bool left_outer) {
            warpdb::ResultTable t;
            {
              py::gil_scoped_release nogil;
              t = db.query_join(name, left_key, right_key, exprs, where,
                                left_outer ? WarpDB::JoinType::Left : WarpDB::JoinType::Inner);
            }
            return joined_arrays(t);
          },
          py::arg("name"), py::arg("left_key"), py::arg("right_key"), py::arg("exprs"), py::arg("where") = "",
          py::arg("left_outer") = false,
          "PK-FK equi-join with an attached table: (names, columns, left row ids, matched right rows; -1 unmatched).")
      .def(
          "query_sql_joined",
          [](WarpDB &db, const std::string &sql) {
            warpdb::ResultTable t;
            {
              py::gil_scoped_release nogil;
              t = db.query_sql_joined(sql);
            }
            return joined_arrays(t);
          },
          py::arg("sql"),
          "SELECT items FROM t [INNER | LEFT [OUTER]] JOIN u ON <left expression> = <right column> [WHERE c] [LIMIT n] "
          "[OFFSET m]: (names, columns, left row ids, matched right rows).")
      .def(
          "query_sql_joined_grouped",
          [](WarpDB &db, const std::string &sql) {
            warpdb::ResultTable t;
            {
              py::gil_scoped_release nogil;
              t = db.query_sql_joined_grouped(sql);
            }
            py::list cols;
            for (const auto &c : t.columns)
              cols.append(py::array_t<float>(static_cast<py::ssize_t>(c.size()), c.data()));
            return py::make_tuple(t.names, cols);
          },
          py::arg("sql"),
          "SELECT key / aggregates FROM t [INNER] JOIN u ON <left expression> = <right column> [WHERE c] GROUP BY key "
          "[HAVING] [ORDER BY] [LIMIT] [OFFSET] (the probe fused into the grouped pass) -> (names, [float32 arrays]).")
      .def(
          "query_sql_windowed",
          [](WarpDB &db, const std::string &sql) {
            warpdb::ResultTable t;
            {
              py::gil_scoped_release nogil;
              t = db.query_sql_windowed(sql);
            }
            return table_arrays(t);
          },
          py::arg("sql"),
          "SELECT plain items and AGG(x) OVER (PARTITION BY k) items FROM t [WHERE c] [LIMIT n] [OFFSET m] "
          "(one grouped pass, then fused broadcast passes of up to four items) -> "
          "(names, [float32 arrays], int64 rows).")
      .def(
          "query_arrow_sql_windowed",
          [](WarpDB &db, const std::string &sql) {
            return export_with<ArrowArray>(
                [&](ArrowArray *a, ArrowSchema *s) { db.query_arrow_sql_windowed(sql, a, s); }, arrow_capsules);
          },
          py::arg("sql"),
          "query_sql_windowed as struct<one float32 child per item, row: int64> (Arrow C Data Interface capsules).")
      .def(
          "query_arrow_select",
          [](WarpDB &db, const std::vector<std::string> &exprs, const std::string &where) {
            return export_with<ArrowArray>(
                [&](ArrowArray *a, ArrowSchema *s) { db.query_arrow_select(exprs, where, a, s); }, arrow_capsules);
          },
          py::arg("exprs"), py::arg("where") = "",
          "query_select as struct<one float32 child per expression, row: int64> (Arrow C Data Interface capsules).")
      .def(
          "query_select_ordered",
          [](WarpDB &db, const std::vector<std::string> &exprs, const std::string &where, const std::string &order_by,
             bool descending, int64_t limit, int64_t offset) {
            warpdb::ResultTable t;
            {
              py::gil_scoped_release nogil;
              t = db.query_select_ordered(exprs, where, order_by, descending, limit, offset);
            }
            return table_arrays(t);
          },
          py::arg("exprs"), py::arg("where"), py::arg("order_by"), py::arg("descending") = false,
          py::arg("limit") = -1, py::arg("offset") = 0,
          "Several expressions of the rows WHERE keeps, ordered by one key expression (one sort or top-K scan, "
          "then a fused row gather) -> (names, [float32 arrays], int64 rows).")
      .def(
          "query_rows",
          [](WarpDB &db, const std::vector<std::string> &exprs, const std::vector<int64_t> &rows) {
            warpdb::ResultTable t;
            {
              py::gil_scoped_release nogil;
              t = db.query_rows(exprs, rows);
            }
            return table_arrays(t);
          },
          py::arg("exprs"), py::arg("rows"),
          "Several expressions at the given row ids (late materialisation) -> (names, [float32 arrays], int64 rows).")
      .def(
          "query_sql_ordered",
          [](WarpDB &db, const std::string &sql) {
            warpdb::ResultTable t;
            {
              py::gil_scoped_release nogil;
              t = db.query_sql_ordered(sql);
            }
            return table_arrays(t);
          },
          py::arg("sql"),
          "SELECT a, b, ... FROM t [WHERE c] ORDER BY o [ASC|DESC] [LIMIT n] [OFFSET m] -> "
          "(names, [float32 arrays], int64 rows).")
      .def(
          "query_arrow_select_ordered",
          [](WarpDB &db, const std::vector<std::string> &exprs, const std::string &where, const std::string &order_by,
             bool descending, int64_t limit, int64_t offset) {
            return export_with<ArrowArray>(
                [&](ArrowArray *a, ArrowSchema *s) {
                  db.query_arrow_select_ordered(exprs, where, order_by, descending, limit, offset, a, s);
                },
                arrow_capsules);
          },
          py::arg("exprs"), py::arg("where"), py::arg("order_by"), py::arg("descending") = false,
          py::arg("limit") = -1, py::arg("offset") = 0,
          "query_select_ordered as struct<one float32 child per expression, row: int64> (Arrow C Data Interface "
          "capsules).")
      .def("query_sum", &WarpDB::query_sum, py::call_guard<py::gil_scoped_release>())
      .def("query_multi_gpu_sum", &WarpDB::query_multi_gpu_sum, py::call_guard<py::gil_scoped_release>())
      .def(
          "query_multi_gpu_group",
          [](WarpDB &db, const std::string &sql, int32_t key_lo) {
            warpdb::GroupResult g;
            {
              py::gil_scoped_release nogil;
              g = db.query_multi_gpu_group(sql, key_lo);
            }
            return group_arrays(g);
          },
          py::arg("sql"), py::arg("key_window_lo") = 0,
          "GROUP BY over every GPU (one RCCL all-reduce of the key window) -> (keys, sums, counts).")
      .def(
          "query_multi_gpu_topk",
          [](WarpDB &db, const std::string &sql) {
            warpdb::TopkResult t;
            {
              py::gil_scoped_release nogil;
              t = db.query_multi_gpu_topk(sql);
            }
            return topk_arrays(t);
          },
          py::arg("sql"), "ORDER BY .. LIMIT k over every GPU (one RCCL all-gather) -> (keys, rows, values).")
      .def(
          "column_stats",
          [](const WarpDB &db) {
            warpdb::StatsMap m;
            {
              py::gil_scoped_release nogil;
              m = warpdb::compute_column_stats(db.table());
            }
            return stats_to_dict(m);
          },
          "Per-column (min, max, null_count, is_int) as the kernels see the values (optimizer statistics).")
      .def(
          "query_optimized",
          [](const WarpDB &db, const std::string &q, py::object stats) {
            std::string e, c;
            warpdb::split_where(q, e, c);
            warpdb::StatsMap m;
            const bool have = !stats.is_none();
            if (have) m = stats_from_dict(stats.cast<py::dict>());
            warpdb::Verdict v;
            std::vector<float> r;
            {
              py::gil_scoped_release nogil;
              r = warpdb::query_optimized(e, c, db.table(), have ? &m : nullptr, &v);
            }
            return py::make_tuple(r, warpdb::verdict_name(v));
          },
          py::arg("query"), py::arg("stats") = py::none(),
          "Dense projection with statistics pushdown -> (values, verdict).")
      .def_property_readonly("num_rows", [](const WarpDB &db) { return db.table().num_rows; })
      .def_property_readonly("column_names", [](const WarpDB &db) {
        std::vector<std::string> n;
        for (const auto &c : db.table().columns) n.push_back(c.name);
        return n;
      });

  // Row shards resident across GPUs (the single-process multi-GPU path:
  // ncclCommInitAll over devices 0..n-1).  Expressions are lowered C
  // strings, as the jit_* entry points take them.
  py::class_<warpdb::ResidentShards>(m, "ResidentShards")
      .def_static(
          "synthetic",
          [](int64_t n_rows, const std::vector<py::tuple> &cols, int devices) {
            std::vector<warpdb::SyntheticColumn> sc;
            for (const auto &t : cols)
              sc.push_back({t[0].cast<std::string>(), t[1].cast<DataType>(), t[2].cast<uint64_t>(), t[3].cast<int>(),
                            t[4].cast<double>(), t[5].cast<double>()});
            py::gil_scoped_release nogil;
            return warpdb::ResidentShards::synthetic(n_rows, sc, devices);
          },
          py::arg("n_rows"), py::arg("columns"), py::arg("devices") = 0,
          "n_rows generated in HBM over `devices` GPUs; columns = [(name, DataType, seed, kind, lo, hi)]")
      .def_property_readonly("num_rows", &warpdb::ResidentShards::num_rows)
      .def_property_readonly("num_shards", &warpdb::ResidentShards::num_shards)
      .def("ranges",
           [](const warpdb::ResidentShards &r) {
             py::list out;
             for (auto &s : r.ranges()) out.append(py::make_tuple(s.device, s.begin, s.end));
             return out;
           })
      .def("sum", &warpdb::ResidentShards::sum, py::arg("expr"), py::arg("cond") = "",
           py::call_guard<py::gil_scoped_release>())
      .def(
          "group_sum",
          [](const warpdb::ResidentShards &r, const std::string &val, const std::string &key, const std::string &cond,
             int32_t key_lo) {
            warpdb::GroupResult g;
            {
              py::gil_scoped_release nogil;
              g = r.group_sum(val, key, cond, key_lo);
            }
            return group_arrays(g);
          },
          py::arg("val"), py::arg("key"), py::arg("cond") = "", py::arg("key_window_lo") = 0)
      .def(
          "topk",
          [](const warpdb::ResidentShards &r, const std::string &order, const std::string &cond,
             const std::string &select, int64_t k, bool descending) {
            warpdb::TopkResult t;
            {
              py::gil_scoped_release nogil;
              t = r.topk(order, cond, select, k, descending);
            }
            return topk_arrays(t);
          },
          py::arg("order"), py::arg("cond") = "", py::arg("select") = "", py::arg("k") = 5,
          py::arg("descending") = true)
      .def("dense", &warpdb::ResidentShards::dense, py::arg("expr"), py::arg("cond") = "",
           py::call_guard<py::gil_scoped_release>())
      .def("set_timing", &warpdb::ResidentShards::set_timing, py::arg("kernels"), py::arg("exchange") = false,
           "time the next queries' main kernels (HIP events) and / or their exchanges")
      .def(
          "take_timing",
          [](warpdb::ResidentShards &r) {
            warpdb::ApiTiming t;
            {
              py::gil_scoped_release nogil;
              t = r.take_timing();
            }
            py::dict d;
            d["kernel_ms"] = t.kernel_ms;
            d["launches"] = t.launches;
            d["exchange_ms"] = t.exchange_ms < 0 ? py::object(py::none()) : py::object(py::float_(t.exchange_ms));
            d["exchanges"] = t.exchanges;
            return d;
          },
          "{kernel_ms: average main-kernel time (slowest device), launches, exchange_ms (None: no collective ran), "
          "exchanges} since the last read");

  m.def(
      "analyze_condition",
      [](const std::string &where, const py::dict &stats) {
        auto ast = parse_expression(tokenize(where));
        return std::string(warpdb::verdict_name(warpdb::analyze_condition(ast.get(), stats_from_dict(stats))));
      },
      py::arg("where"), py::arg("stats"),
      "Interval analysis of a WHERE clause over {column: (min, max, null_count, is_int)}.");

  m.def(
      "load_csv_columns",
      [](const std::string &path, const std::vector<DataType> &schema, int threads) {
        HostTable h;
        {
          py::gil_scoped_release nogil;
          if (threads > 0) setenv("WARPDB_PARSE_THREADS", std::to_string(threads).c_str(), 1);
          h = load_csv_to_host(path, schema);
        }
        py::dict d;
        for (const auto &c : h.columns) {
          std::visit(
              [&](const auto &v) {
                using T = typename std::decay_t<decltype(v)>::value_type;
                if constexpr (std::is_same_v<T, std::string>) {
                  d[py::str(c.name)] = py::cast(v);
                } else {
                  d[py::str(c.name)] = py::array_t<T>(static_cast<py::ssize_t>(v.size()), v.data());
                }
              },
              c.data);
        }
        return d;
      },
      py::arg("path"), py::arg("schema") = std::vector<DataType>{}, py::arg("threads") = 0,
      "Host-side CSV load (load_csv_to_host) as {column: numpy array | list}; no GPU needed.");

  // front end, for tests and tools
  m.def("result_column_names", &warpdb::result_column_names, py::arg("sql"),
        "Result column names of a SELECT list (no table, no GPU).");
  m.def("lower_expression", [](const std::string &e) { return parse_expression(tokenize(e))->to_cuda_expr(); });
  m.def("split_where", [](const std::string &q) {
    std::string e, c;
    warpdb::split_where(q, e, c);
    return py::make_tuple(e, c);
  });
  m.def("tokenize", [](const std::string &s) {
    py::list out;
    for (const auto &t : tokenize(s)) out.append(py::make_tuple(static_cast<int>(t.type), t.value, t.line, t.column));
    return out;
  });
  m.def("parse_query_summary", [](const std::string &sql) {
    QueryAST q = parse_query(tokenize(sql));
    py::dict d;
    py::list sel;
    for (const auto &e : q.select_list) sel.append(e->to_cuda_expr());
    d["select"] = sel;
    d["from"] = q.from_table;
    d["joins"] = q.joins.size();
    d["where"] = q.where ? py::object(py::str((*q.where)->to_cuda_expr())) : py::none();
    d["group_by"] = q.group_by ? py::object(py::int_(q.group_by->keys.size())) : py::none();
    d["having"] = q.having ? py::object(py::str((*q.having)->to_cuda_expr())) : py::none();
    d["order_by"] = q.order_by ? py::object(py::make_tuple(q.order_by->expr->to_cuda_expr(), q.order_by->ascending))
                               : py::none();
    d["limit"] = q.limit ? py::object(py::int_(q.limit->count)) : py::none();
    d["offset"] = q.offset ? py::object(py::int_(q.offset->count)) : py::none();
    d["distinct"] = q.distinct;
    return d;
  });
  m.def("plan_shards", [](int64_t n, int devices) {
    py::list out;
    for (auto &s : warpdb::plan_shards(n, devices)) out.append(py::make_tuple(s.device, s.begin, s.end));
    return out;
  });
}
