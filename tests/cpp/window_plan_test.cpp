// window_plan_test.cpp -- the front end and the planner of
// WarpDB::query_sql_windowed (plan_sql_windowed) without a device: what the
// parser stores of an OVER clause, what it refuses with line and column,
// every refusal of the planner with its message and their order, and what
// accepted queries lower to.
// Build: make -C tests/cpp bin/window_plan_test; run from the repository root.
#include <cstdio>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../warpdb_amd/csrc/warpdb/plan.hpp"

static int failures = 0;
#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                \
    }                                                            \
  } while (0)

using warpdb::NameSet;
using warpdb::WindowedPlan;
static const NameSet kCols{"price", "quantity", "a", "b", "c", "d", "e"};

static WindowedPlan plan(const std::string &sql) { return warpdb::plan_sql_windowed(sql, kCols); }

static std::string refusal(const std::string &sql) {
  try {
    plan(sql);
  } catch (const std::runtime_error &e) {
    return e.what();
  }
  return "<no error>";
}
template <typename F>
static std::string error_of(F &&f) {
  try {
    f();
  } catch (const std::runtime_error &e) {
    return e.what();
  }
  return "<no error>";
}
static bool has(const std::string &s, const std::string &part) { return s.find(part) != std::string::npos; }

static const WindowFunctionNode *window_item(const QueryAST &q, size_t i) {
  return dynamic_cast<const WindowFunctionNode *>(q.select_list.at(i).get());
}

static void parser() {
  QueryAST q = parse_query(tokenize("SELECT price, SUM(price) OVER (PARTITION BY quantity) FROM t WHERE price > 15"));
  const WindowFunctionNode *w = window_item(q, 1);
  CHECK(w && w->agg == AggregationType::Sum && w->expr->to_cuda_expr() == "price[idx]");
  CHECK(w && w->partition_by.size() == 1 && w->partition_by[0]->to_cuda_expr() == "quantity[idx]" && !w->order_by);
  CHECK(!window_item(q, 0) && q.where);

  q = parse_query(tokenize("SELECT COUNT(*) OVER () FROM t"));
  w = window_item(q, 0);
  CHECK(w && w->agg == AggregationType::Count && w->partition_by.empty() && !w->order_by);
  CHECK(w && w->expr->to_cuda_expr() == "1.0f");

  q = parse_query(tokenize("SELECT MAX(a * b) OVER (PARTITION BY (a + 1) * 2, b, discount(c, d)) FROM t"));
  w = window_item(q, 0);
  CHECK(w && w->partition_by.size() == 3);
  CHECK(w && w->partition_by[0]->to_cuda_expr() == "((a[idx] + 1.0f) * 2.0f)");
  CHECK(w && w->partition_by[2]->to_cuda_expr() == "discount(c[idx], d[idx])");

  q = parse_query(tokenize("SELECT AVG(a) OVER (PARTITION BY b ORDER BY c DESC), MIN(a) OVER (ORDER BY c) FROM t"));
  w = window_item(q, 0);
  CHECK(w && w->partition_by.size() == 1 && w->order_by && !w->order_by->ascending);
  CHECK(w && w->order_by && w->order_by->expr->to_cuda_expr() == "c[idx]");
  w = window_item(q, 1);
  CHECK(w && w->partition_by.empty() && w->order_by && w->order_by->ascending);

  // a plain aggregate is still an AggregationNode
  q = parse_query(tokenize("SELECT SUM(a) FROM t"));
  CHECK(!window_item(q, 0) && dynamic_cast<const AggregationNode *>(q.select_list[0].get()));

  // anything else after OVER: a parse error with line and column
  auto parse_error = [](const std::string &sql) { return error_of([&] { parse_query(tokenize(sql)); }); };
  CHECK(parse_error("SELECT SUM(a) OVER w FROM t") == "Expected '(' after OVER at line 1 column 20");
  CHECK(parse_error("SELECT SUM(a) OVER FROM t") == "Expected '(' after OVER at line 1 column 20");
  CHECK(parse_error("SELECT SUM(a) OVER (PARTITION b) FROM t") == "Expected keyword 'BY' at line 1 column 31");
  CHECK(parse_error("SELECT SUM(a) OVER (PARTITION BY) FROM t") ==
        "Expected an expression after PARTITION BY at line 1 column 33");
  CHECK(parse_error("SELECT SUM(a) OVER (PARTITION BY b,) FROM t") ==
        "Expected an expression after PARTITION BY at line 1 column 36");
  CHECK(parse_error("SELECT SUM(a) OVER (ORDER BY) FROM t") == "Expected an expression after ORDER BY at line 1 column 29");
  CHECK(parse_error("SELECT SUM(a) OVER (ROWS 3) FROM t") == "Unexpected token in OVER clause: ROWS at line 1 column 21");
  CHECK(parse_error("SELECT SUM(a) OVER (b) FROM t") == "Unexpected token in OVER clause: b at line 1 column 21");
  CHECK(parse_error("SELECT SUM(a)\n  OVER (PARTITION BY b) c FROM t") == "Expected ')' to close OVER at line 2 column 27");
  CHECK(has(refusal("SELECT SUM(a) OVER (ROWS 3) FROM t"), "Failed to parse SQL: Unexpected token in OVER clause"));
  // a frame or a second key after ORDER BY is reported the same way
  CHECK(parse_error("SELECT SUM(a) OVER (ORDER BY c ROWS BETWEEN 1 AND 2) FROM t") ==
        "Unexpected token in OVER clause: ROWS at line 1 column 32");
  CHECK(parse_error("SELECT SUM(a) OVER (PARTITION BY b ORDER BY c + 1 DESC RANGE 3) FROM t") ==
        "Unexpected token in OVER clause: RANGE at line 1 column 56");
  CHECK(parse_error("SELECT SUM(a) OVER (ORDER BY c, d) FROM t") == "Unexpected token in OVER clause: , at line 1 column 31");
  CHECK(parse_error("SELECT SUM(a) OVER (ORDER BY c ASC DESC) FROM t") ==
        "Unexpected token in OVER clause: DESC at line 1 column 36");
  q = parse_query(tokenize("SELECT SUM(a) OVER (ORDER BY discount(c, d) * (a + 1) DESC) FROM t"));
  w = window_item(q, 0);
  CHECK(w && w->order_by && !w->order_by->ascending &&
        w->order_by->expr->to_cuda_expr() == "(discount(c[idx], d[idx]) * (a[idx] + 1.0f))");
  q = parse_query(tokenize("SELECT SUM(a) OVER (ORDER BY a > 1 AND b < 2 ASC) FROM t"));
  w = window_item(q, 0);
  CHECK(w && w->order_by && w->order_by->ascending && w->order_by->expr->to_cuda_expr() ==
                                                           "((a[idx] > 1.0f) && (b[idx] < 2.0f))");

  // reentrant: the same text parses the same twice, and an error leaves no state behind
  for (int rep = 0; rep < 2; ++rep) {
    CHECK(parse_error("SELECT SUM(a) OVER (ROWS 3) FROM t") == "Unexpected token in OVER clause: ROWS at line 1 column 21");
    q = parse_query(tokenize("SELECT SUM(a) OVER (PARTITION BY b) FROM t"));
    CHECK(window_item(q, 0) && window_item(q, 0)->partition_by.size() == 1);
  }
}

static void accepted() {
  WindowedPlan p = plan("SELECT price, SUM(price) OVER (PARTITION BY quantity) FROM t WHERE price > 15");
  CHECK(p.plain == std::vector<std::string>{"price[idx]"});
  CHECK(p.items.size() == 1 && p.items[0].value == "price[idx]" && p.items[0].agg == AggregationType::Sum);
  CHECK(p.partition == "quantity[idx]" && p.cond == "(price[idx] > 15.0f)");
  CHECK((p.names == std::vector<std::string>{"price", "expr1"}));
  CHECK((p.names == warpdb::result_column_names("SELECT price, SUM(price) OVER (PARTITION BY quantity) FROM t")));
  CHECK((p.output == std::vector<size_t>{0, 1}) && !p.window.limited() && p.window.offset == 0);

  // window items go after the plain expressions, whatever the list order
  p = plan("SELECT AVG(a) OVER (PARTITION BY b + 1), c, MAX(a * 2) OVER (PARTITION BY b + 1), d * 2 FROM t LIMIT 5 OFFSET 2");
  CHECK((p.plain == std::vector<std::string>{"c[idx]", "(d[idx] * 2.0f)"}));
  CHECK(p.items.size() == 2 && p.items[0].agg == AggregationType::Avg && p.items[1].value == "(a[idx] * 2.0f)");
  CHECK((p.output == std::vector<size_t>{2, 0, 3, 1}));
  CHECK(p.partition == "(b[idx] + 1.0f)" && p.window.limit == 5 && p.window.offset == 2 && p.cond.empty());
  CHECK((p.names == std::vector<std::string>{"expr0", "c", "expr2", "expr3"}));

  // OVER () is one partition: the key 0; COUNT(*) counts as elsewhere
  p = plan("SELECT COUNT(*) OVER (), SUM(a) OVER () FROM t");
  CHECK(p.partition == "0" && p.plain.empty() && p.items.size() == 2);
  CHECK(p.items[0].agg == AggregationType::Count && p.items[0].value == "1.0f");

  // a constant key is the same single partition
  p = plan("SELECT SUM(a) OVER (PARTITION BY 0), COUNT(*) OVER (), MAX(a) OVER (PARTITION BY 7) FROM t");
  CHECK(p.partition == "0" && p.items.size() == 3);

  // five aggregates of one value and COUNTs of anything: one distinct value
  p = plan("SELECT SUM(a) OVER (PARTITION BY b), AVG(a) OVER (PARTITION BY b), MIN(a) OVER (PARTITION BY b), "
           "MAX(a) OVER (PARTITION BY b), COUNT(c) OVER (PARTITION BY b), COUNT(d) OVER (PARTITION BY b), "
           "COUNT(e) OVER (PARTITION BY b), COUNT(price) OVER (PARTITION BY b), COUNT(quantity) OVER (PARTITION BY b) "
           "FROM t");
  CHECK(p.items.size() == 9);
  // four distinct values are the most
  p = plan("SELECT SUM(a) OVER (), SUM(b) OVER (), SUM(c) OVER (), SUM(d) OVER () FROM t");
  CHECK(p.items.size() == 4);
  // sixteen items are the most
  std::string many = "SELECT a";
  for (int i = 0; i < 15; ++i) many += ", SUM(a) OVER (PARTITION BY b)";
  CHECK(plan(many + " FROM t").items.size() == 15);
}

static void refusals() {
  const std::string w = "SUM(a) OVER (PARTITION BY b)";
  CHECK(has(refusal("SELECT FROM"), "Failed to parse SQL"));
  CHECK(refusal("SELECT price, SUM(nope) OVER (PARTITION BY b) FROM t") == "SELECT clause: Unknown column: nope");
  CHECK(refusal("SELECT price, SUM(a) OVER (PARTITION BY nope) FROM t") == "SELECT clause: Unknown column: nope");
  CHECK(refusal("SELECT price, SUM(a) OVER (ORDER BY nope) FROM t") == "SELECT clause: Unknown column: nope");
  CHECK(refusal("SELECT price, " + w + " FROM t WHERE nope > 1") == "WHERE clause: Unknown column: nope");
  CHECK(refusal("SELECT price, " + w + " FROM t JOIN u ON a = b") == "JOIN is not supported by query_sql_windowed");
  CHECK(refusal("SELECT price, " + w + " FROM t GROUP BY b") ==
        "GROUP BY is not supported by query_sql_windowed (use query_sql_grouped)");
  CHECK(refusal("SELECT price, " + w + " FROM t HAVING a > 1") == "HAVING is not supported by query_sql_windowed");
  CHECK(refusal("SELECT DISTINCT price, " + w + " FROM t") == "DISTINCT is not supported by query_sql_windowed");
  CHECK(refusal("SELECT price, " + w + " FROM t ORDER BY price") ==
        "ORDER BY is not supported by query_sql_windowed (the result is in row order)");
  CHECK(refusal("SELECT price, quantity FROM t") ==
        "query_sql_windowed needs a window item, AGG(x) OVER (PARTITION BY k) (use query_sql_table)");
  CHECK(refusal("SELECT SUM(a), " + w + " FROM t") ==
        "a plain aggregate beside window items is not supported by query_sql_windowed");
  CHECK(refusal("SELECT price, SUM(a) OVER (PARTITION BY b ORDER BY c) FROM t") ==
        "ORDER BY inside OVER is not supported (PARTITION BY only: no running or framed aggregates)");
  CHECK(refusal("SELECT price, SUM(a) OVER (PARTITION BY b, c) FROM t") == "PARTITION BY supports one key expression");
  CHECK(refusal("SELECT " + w + ", SUM(a) OVER (PARTITION BY c) FROM t") ==
        "window items partition by two different expressions (b[idx] and c[idx]): one is supported");
  CHECK(refusal("SELECT " + w + ", SUM(a) OVER () FROM t") ==
        "window items partition by two different expressions (b[idx] and 0): one is supported");
  std::string many = "SELECT a, b";
  for (int i = 0; i < 15; ++i) many += ", " + w;
  CHECK(refusal(many + " FROM t") == "a select list takes at most 16 expressions");
  CHECK(refusal("SELECT SUM(a) OVER (), SUM(b) OVER (), SUM(c) OVER (), SUM(d) OVER (), MAX(e) OVER () FROM t") ==
        "window items aggregate 5 different expressions: at most 4 are supported");

  // order: unknown column, JOIN, GROUP BY, HAVING, DISTINCT, ORDER BY, no window item, plain aggregate,
  // ORDER BY inside OVER, PARTITION BY keys, two partitions, item count, distinct values
  CHECK(refusal("SELECT DISTINCT nope FROM t JOIN u ON a = b GROUP BY b") == "SELECT clause: Unknown column: nope");
  CHECK(refusal("SELECT DISTINCT price FROM t JOIN u ON a = b GROUP BY b") == "JOIN is not supported by query_sql_windowed");
  CHECK(refusal("SELECT DISTINCT price FROM t GROUP BY b HAVING a > 1 ORDER BY a") ==
        "GROUP BY is not supported by query_sql_windowed (use query_sql_grouped)");
  CHECK(refusal("SELECT DISTINCT price FROM t HAVING a > 1 ORDER BY a") == "HAVING is not supported by query_sql_windowed");
  CHECK(refusal("SELECT DISTINCT price FROM t ORDER BY a") == "DISTINCT is not supported by query_sql_windowed");
  CHECK(refusal("SELECT SUM(a) FROM t ORDER BY a") ==
        "ORDER BY is not supported by query_sql_windowed (the result is in row order)");
  CHECK(has(refusal("SELECT SUM(a) FROM t"), "needs a window item"));
  CHECK(has(refusal("SELECT SUM(a), SUM(a) OVER (PARTITION BY b, c ORDER BY d) FROM t"), "a plain aggregate beside"));
  CHECK(has(refusal("SELECT SUM(a) OVER (PARTITION BY b, c ORDER BY d), SUM(a) OVER () FROM t"), "ORDER BY inside OVER"));
  CHECK(refusal("SELECT SUM(a) OVER (PARTITION BY b, c), SUM(a) OVER () FROM t") == "PARTITION BY supports one key expression");
  std::string both = "SELECT SUM(a) OVER (PARTITION BY c), SUM(b) OVER (), SUM(c) OVER (), SUM(d) OVER (), MAX(e) OVER ()";
  for (int i = 0; i < 12; ++i) both += ", " + w;
  CHECK(has(refusal(both + " FROM t"), "partition by two different expressions"));
  std::string wide = "SELECT SUM(a) OVER (), SUM(b) OVER (), SUM(c) OVER (), SUM(d) OVER (), MAX(e) OVER ()";
  for (int i = 0; i < 12; ++i) wide += ", SUM(a) OVER ()";
  CHECK(refusal(wide + " FROM t") == "a select list takes at most 16 expressions");

  // the other entry points refuse window items with the messages they had
  auto table_refusal = [](const std::string &sql) { return error_of([&] { warpdb::plan_sql_table(sql, kCols); }); };
  CHECK(table_refusal("SELECT price, " + w + " FROM t") == "window functions are not supported by the execution engine");
  CHECK(table_refusal("SELECT price, SUM(a) OVER () FROM t") == "window functions are not supported by the execution engine");
  CHECK(error_of([&] { warpdb::plan_sql_grouped("SELECT b, " + w + " FROM t GROUP BY b", kCols); }) ==
        "window functions are not supported by the execution engine");
  CHECK(error_of([&] { warpdb::plan_sql_ordered("SELECT price, " + w + " FROM t ORDER BY price", kCols); }) ==
        "window functions are not supported by query_sql_ordered");
}

// Every row of tests/golden/facade_errors.tsv that names a window function:
// query_sql_table, query_sql_ordered and query_multi_gpu_group answer it with
// the message the table holds.
static void golden_rows() {
  std::ifstream f("tests/golden/facade_errors.tsv");
  CHECK(f.is_open());
  static const NameSet cols{"price", "quantity"};
  std::string line;
  int rows = 0;
  while (std::getline(f, line)) {
    const size_t a = line.find('\t'), b = line.find('\t', a + 1);
    if (a == std::string::npos || b == std::string::npos) continue;
    const std::string entry = line.substr(0, a), text = line.substr(a + 1, b - a - 1), message = line.substr(b + 1);
    if (!has(text, " OVER ")) continue;
    const std::string got = error_of([&] {
      if (entry == "query_sql_table") warpdb::plan_sql_table(text, cols);
      else if (entry == "query_sql_ordered") warpdb::plan_sql_ordered(text, cols);
      else if (entry == "query_multi_gpu_group") warpdb::plan_multi_gpu_group(text, cols);
      else throw std::runtime_error("no planner call for " + entry);
    });
    if (got != message) {
      std::printf("FAILED %s(\"%s\"): \"%s\", expected \"%s\"\n", entry.c_str(), text.c_str(), got.c_str(),
                  message.c_str());
      ++failures;
    }
    ++rows;
  }
  CHECK(rows >= 7);
}

int main() {
  golden_rows();
  parser();
  accepted();
  refusals();
  if (failures) {
    std::printf("window_plan_test: %d check(s) failed\n", failures);
    return 1;
  }
  std::printf("window_plan_test: all passed\n");
  return 0;
}
