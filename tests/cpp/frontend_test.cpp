// frontend_test.cpp -- C++ API checks of the front end through the public
// headers (include/warpdb), covering the expectations of the reference's
// test_expression / precedence / expression / tokenizer / parsing-error /
// parse_query / identifier-validation tests, and the facade's planner
// (csrc/warpdb/plan.hpp): its refusals against tests/golden/facade_errors.tsv
// (the table tests/test_warpdb_api.py reads against the whole facade), its
// plans, and HAVING / ORDER BY over hand-made groups.  No GPU needed; run
// from the repository root.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <stdexcept>
#include <string>
#include <unordered_set>

#include "warpdb/expression.hpp"
#include "../../warpdb_amd/csrc/warpdb/plan.hpp"

static int failures = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      ++failures;                                                  \
    }                                                              \
  } while (0)

static std::string lower(const std::string &s) { return parse_expression(tokenize(s))->to_cuda_expr(); }

template <typename F>
static std::string error_of(F &&f) {
  try {
    f();
  } catch (const std::runtime_error &e) {
    return e.what();
  }
  return "<no error>";
}

using warpdb::NameSet;
using warpdb::Window;
static const NameSet kCols{"price", "quantity"};

// The message of the planner call behind a facade entry point, on the
// columns of tests/golden/test.csv (4 rows).
static std::string refusal(const std::string &entry, const std::string &text) {
  return error_of([&] {
    if (entry == "query" || entry == "query_multi_gpu") warpdb::lower_query(text, kCols);
    else if (entry == "query_sql") warpdb::plan_sql(text, kCols);
    else if (entry == "query_sql_table") warpdb::plan_sql_table(text, kCols);
    else if (entry == "query_sql_ordered") warpdb::plan_sql_ordered(text, kCols);
    else if (entry == "query_multi_gpu_group") warpdb::plan_multi_gpu_group(text, kCols);
    else if (entry == "query_multi_gpu_topk") warpdb::plan_multi_gpu_topk(text, kCols, 4);
    else throw std::runtime_error("no planner call for " + entry);
  });
}

static void refusals_table() {
  std::ifstream f("tests/golden/facade_errors.tsv");
  CHECK(f.is_open());
  std::string line;
  int rows = 0;
  while (std::getline(f, line)) {
    const size_t a = line.find('\t'), b = line.find('\t', a + 1);
    CHECK(a != std::string::npos && b != std::string::npos);
    if (a == std::string::npos || b == std::string::npos) continue;
    const std::string entry = line.substr(0, a), text = line.substr(a + 1, b - a - 1), message = line.substr(b + 1);
    const std::string got = refusal(entry, text);
    if (got != message) {
      std::printf("FAILED %s(\"%s\"): \"%s\", expected \"%s\"\n", entry.c_str(), text.c_str(), got.c_str(),
                  message.c_str());
      ++failures;
    }
    ++rows;
  }
  CHECK(rows > 100);
}

static void planner_results() {
  using V = std::vector<std::string>;
  // a list of plain expressions, as query_select / query_select_ordered / query_rows lower it
  const warpdb::SelectList list =
      warpdb::lower_select_list({"price", "price * quantity", "discount(price, 0.9)"}, kCols, "query_rows");
  CHECK(list.lowered == (V{"price[idx]", "(price[idx] * quantity[idx])", "discount(price[idx], 0.9f)"}));
  CHECK(list.names == (V{"price", "expr1", "expr2"}));
  CHECK(error_of([] { warpdb::lower_select_list(V(17, "price"), kCols, "query_rows"); }) ==
        "query_rows takes at most 16 expressions");
  CHECK(error_of([] { warpdb::lower_select_list({"price", " "}, kCols, "query_rows"); }) == "Empty query expression");
  const warpdb::Lowered q = warpdb::lower_query("price * quantity WHERE price > 15", kCols);
  CHECK(q.expr == "(price[idx] * quantity[idx])" && q.cond == "(price[idx] > 15.0f)");
  CHECK(warpdb::lower_query("price", kCols).cond.empty() && warpdb::lower_where(" \t", kCols).empty());
  CHECK(warpdb::lower_order_by("price / 2", kCols) == "(price[idx] / 2.0f)");
  CHECK(error_of([] { warpdb::lower_order_by(" ", kCols); }) == "Empty ORDER BY expression");
  CHECK(error_of([] { warpdb::lower_order_by("nope", kCols); }) ==
        "Failed to parse ORDER BY expression: Unknown column: nope");

  // the grouped route of query_sql_table
  const warpdb::TablePlan g =
      warpdb::plan_sql_table("SELECT quantity, SUM(price), COUNT(*), MAX(price) FROM t GROUP BY quantity", kCols);
  CHECK(g.route == warpdb::TablePlan::Route::Grouped && g.value && g.value->to_cuda_expr() == "price[idx]" && g.minmax);
  CHECK(g.names == (V{"quantity", "sum_1", "count_2", "max_3"}) && g.sql.cond.empty());
  CHECK(g.items.size() == 4 && !g.items[0] && g.items[1] == AggregationType::Sum &&
        g.items[2] == AggregationType::Count && g.items[3] == AggregationType::Max);
  // COUNT alone aggregates what it names; MIN / MAX in HAVING selects the MIN / MAX build
  const warpdb::TablePlan c = warpdb::plan_sql_table(
      "SELECT quantity, COUNT(price) FROM t WHERE price > 1 GROUP BY quantity HAVING MIN(price) > 2", kCols);
  CHECK(c.value->to_cuda_expr() == "price[idx]" && c.minmax && c.sql.cond == "(price[idx] > 1.0f)");
  CHECK(!warpdb::plan_sql_table("SELECT quantity, AVG(price) FROM t GROUP BY quantity", kCols).minmax);
  CHECK(warpdb::plan_sql_table("SELECT MAX(price) FROM t", kCols).route == warpdb::TablePlan::Route::Single);
  CHECK(warpdb::plan_sql_table("SELECT DISTINCT price FROM t", kCols).route == warpdb::TablePlan::Route::Single);
  const warpdb::TablePlan r = warpdb::plan_sql_table("SELECT price, price * 2 FROM t LIMIT 3 OFFSET 1", kCols);
  CHECK(r.route == warpdb::TablePlan::Route::Rows && r.lowered == (V{"price[idx]", "(price[idx] * 2.0f)"}) &&
        r.sql.window.offset == 1 && r.sql.window.limit == 3 && r.sql.window.rows_needed(4) == 4 &&
        r.sql.window.rows_needed(100) == 4);

  const warpdb::OrderedPlan o =
      warpdb::plan_sql_ordered("SELECT price, quantity * 2 FROM t WHERE price > 1 ORDER BY quantity DESC LIMIT 2", kCols);
  CHECK(o.names == (V{"price", "expr1"}) && o.lowered == (V{"price[idx]", "(quantity[idx] * 2.0f)"}) &&
        o.cond == "(price[idx] > 1.0f)" && o.order == "quantity[idx]" && o.descending && o.window.offset == 0 &&
        o.window.limit == 2);
  const warpdb::GroupPlan mg =
      warpdb::plan_multi_gpu_group("SELECT AVG(price * 2) FROM t WHERE price > 1 GROUP BY quantity", kCols);
  CHECK(mg.value == "(price[idx] * 2.0f)" && mg.key == "quantity[idx]" && mg.cond == "(price[idx] > 1.0f)");

  // the multi-GPU top-K clamp: offset + limit never beyond the table's rows
  auto topk = [](const char *tail, int64_t n) {
    return warpdb::plan_multi_gpu_topk(std::string("SELECT price * 2 FROM t ORDER BY quantity DESC ") + tail, kCols, n);
  };
  const warpdb::TopkPlan t = topk("LIMIT 10 OFFSET 3", 4);
  CHECK(t.limit == 1 && t.offset == 3 && t.descending && t.order == "quantity[idx]" &&
        t.select == "(price[idx] * 2.0f)" && t.cond.empty());
  CHECK(topk("LIMIT 10 OFFSET 4", 4).limit == 0 && topk("LIMIT 0", 4).limit == 0 && topk("LIMIT 3", 4).limit == 3);
  CHECK(topk("LIMIT 2147483647 OFFSET 2147483647", 4).limit == 0);
  const warpdb::TopkPlan big = topk("LIMIT 2147483647 OFFSET 2147483647", 3000000000);
  CHECK(big.offset == 2147483647 && big.limit == 3000000000 - 2147483647 && big.offset + big.limit == 3000000000);
  CHECK(topk("LIMIT 2147483647 OFFSET 2147483647", INT64_MAX).limit == 2147483647);

  // OFFSET / LIMIT windows, on the result lengths 0, 1 and 5
  using F = std::vector<float>;
  const F five{1, 2, 3, 4, 5};
  const Window all, none(0, 0), past(7, 2), mid(1, 2), tail(3, -1), wide(2, 100);
  CHECK(all.sliced(F{}) == F{} && all.sliced(F{9}) == F{9} && all.sliced(five) == five);
  CHECK(none.sliced(F{}) == F{} && none.sliced(F{9}) == F{} && none.sliced(five) == F{});
  CHECK(past.sliced(F{}) == F{} && past.sliced(F{9}) == F{} && past.sliced(five) == F{});
  CHECK(mid.sliced(F{}) == F{} && mid.sliced(F{9}) == F{} && mid.sliced(five) == (F{2, 3}));
  CHECK(tail.sliced(five) == (F{4, 5}) && wide.sliced(five) == (F{3, 4, 5}));
  CHECK(Window(5, -1).sliced(five) == F{} && Window(4, 1).sliced(five) == F{5});
  CHECK(mid.sliced(std::vector<int64_t>{7, 8, 9, 10}) == (std::vector<int64_t>{8, 9}));
  CHECK(!all.limited() && all.end() == -1 && all.rows_needed(5) == 5 && all.rows_needed(0) == 0);
  CHECK(none.limited() && none.end() == 0 && none.rows_needed(5) == 0);
  CHECK(mid.end() == 3 && mid.rows_needed(5) == 3 && mid.rows_needed(2) == 2 && past.rows_needed(5) == 5);
  const Window neg(-3, -7), huge(INT64_MAX, INT64_MAX);
  CHECK(neg.offset == 0 && !neg.limited() && huge.end() == INT64_MAX && huge.rows_needed(5) == 5);
  CHECK(huge.sliced(five) == F{});
  const Window parsed(parse_query(tokenize("SELECT price FROM t ORDER BY price DESC OFFSET 1 LIMIT 2")));
  CHECK(parsed.offset == 1 && parsed.limit == 2 && parsed.sliced(F{30, 20, 15.25f, 10.5f}) == (F{20, 15.25f}));
  const Window open_end(parse_query(tokenize("SELECT price FROM t OFFSET 2")));
  CHECK(open_end.offset == 2 && !open_end.limited());
}

// The groups of tests/golden/test.csv (price [10.5, 20, 15.25, 30], quantity
// [3, 4, 2, 5]) as wx_group_agg returns them for GROUP BY quantity.
static warpdb::GroupRun test_csv_groups(bool price_times_quantity) {
  warpdb::GroupRun run;
  run.keys = {2, 3, 4, 5};
  run.cnts = {1, 1, 1, 1};
  if (price_times_quantity) run.sums = {30.5, 31.5, 80.0, 150.0};
  else run.sums = {15.25, 10.5, 20.0, 30.0};
  for (double s : run.sums) run.mins.push_back(static_cast<float>(s));
  run.maxs = run.mins;
  return run;
}

// finish() of query_sql's grouped `sql` over `run`: the kept groups in result order
static std::vector<size_t> finished(warpdb::GroupRun run, const std::string &sql) {
  const warpdb::SqlPlan p = warpdb::plan_sql(sql, kCols);
  run.finish(p.ast, p.agg->expr.get(), p.ast.group_by->keys[0].get());
  return run.order;
}

static void having_and_group_order() {
  using O = std::vector<size_t>;
  const warpdb::GroupRun price = test_csv_groups(false), none;
  // the clauses of test_query_sql_reference_expectations and test_query_sql_min_max
  CHECK(finished(price, "SELECT SUM(price) FROM test GROUP BY quantity ORDER BY quantity ASC") == (O{0, 1, 2, 3}));
  CHECK(finished(price, "SELECT SUM(price) FROM test GROUP BY quantity HAVING SUM(price) > 15 ORDER BY quantity ASC") ==
        (O{0, 2, 3}));
  CHECK(finished(price, "SELECT SUM(price) FROM test GROUP BY quantity HAVING COUNT(price) > 1").empty());
  CHECK(finished(price, "SELECT AVG(price) FROM test GROUP BY quantity ORDER BY quantity DESC LIMIT 1") ==
        (O{3, 2, 1, 0}));
  CHECK(finished(price, "SELECT MAX(price) FROM test GROUP BY quantity ORDER BY quantity ASC") == (O{0, 1, 2, 3}));
  CHECK(finished(price, "SELECT SUM(price) FROM test GROUP BY quantity HAVING MIN(price) > 12 ORDER BY quantity ASC") ==
        (O{0, 2, 3}));
  CHECK(finished(test_csv_groups(true), "SELECT MIN(price * quantity) FROM test GROUP BY quantity "
                                        "ORDER BY MIN(price * quantity) DESC LIMIT 2") == (O{3, 2, 1, 0}));
  CHECK(finished(price, "SELECT SUM(price) FROM test GROUP BY quantity ORDER BY SUM(price)") == (O{1, 0, 2, 3}));
  CHECK(price.value_of(AggregationType::Avg, 2) == 20.0 && price.value_of(AggregationType::Count, 2) == 1.0 &&
        price.value_of(AggregationType::Max, 3) == 30.0);
  // HAVING is evaluated per group, so its refusals need a group to show
  const char *other = "SELECT SUM(price) FROM test GROUP BY quantity HAVING SUM(quantity) > 1";
  CHECK(error_of([&] { finished(price, other); }) == "HAVING may only aggregate the selected expression");
  CHECK(error_of([&] { finished(none, other); }) == "<no error>" && finished(none, other).empty());
  CHECK(error_of([&] { finished(price, "SELECT SUM(price) FROM test GROUP BY quantity HAVING discount(price, 1) > 1"); }) ==
        "unsupported HAVING term");
  const char *stray = "SELECT SUM(price) FROM test GROUP BY quantity ORDER BY price";
  CHECK(error_of([&] { finished(price, stray); }) == "ORDER BY with GROUP BY must name the key or an aggregate");
  CHECK(error_of([&] { finished(none, stray); }) == "ORDER BY with GROUP BY must name the key or an aggregate");
}

int main() {
  CHECK(lower("price > 10") == "(price[idx] > 10.0f)");
  CHECK(lower("quantity <= 5") == "(quantity[idx] <= 5.0f)");
  CHECK(lower("discount(price, 0.9)") == "discount(price[idx], 0.9f)");
  CHECK(lower("price > 10 AND quantity < 5") == "((price[idx] > 10.0f) && (quantity[idx] < 5.0f))");
  CHECK(lower("price > 10 OR quantity < 5") == "((price[idx] > 10.0f) || (quantity[idx] < 5.0f))");
  CHECK(lower("price + quantity * 2") == "(price[idx] + (quantity[idx] * 2.0f))");
  CHECK(lower("(price + quantity) * 2") == "((price[idx] + quantity[idx]) * 2.0f)");
  CHECK(parse_logical_and(tokenize("a > 1 AND b < 2"))->to_cuda_expr() == "((a[idx] > 1.0f) && (b[idx] < 2.0f))");

  auto toks = tokenize("price > 10");
  CHECK(toks.size() == 4 && toks[0].type == TokenType::Identifier && toks[1].value == ">" &&
        toks[2].type == TokenType::Number && toks[3].type == TokenType::End);

  CHECK(error_of([] { lower("1 2"); }).find("Unexpected token") != std::string::npos);
  CHECK(error_of([] { lower("(price + 5"); }).find("Expected ')'") != std::string::npos);
  CHECK(error_of([] { tokenize("price & 5"); }).find("Unknown character") != std::string::npos);
  const std::string e = error_of([] { tokenize("price # 1\n"); });
  CHECK(e.find("line 1") != std::string::npos && e.find("column") != std::string::npos);
  const std::string q = error_of([] { parse_query(tokenize("SELECT price")); });
  CHECK(q.find("line") != std::string::npos && q.find("column") != std::string::npos);
  CHECK(error_of([] { parse_query(tokenize("SELECT price FROM test EXTRA")); }).find("Unexpected token") !=
        std::string::npos);

  QueryAST ast = parse_query(tokenize("SELECT SUM(price), quantity FROM sales JOIN items ON sales.id = items.id "
                                      "WHERE price > 10 GROUP BY quantity ORDER BY price DESC LIMIT 5"));
  CHECK(ast.select_list.size() == 2 && !ast.joins.empty() && ast.where.has_value() && ast.group_by.has_value() &&
        ast.order_by.has_value() && ast.limit.has_value());
  CHECK(dynamic_cast<AggregationNode *>(ast.select_list[0].get())->agg_kernel() == "sum");

  QueryAST bad = parse_query(tokenize("SELECT foo FROM test"));
  const std::unordered_set<std::string> cols{"price", "quantity"};
  CHECK(error_of([&] { warpdb::validate_ast(bad.select_list[0].get(), cols); }).find("Unknown column") !=
        std::string::npos);

  std::string ex, cond;
  warpdb::split_where("price * quantity where price > 10", ex, cond);
  CHECK(ex == "price * quantity " && cond == " price > 10");

  refusals_table();
  planner_results();
  having_and_group_order();

  if (failures) return 1;
  std::printf("frontend_test: all passed\n");
  return 0;
}
