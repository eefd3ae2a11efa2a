// group_multi_plan_test.cpp -- the planner of WarpDB::query_sql_grouped
// (plan_sql_grouped) without a device: slot deduplication, hidden slots from
// HAVING / ORDER BY, chunking, names, every refusal and its precedence, and
// the host-side HAVING / ORDER BY over made-up groups (GroupedRun::finish).
// Build: make -C tests/cpp bin/group_multi_plan_test; run from the repository root.
#include <cmath>
#include <cstdio>
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

using warpdb::GroupedPlan;
using warpdb::GroupedRun;
using warpdb::NameSet;
static const NameSet kCols{"price", "quantity", "a", "b", "c"};

static GroupedPlan plan(const std::string &sql) { return warpdb::plan_sql_grouped(sql, kCols); }

static std::string refusal(const std::string &sql) {
  try {
    plan(sql);
  } catch (const std::runtime_error &e) {
    return e.what();
  }
  return "<no error>";
}
static std::string table_refusal(const std::string &sql) {
  try {
    warpdb::plan_sql_table(sql, kCols);
  } catch (const std::runtime_error &e) {
    return e.what();
  }
  return "<no error>";
}
static bool has(const std::string &s, const std::string &part) { return s.find(part) != std::string::npos; }

static void slots() {
  // one expression under three aggregates: one slot that carries both
  GroupedPlan p = plan("SELECT quantity, SUM(price), AVG(price), MAX(price) FROM t GROUP BY quantity");
  CHECK(p.slots.size() == 1 && p.selected_slots == 1);
  CHECK(p.slots[0].lowered == "price[idx]" && p.slots[0].sum && p.slots[0].minmax);
  CHECK(p.items.size() == 4 && !p.items[0].agg && p.items[0].slot == -1);
  CHECK(p.items[1].slot == 0 && p.items[2].slot == 0 && p.items[3].slot == 0);
  CHECK(*p.items[1].agg == AggregationType::Sum && *p.items[3].agg == AggregationType::Max);
  CHECK((p.names == std::vector<std::string>{"quantity", "sum_1", "avg_2", "max_3"}));
  CHECK(p.cond.empty() && p.key->to_cuda_expr() == "quantity[idx]");

  // the issue's query: two expressions, each with what it needs only
  p = plan("SELECT quantity, SUM(price), MAX(price * quantity) FROM t WHERE price > 1 GROUP BY quantity");
  CHECK(p.slots.size() == 2 && p.slots[0].sum && !p.slots[0].minmax && !p.slots[1].sum && p.slots[1].minmax);
  CHECK(p.slots[1].lowered == "(price[idx] * quantity[idx])" && !p.cond.empty());
  CHECK(p.items[2].slot == 1);

  // COUNT rides on any slot; alone it gets one summed slot of what it counts
  p = plan("SELECT COUNT(a), MIN(b), quantity FROM t GROUP BY quantity");
  CHECK(p.slots.size() == 1 && p.slots[0].lowered == "b[idx]" && !p.slots[0].sum && p.slots[0].minmax);
  CHECK(p.items[0].slot == -1 && *p.items[0].agg == AggregationType::Count && p.items[1].slot == 0);
  p = plan("SELECT quantity, COUNT(a) FROM t GROUP BY quantity");
  CHECK(p.slots.size() == 1 && p.slots[0].lowered == "a[idx]" && p.slots[0].sum && !p.slots[0].minmax);
  p = plan("SELECT quantity FROM t GROUP BY quantity");
  CHECK(p.slots.size() == 1 && p.slots[0].lowered == "quantity[idx]" && p.slots[0].sum);

  // hidden slots: aggregates only HAVING / ORDER BY name, after the selected ones
  p = plan("SELECT quantity, SUM(a) FROM t GROUP BY quantity HAVING MAX(b) > 2 AND SUM(a) > 1 ORDER BY AVG(c) DESC");
  CHECK(p.slots.size() == 3 && p.selected_slots == 1);
  CHECK(p.slots[1].lowered == "b[idx]" && p.slots[1].minmax && !p.slots[1].sum);
  CHECK(p.slots[2].lowered == "c[idx]" && p.slots[2].sum && !p.slots[2].minmax);
  CHECK(p.slots[0].sum && !p.slots[0].minmax);
  // a hidden aggregate of a selected expression widens that slot instead
  p = plan("SELECT quantity, SUM(a) FROM t GROUP BY quantity ORDER BY MIN(a)");
  CHECK(p.slots.size() == 1 && p.slots[0].sum && p.slots[0].minmax);
  p = plan("SELECT quantity, SUM(a) FROM t GROUP BY quantity ORDER BY quantity DESC LIMIT 3 OFFSET 1");
  CHECK(p.slots.size() == 1 && p.window.offset == 1 && p.window.limit == 3);

  // five distinct expressions: chunks of four and one
  p = plan("SELECT quantity, SUM(a), SUM(b), SUM(c), SUM(price), MAX(a + b), AVG(a) FROM t GROUP BY quantity");
  CHECK(p.slots.size() == 5);
  auto ch = p.chunks(4);
  CHECK(ch.size() == 2 && ch[0].first == 0 && ch[0].second == 4 && ch[1].first == 4 && ch[1].second == 1);
  CHECK(p.chunks(1).size() == 5);
  CHECK(p.items[6].slot == 0 && p.items[5].slot == 4);
}

static void refusals() {
  const std::string g = " FROM t GROUP BY quantity";
  CHECK(has(refusal("SELECT FROM"), "Failed to parse SQL"));
  CHECK(refusal("SELECT quantity, SUM(nope)" + g) == "SELECT clause: Unknown column: nope");
  CHECK(refusal("SELECT quantity, SUM(a) FROM t WHERE nope > 1 GROUP BY quantity") ==
        "WHERE clause: Unknown column: nope");
  CHECK(refusal("SELECT quantity, SUM(a) FROM t GROUP BY nope") == "GROUP BY: Unknown column: nope");
  CHECK(refusal("SELECT quantity, SUM(a)" + g + " ORDER BY SUM(nope)") == "ORDER BY: Unknown column: nope");
  CHECK(refusal("SELECT quantity, SUM(a)" + g + " HAVING SUM(nope) > 1") == "HAVING clause: Unknown column: nope");
  CHECK(refusal("SELECT quantity, SUM(a) FROM t JOIN u ON a = b GROUP BY quantity") ==
        "JOIN is not supported by the execution engine");
  CHECK(refusal("SELECT quantity, SUM(a) OVER (PARTITION BY b)" + g) ==
        "window functions are not supported by the execution engine");
  CHECK(refusal("SELECT quantity, SUM(a) FROM t") == "query_sql_grouped needs a GROUP BY clause");
  CHECK(refusal("SELECT quantity, SUM(a) FROM t GROUP BY quantity, b") == "GROUP BY supports one key expression");
  CHECK(refusal("SELECT DISTINCT quantity, SUM(a)" + g) == "DISTINCT over a multi-column result is not supported");
  CHECK(refusal("SELECT price, SUM(a)" + g) ==
        "select item 0 must be the GROUP BY key or an aggregate (SUM / AVG / COUNT / MIN / MAX)");
  CHECK(refusal("SELECT quantity, SUM(a)" + g + " ORDER BY price") ==
        "ORDER BY with GROUP BY must name the key or an aggregate");
  std::string many = "SELECT quantity";
  for (int i = 0; i < 16; ++i) many += ", SUM(a + " + std::to_string(i) + ")";
  CHECK(refusal(many + g) == "a select list takes at most 16 expressions");
  // precedence, as in plan_sql_table: unknown column, JOIN, window function, GROUP BY, keys, DISTINCT, count, items
  CHECK(refusal("SELECT quantity, SUM(nope) FROM t JOIN u ON a = b") == "SELECT clause: Unknown column: nope");
  CHECK(refusal("SELECT quantity, SUM(a) OVER (PARTITION BY b) FROM t JOIN u ON a = b") ==
        "JOIN is not supported by the execution engine");
  CHECK(refusal("SELECT price, SUM(a) OVER (PARTITION BY b) FROM t") ==
        "window functions are not supported by the execution engine");
  CHECK(refusal("SELECT price, SUM(a) FROM t") == "query_sql_grouped needs a GROUP BY clause");
  CHECK(refusal("SELECT DISTINCT price, SUM(a) FROM t GROUP BY quantity, b") == "GROUP BY supports one key expression");
  CHECK(refusal("SELECT DISTINCT price, SUM(a)" + g) == "DISTINCT over a multi-column result is not supported");
  CHECK(refusal("SELECT price" + many.substr(15) + g) == "a select list takes at most 16 expressions");
  // the single-value entry point refuses what it refused, with the old text
  CHECK(table_refusal("SELECT quantity, SUM(price), MAX(price * quantity) FROM t GROUP BY quantity") ==
        "GROUP BY select list aggregates two different expressions (price[idx] and (price[idx] * quantity[idx])): "
        "one is supported");
  CHECK(refusal("SELECT quantity, SUM(price), MAX(price * quantity) FROM t GROUP BY quantity") == "<no error>");
}

// HAVING / ORDER BY over aggregates of any slot, on three made-up groups
static void finish() {
  GroupedPlan p =
      plan("SELECT quantity, SUM(a), MAX(b) FROM t GROUP BY quantity HAVING AVG(c) > 1 AND COUNT(a) >= 2 "
           "ORDER BY MIN(b) DESC");
  CHECK(p.slots.size() == 3);
  GroupedRun r;
  r.run.keys = {1, 2, 3, 4};
  r.run.cnts = {2, 2, 1, 4};
  r.slots.resize(3);
  r.slots[0].sums = {10, 20, 30, 40};
  r.slots[1].mins = {5, 7, 9, 6};
  r.slots[1].maxs = {50, 70, 90, 60};
  r.slots[2].sums = {4, 1, 100, 8};  // averages 2, 0.5, 100, 2
  r.finish(p);
  CHECK((r.run.order == std::vector<size_t>{3, 0}));  // groups 4 and 1, by MIN(b) descending
  CHECK(r.value_of(p, AggregationType::Sum, 0, 3) == 40 && r.value_of(p, AggregationType::Max, 1, 0) == 50);
  CHECK(r.value_of(p, AggregationType::Avg, 2, 0) == 2 && r.value_of(p, AggregationType::Count, -1, 3) == 4);
  // the single-slot GroupRun is what it was: HAVING over another expression is refused per group
  warpdb::SqlPlan sp = warpdb::plan_sql("SELECT SUM(a) FROM t GROUP BY quantity HAVING SUM(b) > 1", kCols);
  warpdb::GroupRun g;
  g.keys = {1};
  g.sums = {3};
  g.cnts = {1};
  std::string msg = "<no error>";
  try {
    g.finish(sp.ast, sp.agg->expr.get(), sp.ast.group_by->keys[0].get());
  } catch (const std::runtime_error &e) {
    msg = e.what();
  }
  CHECK(msg == "HAVING may only aggregate the selected expression");
}

int main() {
  slots();
  refusals();
  finish();
  if (failures) {
    std::printf("group_multi_plan_test: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("group_multi_plan_test: all passed\n");
  return 0;
}
