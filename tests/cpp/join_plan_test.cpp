// join_plan_test.cpp -- the front end and the planner of
// WarpDB::query_sql_joined / query_join (plan_sql_joined, plan_join) without
// a device: what the parser stores of a JOIN clause, how names resolve through
// the table qualifiers, both spellings and both orders of the ON condition,
// the prefix of the right table's columns, every refusal with its message
// and their order, LIMIT / OFFSET.
// Build: make -C tests/cpp bin/join_plan_test; run from the repository root.
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

using warpdb::JoinedPlan;
using warpdb::NameSet;
static const NameSet kLeft{"price", "quantity", "cust", "id"};
static const NameSet kRight{"id", "rate", "tier"};

static JoinedPlan plan(const std::string &sql) { return warpdb::plan_sql_joined(sql, kLeft, "u", kRight); }

template <typename F>
static std::string error_of(F &&f) {
  try {
    f();
  } catch (const std::runtime_error &e) {
    return e.what();
  }
  return "<no error>";
}
static std::string refusal(const std::string &sql) {
  return error_of([&] { plan(sql); });
}
static bool has(const std::string &s, const std::string &part) { return s.find(part) != std::string::npos; }

static void parser() {
  // the AST keeps its size (expression.hpp says why); the kind of a JOIN is read off the tokens
  auto left_outer = [](const std::string &sql, size_t i) { return warpdb::join_is_left_outer(tokenize(sql), i); };
  std::string sql = "SELECT price FROM t JOIN u ON cust = u.id WHERE price > 1";
  QueryAST q = parse_query(tokenize(sql));
  CHECK(q.joins.size() == 1 && q.joins[0].table == "u" && !left_outer(sql, 0) && q.where);
  CHECK(q.joins[0].condition->to_cuda_expr() == "(cust[idx] == u.id[idx])");
  sql = "SELECT price FROM t INNER JOIN u ON cust = u.id";
  q = parse_query(tokenize(sql));
  CHECK(q.joins.size() == 1 && !left_outer(sql, 0) && q.from_table == "t");
  sql = "SELECT price FROM t LEFT JOIN u ON cust = u.id LIMIT 3";
  q = parse_query(tokenize(sql));
  CHECK(q.joins.size() == 1 && left_outer(sql, 0) && q.limit && q.limit->count == 3);
  sql = "select price from t left outer join u on cust == u.id";
  q = parse_query(tokenize(sql));
  CHECK(q.joins.size() == 1 && left_outer(sql, 0) && q.joins[0].table == "u" && !left_outer(sql, 1));
  // the next JOIN's own words are not part of the condition before it
  sql = "SELECT price FROM t JOIN u ON cust = u.id LEFT OUTER JOIN v ON cust = v.k INNER JOIN w ON a = b";
  q = parse_query(tokenize(sql));
  CHECK(q.joins.size() == 3 && !left_outer(sql, 0) && left_outer(sql, 1) && !left_outer(sql, 2));
  CHECK(q.joins[0].condition->to_cuda_expr() == "(cust[idx] == u.id[idx])" && q.joins[2].table == "w");
  // the words stay ordinary identifiers anywhere else
  sql = "SELECT left + inner FROM outer WHERE left > 1";
  q = parse_query(tokenize(sql));
  CHECK(sizeof(JoinClause) == sizeof(std::string) + sizeof(ASTNodePtr));
  CHECK(!left_outer(sql, 0) && q.joins.empty() && q.from_table == "outer" && q.select_list[0]->to_cuda_expr() == "(left[idx] + inner[idx])");
}

static void accepted() {
  JoinedPlan p = plan("SELECT price, rate, price * rate FROM t JOIN u ON cust = u.id WHERE price > 15");
  CHECK(!p.left_outer && p.right_table == "u" && p.left_key == "cust[idx]" && p.right_key == "id");
  CHECK((p.names == std::vector<std::string>{"price", "rate", "expr2"}));
  CHECK((p.lowered == std::vector<std::string>{"price[idx]", "wxr_rate[idx]", "(price[idx] * wxr_rate[idx])"}));
  CHECK(p.cond == "(price[idx] > 15.0f)" && p.window.offset == 0 && !p.window.limited());
  // qualified names: `id` is in both tables
  p = plan("SELECT t.id, u.id, t.price, u.tier FROM t LEFT OUTER JOIN u ON t.cust == u.id WHERE u.rate > 1 LIMIT 5 OFFSET 2");
  CHECK(p.left_outer && p.left_key == "cust[idx]" && p.right_key == "id");
  CHECK((p.lowered == std::vector<std::string>{"id[idx]", "wxr_id[idx]", "price[idx]", "wxr_tier[idx]"}));
  CHECK((p.names == std::vector<std::string>{"id", "id", "price", "tier"}));
  CHECK(p.cond == "(wxr_rate[idx] > 1.0f)" && p.window.offset == 2 && p.window.limit == 5);
  // either way round, an expression as the left key, the FROM name as the qualifier
  p = plan("SELECT rate FROM fact INNER JOIN u ON u.id = fact.cust + 1");
  CHECK(p.left_key == "(cust[idx] + 1.0f)" && p.right_key == "id" && !p.left_outer);
  p = plan("SELECT rate FROM fact JOIN u ON tier == quantity * 2");
  CHECK(p.left_key == "(quantity[idx] * 2.0f)" && p.right_key == "tier");
  p = plan("SELECT rate FROM t JOIN u ON t.id = u.id");  // the same name on both sides
  CHECK(p.left_key == "id[idx]" && p.right_key == "id");
  p = plan("SELECT rate FROM t JOIN u ON u.id = t.id OFFSET 7");
  CHECK(p.left_key == "id[idx]" && p.right_key == "id" && p.window.offset == 7 && !p.window.limited());
  // query_join's plan from its parts
  p = warpdb::plan_join("", kLeft, "u", kRight, "cust + 1", "u.id", {"price", "u.id", "rate * 2"}, "tier > 1", true);
  CHECK(p.left_outer && p.left_key == "(cust[idx] + 1.0f)" && p.right_key == "id" && p.cond == "(wxr_tier[idx] > 1.0f)");
  CHECK((p.lowered == std::vector<std::string>{"price[idx]", "wxr_id[idx]", "(wxr_rate[idx] * 2.0f)"}));
  CHECK((p.names == std::vector<std::string>{"price", "id", "expr2"}));
}

static void refusals() {
  const std::string on = " FROM t JOIN u ON cust = u.id ";
  CHECK(refusal("SELECT id" + on) == "SELECT clause: Ambiguous column: id");
  CHECK(refusal("SELECT price" + on + "WHERE id > 1") == "WHERE clause: Ambiguous column: id");
  CHECK(refusal("SELECT nope" + on) == "SELECT clause: Unknown column: nope");
  CHECK(refusal("SELECT t.rate" + on) == "SELECT clause: Unknown column: t.rate");
  CHECK(refusal("SELECT u.price" + on) == "SELECT clause: Unknown column: u.price");
  CHECK(refusal("SELECT v.price" + on) == "SELECT clause: Unknown column: v.price");
  CHECK(refusal("SELECT price FROM t JOIN u ON cust = id") == "JOIN condition: Ambiguous column: id");
  CHECK(refusal("SELECT price FROM t JOIN u ON cust = u.nope") == "JOIN condition: Unknown column: u.nope");
  const std::string shape = "JOIN condition must be <left expression> = <right column>";
  for (const char *c : {"cust > u.id", "cust = u.id + 1", "cust = price", "rate = tier", "cust + rate = u.id", "cust",
                        "cust = u.id AND price > 1", "cust = 3", "u.id + 1 = cust"})
    CHECK(refusal(std::string("SELECT price FROM t JOIN u ON ") + c) == shape);
  // by name, in this order: a second JOIN, GROUP BY, HAVING, DISTINCT, ORDER BY, aggregates, window items
  const std::string all = "SELECT DISTINCT SUM(price), MAX(price) OVER (PARTITION BY cust) FROM t JOIN u ON cust = u.id "
                          "JOIN v ON cust = v.k GROUP BY cust HAVING SUM(price) > 1 ORDER BY cust";
  CHECK(has(refusal(all), "a second JOIN is not supported"));
  const std::string one = "SELECT DISTINCT SUM(price), MAX(price) OVER (PARTITION BY cust) FROM t JOIN u ON cust = u.id ";
  CHECK(has(refusal(one + "GROUP BY cust HAVING SUM(price) > 1 ORDER BY cust"), "GROUP BY is not supported"));
  CHECK(has(refusal(one + "HAVING SUM(price) > 1 ORDER BY cust"), "HAVING is not supported"));
  CHECK(has(refusal(one + "ORDER BY cust"), "DISTINCT is not supported"));
  const std::string two = "SELECT SUM(price), MAX(price) OVER (PARTITION BY cust) FROM t JOIN u ON cust = u.id ";
  CHECK(has(refusal(two + "ORDER BY cust"), "ORDER BY is not supported"));
  CHECK(has(refusal(two), "aggregates are not supported"));
  CHECK(has(refusal("SELECT price, MAX(price) OVER (PARTITION BY cust) FROM t JOIN u ON cust = u.id"),
            "window functions are not supported"));
  // an aggregate or a window item nested inside an item or the WHERE: its columns would go unresolved
  const std::string nested = "aggregates and window functions are not supported inside a joined expression";
  CHECK(refusal("SELECT price + SUM(rate) FROM t JOIN u ON cust = u.id") == "SELECT clause: " + nested);
  CHECK(refusal("SELECT discount(price, MAX(rate)) FROM t JOIN u ON cust = u.id") == "SELECT clause: " + nested);
  CHECK(refusal("SELECT price FROM t JOIN u ON cust = u.id WHERE SUM(rate) > 1") == "WHERE clause: " + nested);
  CHECK(has(refusal("SELECT price FROM t WHERE price > 1"), "needs a JOIN clause"));
  CHECK(refusal("SELECT price FROM t JOIN other ON cust = other.id") == "Unknown table: other (attach it first)");
  CHECK(has(refusal("SELECT price FROM t JOIN ON cust = u.id"), "Failed to parse SQL: Expected table name after JOIN"));
  CHECK(refusal("SELECT FROM t JOIN u ON cust = u.id") == "Empty SELECT list");
  std::string many = "SELECT price";
  for (int i = 0; i < 16; ++i) many += ", price + " + std::to_string(i);
  CHECK(has(refusal(many + on), "at most 16 expressions"));
  // query_join's parts
  auto parts = [](const std::string &lk, const std::string &rk, const std::vector<std::string> &ex,
                  const std::string &where = "") {
    return error_of([&] { warpdb::plan_join("", kLeft, "u", kRight, lk, rk, ex, where, false); });
  };
  CHECK(parts("cust", "id", {}) == "Empty SELECT list");
  CHECK(parts("cust", "id", {" "}) == "Empty query expression");
  CHECK(parts(" ", "id", {"price"}) == "Empty query expression");
  CHECK(parts("cust + rate", "id", {"price"}) == shape);
  CHECK(parts("cust", "nope", {"price"}) == "Unknown column: nope");
  CHECK(parts("cust", "id", {"id"}) == "Ambiguous column: id");
  CHECK(parts("cust", "id", {"price"}, "nope > 1") == "Failed to parse WHERE clause: Unknown column: nope");
  CHECK(has(parts("cust", "id", std::vector<std::string>(17, "price")), "at most 16 expressions"));
}

static void existing_refusals_keep_their_words() {
  const std::string sql = "SELECT price FROM t JOIN u ON cust = u.id";
  const NameSet cols{"price", "cust", "u.id"};
  CHECK(error_of([&] { warpdb::plan_sql(sql, cols); }) == "JOIN is not supported by the execution engine");
  CHECK(error_of([&] { warpdb::plan_sql_table(sql, cols); }) == "JOIN is not supported by the execution engine");
  CHECK(error_of([&] { warpdb::plan_sql_ordered(sql + " ORDER BY price", cols); }) ==
        "JOIN is not supported by query_sql_ordered");
  CHECK(error_of([&] { warpdb::plan_sql_windowed("SELECT SUM(price) OVER () FROM t LEFT JOIN u ON cust = u.id", cols); }) ==
        "JOIN is not supported by query_sql_windowed");
}

int main() {
  parser();
  accepted();
  refusals();
  existing_refusals_keep_their_words();
  if (failures) {
    std::printf("join_plan_test: %d check(s) failed\n", failures);
    return 1;
  }
  std::printf("join_plan_test: all passed\n");
  return 0;
}
