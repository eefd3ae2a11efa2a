// join_group_plan_test.cpp -- the planner of WarpDB::query_sql_joined_grouped
// (plan_sql_joined_grouped) without a device, driven from
// tests/golden/join_group_errors.tsv: what each accepted query lowers to (the
// join keys, the group key, the slots with their masks, the WHERE, the
// window, the items) and every refusal with its message; rows that break
// several rules at once pin the order of the checks.  The same rows are run
// against the whole facade by tests/test_gpu_join_group.py.
//
// A row is  kind <TAB> sql <TAB> expectation  with kind `accept` (the
// expectation is dump()'s text) or `refuse` (the whole message).  The tables:
// t(price, quantity, cust, id) JOIN u(id, rate, tier).
// Build: make -C tests/cpp bin/join_group_plan_test; run from the repository root.
#include <cstdio>
#include <fstream>
#include <sstream>
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

using warpdb::JoinedGroupedPlan;
using warpdb::NameSet;
static const NameSet kLeft{"price", "quantity", "cust", "id"};
static const NameSet kRight{"id", "rate", "tier"};

static JoinedGroupedPlan plan(const std::string &sql) {
  return warpdb::plan_sql_joined_grouped(sql, kLeft, "u", kRight);
}

static const char *agg_name(AggregationType t) {
  switch (t) {
    case AggregationType::Sum: return "sum";
    case AggregationType::Avg: return "avg";
    case AggregationType::Count: return "count";
    case AggregationType::Min: return "min";
    case AggregationType::Max: return "max";
  }
  return "?";
}

// lkey | rkey | key | cond | offset,limit | names | slots expr:S:Q (selected first, `/` before the hidden ones) | items
static std::string dump(const JoinedGroupedPlan &p) {
  std::ostringstream o;
  o << p.left_key << " | " << p.right_key << " | " << p.g.key->to_cuda_expr() << " | " << p.g.cond << " | "
    << p.g.window.offset << "," << p.g.window.limit << " | ";
  for (size_t i = 0; i < p.g.names.size(); ++i) o << (i ? "," : "") << p.g.names[i];
  o << " | ";
  for (size_t s = 0; s < p.g.slots.size(); ++s)
    o << (s == p.g.selected_slots ? " / " : (s ? " " : "")) << p.g.slots[s].lowered << ":" << p.g.slots[s].sum << ":"
      << p.g.slots[s].minmax;
  o << " | ";
  for (size_t i = 0; i < p.g.items.size(); ++i)
    o << (i ? "," : "") << (p.g.items[i].agg ? agg_name(*p.g.items[i].agg) : "key") << "@" << p.g.items[i].slot;
  return o.str();
}

static void table_rows() {
  std::ifstream in("tests/golden/join_group_errors.tsv");
  CHECK(in.good());
  std::string line;
  int accepted = 0, refused = 0;
  while (std::getline(in, line)) {
    if (line.empty() || line[0] == '#') continue;
    const size_t a = line.find('\t'), b = line.find('\t', a + 1);
    CHECK(a != std::string::npos && b != std::string::npos);
    if (a == std::string::npos || b == std::string::npos) continue;
    const std::string kind = line.substr(0, a), sql = line.substr(a + 1, b - a - 1), want = line.substr(b + 1);
    std::string got;
    try {
      got = dump(plan(sql));
      if (kind != "accept") got = "<no error>";
    } catch (const std::runtime_error &e) {
      got = e.what();
      if (kind != "refuse") got = "refused: " + got;
    }
    if (got != want) {
      std::printf("FAILED row: %s\n  want: %s\n  got:  %s\n", sql.c_str(), want.c_str(), got.c_str());
      ++failures;
    }
    (kind == "accept" ? accepted : refused)++;
  }
  CHECK(accepted >= 8 && refused >= 20);
}

static void chunks_and_lookup() {
  // six distinct value expressions: two chunks of at most four slots
  const JoinedGroupedPlan p = plan(
      "SELECT tier, SUM(price), SUM(rate), SUM(price * rate), SUM(quantity), SUM(price + 1), MAX(cust + rate) "
      "FROM t JOIN u ON cust = u.id GROUP BY tier");
  CHECK(p.g.slots.size() == 6);
  const auto c = p.g.chunks(4);
  CHECK(c.size() == 2 && c[0].first == 0 && c[0].second == 4 && c[1].first == 4 && c[1].second == 2);
  // the right table is looked up by the name the query gives it
  int asked = 0;
  const JoinedGroupedPlan q = warpdb::plan_sql_joined_grouped(
      "SELECT tier, COUNT(price) FROM t JOIN dim ON cust = dim.id GROUP BY tier", kLeft, [&](const std::string &n) {
        ++asked;
        return n == "dim" ? &kRight : nullptr;
      });
  CHECK(asked == 1 && q.right_table == "dim" && q.g.slots.size() == 1);
  // the other planners keep their refusals
  auto error_of = [](auto &&f) -> std::string {
    try {
      f();
    } catch (const std::runtime_error &e) {
      return e.what();
    }
    return "<no error>";
  };
  const std::string sql = "SELECT tier, SUM(price) FROM t JOIN u ON cust = u.id GROUP BY tier";
  CHECK(error_of([&] { warpdb::plan_sql_joined(sql, kLeft, "u", kRight); }) ==
        "GROUP BY is not supported by query_sql_joined");
  CHECK(error_of([&] { warpdb::plan_sql_joined("SELECT SUM(rate) FROM t JOIN u ON cust = u.id", kLeft, "u", kRight); }) ==
        "aggregates are not supported by query_sql_joined (plain expressions only)");
  CHECK(error_of([&] {
          warpdb::plan_sql_joined("SELECT price + SUM(rate) FROM t JOIN u ON cust = u.id", kLeft, "u", kRight);
        }).find("not supported") != std::string::npos);
}

int main() {
  table_rows();
  chunks_and_lookup();
  if (failures) {
    std::printf("join_group_plan_test: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("join_group_plan_test: all passed\n");
  return 0;
}
