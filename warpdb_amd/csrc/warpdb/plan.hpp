// plan.hpp -- the planner of the WarpDB facade (not installed): everything an
// entry point decides before its first device call.  Which inputs it refuses,
// with which message and in which order, and what the accepted ones lower to.
// No device call is made here, so all of it is testable without a GPU
// (tests/cpp/frontend_test.cpp, sanitize_test.cpp); warpdb.cpp runs the plans.
//
// A refusal the facade raises only after a device call (it depends on the
// groups or rows that call returned, or the call's own failure comes first)
// is not hoisted into a plan: errors keep their place relative to device calls.
#pragma once
#include <algorithm>
#include <cstdint>
#include <functional>
#include <initializer_list>
#include <optional>
#include <string>
#include <unordered_set>
#include <vector>

#include "warpdb/warpdb.hpp"

namespace warpdb {

using NameSet = std::unordered_set<std::string>;

// The column names of a Table, a HostTable, anything with .columns[i].name.
template <typename T>
NameSet names_of(const T &t) {
  NameSet s;
  for (const auto &c : t.columns) s.insert(c.name);
  return s;
}

// Every column reference must name a table column (src/warpdb.cpp:19-44).
void validate_ast(const ASTNode *node, const NameSet &cols);
bool blank(const std::string &s);
bool same_expr(const ASTNode *a, const ASTNode *b);  // both set, and the same lowered text
bool uses_minmax(const ASTNode *n);
// Result column name of select item `pos` (see result_column_names).
std::string column_name(const ASTNode *n, size_t pos);

// parse_query(tokenize(sql)) with the "Failed to parse SQL: " prefix.
QueryAST parse_sql(const std::string &sql);

// validate_ast over the named clauses, in the order given, each failure
// prefixed with its clause ("SELECT clause: ", "JOIN condition: ", ...).
enum class Clause { Select, Join, Where, GroupBy, OrderBy };
void validate_clauses(const QueryAST &ast, const NameSet &cols, std::initializer_list<Clause> clauses);

// "expr [WHERE cond]" split, parsed, validated and lowered, with the
// reference's error prefixes; cond is empty when there is no WHERE.
struct Lowered {
  std::string expr, cond;
};
Lowered lower_query(const std::string &query, const NameSet &cols);
// A WHERE text ("" when blank) and an ORDER BY text (never blank, no aggregate).
std::string lower_where(const std::string &where, const NameSet &cols);
std::string lower_order_by(const std::string &order_by, const NameSet &cols);
// A list of plain expressions and their result names; `who` names the entry
// point in the messages.
struct SelectList {
  std::vector<std::string> lowered, names;
};
SelectList lower_select_list(const std::vector<std::string> &exprs, const NameSet &cols, const char *who);

// OFFSET / LIMIT: positions [offset, offset + limit) of a result.
struct Window {
  int64_t offset = 0;  // >= 0
  int64_t limit = -1;  // < 0: to the end
  Window() = default;
  Window(int64_t off, int64_t lim) : offset(std::max<int64_t>(0, off)), limit(lim < 0 ? -1 : lim) {}
  // the query's OFFSET and LIMIT clauses, negative counts taken as 0
  explicit Window(const QueryAST &ast)
      : Window(ast.offset ? std::max(0, ast.offset->count) : 0, ast.limit ? std::max(0, ast.limit->count) : -1) {}
  bool limited() const { return limit >= 0; }
  // offset + limit, saturating; -1 without a limit
  int64_t end() const { return limit < 0 ? -1 : (limit > INT64_MAX - offset ? INT64_MAX : offset + limit); }
  // how many leading rows of an n-row result must be computed
  int64_t rows_needed(int64_t n) const { return limited() ? std::min(n, end()) : n; }
  template <typename T>
  void apply(std::vector<T> &r) const {
    if (static_cast<uint64_t>(offset) >= r.size()) {
      r.clear();
      return;
    }
    r.erase(r.begin(), r.begin() + static_cast<long>(offset));
    if (limited() && r.size() > static_cast<uint64_t>(limit)) r.resize(static_cast<size_t>(limit));
  }
  template <typename T>
  std::vector<T> sliced(std::vector<T> r) const {
    apply(r);
    return r;
  }
};

// query_multi_gpu_group: "SELECT <SUM|COUNT|AVG>(value) FROM t [WHERE cond] GROUP BY key"
struct GroupPlan {
  std::string value, key, cond;
};
GroupPlan plan_multi_gpu_group(const std::string &sql, const NameSet &cols);

// query_multi_gpu_topk: limit is clamped so that offset + limit <= n_rows
// (0: an empty result, nothing runs).
struct TopkPlan {
  std::string order, cond, select;
  bool descending = false;
  int64_t offset = 0, limit = 0;
};
TopkPlan plan_multi_gpu_topk(const std::string &sql, const NameSet &cols, int64_t n_rows);

// query_sql_ordered
struct OrderedPlan {
  std::vector<std::string> names, lowered;
  std::string cond, order;
  bool descending = false;
  Window window;
};
OrderedPlan plan_sql_ordered(const std::string &sql, const NameSet &cols);

// query_sql: the validated query.  Which route it takes from here depends on
// device results, so the executor reads the AST.
struct SqlPlan {
  QueryAST ast;
  std::string cond;
  Window window;
  const AggregationNode *agg = nullptr;  // select item 0 when it is an aggregate (points into ast)
};
SqlPlan plan_sql(const std::string &sql, const NameSet &cols);
// MIN / MAX anywhere (SELECT, HAVING, ORDER BY) selects the MIN / MAX build of a grouped query
bool grouped_minmax(const QueryAST &ast, bool select_minmax);

// query_sql_table
struct TablePlan {
  enum class Route {
    Single,   // one item that query_sql answers whole (sql)
    Grouped,  // GROUP BY key: the key and aggregates of one common value expression
    Rows,     // plain items in row order (lowered)
  } route = Route::Rows;
  std::vector<std::string> names;
  SqlPlan sql;
  // Grouped: the common value expression (points into sql.ast), whether the
  // MIN / MAX build is needed, and per item its aggregate (none: the key)
  const ASTNode *value = nullptr;
  bool minmax = false;
  std::vector<std::optional<AggregationType>> items;
  std::vector<std::string> lowered;  // Rows
};
TablePlan plan_sql_table(const std::string &sql, const NameSet &cols);

// One grouped query's groups as wx_group_agg returns them (ascending key
// order) and, after finish(), the groups HAVING keeps in result order.
struct GroupRun {
  std::vector<int32_t> keys;
  std::vector<double> sums;
  std::vector<int64_t> cnts;
  std::vector<float> mins, maxs;  // MIN / MAX builds only
  std::vector<size_t> order;      // the groups HAVING keeps, in result order
  // per-group aggregate value (AggData, src/warpdb.cpp:375-385)
  double value_of(AggregationType t, size_t i) const;
  // HAVING, then ORDER BY, over the groups; `val` is the aggregated
  // expression, `key` the GROUP BY key.  Its refusals are raised per group
  // (HAVING: never with zero groups) and so only after the device call.
  void finish(const QueryAST &ast, const ASTNode *val, const ASTNode *key);
  // The same over aggregates of any expression: agg_value(a, i, having) is
  // aggregate `a` of group i (having: asked by HAVING, else by ORDER BY).
  using AggValue = std::function<double(const AggregationNode *a, size_t i, bool having)>;
  void finish(const QueryAST &ast, const ASTNode *key, const AggValue &agg_value);
};

// query_sql_grouped: "SELECT items FROM t [WHERE c] GROUP BY k [HAVING h]
// [ORDER BY o [ASC|DESC]] [LIMIT n] [OFFSET m]", each item the key or SUM /
// AVG / COUNT / MIN / MAX of any value expression.  The value expressions are
// deduplicated by their lowered text into slots: those of the select list
// first, then the hidden ones only HAVING / ORDER BY aggregate.  COUNT needs
// no slot of its own (every aggregate of a group sees the same rows); a query
// that only counts gets one summed slot to run on.
struct GroupedPlan {
  QueryAST ast;
  std::string cond;
  Window window;
  std::vector<std::string> names;
  const ASTNode *key = nullptr;  // points into ast
  struct Slot {
    std::string lowered;
    bool sum = false, minmax = false;  // SUM / AVG need the sum, MIN / MAX the extremes
  };
  std::vector<Slot> slots;
  size_t selected_slots = 0;  // slots [0, selected_slots) come from the select list
  struct Item {
    std::optional<AggregationType> agg;  // none: the key
    int slot = -1;                       // -1: the key, or a COUNT (the shared count)
  };
  std::vector<Item> items;
  // the slot of an aggregate's expression (-1: none, e.g. a COUNT of an expression nothing else aggregates)
  int slot_of(const AggregationNode *a) const;
  // the slots in chunks of at most `width` (WX_GROUP_MAX_VALUES): [first, first + count)
  std::vector<std::pair<size_t, size_t>> chunks(size_t width) const;
};
GroupedPlan plan_sql_grouped(const std::string &sql, const NameSet &cols);

// query_sql_windowed: "SELECT items FROM t [WHERE c] [LIMIT n] [OFFSET m]",
// each item a plain expression or SUM / AVG / COUNT / MIN / MAX (value) OVER
// (PARTITION BY key), at least one of them a window item and all of them over
// the one partition key (compared by its lowering; OVER () is the key `0`,
// one partition).  wx_window_select takes the plain expressions first, then
// the window items: `output[i]` is where select item i lands in that order.
struct WindowedPlan {
  std::string cond, partition;
  Window window;
  std::vector<std::string> names;
  std::vector<std::string> plain;  // lowered plain expressions, in list order
  struct Item {
    std::string value;  // lowered value expression
    AggregationType agg;
  };
  std::vector<Item> items;  // the window items, in list order
  std::vector<size_t> output;
};
WindowedPlan plan_sql_windowed(const std::string &sql, const NameSet &cols);

// query_sql_joined: "SELECT items FROM t [INNER] JOIN u ON c [WHERE w] [LIMIT n]
// [OFFSET m]" (or LEFT [OUTER] JOIN), each item a plain expression over the
// columns of both tables.  c is <expression over t's columns> = <bare column
// of u>, with = or ==, either way round.  A name may be qualified with its
// table (t.price, u.rate); an unqualified name found in both tables is
// ambiguous.  The lowered texts name u's columns with the prefix
// kJoinRightPrefix, so equal names in the two tables never collide.
extern const char *const kJoinRightPrefix;  // "wxr_"
struct JoinedPlan {
  std::string right_table;  // u
  bool left_outer = false;
  std::string left_key;     // lowered, over t's columns
  std::string right_key;    // u's column, by its own name
  std::vector<std::string> names, lowered;
  std::string cond;
  Window window;
};
JoinedPlan plan_sql_joined(const std::string &sql, const NameSet &left_cols, const std::string &right_name,
                           const NameSet &right_cols);
// The same with the right table looked up by the name the query gives it
// (null: no such table), so that the query is parsed once.
using JoinTables = std::function<const NameSet *(const std::string &name)>;
JoinedPlan plan_sql_joined(const std::string &sql, const NameSet &left_cols, const JoinTables &right_cols_of);
// Whether the join_index-th JOIN of a token list is LEFT [OUTER] JOIN.  The
// AST cannot say: JoinClause keeps its size (include/warpdb/expression.hpp).
bool join_is_left_outer(const std::vector<Token> &tokens, size_t join_index);
// query_join: the same plan from its parts (left_key an expression over the
// left columns, right_key a column of the right table, exprs and where over
// both; names unqualified or qualified with `left_name` / `right_name`).
JoinedPlan plan_join(const std::string &left_name, const NameSet &left_cols, const std::string &right_name,
                     const NameSet &right_cols, const std::string &left_key, const std::string &right_key,
                     const std::vector<std::string> &exprs, const std::string &where, bool left_outer);

// query_sql_joined_grouped: "SELECT items FROM t [INNER] JOIN u ON c [WHERE w]
// GROUP BY k [HAVING h] [ORDER BY o [ASC|DESC]] [LIMIT n] [OFFSET m]", each
// item the key or SUM / AVG / COUNT / MIN / MAX of any expression; every
// expression, the key and the WHERE are over the columns of both tables.  The
// ON condition and the names follow plan_sql_joined (qualified or not, u's
// columns lowered under kJoinRightPrefix), the slots GroupedPlan: `g` is the
// grouped plan over the resolved tree, so GroupedRun::finish runs on it as it
// is.  LEFT JOIN is refused: an unmatched row would need NULL-aware aggregates.
struct JoinedGroupedPlan {
  std::string right_table;  // u
  std::string left_key;     // lowered, over t's columns
  std::string right_key;    // u's column, by its own name
  GroupedPlan g;
};
JoinedGroupedPlan plan_sql_joined_grouped(const std::string &sql, const NameSet &left_cols,
                                          const JoinTables &right_cols_of);
JoinedGroupedPlan plan_sql_joined_grouped(const std::string &sql, const NameSet &left_cols,
                                          const std::string &right_name, const NameSet &right_cols);

// The groups of a GroupedPlan: keys and counts (shared), one set of
// aggregates per slot.  run.order after finish() as in GroupRun.
struct GroupedRun {
  GroupRun run;  // keys, cnts, order (its sums / mins / maxs stay empty)
  struct SlotData {
    std::vector<double> sums;
    std::vector<float> mins, maxs;
  };
  std::vector<SlotData> slots;
  double value_of(const GroupedPlan &p, AggregationType t, int slot, size_t i) const;
  void finish(const GroupedPlan &p);
};

}  // namespace warpdb
