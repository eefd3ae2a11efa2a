// plan.cpp -- the facade's planner (plan.hpp): validation, lowering and the
// per-entry-point plans.  Front-end headers only, no device call.
// Reference: src/warpdb.cpp:19-44, 204-240, 330-423.
#include "plan.hpp"

#include <cctype>
#include <cmath>
#include <functional>
#include <stdexcept>

namespace warpdb {

void validate_ast(const ASTNode *node, const NameSet &cols) {
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

bool blank(const std::string &s) {
  return std::all_of(s.begin(), s.end(), [](char c) { return std::isspace(static_cast<unsigned char>(c)); });
}

bool same_expr(const ASTNode *a, const ASTNode *b) { return a && b && a->to_cuda_expr() == b->to_cuda_expr(); }

bool uses_minmax(const ASTNode *n) {
  if (!n) return false;
  if (auto a = dynamic_cast<const AggregationNode *>(n))
    return a->agg == AggregationType::Min || a->agg == AggregationType::Max;
  if (auto b = dynamic_cast<const BinaryOpNode *>(n)) return uses_minmax(b->left.get()) || uses_minmax(b->right.get());
  return false;
}

std::string column_name(const ASTNode *n, size_t pos) {
  if (auto v = dynamic_cast<const VariableNode *>(n)) return v->name;
  if (auto a = dynamic_cast<const AggregationNode *>(n)) return a->agg_kernel() + "_" + std::to_string(pos);
  return "expr" + std::to_string(pos);
}

QueryAST parse_sql(const std::string &sql) {
  try {
    return parse_query(tokenize(sql));
  } catch (const std::exception &e) {
    throw std::runtime_error(std::string("Failed to parse SQL: ") + e.what());
  }
}

std::vector<std::string> result_column_names(const std::string &sql) {
  const QueryAST ast = parse_sql(sql);
  std::vector<std::string> names;
  for (size_t i = 0; i < ast.select_list.size(); ++i) names.push_back(column_name(ast.select_list[i].get(), i));
  return names;
}

void validate_clauses(const QueryAST &ast, const NameSet &cols, std::initializer_list<Clause> clauses) {
  auto check = [&](const ASTNode *n, const char *ctx) {
    try {
      validate_ast(n, cols);
    } catch (const std::exception &e) {
      throw std::runtime_error(std::string(ctx) + ": " + e.what());
    }
  };
  for (Clause c : clauses) {
    switch (c) {
      case Clause::Select:
        for (const auto &e : ast.select_list) check(e.get(), "SELECT clause");
        break;
      case Clause::Join:
        for (const auto &j : ast.joins) check(j.condition.get(), "JOIN condition");
        break;
      case Clause::Where:
        if (ast.where) check(ast.where->get(), "WHERE clause");
        break;
      case Clause::GroupBy:
        if (ast.group_by)
          for (const auto &k : ast.group_by->keys) check(k.get(), "GROUP BY");
        break;
      case Clause::OrderBy:
        if (ast.order_by) check(ast.order_by->expr.get(), "ORDER BY");
        break;
    }
  }
}

namespace {
ASTNodePtr parse_plain(const std::string &text) {
  try {
    return parse_expression(tokenize(text));
  } catch (const std::exception &err) {
    throw std::runtime_error(std::string("Failed to parse expression: ") + err.what());
  }
}

std::string lowered_where(const QueryAST &ast) { return ast.where ? (*ast.where)->to_cuda_expr() : std::string(); }

bool is_agg(const ASTNode *n) { return dynamic_cast<const AggregationNode *>(n) != nullptr; }
bool is_window(const ASTNode *n) { return dynamic_cast<const WindowFunctionNode *>(n) != nullptr; }

const char *const kTooManyItems = "a select list takes at most ";
}  // namespace

Lowered lower_query(const std::string &query, const NameSet &cols) {
  if (query.empty()) throw std::runtime_error("Empty query expression");
  std::string e, c;
  split_where(query, e, c);
  const ASTNodePtr ex = parse_plain(e);
  validate_ast(ex.get(), cols);
  Lowered q;
  q.expr = ex->to_cuda_expr();
  q.cond = lower_where(c, cols);
  return q;
}

std::string lower_where(const std::string &where, const NameSet &cols) {
  if (blank(where)) return {};
  try {
    const ASTNodePtr cx = parse_expression(tokenize(where));
    validate_ast(cx.get(), cols);
    return cx->to_cuda_expr();
  } catch (const std::exception &err) {
    throw std::runtime_error(std::string("Failed to parse WHERE clause: ") + err.what());
  }
}

std::string lower_order_by(const std::string &order_by, const NameSet &cols) {
  if (blank(order_by)) throw std::runtime_error("Empty ORDER BY expression");
  try {
    const ASTNodePtr ox = parse_expression(tokenize(order_by));
    validate_ast(ox.get(), cols);
    if (is_agg(ox.get())) throw std::runtime_error("aggregates are not supported here");
    return ox->to_cuda_expr();
  } catch (const std::exception &err) {
    throw std::runtime_error(std::string("Failed to parse ORDER BY expression: ") + err.what());
  }
}

SelectList lower_select_list(const std::vector<std::string> &exprs, const NameSet &cols, const char *who) {
  if (exprs.empty()) throw std::runtime_error("Empty SELECT list");
  if (exprs.size() > WarpDB::kMaxSelectExprs)
    throw std::runtime_error(std::string(who) + " takes at most " + std::to_string(WarpDB::kMaxSelectExprs) +
                             " expressions");
  SelectList list;
  for (size_t i = 0; i < exprs.size(); ++i) {
    if (blank(exprs[i])) throw std::runtime_error("Empty query expression");
    const ASTNodePtr ex = parse_plain(exprs[i]);
    validate_ast(ex.get(), cols);
    if (is_agg(ex.get())) throw std::runtime_error(std::string(who) + " takes plain expressions, not aggregates");
    list.lowered.push_back(ex->to_cuda_expr());
    list.names.push_back(column_name(ex.get(), i));
  }
  return list;
}

GroupPlan plan_multi_gpu_group(const std::string &sql, const NameSet &cols) {
  const QueryAST ast = parse_sql(sql);
  auto *agg = ast.select_list.empty() ? nullptr : dynamic_cast<const AggregationNode *>(ast.select_list[0].get());
  if (!ast.group_by || !agg)
    throw std::runtime_error("query_multi_gpu_group expects SELECT <agg>(expr) ... GROUP BY key");
  if (ast.group_by->keys.size() != 1) throw std::runtime_error("GROUP BY supports one key expression");
  if (!ast.joins.empty()) throw std::runtime_error("JOIN is not supported by the execution engine");
  const std::string kind = agg->agg_kernel();
  if (kind != "sum" && kind != "count" && kind != "avg")  // the shards exchange (sum, count) only
    throw std::runtime_error("query_multi_gpu_group supports SUM / COUNT / AVG, not " + kind);
  const ASTNode *key = ast.group_by->keys[0].get();
  validate_ast(agg->expr.get(), cols);
  validate_ast(key, cols);
  if (ast.where) validate_ast(ast.where->get(), cols);
  // SUM / COUNT / AVG all derive from the (sum, count) the shards exchange
  GroupPlan p;
  p.value = agg->expr->to_cuda_expr();
  p.key = key->to_cuda_expr();
  p.cond = lowered_where(ast);
  return p;
}

TopkPlan plan_multi_gpu_topk(const std::string &sql, const NameSet &cols, int64_t n_rows) {
  const QueryAST ast = parse_sql(sql);
  if (ast.select_list.size() != 1 || ast.group_by || ast.distinct || !ast.order_by || !ast.limit)
    throw std::runtime_error("query_multi_gpu_topk expects SELECT expr FROM t [WHERE c] ORDER BY o [DESC] LIMIT k");
  if (is_agg(ast.select_list[0].get()))
    throw std::runtime_error("query_multi_gpu_topk takes a plain SELECT expression");
  if (!ast.joins.empty()) throw std::runtime_error("JOIN is not supported by the execution engine");
  TopkPlan p;
  p.offset = ast.offset ? ast.offset->count : 0;
  p.limit = ast.limit->count;
  if (p.offset < 0 || p.limit < 0) throw std::runtime_error("query_multi_gpu_topk needs OFFSET, LIMIT >= 0");
  // nothing beyond the table: LIMIT 0 or OFFSET >= rows is an empty result
  // (no head is gathered); otherwise offset + limit <= rows, computed without
  // overflow, so each shard's head record holds at most the table's rows
  p.limit = p.offset >= n_rows ? 0 : std::min(p.limit, n_rows - p.offset);
  validate_ast(ast.select_list[0].get(), cols);
  validate_ast(ast.order_by->expr.get(), cols);
  if (ast.where) validate_ast(ast.where->get(), cols);
  p.order = ast.order_by->expr->to_cuda_expr();
  p.cond = lowered_where(ast);
  p.select = ast.select_list[0]->to_cuda_expr();
  p.descending = !ast.order_by->ascending;
  return p;
}

OrderedPlan plan_sql_ordered(const std::string &sql, const NameSet &cols) {
  const QueryAST ast = parse_sql(sql);
  if (ast.select_list.empty()) throw std::runtime_error("Empty SELECT list");
  if (!ast.joins.empty()) throw std::runtime_error("JOIN is not supported by query_sql_ordered");
  if (ast.group_by) throw std::runtime_error("GROUP BY is not supported by query_sql_ordered (use query_sql_table)");
  if (ast.distinct) throw std::runtime_error("DISTINCT is not supported by query_sql_ordered");
  for (const auto &e : ast.select_list) {
    if (is_window(e.get())) throw std::runtime_error("window functions are not supported by query_sql_ordered");
    if (is_agg(e.get()))
      throw std::runtime_error("aggregates are not supported by query_sql_ordered (plain expressions only)");
  }
  if (!ast.order_by) throw std::runtime_error("query_sql_ordered needs an ORDER BY clause");
  if (is_agg(ast.order_by->expr.get()))
    throw std::runtime_error("aggregates are not supported by query_sql_ordered (plain expressions only)");
  validate_clauses(ast, cols, {Clause::Select, Clause::Where, Clause::OrderBy});
  const size_t m = ast.select_list.size();
  if (m > WarpDB::kMaxSelectExprs)
    throw std::runtime_error(kTooManyItems + std::to_string(WarpDB::kMaxSelectExprs) + " expressions");
  OrderedPlan p;
  for (size_t i = 0; i < m; ++i) {
    p.names.push_back(column_name(ast.select_list[i].get(), i));
    p.lowered.push_back(ast.select_list[i]->to_cuda_expr());
  }
  p.cond = lowered_where(ast);
  p.order = ast.order_by->expr->to_cuda_expr();
  p.descending = !ast.order_by->ascending;
  p.window = Window(ast);
  return p;
}

namespace {
// What query_sql and query_sql_table check first, in this order.
SqlPlan checked_sql(const std::string &sql, const NameSet &cols) {
  SqlPlan p;
  p.ast = parse_sql(sql);
  if (p.ast.select_list.empty()) throw std::runtime_error("Empty SELECT list");
  validate_clauses(p.ast, cols, {Clause::Select, Clause::Join, Clause::Where, Clause::GroupBy, Clause::OrderBy});
  if (!p.ast.joins.empty()) throw std::runtime_error("JOIN is not supported by the execution engine");
  p.cond = lowered_where(p.ast);
  p.window = Window(p.ast);
  p.agg = dynamic_cast<const AggregationNode *>(p.ast.select_list[0].get());
  return p;
}

// query_sql's own refusals of a grouped query
void check_sql_group(const SqlPlan &p) {
  if (!p.ast.group_by) return;
  if (!p.agg) throw std::runtime_error("Only aggregation queries supported with GROUP BY");
  if (p.ast.group_by->keys.size() != 1) throw std::runtime_error("GROUP BY supports one key expression");
}
}  // namespace

SqlPlan plan_sql(const std::string &sql, const NameSet &cols) {
  SqlPlan p = checked_sql(sql, cols);
  check_sql_group(p);
  return p;
}

bool grouped_minmax(const QueryAST &ast, bool select_minmax) {
  return select_minmax || (ast.having && uses_minmax(ast.having->get())) ||
         (ast.order_by && uses_minmax(ast.order_by->expr.get()));
}

TablePlan plan_sql_table(const std::string &sql, const NameSet &cols) {
  TablePlan p;
  p.sql = checked_sql(sql, cols);
  const QueryAST &ast = p.sql.ast;
  const size_t m = ast.select_list.size();
  for (size_t i = 0; i < m; ++i) p.names.push_back(column_name(ast.select_list[i].get(), i));
  for (const auto &e : ast.select_list)
    if (is_window(e.get())) throw std::runtime_error("window functions are not supported by the execution engine");

  // one item that query_sql answers whole: an aggregate, or an ordered /
  // distinct projection (no row ids: the rows are aggregated or permuted)
  if (m == 1 && (p.sql.agg || (!ast.group_by && (ast.order_by || ast.distinct)))) {
    check_sql_group(p.sql);
    p.route = TablePlan::Route::Single;
    return p;
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
        p.items.push_back(a->agg);
      } else if (same_expr(item, key)) {
        p.items.push_back(std::nullopt);
      } else {
        throw std::runtime_error("select item " + std::to_string(i) +
                                 " must be the GROUP BY key or an aggregate (SUM / AVG / COUNT / MIN / MAX)");
      }
    }
    p.value = val ? val : (counted ? counted : key);
    p.minmax = grouped_minmax(ast, mm);
    p.route = TablePlan::Route::Grouped;
    return p;
  }

  for (const auto &e : ast.select_list)
    if (is_agg(e.get())) throw std::runtime_error("aggregates beside other select items need GROUP BY: not supported");
  if (ast.order_by || ast.distinct)
    throw std::runtime_error("ORDER BY / DISTINCT over a multi-column result is not supported (row order only)");
  if (m > WarpDB::kMaxSelectExprs)
    throw std::runtime_error(kTooManyItems + std::to_string(WarpDB::kMaxSelectExprs) + " expressions");
  for (const auto &e : ast.select_list) p.lowered.push_back(e->to_cuda_expr());
  p.route = TablePlan::Route::Rows;
  return p;
}

double GroupRun::value_of(AggregationType t, size_t i) const {
  switch (t) {
    case AggregationType::Sum: return sums[i];
    case AggregationType::Avg: return sums[i] / static_cast<double>(cnts[i]);
    case AggregationType::Count: return static_cast<double>(cnts[i]);
    case AggregationType::Min: return mins[i];
    case AggregationType::Max: return maxs[i];
  }
  return NAN;
}

void GroupRun::finish(const QueryAST &ast, const ASTNode *val, const ASTNode *key) {
  finish(ast, key, [&](const AggregationNode *a, size_t i, bool having) {
    if (having && !same_expr(a->expr.get(), val) && a->agg != AggregationType::Count)
      throw std::runtime_error("HAVING may only aggregate the selected expression");
    return value_of(a->agg, i);
  });
}

void GroupRun::finish(const QueryAST &ast, const ASTNode *key, const AggValue &agg_value) {
  // HAVING over the (few) aggregated groups, with the reference's
  // comparison semantics (src/warpdb.cpp:387-423)
  std::function<double(const ASTNode *, size_t)> having = [&](const ASTNode *n, size_t i) -> double {
    if (auto c = dynamic_cast<const ConstantNode *>(n)) return std::stod(c->value);
    if (auto a = dynamic_cast<const AggregationNode *>(n)) return agg_value(a, i, true);
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
  order.clear();
  for (size_t i = 0; i < keys.size(); ++i)
    if (!ast.having || having(ast.having->get(), i) != 0.0) order.push_back(i);
  if (ast.order_by) {  // groups arrive in ascending key order
    const ASTNode *ob = ast.order_by->expr.get();
    auto *oagg = dynamic_cast<const AggregationNode *>(ob);
    if (oagg) {
      std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
        const double x = agg_value(oagg, a, false), y = agg_value(oagg, b, false);
        return ast.order_by->ascending ? x < y : x > y;
      });
    } else if (same_expr(ob, key)) {
      if (!ast.order_by->ascending) std::reverse(order.begin(), order.end());
    } else {
      throw std::runtime_error("ORDER BY with GROUP BY must name the key or an aggregate");
    }
  }
}

// ------------------------------------------------------- query_sql_grouped
int GroupedPlan::slot_of(const AggregationNode *a) const {
  const std::string text = a->expr->to_cuda_expr();
  for (size_t s = 0; s < slots.size(); ++s)
    if (slots[s].lowered == text) return static_cast<int>(s);
  return -1;
}

std::vector<std::pair<size_t, size_t>> GroupedPlan::chunks(size_t width) const {
  std::vector<std::pair<size_t, size_t>> c;
  for (size_t first = 0; first < slots.size(); first += width)
    c.emplace_back(first, std::min(width, slots.size() - first));
  return c;
}

// The items and the slots of a grouped plan whose ast, key and names are set:
// select items first, then the aggregates only HAVING / ORDER BY name.  With
// `cols`, a hidden aggregate's argument is validated against them under its
// clause's prefix (plan_sql_grouped); a caller that resolved every name
// already passes none (plan_sql_joined_grouped).
static void fill_group_slots(GroupedPlan &p, const NameSet *cols) {
  const QueryAST &ast = p.ast;
  const size_t m = ast.select_list.size();
  // the slot of an aggregate's expression, made on first use; COUNT takes none
  auto use = [&](const AggregationNode *a) -> int {
    if (a->agg == AggregationType::Count) return -1;
    int s = p.slot_of(a);
    if (s < 0) {
      p.slots.push_back({a->expr->to_cuda_expr(), false, false});
      s = static_cast<int>(p.slots.size()) - 1;
    }
    const bool mm = a->agg == AggregationType::Min || a->agg == AggregationType::Max;
    p.slots[static_cast<size_t>(s)].sum = p.slots[static_cast<size_t>(s)].sum || !mm;
    p.slots[static_cast<size_t>(s)].minmax = p.slots[static_cast<size_t>(s)].minmax || mm;
    return s;
  };
  const AggregationNode *counted = nullptr;
  for (size_t i = 0; i < m; ++i) {
    const ASTNode *item = ast.select_list[i].get();
    if (auto a = dynamic_cast<const AggregationNode *>(item)) {
      if (a->agg == AggregationType::Count && !counted) counted = a;
      p.items.push_back({a->agg, use(a)});
    } else if (same_expr(item, p.key)) {
      p.items.push_back({std::nullopt, -1});
    } else {
      throw std::runtime_error("select item " + std::to_string(i) +
                               " must be the GROUP BY key or an aggregate (SUM / AVG / COUNT / MIN / MAX)");
    }
  }
  p.selected_slots = p.slots.size();
  // aggregates that only HAVING / ORDER BY name: hidden slots
  std::function<void(const ASTNode *, const char *)> hidden = [&](const ASTNode *n, const char *ctx) {
    if (auto a = dynamic_cast<const AggregationNode *>(n)) {
      try {
        if (cols) validate_ast(a->expr.get(), *cols);
      } catch (const std::exception &e) {
        throw std::runtime_error(std::string(ctx) + ": " + e.what());
      }
      if (a->agg == AggregationType::Count && !counted) counted = a;
      use(a);
    } else if (auto b = dynamic_cast<const BinaryOpNode *>(n)) {
      hidden(b->left.get(), ctx);
      hidden(b->right.get(), ctx);
    }
  };
  if (ast.having) hidden(ast.having->get(), "HAVING clause");
  if (ast.order_by) {
    const ASTNode *ob = ast.order_by->expr.get();
    if (!is_agg(ob) && !same_expr(ob, p.key))
      throw std::runtime_error("ORDER BY with GROUP BY must name the key or an aggregate");
    hidden(ob, "ORDER BY");
  }
  // nothing but the key and COUNTs: one summed slot to run on (what is counted, else the key)
  if (p.slots.empty()) p.slots.push_back({(counted ? counted->expr.get() : p.key)->to_cuda_expr(), true, false});
}

GroupedPlan plan_sql_grouped(const std::string &sql, const NameSet &cols) {
  GroupedPlan p;
  {
    SqlPlan checked = checked_sql(sql, cols);  // plan_sql_table's first checks, in its order
    p.ast = std::move(checked.ast);
    p.cond = std::move(checked.cond);
    p.window = checked.window;
  }
  const QueryAST &ast = p.ast;
  const size_t m = ast.select_list.size();
  for (size_t i = 0; i < m; ++i) p.names.push_back(column_name(ast.select_list[i].get(), i));
  for (const auto &e : ast.select_list)
    if (is_window(e.get())) throw std::runtime_error("window functions are not supported by the execution engine");
  if (!ast.group_by) throw std::runtime_error("query_sql_grouped needs a GROUP BY clause");
  if (ast.group_by->keys.size() != 1) throw std::runtime_error("GROUP BY supports one key expression");
  if (ast.distinct) throw std::runtime_error("DISTINCT over a multi-column result is not supported");
  if (m > WarpDB::kMaxSelectExprs)
    throw std::runtime_error(kTooManyItems + std::to_string(WarpDB::kMaxSelectExprs) + " expressions");
  p.key = ast.group_by->keys[0].get();

  fill_group_slots(p, &cols);
  return p;
}

double GroupedRun::value_of(const GroupedPlan &p, AggregationType t, int slot, size_t i) const {
  if (t == AggregationType::Count) return static_cast<double>(run.cnts[i]);
  if (slot < 0 || static_cast<size_t>(slot) >= slots.size()) throw std::runtime_error("aggregate without a slot");
  const SlotData &s = slots[static_cast<size_t>(slot)];
  switch (t) {
    case AggregationType::Sum: return s.sums[i];
    case AggregationType::Avg: return s.sums[i] / static_cast<double>(run.cnts[i]);
    case AggregationType::Min: return s.mins[i];
    case AggregationType::Max: return s.maxs[i];
    default: break;
  }
  (void)p;
  return NAN;
}

void GroupedRun::finish(const GroupedPlan &p) {
  run.finish(p.ast, p.key,
             [&](const AggregationNode *a, size_t i, bool) { return value_of(p, a->agg, p.slot_of(a), i); });
}

// ------------------------------------------------------ query_sql_windowed
WindowedPlan plan_sql_windowed(const std::string &sql, const NameSet &cols) {
  const QueryAST ast = parse_sql(sql);
  if (ast.select_list.empty()) throw std::runtime_error("Empty SELECT list");
  validate_clauses(ast, cols, {Clause::Select, Clause::Join, Clause::Where, Clause::GroupBy, Clause::OrderBy});
  if (!ast.joins.empty()) throw std::runtime_error("JOIN is not supported by query_sql_windowed");
  if (ast.group_by)
    throw std::runtime_error("GROUP BY is not supported by query_sql_windowed (use query_sql_grouped)");
  if (ast.having) throw std::runtime_error("HAVING is not supported by query_sql_windowed");
  if (ast.distinct) throw std::runtime_error("DISTINCT is not supported by query_sql_windowed");
  if (ast.order_by)
    throw std::runtime_error("ORDER BY is not supported by query_sql_windowed (the result is in row order)");
  const size_t m = ast.select_list.size();
  std::vector<const WindowFunctionNode *> wins;
  for (const auto &e : ast.select_list)
    if (auto w = dynamic_cast<const WindowFunctionNode *>(e.get())) wins.push_back(w);
  if (wins.empty())
    throw std::runtime_error("query_sql_windowed needs a window item, AGG(x) OVER (PARTITION BY k) (use query_sql_table)");
  for (const auto &e : ast.select_list)
    if (is_agg(e.get()))
      throw std::runtime_error("a plain aggregate beside window items is not supported by query_sql_windowed");
  for (const auto *w : wins)
    if (w->order_by)
      throw std::runtime_error("ORDER BY inside OVER is not supported (PARTITION BY only: no running or framed "
                               "aggregates)");
  for (const auto *w : wins)
    if (w->partition_by.size() > 1) throw std::runtime_error("PARTITION BY supports one key expression");
  // OVER () and a constant key (PARTITION BY 0) name the same single partition: the key 0
  auto partition_of = [](const WindowFunctionNode *w) {
    if (w->partition_by.empty() || dynamic_cast<const ConstantNode *>(w->partition_by[0].get()))
      return std::string("0");
    return w->partition_by[0]->to_cuda_expr();
  };
  for (const auto *w : wins) {
    if (!w->partition_by.empty() && (is_agg(w->partition_by[0].get()) || is_window(w->partition_by[0].get())))
      throw std::runtime_error("PARTITION BY takes a plain expression, not an aggregate");
    if (partition_of(w) != partition_of(wins[0]))
      throw std::runtime_error("window items partition by two different expressions (" + partition_of(wins[0]) +
                               " and " + partition_of(w) + "): one is supported");
  }
  if (m > WarpDB::kMaxSelectExprs)
    throw std::runtime_error(kTooManyItems + std::to_string(WarpDB::kMaxSelectExprs) + " expressions");
  // distinct value expressions: a COUNT counts the partition's rows whatever it names
  std::vector<std::string> values;
  for (const auto *w : wins) {
    const std::string v = w->expr->to_cuda_expr();
    if (w->agg != AggregationType::Count && std::find(values.begin(), values.end(), v) == values.end())
      values.push_back(v);
  }
  if (values.size() > WarpDB::kMaxWindowValues)
    throw std::runtime_error("window items aggregate " + std::to_string(values.size()) +
                             " different expressions: at most " + std::to_string(WarpDB::kMaxWindowValues) +
                             " are supported");
  WindowedPlan p;
  p.cond = lowered_where(ast);
  p.partition = partition_of(wins[0]);
  p.window = Window(ast);
  for (size_t i = 0; i < m; ++i) {
    const ASTNode *item = ast.select_list[i].get();
    p.names.push_back(column_name(item, i));
    if (auto w = dynamic_cast<const WindowFunctionNode *>(item)) p.items.push_back({w->expr->to_cuda_expr(), w->agg});
    else p.plain.push_back(item->to_cuda_expr());
  }
  size_t next_plain = 0, next_item = p.plain.size();
  for (size_t i = 0; i < m; ++i) p.output.push_back(is_window(ast.select_list[i].get()) ? next_item++ : next_plain++);
  return p;
}

// -------------------------------------------------------- query_sql_joined
const char *const kJoinRightPrefix = "wxr_";

namespace {
// Resolves every column reference of a tree against the two tables and
// rewrites it to the name the execution layer sees: the bare column for the
// left table, kJoinRightPrefix + column for the right one.
struct JoinScope {
  const std::string &left_name;
  const NameSet &left_cols;
  const std::string &right_name;
  const NameSet &right_cols;
  bool left = false, right = false;  // which sides the trees resolved so far name
  bool aggs = false;                 // descend into an aggregate's argument (the grouped join's items)

  void resolve(VariableNode &v) {
    const std::string written = v.name;
    const auto dot = written.find('.');
    bool to_right;
    std::string col = written;
    if (dot != std::string::npos) {
      const std::string q = written.substr(0, dot);
      col = written.substr(dot + 1);
      if (q == left_name && left_cols.count(col)) to_right = false;
      else if (q == right_name && right_cols.count(col)) to_right = true;
      else throw std::runtime_error("Unknown column: " + written);
    } else {
      const bool l = left_cols.count(col) != 0, r = right_cols.count(col) != 0;
      if (l && r) throw std::runtime_error("Ambiguous column: " + written);
      if (!l && !r) throw std::runtime_error("Unknown column: " + written);
      to_right = r;
    }
    v.name = to_right ? kJoinRightPrefix + col : col;
    (to_right ? right : left) = true;
  }
  void resolve(ASTNode *n) {
    if (!n) return;
    if (auto v = dynamic_cast<VariableNode *>(n)) {
      resolve(*v);
    } else if (auto b = dynamic_cast<BinaryOpNode *>(n)) {
      resolve(b->left.get());
      resolve(b->right.get());
    } else if (auto f = dynamic_cast<FunctionCallNode *>(n)) {
      for (auto &a : f->args) resolve(a.get());
    } else if (auto a = aggs ? dynamic_cast<AggregationNode *>(n) : nullptr) {
      resolve(a->expr.get());
    } else if (!dynamic_cast<ConstantNode *>(n)) {
      // an aggregate or a window item inside an expression: its columns would go unresolved
      throw std::runtime_error("aggregates and window functions are not supported inside a joined expression");
    }
  }
};

// the column a bare reference names, without its qualifier
std::string joined_name(const ASTNode *n, size_t pos) {
  if (auto v = dynamic_cast<const VariableNode *>(n)) {
    const auto dot = v->name.find('.');
    return dot == std::string::npos ? v->name : v->name.substr(dot + 1);
  }
  return column_name(n, pos);
}

const char *const kJoinCondition = "JOIN condition must be <left expression> = <right column>";

// The ON condition of a join, <left expression> = <right column> either way
// round: the lowered left key and the right column by its own name.
void lower_on(const std::string &left_name, const NameSet &left_cols, JoinClause &j, const NameSet &right_cols,
              std::string &left_key, std::string &right_key) {
  auto *on = dynamic_cast<BinaryOpNode *>(j.condition.get());
  if (!on || (on->op != "==" && on->op != "=")) throw std::runtime_error(kJoinCondition);
  JoinScope ls{left_name, left_cols, j.table, right_cols}, rs{left_name, left_cols, j.table, right_cols};
  try {
    ls.resolve(on->left.get());
    rs.resolve(on->right.get());
  } catch (const std::exception &e) {
    throw std::runtime_error(std::string("JOIN condition: ") + e.what());
  }
  // which tables each side names: {left table, right table}
  bool key_names[2] = {ls.left, ls.right}, col_names[2] = {rs.left, rs.right};
  ASTNode *key_side = on->left.get(), *col_side = on->right.get();
  if (dynamic_cast<VariableNode *>(on->left.get()) && ls.right && !ls.left && !rs.right) {
    std::swap(key_side, col_side);
    std::swap(key_names, col_names);
  }
  auto *rcol = dynamic_cast<VariableNode *>(col_side);
  if (!rcol || !col_names[1] || col_names[0] || key_names[1]) throw std::runtime_error(kJoinCondition);
  left_key = key_side->to_cuda_expr();
  right_key = rcol->name.substr(std::string(kJoinRightPrefix).size());
}
}  // namespace

bool join_is_left_outer(const std::vector<Token> &tokens, size_t join_index) {
  auto word = [&](size_t p, const char *w) {
    if (tokens[p].type != TokenType::Identifier) return false;
    std::string u = tokens[p].value;
    for (char &ch : u) ch = static_cast<char>(std::toupper(static_cast<unsigned char>(ch)));
    return u == w;
  };
  size_t seen = 0;
  for (size_t i = 0; i < tokens.size(); ++i) {
    if (tokens[i].type != TokenType::Keyword || tokens[i].value != "JOIN" || seen++ != join_index) continue;
    return (i >= 1 && word(i - 1, "LEFT")) || (i >= 2 && word(i - 1, "OUTER") && word(i - 2, "LEFT"));
  }
  return false;
}

JoinedPlan plan_sql_joined(const std::string &sql, const NameSet &left_cols, const std::string &right_name,
                           const NameSet &right_cols) {
  return plan_sql_joined(sql, left_cols,
                         [&](const std::string &name) { return name == right_name ? &right_cols : nullptr; });
}

JoinedPlan plan_sql_joined(const std::string &sql, const NameSet &left_cols, const JoinTables &right_cols_of) {
  std::vector<Token> tokens;
  QueryAST ast;
  try {
    tokens = tokenize(sql);
    ast = parse_query(tokens);
  } catch (const std::exception &e) {
    throw std::runtime_error(std::string("Failed to parse SQL: ") + e.what());
  }
  if (ast.select_list.empty()) throw std::runtime_error("Empty SELECT list");
  if (ast.joins.empty()) throw std::runtime_error("query_sql_joined needs a JOIN clause (use query_sql_table)");
  if (ast.joins.size() > 1) throw std::runtime_error("a second JOIN is not supported by query_sql_joined");
  if (ast.group_by) throw std::runtime_error("GROUP BY is not supported by query_sql_joined");
  if (ast.having) throw std::runtime_error("HAVING is not supported by query_sql_joined");
  if (ast.distinct) throw std::runtime_error("DISTINCT is not supported by query_sql_joined");
  if (ast.order_by) throw std::runtime_error("ORDER BY is not supported by query_sql_joined (the result is in row order)");
  for (const auto &e : ast.select_list)
    if (is_agg(e.get()))
      throw std::runtime_error("aggregates are not supported by query_sql_joined (plain expressions only)");
  for (const auto &e : ast.select_list)
    if (is_window(e.get())) throw std::runtime_error("window functions are not supported by query_sql_joined");
  JoinClause &j = ast.joins[0];
  const NameSet *right = right_cols_of(j.table);
  if (!right) throw std::runtime_error("Unknown table: " + j.table + " (attach it first)");
  const NameSet &right_cols = *right;
  if (ast.select_list.size() > WarpDB::kMaxSelectExprs)
    throw std::runtime_error(kTooManyItems + std::to_string(WarpDB::kMaxSelectExprs) + " expressions");
  JoinedPlan p;
  p.right_table = j.table;
  p.left_outer = join_is_left_outer(tokens, 0);
  lower_on(ast.from_table, left_cols, j, right_cols, p.left_key, p.right_key);
  JoinScope scope{ast.from_table, left_cols, j.table, right_cols};
  for (size_t i = 0; i < ast.select_list.size(); ++i) {
    p.names.push_back(joined_name(ast.select_list[i].get(), i));
    try {
      scope.resolve(ast.select_list[i].get());
    } catch (const std::exception &e) {
      throw std::runtime_error(std::string("SELECT clause: ") + e.what());
    }
    p.lowered.push_back(ast.select_list[i]->to_cuda_expr());
  }
  if (ast.where) {
    try {
      scope.resolve(ast.where->get());
    } catch (const std::exception &e) {
      throw std::runtime_error(std::string("WHERE clause: ") + e.what());
    }
  }
  p.cond = lowered_where(ast);
  p.window = Window(ast);
  return p;
}

JoinedPlan plan_join(const std::string &left_name, const NameSet &left_cols, const std::string &right_name,
                     const NameSet &right_cols, const std::string &left_key, const std::string &right_key,
                     const std::vector<std::string> &exprs, const std::string &where, bool left_outer) {
  if (exprs.empty()) throw std::runtime_error("Empty SELECT list");
  if (exprs.size() > WarpDB::kMaxSelectExprs)
    throw std::runtime_error("query_join takes at most " + std::to_string(WarpDB::kMaxSelectExprs) + " expressions");
  JoinedPlan p;
  p.right_table = right_name;
  p.left_outer = left_outer;
  if (blank(left_key)) throw std::runtime_error("Empty query expression");
  const ASTNodePtr key = parse_plain(left_key);
  JoinScope ks{left_name, left_cols, right_name, right_cols};
  ks.resolve(key.get());
  if (ks.right || is_agg(key.get())) throw std::runtime_error(kJoinCondition);
  p.left_key = key->to_cuda_expr();
  const auto dot = right_key.find('.');
  p.right_key = dot != std::string::npos && right_key.substr(0, dot) == right_name ? right_key.substr(dot + 1) : right_key;
  if (!right_cols.count(p.right_key)) throw std::runtime_error("Unknown column: " + right_key);
  JoinScope scope{left_name, left_cols, right_name, right_cols};
  for (size_t i = 0; i < exprs.size(); ++i) {
    if (blank(exprs[i])) throw std::runtime_error("Empty query expression");
    const ASTNodePtr ex = parse_plain(exprs[i]);
    if (is_agg(ex.get())) throw std::runtime_error("query_join takes plain expressions, not aggregates");
    p.names.push_back(joined_name(ex.get(), i));
    scope.resolve(ex.get());
    p.lowered.push_back(ex->to_cuda_expr());
  }
  if (!blank(where)) {
    try {
      const ASTNodePtr cx = parse_expression(tokenize(where));
      scope.resolve(cx.get());
      p.cond = cx->to_cuda_expr();
    } catch (const std::exception &err) {
      throw std::runtime_error(std::string("Failed to parse WHERE clause: ") + err.what());
    }
  }
  return p;
}

// ------------------------------------------------ query_sql_joined_grouped
JoinedGroupedPlan plan_sql_joined_grouped(const std::string &sql, const NameSet &left_cols,
                                          const std::string &right_name, const NameSet &right_cols) {
  return plan_sql_joined_grouped(sql, left_cols,
                                 [&](const std::string &name) { return name == right_name ? &right_cols : nullptr; });
}

JoinedGroupedPlan plan_sql_joined_grouped(const std::string &sql, const NameSet &left_cols,
                                          const JoinTables &right_cols_of) {
  std::vector<Token> tokens;
  JoinedGroupedPlan out;
  GroupedPlan &p = out.g;
  try {
    tokens = tokenize(sql);
    p.ast = parse_query(tokens);
  } catch (const std::exception &e) {
    throw std::runtime_error(std::string("Failed to parse SQL: ") + e.what());
  }
  QueryAST &ast = p.ast;
  if (ast.select_list.empty()) throw std::runtime_error("Empty SELECT list");
  if (ast.joins.empty())
    throw std::runtime_error("query_sql_joined_grouped needs a JOIN clause (use query_sql_grouped)");
  if (ast.joins.size() > 1) throw std::runtime_error("a second JOIN is not supported by query_sql_joined_grouped");
  if (join_is_left_outer(tokens, 0))
    throw std::runtime_error("LEFT JOIN under GROUP BY is not supported (an unmatched row needs NULL-aware "
                             "aggregates)");
  if (!ast.group_by)
    throw std::runtime_error("query_sql_joined_grouped needs a GROUP BY clause (use query_sql_joined)");
  if (ast.group_by->keys.size() != 1) throw std::runtime_error("GROUP BY supports one key expression");
  if (ast.distinct) throw std::runtime_error("DISTINCT is not supported by query_sql_joined_grouped");
  for (const auto &e : ast.select_list)
    if (is_window(e.get())) throw std::runtime_error("window functions are not supported by query_sql_joined_grouped");
  JoinClause &j = ast.joins[0];
  const NameSet *right = right_cols_of(j.table);
  if (!right) throw std::runtime_error("Unknown table: " + j.table + " (attach it first)");
  const NameSet &right_cols = *right;
  const size_t m = ast.select_list.size();
  if (m > WarpDB::kMaxSelectExprs)
    throw std::runtime_error(kTooManyItems + std::to_string(WarpDB::kMaxSelectExprs) + " expressions");
  out.right_table = j.table;
  lower_on(ast.from_table, left_cols, j, right_cols, out.left_key, out.right_key);
  // every name of every clause to the name the execution layer sees, aggregates' arguments included
  JoinScope scope{ast.from_table, left_cols, j.table, right_cols};
  scope.aggs = true;
  auto resolve = [&](ASTNode *n, const char *clause) {
    try {
      scope.resolve(n);
    } catch (const std::exception &e) {
      throw std::runtime_error(std::string(clause) + e.what());
    }
  };
  for (size_t i = 0; i < m; ++i) {
    p.names.push_back(joined_name(ast.select_list[i].get(), i));
    resolve(ast.select_list[i].get(), "SELECT clause: ");
  }
  if (ast.where) resolve(ast.where->get(), "WHERE clause: ");
  resolve(ast.group_by->keys[0].get(), "GROUP BY clause: ");
  if (ast.having) resolve(ast.having->get(), "HAVING clause: ");
  if (ast.order_by) resolve(ast.order_by->expr.get(), "ORDER BY: ");
  p.cond = lowered_where(ast);
  p.window = Window(ast);
  p.key = ast.group_by->keys[0].get();
  if (is_agg(p.key)) throw std::runtime_error("GROUP BY takes a plain expression, not an aggregate");

  fill_group_slots(p, nullptr);  // the names are resolved already
  return out;
}

}  // namespace warpdb
