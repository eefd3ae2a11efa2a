// optimizer.cpp -- statistics pushdown (reference: src/optimizer.cpp, whose
// analyze_condition() at :13-17 leaves both verdicts false).
//
// The WHERE tree is evaluated over intervals: every column contributes the
// range of its values as the kernel sees them (float conversion; integer
// arithmetic kept integer as in C), constants their float literal, and
// arithmetic widens outward by one double ulp per step and rounds outward to
// float, so the verdict holds for the float computation the kernel performs.
// NaN is tracked separately: comparisons with NaN are false (so a column
// holding NaN can never make `x > c` always true), `!=` with NaN is true, and
// a bare numeric condition is true for NaN (C++ truthiness, the kernel's
// static_cast<bool>).
#include "warpdb/optimizer.hpp"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <iostream>
#include <limits>
#include <set>
#include <stdexcept>

#include "internal.hpp"
#include "warpexec.h"

namespace warpdb {
namespace {

constexpr double kInf = std::numeric_limits<double>::infinity();

struct Iv {
  bool known = false;  // bounds valid
  double lo = -kInf, hi = kInf;
  bool nan = true;     // a row may evaluate to NaN
  bool is_int = false;
};

Iv unknown() { return Iv{}; }

Iv point(double v, bool is_int) {
  Iv r;
  r.known = true;
  r.lo = r.hi = v;
  r.nan = false;
  r.is_int = is_int;
  return r;
}

// outward rounding of a double bound to the float the kernel would produce
double down_f(double v) {
  if (std::isinf(v)) return v;
  v = std::nextafter(v, -kInf);
  float f = static_cast<float>(v);
  if (static_cast<double>(f) > v) f = std::nextafter(f, -std::numeric_limits<float>::infinity());
  return f;
}
double up_f(double v) {
  if (std::isinf(v)) return v;
  v = std::nextafter(v, kInf);
  float f = static_cast<float>(v);
  if (static_cast<double>(f) < v) f = std::nextafter(f, std::numeric_limits<float>::infinity());
  return f;
}

Iv arith(const std::string &op, const Iv &a, const Iv &b) {
  if (!a.known || !b.known) return unknown();
  Iv r;
  r.known = true;
  r.is_int = a.is_int && b.is_int;
  r.nan = a.nan || b.nan;
  double c[4];
  if (op == "/") {
    if (b.lo <= 0.0 && b.hi >= 0.0) return unknown();  // division by a range holding 0
    c[0] = a.lo / b.lo, c[1] = a.lo / b.hi, c[2] = a.hi / b.lo, c[3] = a.hi / b.hi;
    if (r.is_int)
      for (double &x : c) x = std::trunc(x);  // C integer division
  } else if (op == "*") {
    c[0] = a.lo * b.lo, c[1] = a.lo * b.hi, c[2] = a.hi * b.lo, c[3] = a.hi * b.hi;
  } else if (op == "+") {
    c[0] = c[1] = a.lo + b.lo, c[2] = c[3] = a.hi + b.hi;
  } else if (op == "-") {
    c[0] = c[1] = a.lo - b.hi, c[2] = c[3] = a.hi - b.lo;
  } else {
    return unknown();
  }
  for (double x : c)
    if (std::isnan(x)) return unknown();  // inf - inf, 0 * inf
  r.lo = *std::min_element(c, c + 4);
  r.hi = *std::max_element(c, c + 4);
  if (std::isinf(r.lo) || std::isinf(r.hi)) r.nan = true;  // inf may meet inf later
  if (r.is_int) {
    if (r.lo < -2147483648.0 || r.hi > 2147483647.0) return unknown();  // int overflow
  } else {
    r.lo = down_f(r.lo);
    r.hi = up_f(r.hi);
  }
  return r;
}

Verdict compare(const std::string &op, const Iv &a, const Iv &b) {
  if (!a.known || !b.known) return Verdict::Unknown;
  const bool nan = a.nan || b.nan;
  bool at = false, af = false;
  if (op == ">") {
    at = a.lo > b.hi;
    af = a.hi <= b.lo;
  } else if (op == ">=") {
    at = a.lo >= b.hi;
    af = a.hi < b.lo;
  } else if (op == "<") {
    at = a.hi < b.lo;
    af = a.lo >= b.hi;
  } else if (op == "<=") {
    at = a.hi <= b.lo;
    af = a.lo > b.hi;
  } else if (op == "==") {
    at = a.lo == a.hi && b.lo == b.hi && a.lo == b.lo;
    af = a.hi < b.lo || b.hi < a.lo;
  } else if (op == "!=") {
    // NaN != x is true: it can only spoil "always false"
    const bool disjoint = a.hi < b.lo || b.hi < a.lo;
    const bool same = a.lo == a.hi && b.lo == b.hi && a.lo == b.lo;
    if (disjoint) return Verdict::AlwaysTrue;
    if (same && !nan) return Verdict::AlwaysFalse;
    return Verdict::Unknown;
  } else {
    return Verdict::Unknown;
  }
  if (at && !nan) return Verdict::AlwaysTrue;
  if (af) return Verdict::AlwaysFalse;
  return Verdict::Unknown;
}

bool is_cmp(const std::string &op) {
  return op == ">" || op == ">=" || op == "<" || op == "<=" || op == "==" || op == "!=";
}

Verdict verdict_of(const ASTNode *n, const StatsMap &st);

Iv bool_iv(Verdict v) {
  if (v == Verdict::AlwaysTrue) return point(1.0, true);
  if (v == Verdict::AlwaysFalse) return point(0.0, true);
  Iv r = point(0.0, true);
  r.hi = 1.0;
  return r;
}

Iv interval(const ASTNode *n, const StatsMap &st) {
  if (auto c = dynamic_cast<const ConstantNode *>(n)) {
    try {
      return point(static_cast<double>(std::stof(c->value)), false);  // lowered as a float literal
    } catch (...) {
      return unknown();
    }
  }
  if (auto v = dynamic_cast<const VariableNode *>(n)) {
    auto it = st.find(v->name);
    if (it == st.end() || !it->second.known) return unknown();
    Iv r;
    r.known = true;
    r.lo = it->second.min;
    r.hi = it->second.max;
    r.nan = it->second.null_count > 0;
    r.is_int = it->second.is_int;
    return r;
  }
  if (auto b = dynamic_cast<const BinaryOpNode *>(n)) {
    if (is_cmp(b->op) || b->op == "&&" || b->op == "||") return bool_iv(verdict_of(n, st));
    return arith(b->op, interval(b->left.get(), st), interval(b->right.get(), st));
  }
  return unknown();  // function calls (custom.cu), aggregates
}

Verdict verdict_of(const ASTNode *n, const StatsMap &st) {
  if (auto b = dynamic_cast<const BinaryOpNode *>(n)) {
    if (b->op == "&&" || b->op == "||") {
      const Verdict l = verdict_of(b->left.get(), st), r = verdict_of(b->right.get(), st);
      if (b->op == "&&") {
        if (l == Verdict::AlwaysFalse || r == Verdict::AlwaysFalse) return Verdict::AlwaysFalse;
        if (l == Verdict::AlwaysTrue && r == Verdict::AlwaysTrue) return Verdict::AlwaysTrue;
      } else {
        if (l == Verdict::AlwaysTrue || r == Verdict::AlwaysTrue) return Verdict::AlwaysTrue;
        if (l == Verdict::AlwaysFalse && r == Verdict::AlwaysFalse) return Verdict::AlwaysFalse;
      }
      return Verdict::Unknown;
    }
    if (is_cmp(b->op)) return compare(b->op, interval(b->left.get(), st), interval(b->right.get(), st));
  }
  // a numeric condition: true where the value is non-zero (NaN included)
  const Iv v = interval(n, st);
  if (!v.known) return Verdict::Unknown;
  if (v.lo > 0.0 || v.hi < 0.0) return Verdict::AlwaysTrue;
  if (v.lo == 0.0 && v.hi == 0.0 && !v.nan) return Verdict::AlwaysFalse;
  return Verdict::Unknown;
}

void collect(const ASTNode *n, std::set<std::string> &out) {
  if (!n) return;
  if (auto v = dynamic_cast<const VariableNode *>(n)) out.insert(v->name);
  if (auto b = dynamic_cast<const BinaryOpNode *>(n)) {
    collect(b->left.get(), out);
    collect(b->right.get(), out);
  }
  if (auto f = dynamic_cast<const FunctionCallNode *>(n))
    for (const auto &a : f->args) collect(a.get(), out);
  if (auto a = dynamic_cast<const AggregationNode *>(n)) collect(a->expr.get(), out);
}

}  // namespace

const char *verdict_name(Verdict v) {
  switch (v) {
    case Verdict::AlwaysTrue: return "always_true";
    case Verdict::AlwaysFalse: return "always_false";
    default: return "unknown";
  }
}

std::vector<std::string> referenced_columns(const ASTNode *n) {
  std::set<std::string> s;
  collect(n, s);
  return {s.begin(), s.end()};
}

Verdict analyze_condition(const ASTNode *cond, const StatsMap &stats) {
  if (!cond) return Verdict::AlwaysTrue;
  return verdict_of(cond, stats);
}

StatsMap compute_column_stats(const Table &table, const std::vector<std::string> &names) {
  StatsMap out;
  WxTableView v(table);
  wx_launch L = sync_launch(table.device);
  for (const auto &c : table.columns) {
    if (!names.empty() && std::find(names.begin(), names.end(), c.name) == names.end()) continue;
    ColumnRange r;
    r.is_int = c.type == DataType::Int32 || c.type == DataType::Int64;
    if (c.type == DataType::Float64 || c.type == DataType::String || table.num_rows == 0) {
      out[c.name] = r;  // not bounded (Float64 compares in double; the stats are float)
      continue;
    }
    const std::string e = c.name + "[idx]";
    const std::string not_nan = "(" + e + " == " + e + ")";
    wx_stats st{};
    wx_call(wx_reduce_stats, &v.table, e.c_str(), r.is_int ? "" : not_nan.c_str(), &L, nullptr, &st);
    r.null_count = table.num_rows - st.count;
    if (st.min == st.min && st.max == st.max) {
      r.min = st.min;
      r.max = st.max;
      // integers beyond 2^24 do not survive the float conversion exactly
      r.known = !r.is_int || std::max(std::fabs(r.min), std::fabs(r.max)) <= 16777216.0;
    }
    out[c.name] = r;
  }
  return out;
}

TableStats to_table_stats(const StatsMap &stats) {
  TableStats t;
  auto p = stats.find("price");
  if (p != stats.end() && p->second.known) {
    t.price.min = static_cast<float>(p->second.min);
    t.price.max = static_cast<float>(p->second.max);
    t.price.null_count = static_cast<int>(p->second.null_count);
  }
  auto q = stats.find("quantity");
  if (q != stats.end() && q->second.known) {
    t.quantity.min = static_cast<int>(q->second.min);
    t.quantity.max = static_cast<int>(q->second.max);
    t.quantity.null_count = static_cast<int>(q->second.null_count);
  }
  return t;
}

std::vector<float> query_optimized(const std::string &expr_part, const std::string &where_part, const Table &table,
                                   const StatsMap *stats, Verdict *verdict_out) {
  auto expr_ast = parse_expression(tokenize(expr_part));
  ASTNodePtr cond_ast;
  if (!where_part.empty()) cond_ast = parse_expression(tokenize(where_part));
  Verdict verdict = Verdict::AlwaysTrue;
  if (cond_ast) {
    StatsMap local;
    if (!stats) {
      local = compute_column_stats(table, referenced_columns(cond_ast.get()));
      stats = &local;
    }
    verdict = analyze_condition(cond_ast.get(), *stats);
  }
  if (verdict_out) *verdict_out = verdict;
  const int64_t n = table.num_rows;
  if (verdict == Verdict::AlwaysFalse) return std::vector<float>(static_cast<size_t>(n), 0.0f);
  const std::string expr = expr_ast->to_cuda_expr();
  const std::string cond = (cond_ast && verdict != Verdict::AlwaysTrue) ? cond_ast->to_cuda_expr() : std::string();
  WxTableView v(table);
  wx_launch L = sync_launch(table.device);
  DeviceBuffer out(table.device, sizeof(float) * static_cast<size_t>(n));
  wx_call(wx_project_filter, &v.table, expr.c_str(), cond.c_str(), &L, WX_MODE_DENSE_FILL,
          static_cast<float *>(out.ptr), nullptr, 0, 0, nullptr, nullptr);
  std::vector<float> h = host_result(static_cast<size_t>(n));
  if (n) {
    DevGuard g(table.device);
    copy_d2h(table.device, nullptr, h.data(), out.ptr, sizeof(float) * static_cast<size_t>(n));
  }
  return h;
}

}  // namespace warpdb

void analyze_condition(const ASTNode *cond, const TableStats &stats, bool &always_true, bool &always_false) {
  warpdb::StatsMap m;
  warpdb::ColumnRange p, q;
  p.known = true;
  p.min = stats.price.min;
  p.max = stats.price.max;
  p.null_count = stats.price.null_count;
  q.known = true;
  q.is_int = true;
  q.min = stats.quantity.min;
  q.max = stats.quantity.max;
  q.null_count = stats.quantity.null_count;
  m["price"] = p;
  m["quantity"] = q;
  const warpdb::Verdict v = warpdb::analyze_condition(cond, m);
  always_true = v == warpdb::Verdict::AlwaysTrue;
  always_false = v == warpdb::Verdict::AlwaysFalse;
}

void execute_query_optimized(const std::string &expr_part, const std::string &where_part, Table &table) {
  warpdb::Verdict v = warpdb::Verdict::Unknown;
  const std::vector<float> r = warpdb::query_optimized(expr_part, where_part, table, nullptr, &v);
  if (v == warpdb::Verdict::AlwaysFalse) {
    std::cout << "[Optimizer] Filter eliminates all rows.\n";
    return;
  }
  for (size_t i = 0; i < r.size(); ++i) std::cout << "Result[" << i << "] = " << r[i] << "\n";
}
