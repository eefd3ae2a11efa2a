// sanitize_test.cpp -- host code of the product under AddressSanitizer and
// UndefinedBehaviorSanitizer (no GPU): the expression / SQL front end on
// random token soup and pathological nesting, and the parallel CSV parser
// (csv_parse.cpp) against a sequential std::getline + strto* reading of the
// same text, including blanks, '+', hex, CRLF, blank lines, missing cells;
// the facade's planner (plan.cpp) on the same token soup; the streaming CSV
// chunk reader against one parse of the whole text, refilled every few bytes;
// and warpexec's code generator (codegen.cpp), which parses expression text
// and define lists that come from outside.
// Built by `make -C tests/cpp sanitize_test` with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "warpdb/expression.hpp"
#include "../../warpdb_amd/csrc/warpdb/internal.hpp"
#include "../../warpdb_amd/csrc/warpdb/plan.hpp"
#include "../../warpdb_amd/csrc/warpexec/wx_host.hpp"

static int failures = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      ++failures;                                                  \
    }                                                              \
  } while (0)

// Every planner entry on one SQL text / one expression text: a refusal is a
// std::runtime_error, anything else escapes and ends the program.  A text
// the parser itself refuses gives every entry the same error: one call then.
static int plan_sql_text(const std::string &s, bool parses = true) {
  static const warpdb::NameSet cols{"price", "quantity", "t"};
  int planned = 0;
  auto run = [&](auto &&plan) {
    try {
      plan();
      ++planned;
    } catch (const std::runtime_error &) {
    }
  };
  run([&] { (void)warpdb::plan_sql(s, cols); });
  if (!parses) return planned;
  run([&] { (void)warpdb::plan_sql_table(s, cols); });
  run([&] { (void)warpdb::plan_sql_ordered(s, cols); });
  run([&] { (void)warpdb::plan_multi_gpu_group(s, cols); });
  run([&] { (void)warpdb::plan_multi_gpu_topk(s, cols, 4); });
  run([&] { (void)warpdb::result_column_names(s); });
  return planned;
}

static int lower_expression_text(const std::string &s, bool parses) {
  static const warpdb::NameSet cols{"price", "quantity", "t"};
  int lowered = 0;
  auto run = [&](auto &&lower) {
    try {
      lower();
      ++lowered;
    } catch (const std::runtime_error &) {
    }
  };
  run([&] { (void)warpdb::lower_query(s, cols); });  // (splits at WHERE first: it may accept what the parser refuses)
  if (!parses) return lowered;
  run([&] { (void)warpdb::lower_select_list({"price", s}, cols, "fuzz"); });
  run([&] { (void)warpdb::lower_where(s, cols); });
  run([&] { (void)warpdb::lower_order_by(s, cols); });
  return lowered;
}

static void fuzz_front_end() {
  const char *atoms[] = {"price", "quantity", "1", "2.5", ".5", "10.", "(", ")", "+", "-", "*", "/", ">", "<",
                         ">=", "<=", "==", "!=", "=", "AND", "OR", "discount", ",", "a.b", "SUM", "COUNT", "*",
                         "WHERE", "SELECT", "FROM", "GROUP", "BY", "ORDER", "DESC", "LIMIT", "OFFSET", "HAVING",
                         "DISTINCT", "JOIN", "ON", "t", "99999999999", "@", "\n", " "};
  const int na = sizeof(atoms) / sizeof(atoms[0]);
  std::mt19937 rng(12345);
  int parsed = 0, rejected = 0, planned = 0, lowered = 0;
  for (int it = 0; it < 40000; ++it) {
    std::string s;
    const int len = 1 + static_cast<int>(rng() % 14);
    if (it % 2) s = "SELECT ";
    for (int k = 0; k < len; ++k) s += std::string(atoms[rng() % na]) + (rng() % 3 ? " " : "");
    bool parses = true;
    try {
      if (it % 2) {
        QueryAST q = parse_query(tokenize(s));
        for (auto &e : q.select_list) (void)e->to_cuda_expr();
      } else {
        (void)parse_expression(tokenize(s))->to_cuda_expr();
      }
      ++parsed;
    } catch (const std::runtime_error &) {
      ++rejected;
      parses = false;
    }
    if (it % 2) planned += plan_sql_text(s, parses);
    else lowered += lower_expression_text(s, parses);
  }
  CHECK(parsed > 100 && rejected > 100);
  CHECK(lowered > 100);  // (the token soup rarely gets as far as FROM <table>: the clause soup below does)
  // SQL put together clause by clause, so that most texts parse and every
  // planner takes its later branches; a grouped query_sql plan also runs
  // HAVING and ORDER BY over four hand-made groups
  const char *items[] = {"price", "quantity", "nope", "price * 2", "discount(price, 1)", "SUM(price)", "COUNT(*)",
                         "MIN(price * quantity)", "AVG(nope)", "SUM(price) OVER (PARTITION BY quantity)"};
  const char *conds[] = {"price > 1", "nope > 1", "price > 1 AND quantity < 9"};
  const char *keys[] = {"quantity", "price, quantity", "nope", "quantity + 1"};
  const char *havings[] = {"SUM(price) > 15", "COUNT(*) > 1 OR MIN(price) < 12", "SUM(quantity) > 1", "quantity = 2",
                           "nope > 1"};
  const char *orders[] = {"price", "quantity", "nope", "SUM(price)", "MAX(price)", "price * quantity"};
  const char *counts[] = {"0", "1", "3", "40", "2147483647"};
  auto pick = [&](auto &list) { return std::string(list[rng() % (sizeof(list) / sizeof(list[0]))]); };
  int finished = 0;
  for (int it = 0; it < 5000; ++it) {
    std::string s = rng() % 8 ? "SELECT " : "SELECT DISTINCT ";
    const int n_items = rng() % 50 ? 1 + static_cast<int>(rng() % 3) : 17;
    for (int k = 0; k < n_items; ++k) s += (k ? ", " : "") + pick(items);
    s += " FROM t";
    if (rng() % 10 == 0) s += " JOIN u ON " + pick(conds);
    if (rng() % 2) s += " WHERE " + pick(conds);
    if (rng() % 2) s += " GROUP BY " + pick(keys);
    if (rng() % 4 == 0) s += " HAVING " + pick(havings);
    if (rng() % 2) s += " ORDER BY " + pick(orders) + (rng() % 2 ? " DESC" : "");
    if (rng() % 2) s += " LIMIT " + pick(counts);
    if (rng() % 3 == 0) s += " OFFSET " + pick(counts);
    planned += plan_sql_text(s);
    try {
      const warpdb::SqlPlan p = warpdb::plan_sql(s, warpdb::NameSet{"price", "quantity"});
      if (!p.ast.group_by) continue;
      warpdb::GroupRun run;
      run.keys = {2, 3, 4, 5};
      run.sums = {15.25, 10.5, 20.0, 30.0};
      run.cnts = {1, 1, 1, 1};
      run.mins = run.maxs = {15.25f, 10.5f, 20.0f, 30.0f};
      run.finish(p.ast, p.agg->expr.get(), p.ast.group_by->keys[0].get());
      std::vector<size_t> kept = run.order;
      p.window.apply(kept);
      finished += kept.size() <= 4;
    } catch (const std::runtime_error &) {
    }
  }
    CHECK(planned > 1000 && finished > 100);
  // nesting: a deep nest is an error, not a stack overflow
  for (const char *open : {"(", "f("}) {
    std::string deep;
    for (int i = 0; i < 100000; ++i) deep += open;
    deep += "1";
    bool threw = false;
    try {
      (void)parse_expression(tokenize(deep));
    } catch (const std::runtime_error &e) {
      threw = std::string(e.what()).find("nested too deeply") != std::string::npos;
    }
    CHECK(threw);
  }
  std::string ok = "1";
  for (int i = 0; i < 200; ++i) ok = "(" + ok + " + 1)";
  CHECK(parse_expression(tokenize(ok))->to_cuda_expr().size() > 200);
  bool threw = false;
  try {
    (void)parse_query(tokenize("SELECT price FROM t LIMIT 99999999999"));
  } catch (const std::runtime_error &) {
    threw = true;
  }
  CHECK(threw);
}

// Sequential reading of the same text: std::getline, split on ',', strto*.
static bool sequential(const std::string &text, std::vector<float> &f, std::vector<int32_t> &i,
                       std::vector<double> &d) {
  std::istringstream in(text);
  std::string line;
  while (std::getline(in, line)) {
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty()) continue;
    std::vector<std::string> cells;
    std::stringstream ss(line);
    std::string c;
    while (std::getline(ss, c, ',')) cells.push_back(c);
    if (cells.size() < 3) return false;
    char *end = nullptr;
    const float fv = std::strtof(cells[0].c_str(), &end);
    if (end == cells[0].c_str()) return false;
    const long iv = std::strtol(cells[1].c_str(), &end, 10);
    if (end == cells[1].c_str()) return false;
    const double dv = std::strtod(cells[2].c_str(), &end);
    if (end == cells[2].c_str()) return false;
    f.push_back(fv);
    i.push_back(static_cast<int32_t>(iv));
    d.push_back(dv);
  }
  return true;
}

static HostTable empty_table() {
  HostTable t;
  t.columns.push_back({"a", DataType::Float32, std::vector<float>{}});
  t.columns.push_back({"b", DataType::Int32, std::vector<int32_t>{}});
  t.columns.push_back({"c", DataType::Float64, std::vector<double>{}});
  return t;
}

// CSV text of three numeric columns: blank lines, CRLF, cells only strto* reads
static std::string csv_text(int rows) {
  std::mt19937 rng(777);
  const char *odd_f[] = {" 1.5", "+2", "0x1p3", "1e3", "-0", "nan", "inf", "3.25 ", "1e-50"};
  std::string text;
  for (int r = 0; r < rows; ++r) {
    const unsigned k = rng() % 50;
    if (k == 0) {
      text += (rng() % 2) ? "\n" : "\r\n";  // blank line
      continue;
    }
    char buf[128];
    if (k == 1) std::snprintf(buf, sizeof buf, "%s,%d,%s", odd_f[rng() % 9], static_cast<int>(rng() % 1000) - 500,
                              odd_f[rng() % 9]);
    else std::snprintf(buf, sizeof buf, "%.9g,%d,%.17g", (rng() % 100000) / 7.0, static_cast<int>(rng() % 2000001) - 1000000,
                       (rng() % 1000000) / 3.0);
    text += buf;
    text += (rng() % 5) ? "\n" : "\r\n";
  }
  return text;
}

static void fuzz_csv() {
  const std::string text = csv_text(120000);  // > 2 MiB: several parser ranges
  std::vector<float> rf;
  std::vector<int32_t> ri;
  std::vector<double> rd;
  CHECK(sequential(text, rf, ri, rd));
  for (int threads : {1, 3, 8}) {
    HostTable t = empty_table();
    warpdb::parse_csv_rows(text.data(), text.data() + text.size(), t, threads);
    const auto &f = std::get<std::vector<float>>(t.columns[0].data);
    const auto &i = std::get<std::vector<int32_t>>(t.columns[1].data);
    const auto &d = std::get<std::vector<double>>(t.columns[2].data);
    CHECK(f.size() == rf.size() && i == ri);
    bool same = f.size() == rf.size() && d.size() == rd.size();
    for (size_t r = 0; same && r < f.size(); ++r)
      same = (std::memcmp(&f[r], &rf[r], 4) == 0 || (std::isnan(f[r]) && std::isnan(rf[r]))) &&
             (std::memcmp(&d[r], &rd[r], 8) == 0 || (std::isnan(d[r]) && std::isnan(rd[r])));
    CHECK(same);
  }
  // an unparsable cell is an error (the sequential loader's message), and the
  // table is left as it was
  const std::string bad = text + "1.5,abc,2\n";
  HostTable t = empty_table();
  bool threw = false;
  try {
    warpdb::parse_csv_rows(bad.data(), bad.data() + bad.size(), t, 4);
  } catch (const std::runtime_error &e) {
    threw = std::string(e.what()).find("Invalid numeric value in CSV: 'abc'") != std::string::npos;
  }
  CHECK(threw && t.num_rows() == 0);
  // missing cells and an empty text
  const std::string short_row = "1.5,2\n";
  threw = false;
  try {
    warpdb::parse_csv_rows(short_row.data(), short_row.data() + short_row.size(), t, 2);
  } catch (const std::runtime_error &) {
    threw = true;
  }
  CHECK(threw);
  warpdb::parse_csv_rows(short_row.data(), short_row.data(), t, 2);
  CHECK(t.num_rows() == 0);
}

static bool same_bits(const HostTable &a, const HostTable &b) {
  if (a.columns.size() != b.columns.size()) return false;
  for (size_t c = 0; c < a.columns.size(); ++c) {
    const auto &x = std::get<std::vector<float>>(a.columns[c].data), &y = std::get<std::vector<float>>(b.columns[c].data);
    if (x.size() != y.size() || (!x.empty() && std::memcmp(x.data(), y.data(), 4 * x.size()) != 0)) return false;
  }
  return true;
}

// The streaming chunk reader (query_multi_gpu_csv's parser thread) against
// one parse of the whole text: every chunk but the last holds rows_per_chunk
// rows, none is empty, and together they are the text's rows.  Blocks of 1
// and 7 bytes put a refill inside a line, on a '\r', on a '\n' and at the end.
static void csv_chunks() {
  const std::vector<std::string> names{"a", "b", "c"};
  auto float_table = [&] {
    HostTable t;
    for (const auto &n : names) t.columns.push_back({n, DataType::Float32, std::vector<float>{}});
    return t;
  };
  std::string text = csv_text(1500);
  while (!text.empty() && (text.back() == '\n' || text.back() == '\r')) text.pop_back();  // no newline after the last line
  HostTable whole = float_table();
  warpdb::parse_csv_rows(text.data(), text.data() + text.size(), whole, 1);
  const int64_t rows = whole.num_rows();
  CHECK(rows > 1400 && rows < 1500);  // some of the 1500 lines are blank
  for (int64_t rpc : {int64_t(1), int64_t(3), rows, rows + 1}) {
    for (size_t block : {size_t(1), size_t(7), size_t(4096)}) {
      std::istringstream in(text);
      warpdb::CsvChunkReader reader(in, names, rpc, block);
      HostTable all = float_table(), chunk;
      bool sized = true;
      int64_t last = rpc;
      while (reader.next(chunk)) {
        sized = sized && last == rpc && chunk.num_rows() > 0 && chunk.num_rows() <= rpc &&
                chunk.columns.size() == names.size();
        last = chunk.num_rows();
        for (size_t c = 0; sized && c < names.size(); ++c) {
          const auto &v = std::get<std::vector<float>>(chunk.columns[c].data);
          auto &dst = std::get<std::vector<float>>(all.columns[c].data);
          dst.insert(dst.end(), v.begin(), v.end());
        }
      }
      CHECK(sized && same_bits(all, whole));
      CHECK(!reader.next(chunk));  // exhausted stays exhausted
    }
  }
  for (const char *blank_only : {"", "\n", "\r\n", "\n\r\n\n\r\n"}) {
    for (size_t block : {size_t(1), size_t(7), size_t(4096)}) {
      std::istringstream in(blank_only);
      warpdb::CsvChunkReader reader(in, names, 2, block);
      HostTable chunk;
      CHECK(!reader.next(chunk));
    }
  }
  // a bad cell is the parser's error, from whichever chunk holds it
  std::istringstream bad("1,2,3\n4,x,6\n");
  warpdb::CsvChunkReader reader(bad, names, 1, 7);
  HostTable chunk;
  CHECK(reader.next(chunk) && chunk.num_rows() == 1);
  bool threw = false;
  try {
    (void)reader.next(chunk);
  } catch (const std::runtime_error &e) {
    threw = std::string(e.what()).find("Invalid numeric value in CSV: 'x'") != std::string::npos;
  }
  CHECK(threw);
}

static std::vector<std::string> identifiers(const char *s) {
  std::vector<std::string> ids;
  wx::scan_identifiers(s, ids);
  return ids;
}

static bool rejects(const wx_table &t, const char *expr, wx_status st) {
  try {
    (void)wx::used_columns(&t, {expr});
  } catch (const wx::WxError &e) {
    return e.st == st;
  }
  return false;
}

// warpexec's code generator on the edges of its text parsing (no HIP call:
// codegen.cpp is compiled into this program as it is into libwarpexec.so)
static void codegen_text() {
  using V = std::vector<std::string>;
  CHECK(identifiers(nullptr).empty() && identifiers("").empty() && identifiers(" \t(+)").empty());
  CHECK(identifiers("price") == V{"price"});                     // an identifier ends the string
  CHECK(identifiers("f (x) + g\t(y[idx]) + h ") == (V{"x", "y", "idx", "h"}));  // blanks before '(': a call
  CHECK(identifiers("1e5f + 10.0f*a_1 - .5 + 0x1F + 7") == V{"a_1"});  // literals and their suffixes
  CHECK(identifiers("_x1e5(") .empty() && identifiers("9") .empty());

  float cell = 0;
  const wx_col cols[] = {{"price", WX_FLOAT32, &cell}, {nullptr, WX_FLOAT32, &cell}, {"note", WX_STRING, &cell},
                         {"qty", WX_INT64, nullptr}};
  const wx_table t{1, 4, cols}, none{0, 0, nullptr};
  CHECK(wx::used_columns(&none, {}).empty() && wx::used_columns(&none, {nullptr, "", "price[idx]"}).empty());
  const auto used = wx::used_columns(&t, {"price(1) + price[idx]", nullptr, "note(2)"});
  CHECK(used.size() == 1 && used[0].name == "price" && std::string(used[0].ctype) == "float" &&
        used[0].table_index == 0);
  CHECK(rejects(t, "note[idx]", WX_ERR_UNSUPPORTED));  // a string column
  CHECK(rejects(t, "qty[idx]", WX_ERR_INVALID));       // no device pointer
  std::vector<std::string> names;
  std::vector<wx_col> many;
  std::string all;
  for (int i = 0; i < WX_MAX_COLS + 1; ++i) names.push_back("c" + std::to_string(i));
  for (auto &n : names) {
    many.push_back({n.c_str(), WX_INT32, &cell});
    all += n + "[idx] ";
  }
  CHECK(rejects(wx_table{1, (int32_t)many.size(), many.data()}, all.c_str(), WX_ERR_UNSUPPORTED));

  CHECK(wx::define_value("", "A", 7) == 7 && wx::define_value("A", "A", 7) == 7 && wx::define_value("AB=5", "A", 7) == 7);
  CHECK(wx::define_value("A=", "A", 7) == 0 && wx::define_value("A=x", "A", 7) == 0 && wx::define_value("=3", "", 7) == 3);
  CHECK(wx::define_value(",,A=3,,", "A", 7) == 3 && wx::define_value("A=3,B,A=4,", "A", 7) == 4);

  wx::Spec spec;
  spec.op = WX_OP_UTIL;
  spec.extra = ",,A=1,,B,=3,C=,";  // empty items, an empty name, an empty value
  const std::string src = spec.source();
  CHECK(src.find("#define A 1\n#define B 1\n#define  3\n#define C \n") != std::string::npos);
  CHECK(src.find("#define WX_DIAG 1") == std::string::npos && src.find("wx_util.hip") != std::string::npos);
  spec.extra = "WX_GP_DIAG";
  CHECK(spec.source().find("#define WX_DIAG 1\n#define WX_GP_DIAG 1\n") != std::string::npos);
  CHECK(spec.key_string().find("|x=WX_GP_DIAG|") != std::string::npos);
}

int main() {
  fuzz_front_end();
  fuzz_csv();
  csv_chunks();
  codegen_text();
  if (failures) return 1;
  std::printf("sanitize_test: all passed\n");
  return 0;
}
