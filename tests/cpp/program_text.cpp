// program_text.cpp -- prints the program text of a module that the C ABI does
// not hand out: `select N` (N expressions), `window P W [search]` (one launch
// of P plain outputs followed by W window items), `group_multi N SUMS MMS`
// (N values with these masks) or `join_group N SUMS MMS [direct|hash [left]]`
// (the same under a join; `left`: the WHERE names no right column) over a
// table of price f32, quantity i32 (the right table: id i32, rate f32).  No GPU and no HIP call:
// codegen.cpp is compiled into this program as it is into libwarpexec.so.
// Build: make -C tests/cpp bin/program_text (tests/test_select_multi_abi.py,
// tests/test_window_host.py and tests/test_group_multi_host.py read its
// output).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../warpdb_amd/csrc/warpexec/wx_host.hpp"

int main(int argc, char **argv) {
  const std::string kind = argc > 1 ? argv[1] : "";
  const int a = argc > 2 ? std::atoi(argv[2]) : 0, b = argc > 3 ? std::atoi(argv[3]) : 0;
  float cell = 0;
  const wx_col cols[] = {{"price", WX_FLOAT32, &cell}, {"quantity", WX_INT32, &cell}};
  const wx_table t{1 << 20, 2, cols};
  wx_launch L = wx::default_launch();
  L.flags = WX_F_NO_CUSTOM;
  const char *plain[] = {"price[idx]", "(price[idx] * 2.0f)", "(float)quantity[idx]", "(price[idx] + 1.0f)"};
  const char *cond = "(price[idx] > 15.0f)";
  try {
    wx::Spec spec;
    if (kind == "select" && a >= 2 && a <= 4) {
      spec = wx::select_spec(&t, plain, a, cond, L);
    } else if (kind == "window" && a >= 0 && b >= 1 && a + b <= 4) {
      std::vector<const char *> exprs(plain, plain + a);
      exprs.resize(a + b, nullptr);
      spec = wx::window_spec(&t, exprs.data(), a + b, ((1 << b) - 1) << a, argc > 4, "quantity[idx]", cond, L);
    } else if (kind == "group_multi" && a >= 2 && a <= 4) {
      spec = wx::group_multi_spec(&t, plain, a, b, argc > 4 ? std::atoi(argv[4]) : 0, "quantity[idx]", cond, L);
    } else if (kind == "join_group" && a >= 1 && a <= 4) {
      const wx_col rcols[] = {{"id", WX_INT32, &cell}, {"rate", WX_FLOAT32, &cell}};
      const wx_table r{1 << 10, 2, rcols};
      spec = wx::join_group_spec(&t, &r, plain, a, b, argc > 4 ? std::atoi(argv[4]) : 0,
                                 argc > 5 && std::string(argv[5]) == "direct" ? WX_JOIN_FORM_DIRECT : WX_JOIN_FORM_HASH,
                                 "quantity[idx]", "quantity[idx]", argc > 6 ? cond : "(price[idx] > rate[idx])", L);
    } else {
      std::fprintf(stderr,
                   "usage: program_text select N | window P W [search] | group_multi N SUMS MMS | "
                   "join_group N SUMS MMS [direct|hash [left]]\n");
      return 2;
    }
    std::fputs(spec.source().c_str(), stdout);
  } catch (const wx::WxError &e) {
    std::fprintf(stderr, "program_text: %s\n", e.msg.c_str());
    return 1;
  }
  return 0;
}
