// wx_join_group_args.h -- argument block and geometry of the JOIN under
// GROUP BY (wx_join_group.hip).  Shared by the host runtime and the device
// templates like wx_args.h; wx_group_multi_args.h (WxGroupMultiArgs,
// WX_GM_LDS_BYTES) and wx_join_args.h (the forms, WX_JOIN_TABLE_BYTES) must
// come first.  Plain C++ only.
#ifndef WX_JOIN_GROUP_ARGS_H
#define WX_JOIN_GROUP_ARGS_H

// after wx_join_args.h's WX_OP_JOIN_TABLE 9.  The prelude of such a module
// also defines WX_JOIN_GROUP, which the sources shared with other families
// (wx_group_multi.hip, wx_join.hip) test: they come before this header in a
// module's text.
#define WX_OP_JOIN_GROUP 10

// The workgroup of wx_join_group.  The LDS holds wx_group_multi's window,
// WX_GROUP_WINDOW x (4 + 8 (s + q)) bytes for s summed and q MIN / MAX values,
// and in the direct form the 16 KiB rows[] table beside it:
//   direct, s + q <= 3: at most 73 728 B, two workgroups of 512 threads per CU
//                       (s + q = 4 would take 2 x 88 KiB);
//   hash,   s + q <= 4: at most 73 728 B, likewise;
//   above (up to 155 648 B at s = q = 4, direct): one workgroup of 1024 threads.
// Either way a CU holds 16 waves.
#define WX_JG_LDS_LIMIT (160 * 1024)
#define WX_JG_LDS_BYTES(s, q, form) \
  (WX_GM_LDS_BYTES(s, q) + ((form) == WX_JOIN_FORM_DIRECT ? WX_JOIN_TABLE_BYTES : 0))
#define WX_JG_PER_CU(s, q, form) (((s) + (q)) <= ((form) == WX_JOIN_FORM_DIRECT ? 3 : 4) ? 2 : 1)
#define WX_JG_BLOCK(s, q, form) (WX_JG_PER_CU(s, q, form) == 2 ? 512 : 1024)

// The left table's columns, the row count and every accumulator are
// wx_group_multi's block (g.key_lo is the key window's start; g.ctrs the group
// counters); the rest is the probe's, under the names wx_join.hip's lookup
// text reads: c.ctrs the workspace counters ([1] error bits), key_lo / span
// the direct table's range, mask / shift the hash table's.
struct WxJoinGroupArgs {
  WxGroupMultiArgs g;
  struct {
    wx_u64 *ctrs;
  } c;
  const void *rcol[WX_MAX_COLS];  // the referenced right columns (WX_RCOLS slots)
  const int *rows;                // direct form: [WX_JOIN_DIRECT_BINS]
  const wx_u64 *slots;            // hash form: [mask + 1]
  int key_lo;
  wx_u32 span;
  wx_u32 mask;
  int shift;
};

#endif  // WX_JOIN_GROUP_ARGS_H
