// wx_group_multi_args.h -- argument blocks and geometry of the multi-value
// GROUP BY (wx_group_multi.hip).  Shared by the host runtime and the device
// templates like wx_args.h, which must come first (WX_MAX_COLS, wx_u64,
// WX_GROUP_WINDOW).  Plain C++ only.  It lives beside wx_args.h rather than in
// it so the text every other module is built from -- and with it their cached
// code objects -- stays what it was.
#ifndef WX_GROUP_MULTI_ARGS_H
#define WX_GROUP_MULTI_ARGS_H

#define WX_OP_GROUP_MULTI 7  // after wx_gather_args.h's WX_OP_GATHER 6

#define WX_GM_MAX 4  // WX_GROUP_MAX_VALUES of include/warpexec.h

// The workgroup of wx_group_multi (host and device agree through this header,
// as they do through WX_GBLOCK for wx_group_sum).  A window bin holds one u32
// count, one double per summed value (s of them) and two order-mapped u32 per
// MIN / MAX value (q of them): WX_GROUP_WINDOW x (4 + 8 s + 8 q) bytes.
//   s + q <= 4: at most 73 728 B, two workgroups of 512 threads per CU;
//   above (up to 139 264 B at s = q = 4): one workgroup of 1024 threads.
// Either way a CU holds 16 waves.
#define WX_GM_LDS_BYTES(s, q) (WX_GROUP_WINDOW * (4 + 8 * ((s) + (q))))
#define WX_GM_BLOCK(s, q) (((s) + (q)) <= 4 ? 512 : 1024)
#define WX_GM_PER_CU(s, q) (((s) + (q)) <= 4 ? 2 : 1)

// Accumulators.  The count window, the general-key table's tags, counts and
// used list and the counter words are wx_group_sum's own (WxGroupArgs); the
// value planes are this family's: plane p of the summed values is the p-th
// set bit of the sum mask, likewise for MIN / MAX.  Idle values (restored by
// wx_group_multi_finalize): sums and counts 0, tags 0, minima ~0, maxima 0.
struct WxGroupPlanes {
  wx_u64 *win_cnt;  // [WX_GROUP_WINDOW]
  double *win_sum;  // [s][WX_GROUP_WINDOW]
  wx_u32 *win_min;  // [q][WX_GROUP_WINDOW] order-mapped, ~0 = none
  wx_u32 *win_max;  // [q][WX_GROUP_WINDOW] order-mapped, 0 = none
  wx_u64 *h_tag;    // [hcap] 0 = empty, else (u32)key | 1<<32
  wx_u64 *h_cnt;    // [hcap]
  wx_u32 *h_used;   // [hcap] slots taken, in insertion order
  double *h_sum;    // [s][hcap]
  wx_u32 *h_min;    // [q][hcap]
  wx_u32 *h_max;    // [q][hcap]
  wx_u64 *ctrs;     // [0] used slots, [1] error bits
  wx_u32 hmask;     // hcap - 1 (hcap a power of two)
  int key_lo;       // the window's first key
};

struct WxGroupMultiArgs {
  const void *col[WX_MAX_COLS];
  wx_i64 n_rows;
  WxGroupPlanes acc;
};

struct WxGroupMultiFinArgs {
  WxGroupPlanes acc;
  const wx_u64 *sorted;  // nullable: general-key entries pre-sorted on the device (> WX_GROUP_HSORT_MAX)
  int *out_keys;
  wx_i64 *out_counts;
  double *out_sums[WX_GM_MAX];  // by value; null where the value carries no SUM
  float *out_mins[WX_GM_MAX];   // by value; each nullable
  float *out_maxs[WX_GM_MAX];
  wx_i64 *n_groups_out;
  wx_i64 capacity;
};

#endif  // WX_GROUP_MULTI_ARGS_H
