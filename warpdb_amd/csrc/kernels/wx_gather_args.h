// wx_gather_args.h -- argument block of the multi-output row gather
// (wx_gather.hip).  Shared by the host runtime and the device templates like
// wx_args.h, which must come first (WX_MAX_COLS, wx_i64).  Plain C++ only.
#ifndef WX_GATHER_ARGS_H
#define WX_GATHER_ARGS_H

#define WX_OP_GATHER 6  // after wx_args.h's WX_OP_UTIL 5

#define WX_GATHER_MAX_OUT 4  // WX_MAX_OUTPUTS of include/warpexec.h

// Gather geometry: a thread owns WX_GATHER_UNROLL quads of 4 consecutive
// output positions per workgroup iteration and issues all their column loads
// before the first use (profiles/select_ordered_geometry.txt).  The host
// passes its choice; the diagnostic define list may override it.
#ifndef WX_GATHER_BLOCK
#define WX_GATHER_BLOCK 256
#endif
#ifndef WX_GATHER_UNROLL
#define WX_GATHER_UNROLL 2
#endif
#define WX_GATHER_TILE (WX_GATHER_BLOCK * 4 * WX_GATHER_UNROLL)  // positions per workgroup iteration

struct WxGatherArgs {
  const void *col[WX_MAX_COLS];
  const void *rows;        // [count] row ids, int32 or int64 (idx64)
  const wx_i64 *d_count;   // nullable: the count is min(count, *d_count)
  float *out_val[WX_GATHER_MAX_OUT];  // each nullable; [j][k] = static_cast<float>(expression j) at row k
  wx_i64 *out_rows;        // nullable; [k] = out_row_base + row
  wx_i64 count;
  wx_i64 n_rows;
  wx_i64 row_base;         // row = rows[k] - row_base
  wx_i64 out_row_base;
  int idx64;
};

#endif  // WX_GATHER_ARGS_H
