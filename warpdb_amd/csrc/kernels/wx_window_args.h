// wx_window_args.h -- argument blocks of the window-aggregate broadcast
// (wx_window.hip).  Shared by the host runtime and the device templates like
// wx_args.h and wx_select_args.h, which must come first (WxCompactArgs,
// WX_SELECT_MAX_OUT, WX_SELECT_LDS_BUDGET).  Plain C++ only.
#ifndef WX_WINDOW_ARGS_H
#define WX_WINDOW_ARGS_H

#define WX_OP_WINDOW_TABLE 8  // after wx_group_multi_args.h's WX_OP_GROUP_MULTI 7: wx_window_range + wx_window_table
#define WX_WIN_BINS 2048      // dense form: most keys of a partition table (WX_GROUP_WINDOW_BINS)
#define WX_WIN_MAX_ITEMS 16   // window items of one call (WX_ORDERED_MAX_EXPRS)
#define WX_WIN_MAX_VALUES 4   // distinct value expressions of one call (WX_GROUP_MAX_VALUES)
#define WX_WIN_TBLOCK 1024    // wx_window_table workgroup size
// aggregate of a window item: the numbering of WX_WIN_* in include/warpexec.h
#define WX_WAGG_SUM 0
#define WX_WAGG_AVG 1
#define WX_WAGG_COUNT 2
#define WX_WAGG_MIN 3
#define WX_WAGG_MAX 4

// The dense form keeps one 2048-entry f32 plane per window item of the
// launch in LDS, beside the two stage buffers of the compaction: what is
// left of WX_SELECT_LDS_BUDGET decides the tile (WX_SELECT_ROW_BYTES).
#define WX_WIN_TABLE_BYTES(n_items) ((n_items) * WX_WIN_BINS * 4)

// One launch of the broadcast compaction: up to WX_SELECT_MAX_OUT outputs,
// each a plain expression or a window item (bit j of the module's
// WX_WIN_MASK).  A window output j reads plane[j]: WX_WIN_BINS entries
// indexed by key - key_lo (dense form), or n_groups entries beside the
// sorted keys (search form).  Every lookup is clamped: a key outside
// [key_lo, key_lo + span), or one the search does not find, reads nothing
// outside the table and yields NaN.
struct WxWindowArgs {
  WxCompactArgs c;  // columns, row ids, status words, counters, count: as the single-output kernel (out_val unused)
  float *out_val[WX_SELECT_MAX_OUT];        // each nullable
  const float *plane[WX_SELECT_MAX_OUT];    // null for a plain output
  const int *keys;   // search form: the partitions' keys, ascending, [n_groups] (at least one entry allocated)
  int key_lo;        // dense form
  wx_u32 span;       // dense form: keys lie in [key_lo, key_lo + span), span <= WX_WIN_BINS
  wx_u32 n_groups;   // search form
};

// wx_window_range: {group count, first key | last key << 32} of the group pass, 16 bytes
struct WxWindowRangeArgs {
  const wx_i64 *n_groups;
  const int *keys;   // [capacity]
  wx_i64 capacity;
  wx_i64 *out;       // [2]
};

// wx_window_table: the group pass's results -> one f32 plane per window item.
struct WxWindowTableArgs {
  const int *keys;         // [n_groups] ascending
  const wx_i64 *counts;    // [n_groups]
  const double *sums[WX_WIN_MAX_VALUES];  // per distinct value; null when no item needs it
  const float *mins[WX_WIN_MAX_VALUES];
  const float *maxs[WX_WIN_MAX_VALUES];
  float *planes;           // [n_items][stride]
  wx_i64 n_groups;
  wx_i64 stride;           // WX_WIN_BINS (dense) or max(n_groups, 1) (search)
  int key_lo;
  wx_u32 span;
  int search;              // 0: entry key - key_lo, absent bins NaN; 1: entry g
  int n_items;
  signed char agg[WX_WIN_MAX_ITEMS];  // WX_WAGG_*
  signed char val[WX_WIN_MAX_ITEMS];  // which value's sums / mins / maxs
};

#endif  // WX_WINDOW_ARGS_H
