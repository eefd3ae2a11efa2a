// wx_select_args.h -- argument block of the multi-output ordered compaction
// (wx_select.hip).  Shared by the host runtime and the device templates like
// wx_args.h, which must come first (WxCompactArgs).  Plain C++ only.
#ifndef WX_SELECT_ARGS_H
#define WX_SELECT_ARGS_H

#define WX_SELECT_MAX_OUT 4  // WX_MAX_OUTPUTS of include/warpexec.h

// Compaction geometry per output count: every staged row costs 4 B per
// output plus a 2-byte tile-local offset, in two stage buffers, so the tile
// shrinks as the outputs grow (WX_SELECT_LDS_BUDGET bytes for both buffers).
#define WX_SELECT_LDS_BUDGET (150 * 1024)
#define WX_SELECT_ROW_BYTES(nout) (2 * (4 * (nout) + 2))

struct WxSelectArgs {
  WxCompactArgs c;  // columns, row ids, status words, counters, count: as the single-output kernel (out_val unused)
  float *out_val[WX_SELECT_MAX_OUT];  // each nullable; [j] receives static_cast<float>(expression j)
};

#endif  // WX_SELECT_ARGS_H
