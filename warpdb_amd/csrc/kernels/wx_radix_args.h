// wx_radix_args.h -- geometry of the radix sort's histogram pass
// (wx_radix_hist_*, wx_radix.hip).  Shared by the host runtime
// (wx_sort_hist_span_keys) and the util module's device text like wx_args.h,
// which holds the tile geometry (WX_RS_BLOCK / WX_RS_ITEMS) and must come
// first.  Plain C++ only.
#ifndef WX_RADIX_ARGS_H
#define WX_RADIX_ARGS_H

// One 1024-thread workgroup per CU; a workgroup reads one span of
// WX_RS_HBLOCK x WX_RS_HUNROLL 16-byte loads (4 keys each) per iteration.
#define WX_RS_HBLOCK 1024
#ifndef WX_RS_HUNROLL
#define WX_RS_HUNROLL 4  // 16-byte loads in flight per thread (64 B): the kernel is latency-bound below that
#endif

#endif  // WX_RADIX_ARGS_H
