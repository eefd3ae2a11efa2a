// wx_select.hip -- multi-column SELECT: the hooks of the multi-output ordered
// compaction (appended after wx_compact.hip in a WX_OP_COMPACT module whose
// prelude defines WX_NOUT; wx_compact_multi.hip, appended after it, holds the
// kernels and says what each hook is)

// ===========================================================================
#if WX_OP == WX_OP_COMPACT && defined(WX_NOUT)
// WX_NOUT expressions (WX_EXPR, WX_EXPR1 .. WX_EXPR3) of one filtered result
// in one pass, out_val[j][k] = static_cast<float>(expression j) of the k-th
// passing row: the plain case of the shared kernels -- no window output, so
// no key, no table in LDS and nothing to set up.
#define WX_CM_NOUT WX_NOUT
#define WX_CM_ARGS WxSelectArgs
#define WX_CM_MASK 0
#define WX_CM_ROW()
#define WX_CM_SETUP()
#define WX_CM_LDS
#define WX_CM_FILL_LDS(NTHREADS)
#define WX_CM_DEEP wx_select_compact_deep
#define WX_CM_TICKET wx_select_compact_ticket
#endif
