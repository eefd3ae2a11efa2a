// wx_window.hip -- window aggregates: AGG(x) OVER (PARTITION BY k) broadcast
// to the passing rows inside a multi-output ordered compaction.  Two modules
// are built from it: the table module (WX_OP_WINDOW_TABLE, no expression) and
// the broadcast (appended after wx_compact.hip in a WX_OP_COMPACT module whose
// prelude defines WX_WIN_NOUT: the lookup macros and the hooks of the
// multi-output ordered compaction; wx_compact_multi.hip, appended after it,
// holds the kernels and says what each hook is)

// ===========================================================================
#if WX_OP == WX_OP_WINDOW_TABLE
// The table module: it names no expression, so one program serves every
// window query.
//
// What the host needs of the group pass to choose the form, gathered into
// one 16-byte record so that one copy and one synchronisation fetch it:
// {group count, first key, last key}.  A count the group pass could not
// establish (negative) or one beyond the capacity reads no key.
extern "C" __global__ void wx_window_range(WxWindowRangeArgs wx_r) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const wx_i64 g = *wx_r.n_groups;
  int first = 0, last = 0;
  if (g > 0 && g <= wx_r.capacity) {
    first = wx_r.keys[0];
    last = wx_r.keys[g - 1];
  }
  wx_r.out[0] = g;
  reinterpret_cast<int *>(wx_r.out + 1)[0] = first;
  reinterpret_cast<int *>(wx_r.out + 1)[1] = last;
}

// One f32 plane per window item from the group pass's results (sorted keys,
// double sums, int64 counts, f32 minima and maxima), with the conversions
// query_sql_grouped applies on the host: SUM (float)sum, AVG (float)(sum /
// (double)count), COUNT (float)count, MIN / MAX as they are.  Dense form: one
// workgroup fills every plane with NaN, then writes entry key - key_lo of
// each group (a key outside the span is skipped).  Search form: entry g, any
// grid.
extern "C" __global__ __launch_bounds__(WX_WIN_TBLOCK) void wx_window_table(WxWindowTableArgs wx_t) {
  const wx_u32 span = wx_t.span < (wx_u32)WX_WIN_BINS ? wx_t.span : (wx_u32)WX_WIN_BINS;
  const int n_items = wx_t.n_items < WX_WIN_MAX_ITEMS ? wx_t.n_items : WX_WIN_MAX_ITEMS;
  if (!wx_t.search) {
    if (blockIdx.x != 0) return;
    const float nan = __uint_as_float(0x7fc00000u);
    for (int i = (int)threadIdx.x; i < n_items * WX_WIN_BINS; i += WX_WIN_TBLOCK) wx_t.planes[i] = nan;
    __syncthreads();
  }
  for (wx_i64 g = (wx_i64)blockIdx.x * WX_WIN_TBLOCK + threadIdx.x; g < wx_t.n_groups;
       g += (wx_i64)gridDim.x * WX_WIN_TBLOCK) {
    wx_i64 slot = g;
    if (!wx_t.search) {
      const wx_u32 d = (wx_u32)wx_t.keys[g] - (wx_u32)wx_t.key_lo;
      if (d >= span) continue;
      slot = (wx_i64)d;
    } else if (g >= wx_t.stride) {
      continue;
    }
    const wx_i64 cnt = wx_t.counts[g];
    for (int it = 0; it < n_items; ++it) {
      const int v = wx_t.val[it] & (WX_WIN_MAX_VALUES - 1);
      float r;
      switch (wx_t.agg[it]) {
        case WX_WAGG_SUM: r = (float)wx_t.sums[v][g]; break;
        case WX_WAGG_AVG: r = (float)(wx_t.sums[v][g] / (double)cnt); break;
        case WX_WAGG_COUNT: r = (float)cnt; break;
        case WX_WAGG_MIN: r = wx_t.mins[v][g]; break;
        default: r = wx_t.maxs[v][g]; break;
      }
      wx_t.planes[(wx_i64)it * wx_t.stride + slot] = r;
    }
  }
}
#endif

// ===========================================================================
#if WX_OP == WX_OP_COMPACT && defined(WX_WIN_NOUT)
// The prelude defines, beside the compaction's own:
//   WX_WIN_NOUT    outputs of this launch, 1 .. WX_SELECT_MAX_OUT
//   WX_WIN_MASK    bit j set: output j is a window item, else the plain
//                  expression WX_EXPR / WX_EXPR1 .. WX_EXPR3
//   WX_WIN_NITEMS  popcount(WX_WIN_MASK)
//   WX_WIN_SEARCH  0: dense form, 1: search form
//   WX_KEY         the partition expression, evaluated once per row
// A window output is plane[slot(static_cast<int>(WX_KEY))] of its item's
// plane (wx_window_table above fills the planes from the group pass).
//
// The kernels evaluate every output of every row of a tile: rows the WHERE
// drops and the rows of the last tile past n_rows (zero-filled registers) too.  Their keys belong to no partition, so
// the lookup is clamped before it addresses anything: wx_hit says whether
// the key is in the table, wx_slot is 0 when it is not, and the value is NaN
// unless wx_hit.  Slot 0 always exists (the LDS planes; the host allocates
// at least one entry of the search form's keys and planes).
static_assert(__builtin_popcount((unsigned)WX_WIN_MASK) == WX_WIN_NITEMS, "WX_WIN_NITEMS is the mask's bit count");
static_assert(((unsigned)WX_WIN_MASK >> WX_WIN_NOUT) == 0u && WX_WIN_NITEMS >= 1, "window mask out of range");
// the LDS plane of output j: the window outputs below it
#define WX_WIN_PLANE(j) __builtin_popcount((unsigned)WX_WIN_MASK & ((1u << (j)) - 1u))

#if WX_WIN_SEARCH
// Branch-free binary search over the ascending keys: wx_pos counts the keys
// <= wx_key.  Every probe index is below n_groups (an out-of-range probe
// reads entry 0 and is ignored); no probe at all when there are no groups.
// The keys are re-read by every row and stay in L2: plain loads.
#define WX_WIN_SLOT()                                                        \
  wx_u32 wx_pos = 0u;                                                        \
  int wx_last = 0;                                                           \
  for (wx_u32 wx_st = wx_top; wx_st != 0u; wx_st >>= 1) {                    \
    const wx_u32 wx_nx = wx_pos + wx_st;                                     \
    const bool wx_in = wx_nx <= wx_s.n_groups;                               \
    const int wx_kv = wx_s.keys[wx_in ? wx_nx - 1u : 0u];                    \
    const bool wx_go = wx_in && wx_kv <= wx_key;                             \
    wx_pos = wx_go ? wx_nx : wx_pos;                                         \
    wx_last = wx_go ? wx_kv : wx_last;                                       \
  }                                                                          \
  const bool wx_hit = wx_pos != 0u && wx_last == wx_key;                     \
  const wx_u32 wx_slot = wx_hit ? wx_pos - 1u : 0u;
#define WX_WIN_GET(j) (wx_hit ? wx_s.plane[j][wx_slot] : wx_nan)
#else
// key - key_lo in 32-bit wrap-around arithmetic: exact for every int key,
// because key_lo + span - 1 is itself an int (the largest key of the table)
#define WX_WIN_SLOT()                                                        \
  const wx_u32 wx_d = (wx_u32)wx_key - (wx_u32)wx_s.key_lo;                  \
  const bool wx_hit = wx_d < wx_span;                                        \
  const wx_u32 wx_slot = wx_hit ? wx_d : 0u;
#define WX_WIN_GET(j) (wx_hit ? s_tab[WX_WIN_PLANE(j) * WX_WIN_BINS + wx_slot] : wx_nan)
#endif

// What a kernel sets up once: NaN, and the clamped span (dense) or the
// search's first step, the largest power of two <= n_groups (0: no groups);
// and what it keeps in LDS: the launch's planes in the dense form.
#if WX_WIN_SEARCH
#define WX_WIN_SETUP()                                         \
  const float wx_nan = __uint_as_float(0x7fc00000u);           \
  const wx_u32 wx_top = wx_s.n_groups ? 1u << (31 - __builtin_clz(wx_s.n_groups)) : 0u;
#define WX_WIN_FILL_LDS(NTHREADS)
#define WX_WIN_LDS
#else
#define WX_WIN_SETUP()                                         \
  const float wx_nan = __uint_as_float(0x7fc00000u);           \
  const wx_u32 wx_span = wx_s.span < (wx_u32)WX_WIN_BINS ? wx_s.span : (wx_u32)WX_WIN_BINS;
// the launch's planes into LDS, once per workgroup (a barrier must follow)
#define WX_WIN_FILL_LDS(NTHREADS)                                                   \
  _Pragma("unroll") for (int wx_o = 0; wx_o < WX_WIN_NOUT; ++wx_o) {                \
    if (((unsigned)WX_WIN_MASK >> wx_o) & 1u) {                                     \
      const float *wx_pl = wx_s.plane[wx_o];                                        \
      float *wx_dst = s_tab + WX_WIN_PLANE(wx_o) * WX_WIN_BINS;                     \
      for (int wx_i = (int)threadIdx.x; wx_i < WX_WIN_BINS; wx_i += (NTHREADS))     \
        wx_dst[wx_i] = wx_pl[wx_i];                                                 \
    }                                                                               \
  }
#define WX_WIN_LDS __shared__ float s_tab[WX_WIN_NITEMS * WX_WIN_BINS];
#endif

// The hooks of wx_compact_multi.hip's two kernels.  A row works out its key
// and slot once, whatever the number of window outputs; the dense form keeps
// WX_WIN_NITEMS x 8 KiB of planes in LDS beside the stage buffers, copied
// before the first tile.
#define WX_CM_NOUT WX_WIN_NOUT
#define WX_CM_ARGS WxWindowArgs
#define WX_CM_MASK WX_WIN_MASK
#define WX_CM_GET(j) WX_WIN_GET(j)
#define WX_CM_ROW()                            \
  const int wx_key = static_cast<int>(WX_KEY); \
  WX_WIN_SLOT()
#define WX_CM_SETUP() WX_WIN_SETUP()
#define WX_CM_LDS WX_WIN_LDS
#define WX_CM_FILL_LDS(NTHREADS) WX_WIN_FILL_LDS(NTHREADS)
#define WX_CM_DEEP wx_window_compact_deep
#define WX_CM_TICKET wx_window_compact_ticket
#endif
