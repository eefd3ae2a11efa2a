// wx_window.hip -- window aggregates: AGG(x) OVER (PARTITION BY k) broadcast
// to the passing rows inside a multi-output ordered compaction.  Two modules
// are built from it: the table module (WX_OP_WINDOW_TABLE, no expression) and
// the broadcast (appended after wx_compact.hip in a WX_OP_COMPACT module whose
// prelude defines WX_WIN_NOUT; it reuses that file's tile macros, status
// words, wx_lookback and wx_retire unchanged, as wx_select.hip does)

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
// The kernels evaluate every output of every row of a tile, as
// wx_select.hip's do: rows the WHERE drops and the rows of the last tile past
// n_rows (zero-filled registers) too.  Their keys belong to no partition, so
// the lookup is clamped before it addresses anything: wx_hit says whether
// the key is in the table, wx_slot is 0 when it is not, and the value is NaN
// unless wx_hit.  Slot 0 always exists (the LDS planes; the host allocates
// at least one entry of the search form's keys and planes).
#if WX_WIN_NOUT < 1 || WX_WIN_NOUT > WX_SELECT_MAX_OUT
#error "WX_WIN_NOUT must be between 1 and 4"
#endif
#if WX_COMPACT_GROUPS > 8
#error "at most 8 row quads per thread: a thread's keep bits share one 32-bit word"
#endif
#define WX_WN WX_WIN_NOUT
static_assert(__builtin_popcount((unsigned)WX_WIN_MASK) == WX_WIN_NITEMS, "WX_WIN_NITEMS is the mask's bit count");
static_assert(((unsigned)WX_WIN_MASK >> WX_WN) == 0u && WX_WIN_NITEMS >= 1, "window mask out of range");
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

#if (WX_WIN_MASK >> 0) & 1
#define WX_WIN_EVAL0(V) V[0][wx_g][wx_e] = WX_WIN_GET(0);
#else
#define WX_WIN_EVAL0(V) V[0][wx_g][wx_e] = static_cast<float>(WX_EXPR);
#endif
#if WX_WN <= 1
#define WX_WIN_EVAL1(V)
#elif (WX_WIN_MASK >> 1) & 1
#define WX_WIN_EVAL1(V) V[1][wx_g][wx_e] = WX_WIN_GET(1);
#else
#define WX_WIN_EVAL1(V) V[1][wx_g][wx_e] = static_cast<float>(WX_EXPR1);
#endif
#if WX_WN <= 2
#define WX_WIN_EVAL2(V)
#elif (WX_WIN_MASK >> 2) & 1
#define WX_WIN_EVAL2(V) V[2][wx_g][wx_e] = WX_WIN_GET(2);
#else
#define WX_WIN_EVAL2(V) V[2][wx_g][wx_e] = static_cast<float>(WX_EXPR2);
#endif
#if WX_WN <= 3
#define WX_WIN_EVAL3(V)
#elif (WX_WIN_MASK >> 3) & 1
#define WX_WIN_EVAL3(V) V[3][wx_g][wx_e] = WX_WIN_GET(3);
#else
#define WX_WIN_EVAL3(V) V[3][wx_g][wx_e] = static_cast<float>(WX_EXPR3);
#endif
#define WX_WIN_EVAL(V)                           \
  {                                              \
    const int wx_key = static_cast<int>(WX_KEY); \
    WX_WIN_SLOT()                                \
    WX_WIN_EVAL0(V) WX_WIN_EVAL1(V) WX_WIN_EVAL2(V) WX_WIN_EVAL3(V) \
  }

// What a kernel sets up once: NaN, and the clamped span (dense) or the
// search's first step, the largest power of two <= n_groups (0: no groups).
#if WX_WIN_SEARCH
#define WX_WIN_SETUP()                                         \
  const float wx_nan = __uint_as_float(0x7fc00000u);           \
  const wx_u32 wx_top = wx_s.n_groups ? 1u << (31 - __builtin_clz(wx_s.n_groups)) : 0u;
#define WX_WIN_FILL_LDS(NTHREADS)
#else
#define WX_WIN_SETUP()                                         \
  const float wx_nan = __uint_as_float(0x7fc00000u);           \
  const wx_u32 wx_span = wx_s.span < (wx_u32)WX_WIN_BINS ? wx_s.span : (wx_u32)WX_WIN_BINS;
// the launch's planes into LDS, once per workgroup (a barrier must follow)
#define WX_WIN_FILL_LDS(NTHREADS)                                                   \
  _Pragma("unroll") for (int wx_o = 0; wx_o < WX_WN; ++wx_o) {                      \
    if (((unsigned)WX_WIN_MASK >> wx_o) & 1u) {                                     \
      const float *wx_pl = wx_s.plane[wx_o];                                        \
      float *wx_dst = s_tab + WX_WIN_PLANE(wx_o) * WX_WIN_BINS;                     \
      for (int wx_i = (int)threadIdx.x; wx_i < WX_WIN_BINS; wx_i += (NTHREADS))     \
        wx_dst[wx_i] = wx_pl[wx_i];                                                 \
    }                                                                               \
  }
#endif

// The pipelined kernel: wx_select_compact_deep's schedule (iteration k
// evaluates and ranks t_k and issues t_{k+1}'s loads; the control wave
// publishes t_k, takes the ticket of iteration k + 2 and resolves t_{k-1}
// while the data waves write t_{k-2} out of LDS and stage t_k), with
// 2 x WX_TILE x (4 * WX_WN + 2) B of stage buffers and, in the dense form,
// WX_WIN_NITEMS x 8 KiB of planes copied into LDS before the first tile.
extern "C" __global__ __launch_bounds__(WX_CBLOCK, 1) void wx_window_compact_deep(WxWindowArgs wx_s) {
  const WxCompactArgs &wx_a = wx_s.c;
  const wx_u64 wx_E = (wx_u64)wx_a.epoch << WX_EPOCH_SHIFT;
  __shared__ wx_u32 s_cnt[WX_DWAVES][WX_GROUPS];
  __shared__ float s_val[2][WX_WN][WX_TILE];
  __shared__ unsigned short s_off[2][WX_TILE];
  __shared__ wx_i64 s_excl[2];
  __shared__ wx_i64 s_tiles[4];
#if !WX_WIN_SEARCH
  __shared__ float s_tab[WX_WIN_NITEMS * WX_WIN_BINS];
#endif
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool control = wave == WX_DWAVES;
  const int wx_dt = tid;
  WX_WIN_SETUP()
  if (tid == 0) {
    const wx_i64 t0 = (wx_i64)__hip_atomic_fetch_add(&wx_a.ctrs[0], 2ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_tiles[0] = t0;
    s_tiles[1] = t0 + 1;
  }
  WX_WIN_FILL_LDS(WX_CBLOCK)
  __syncthreads();
  wx_i64 tile = s_tiles[0];
  wx_i64 tile1 = -1, tile2 = -1;   // tiles of iterations k - 1 and k - 2
  wx_u32 tot1 = 0, tot2 = 0;       // their passing counts
  WX_COLS(WX_DECL_TILE_IN)
  if (!control && tile < wx_a.n_tiles) {
    const wx_i64 wx_tb = tile * WX_TILE;
#pragma unroll
    for (int wx_g = 0; wx_g < WX_GROUPS; ++wx_g) { WX_COLS(WX_LOAD_TILE_IN) }
  }
  for (int k = 0;; ++k) {
    const bool have = tile < wx_a.n_tiles;
    const bool have1 = k >= 1 && tile1 < wx_a.n_tiles;
    const bool have2 = k >= 2 && tile2 < wx_a.n_tiles;
    if (!have && !have1 && !have2) break;
    const wx_i64 next_tile = s_tiles[(k + 1) & 3];
    const wx_i64 tile_base = tile * WX_TILE;
    const int cur = k & 1;  // t_k is staged in buffer cur, t_{k-2} is read from it first
    wx_u32 wx_kb = 0;
    float wx_val[WX_WN][WX_GROUPS][4];
    wx_u32 lane_pre[WX_GROUPS];
    // phase 1 (data): evaluate t_k, issue t_{k+1}'s loads, rank t_k
    if (!control && have) {
      const wx_u32 wx_rows = (wx_u32)(wx_a.n_rows - tile_base < WX_TILE ? wx_a.n_rows - tile_base : WX_TILE);
#pragma unroll
      for (int wx_g = 0; wx_g < WX_GROUPS; ++wx_g) {
#pragma unroll
        for (int wx_e = 0; wx_e < 4; ++wx_e) {
          WX_COLS(WX_BIND_TILE_IN)
          const wx_u32 wx_lrow = (wx_u32)(wx_g * (WX_DTHREADS * 4) + wx_dt * 4 + wx_e);
          const wx_i64 idx = tile_base + wx_lrow;
          (void)idx;
          bool wx_k = wx_lrow < wx_rows;
          wx_k = wx_k && WX_EVAL_COND();
          wx_kb |= (wx_k ? 1u : 0u) << (wx_g * 4 + wx_e);
          WX_WIN_EVAL(wx_val)
        }
      }
      if (next_tile < wx_a.n_tiles) {
        const wx_i64 wx_tb = next_tile * WX_TILE;
#pragma unroll
        for (int wx_g = 0; wx_g < WX_GROUPS; ++wx_g) { WX_COLS(WX_LOAD_TILE_IN) }
      }
#pragma unroll
      for (int g = 0; g < WX_GROUPS; ++g) {
        wx_u32 pre = 0, tot = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const wx_u64 m = __builtin_amdgcn_ballot_w64(((wx_kb >> (g * 4 + e)) & 1u) != 0u);
          pre += wx::lanes_below(m);
          tot += (wx_u32)__builtin_popcountll(m);
        }
        lane_pre[g] = pre;
        if (lane == 0) s_cnt[wave][g] = tot;
      }
    }
    __syncthreads();
    // phase 2: control publishes t_k's aggregate and fetches the tile of
    // iteration k + 2; data waves write t_{k-2} out of buffer cur
    wx_u32 block_total = 0;
    wx_u32 grp_base[WX_GROUPS];
    if (have) { WX_BASES(s_cnt) }
    if (control) {
      if (lane == 0) {
        if (have) wx::st_agent(&wx_a.status[tile], wx_E | (tile == 0 ? WX_FLAG_P : WX_FLAG_A) | (wx_u64)block_total);
        s_tiles[(k + 2) & 3] = next_tile < wx_a.n_tiles
                                   ? (wx_i64)__hip_atomic_fetch_add(&wx_a.ctrs[0], 1ull, __ATOMIC_RELAXED,
                                                                    __HIP_MEMORY_SCOPE_AGENT)
                                   : wx_a.n_tiles;
      }
    } else if (have2) {
      // write t_{k-2}'s passing rows at the offset resolved in iteration k - 1:
      // positions [excl, end) of every output, of which [b0, b1) is the
      // 16-byte body (b0 on a 32-element boundary, b1 - b0 a multiple of 4)
      const wx_i64 excl = s_excl[cur];
      const wx_i64 prev_base = wx_a.row_base + tile2 * WX_TILE;
      const unsigned short *so = s_off[cur];
      const wx_i64 end = excl + (wx_i64)tot2;
      wx_i64 b0 = (excl + 31) & ~(wx_i64)31;
      if (b0 > end) b0 = end;
      const wx_i64 b1 = b0 + ((end - b0) & ~(wx_i64)3);
      const int n_head = (int)(b0 - excl), n_edge = n_head + (int)(end - b1);
      for (int j = wx_dt; j < n_edge; j += WX_DTHREADS) {
        const wx_i64 pos = j < n_head ? excl + j : b1 + (j - n_head);
        const int i = (int)(pos - excl);
#pragma unroll
        for (int o = 0; o < WX_WN; ++o)
          if (wx_s.out_val[o]) wx_s.out_val[o][pos] = s_val[cur][o][i];
        if (wx_a.out_idx) {
          const wx_i64 gi = prev_base + so[i];
          if (wx_a.idx64) static_cast<wx_i64 *>(wx_a.out_idx)[pos] = gi;
          else static_cast<int *>(wx_a.out_idx)[pos] = (int)gi;
        }
      }
      for (wx_i64 q = b0 + 4 * (wx_i64)wx_dt; q < b1; q += 4 * (wx_i64)WX_DTHREADS) {
        const int i = (int)(q - excl);
#pragma unroll
        for (int o = 0; o < WX_WN; ++o) {
          if (wx_s.out_val[o]) {
            typedef float v4f __attribute__((ext_vector_type(4)));
            const float *sv = s_val[cur][o];
            const v4f v = {sv[i], sv[i + 1], sv[i + 2], sv[i + 3]};
            wx::st_sel<WX_DEEP_NT_STORE>(reinterpret_cast<v4f *>(wx_s.out_val[o] + q), v);
          }
        }
        if (wx_a.out_idx) {
          const wx_u32 o0 = so[i], o1 = so[i + 1], o2 = so[i + 2], o3 = so[i + 3];
          if (wx_a.idx64) {
            typedef long long v2l __attribute__((ext_vector_type(2)));
            wx_i64 *o = static_cast<wx_i64 *>(wx_a.out_idx) + q;
            const v2l x = {(long long)(prev_base + o0), (long long)(prev_base + o1)};
            const v2l y = {(long long)(prev_base + o2), (long long)(prev_base + o3)};
            wx::st_sel<WX_DEEP_NT_STORE>(reinterpret_cast<v2l *>(o), x);
            wx::st_sel<WX_DEEP_NT_STORE>(reinterpret_cast<v2l *>(o + 2), y);
          } else {
            typedef int v4i __attribute__((ext_vector_type(4)));
            const unsigned base = (unsigned)prev_base;
            const v4i x = {(int)(base + o0), (int)(base + o1), (int)(base + o2), (int)(base + o3)};
            wx::st_sel<WX_DEEP_NT_STORE>(reinterpret_cast<v4i *>(static_cast<int *>(wx_a.out_idx) + q), x);
          }
        }
      }
    }
    __syncthreads();
    // phase 3: data waves stage t_k into buffer cur; the control wave
    // resolves t_{k-1}'s offset (published one iteration ago)
    if (control) {
      if (have1) {
        wx_i64 excl = 0;
        if (tile1 > 0) {
          excl = wx_lookback(wx_a, tile1);
          if (lane == 0) wx::st_agent(&wx_a.status[tile1], wx_E | WX_FLAG_P | (wx_u64)(excl + tot1));
        }
        if (lane == 0) {
          s_excl[cur ^ 1] = excl;  // read when t_{k-1} is written, in iteration k + 1
          if (tile1 == wx_a.n_tiles - 1 && wx_a.count_out) *wx_a.count_out = excl + tot1;
        }
      }
    } else if (have) {
#pragma unroll
      for (int g = 0; g < WX_GROUPS; ++g) {
        wx_u32 pos = grp_base[g] + lane_pre[g];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if ((wx_kb >> (g * 4 + e)) & 1u) {
#pragma unroll
            for (int o = 0; o < WX_WN; ++o) s_val[cur][o][pos] = wx_val[o][g][e];
            s_off[cur][pos] = (unsigned short)(g * (WX_DTHREADS * 4) + wx_dt * 4 + e);
            ++pos;
          }
        }
      }
    }
    tile2 = tile1;
    tot2 = tot1;
    tile1 = tile;
    tot1 = have ? block_total : 0u;
    tile = next_tile;
  }
  if (tid == 0) wx_retire(wx_a.ctrs);
}

// One tile per workgroup, taken from a ticket counter (robust fallback,
// WARPDB_COMPACT_SCHED=ticket): no LDS staging, each lane writes its own
// passing rows; the dense form copies the planes into LDS per workgroup.
extern "C" __global__ __launch_bounds__(WX_DTHREADS) void wx_window_compact_ticket(WxWindowArgs wx_s) {
  const WxCompactArgs &wx_a = wx_s.c;
  const wx_u64 wx_E = (wx_u64)wx_a.epoch << WX_EPOCH_SHIFT;
  __shared__ wx_u32 s_cnt[WX_DWAVES][WX_GROUPS];
  __shared__ wx_i64 s_excl;
  __shared__ wx_u32 s_tile;
#if !WX_WIN_SEARCH
  __shared__ float s_tab[WX_WIN_NITEMS * WX_WIN_BINS];
#endif
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wx_dt = tid;
  WX_WIN_SETUP()
  if (tid == 0)
    s_tile = (wx_u32)__hip_atomic_fetch_add(&wx_a.ctrs[0], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  WX_WIN_FILL_LDS(WX_DTHREADS)
  __syncthreads();
  const wx_i64 tile = s_tile;
  const wx_i64 tile_base = tile * WX_TILE;
  WX_COLS(WX_DECL_TILE_IN)
  {
    const wx_i64 wx_tb = tile_base;
#pragma unroll
    for (int wx_g = 0; wx_g < WX_GROUPS; ++wx_g) { WX_COLS(WX_LOAD_TILE_IN) }
  }
  bool wx_keep[WX_GROUPS][4];
  float wx_val[WX_WN][WX_GROUPS][4];
  wx_u32 lane_pre[WX_GROUPS];
#pragma unroll
  for (int wx_g = 0; wx_g < WX_GROUPS; ++wx_g) {
#pragma unroll
    for (int wx_e = 0; wx_e < 4; ++wx_e) {
      WX_COLS(WX_BIND_TILE_IN)
      const wx_i64 idx = tile_base + (wx_i64)wx_g * (WX_DTHREADS * 4) + (wx_i64)wx_dt * 4 + wx_e;
      bool wx_k = idx < wx_a.n_rows;
      wx_k = wx_k && WX_EVAL_COND();
      wx_keep[wx_g][wx_e] = wx_k;
      WX_WIN_EVAL(wx_val)
    }
  }
#pragma unroll
  for (int g = 0; g < WX_GROUPS; ++g) {
    wx_u32 pre = 0, tot = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const wx_u64 m = __builtin_amdgcn_ballot_w64(wx_keep[g][e]);
      pre += wx::lanes_below(m);
      tot += (wx_u32)__builtin_popcountll(m);
    }
    lane_pre[g] = pre;
    if (lane == 0) s_cnt[wave][g] = tot;
  }
  __syncthreads();
  wx_u32 block_total = 0;
  wx_u32 grp_base[WX_GROUPS];
  WX_BASES(s_cnt)
  if (wave == 0) {
    wx_i64 excl = 0;
    if (tile == 0) {
      if (lane == 0) wx::st_agent(&wx_a.status[0], wx_E | WX_FLAG_P | (wx_u64)block_total);
    } else {
      if (lane == 0) wx::st_agent(&wx_a.status[tile], wx_E | WX_FLAG_A | (wx_u64)block_total);
      excl = wx_lookback(wx_a, tile);
      if (lane == 0) wx::st_agent(&wx_a.status[tile], wx_E | WX_FLAG_P | (wx_u64)(excl + block_total));
    }
    if (lane == 0) s_excl = excl;
  }
  __syncthreads();
  const wx_i64 excl = s_excl;
#pragma unroll
  for (int g = 0; g < WX_GROUPS; ++g) {
    const wx_i64 r0 = tile_base + (wx_i64)g * (WX_DTHREADS * 4) + (wx_i64)tid * 4;
    wx_i64 pos = excl + grp_base[g] + lane_pre[g];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (wx_keep[g][e]) {
#pragma unroll
        for (int o = 0; o < WX_WN; ++o)
          if (wx_s.out_val[o]) wx_s.out_val[o][pos] = wx_val[o][g][e];
        if (wx_a.out_idx) {
          const wx_i64 gi = wx_a.row_base + r0 + e;
          if (wx_a.idx64) static_cast<wx_i64 *>(wx_a.out_idx)[pos] = gi;
          else static_cast<int *>(wx_a.out_idx)[pos] = (int)gi;
        }
        ++pos;
      }
    }
  }
  if (tid == 0 && tile == wx_a.n_tiles - 1 && wx_a.count_out) *wx_a.count_out = excl + block_total;
  if (tid == 0) wx_retire(wx_a.ctrs);
}
#endif
