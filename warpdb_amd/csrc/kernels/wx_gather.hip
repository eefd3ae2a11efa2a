// wx_gather.hip -- multi-output row gather (ORDER BY over a multi-column
// SELECT, late materialisation): WX_NOUT expressions evaluated at a list of
// row ids.  (Appended after wx_common.hip and wx_gather_args.h in a
// WX_OP_GATHER module.)

// ===========================================================================
#if WX_OP == WX_OP_GATHER
#ifndef WX_NOUT
#define WX_NOUT 1  // the prelude defines it for two or more expressions
#endif
#if WX_NOUT < 1 || WX_NOUT > WX_GATHER_MAX_OUT
#error "WX_NOUT must be between 1 and 4"
#endif
#if WX_GATHER_UNROLL < 1 || WX_GATHER_UNROLL > 8 || WX_GATHER_BLOCK < 64 || WX_GATHER_BLOCK > 1024 || (WX_GATHER_BLOCK & 63)
#error "gather geometry: 1..8 quads per thread, a block of 64..1024 threads in whole waves"
#endif
// Written once, read by a later launch or the host: nontemporal 16-byte stores.
#ifndef WX_GATHER_NT_STORE
#define WX_GATHER_NT_STORE 1
#endif

// A thread's gathered column values: [quad][row of the quad].  Every
// referenced column is loaded once per row, however many expressions use it.
#define WX_G_DECL(name, T, slot) T wx_g##slot[WX_GATHER_UNROLL][4];
#define WX_G_LOAD(name, T, slot) \
  wx_g##slot[wx_u][wx_e] = static_cast<const T *>(wx_a.col[slot])[wx_row[wx_u][wx_e]];
#define WX_G_LOAD_GUARDED(name, T, slot) \
  wx_g##slot[wx_u][wx_e] = 0;            \
  if (wx_ok) wx_g##slot[wx_u][wx_e] = static_cast<const T *>(wx_a.col[slot])[wx_row[wx_u][wx_e]];
#define WX_G_BIND(name, T, slot) const ::wx::reg<T> name{wx_g##slot[wx_u][wx_e]};

#if WX_NOUT > 1
#define WX_G_EVAL1 wx_val[1][wx_e] = wx_ok ? static_cast<float>(WX_EXPR1) : wx_nan;
#else
#define WX_G_EVAL1
#endif
#if WX_NOUT > 2
#define WX_G_EVAL2 wx_val[2][wx_e] = wx_ok ? static_cast<float>(WX_EXPR2) : wx_nan;
#else
#define WX_G_EVAL2
#endif
#if WX_NOUT > 3
#define WX_G_EVAL3 wx_val[3][wx_e] = wx_ok ? static_cast<float>(WX_EXPR3) : wx_nan;
#else
#define WX_G_EVAL3
#endif

#define WX_G_SPAN ((wx_i64)WX_GATHER_BLOCK * WX_GATHER_UNROLL)
#define WX_G_QUAD(u) (wx_base + (wx_i64)(u) * WX_GATHER_BLOCK + threadIdx.x)
#define WX_G_IN_TABLE(r) ((wx_u64)(r) < (wx_u64)wx_a.n_rows)

// out_val[j][k] = static_cast<float>(expression j) at row rows[k] - row_base
// and out_rows[k] = out_row_base + that row, for k < min(count, *d_count).
// A thread owns quads of 4 consecutive positions: one 16-byte load of ids
// (two for 8-byte ids), then all 4 x columns loads of its WX_GATHER_UNROLL
// quads before the first use, so a wave keeps 64 x 4 x UNROLL x columns
// independent misses in flight; 16-byte nontemporal stores for full quads of
// 16-byte aligned outputs, scalar stores otherwise (the last partial quad,
// offset pointers).  A row id outside [0, n_rows) issues no load and every
// output reads NaN there; nothing is written at k >= count.
extern "C" __global__ __launch_bounds__(WX_GATHER_BLOCK) void wx_select_gather(WxGatherArgs wx_a) {
  wx_i64 wx_cnt = wx_a.count;
  if (wx_a.d_count) {
    const wx_i64 wx_dc = *wx_a.d_count;
    if (wx_dc < wx_cnt) wx_cnt = wx_dc;
  }
  if (wx_cnt <= 0) return;
  const wx_i64 wx_nq = (wx_cnt + 3) >> 2;
  const float wx_nan = __uint_as_float(0x7fc00000u);
  const bool wx_ids16 = (reinterpret_cast<wx_u64>(wx_a.rows) & 15ull) == 0ull;
  const bool wx_rows16 = (reinterpret_cast<wx_u64>(wx_a.out_rows) & 15ull) == 0ull;
  for (wx_i64 wx_base = (wx_i64)blockIdx.x * WX_G_SPAN; wx_base < wx_nq; wx_base += (wx_i64)gridDim.x * WX_G_SPAN) {
    // the ids of this thread's quads; -1 (outside any table) past the count.
    // All of a thread's quads inside the count (every workgroup iteration but
    // the last): 16-byte loads, issued together.
    wx_i64 wx_row[WX_GATHER_UNROLL][4];
    if (wx_ids16 && (WX_G_QUAD(WX_GATHER_UNROLL - 1) << 2) + 4 <= wx_cnt) {
      if (wx_a.idx64) {
        typedef long long v2l __attribute__((ext_vector_type(2)));
        v2l x[WX_GATHER_UNROLL], y[WX_GATHER_UNROLL];
#pragma unroll
        for (int wx_u = 0; wx_u < WX_GATHER_UNROLL; ++wx_u) {
          const v2l *p = reinterpret_cast<const v2l *>(static_cast<const wx_i64 *>(wx_a.rows) + (WX_G_QUAD(wx_u) << 2));
          x[wx_u] = ::wx::ldv(p);
          y[wx_u] = ::wx::ldv(p + 1);
        }
#pragma unroll
        for (int wx_u = 0; wx_u < WX_GATHER_UNROLL; ++wx_u) {
          wx_row[wx_u][0] = x[wx_u].x - wx_a.row_base;
          wx_row[wx_u][1] = x[wx_u].y - wx_a.row_base;
          wx_row[wx_u][2] = y[wx_u].x - wx_a.row_base;
          wx_row[wx_u][3] = y[wx_u].y - wx_a.row_base;
        }
      } else {
        typedef int v4i __attribute__((ext_vector_type(4)));
        v4i x[WX_GATHER_UNROLL];
#pragma unroll
        for (int wx_u = 0; wx_u < WX_GATHER_UNROLL; ++wx_u)
          x[wx_u] = ::wx::ldv(reinterpret_cast<const v4i *>(static_cast<const int *>(wx_a.rows) + (WX_G_QUAD(wx_u) << 2)));
#pragma unroll
        for (int wx_u = 0; wx_u < WX_GATHER_UNROLL; ++wx_u) {
          wx_row[wx_u][0] = (wx_i64)x[wx_u].x - wx_a.row_base;
          wx_row[wx_u][1] = (wx_i64)x[wx_u].y - wx_a.row_base;
          wx_row[wx_u][2] = (wx_i64)x[wx_u].z - wx_a.row_base;
          wx_row[wx_u][3] = (wx_i64)x[wx_u].w - wx_a.row_base;
        }
      }
    } else {
#pragma unroll
      for (int wx_u = 0; wx_u < WX_GATHER_UNROLL; ++wx_u) {
#pragma unroll
        for (int wx_e = 0; wx_e < 4; ++wx_e) {
          const wx_i64 wx_p = (WX_G_QUAD(wx_u) << 2) + wx_e;
          wx_i64 r = -1;
          if (wx_p < wx_cnt)
            r = (wx_a.idx64 ? static_cast<const wx_i64 *>(wx_a.rows)[wx_p]
                            : (wx_i64) static_cast<const int *>(wx_a.rows)[wx_p]) -
                wx_a.row_base;
          wx_row[wx_u][wx_e] = r;
        }
      }
    }
    bool wx_all = true;
#pragma unroll
    for (int wx_u = 0; wx_u < WX_GATHER_UNROLL; ++wx_u) {
#pragma unroll
      for (int wx_e = 0; wx_e < 4; ++wx_e) wx_all = wx_all && WX_G_IN_TABLE(wx_row[wx_u][wx_e]);
    }
    // every column load of every row before the first use: unconditional
    // when all of the thread's ids are inside the table (the usual case), so
    // the compiler batches them; guarded row by row otherwise
    WX_COLS(WX_G_DECL)
    if (wx_all) {
#pragma unroll
      for (int wx_u = 0; wx_u < WX_GATHER_UNROLL; ++wx_u) {
#pragma unroll
        for (int wx_e = 0; wx_e < 4; ++wx_e) { WX_COLS(WX_G_LOAD) }
      }
    } else {
#pragma unroll
      for (int wx_u = 0; wx_u < WX_GATHER_UNROLL; ++wx_u) {
#pragma unroll
        for (int wx_e = 0; wx_e < 4; ++wx_e) {
          const bool wx_ok = WX_G_IN_TABLE(wx_row[wx_u][wx_e]);
          (void)wx_ok;
          WX_COLS(WX_G_LOAD_GUARDED)
        }
      }
    }
#pragma unroll
    for (int wx_u = 0; wx_u < WX_GATHER_UNROLL; ++wx_u) {
      const wx_i64 wx_p0 = WX_G_QUAD(wx_u) << 2;
      if (wx_p0 < wx_cnt) {
        float wx_val[WX_NOUT][4];
#pragma unroll
        for (int wx_e = 0; wx_e < 4; ++wx_e) {
          WX_COLS(WX_G_BIND)
          const wx_i64 idx = wx_row[wx_u][wx_e];
          (void)idx;
          const bool wx_ok = WX_G_IN_TABLE(wx_row[wx_u][wx_e]);
          wx_val[0][wx_e] = wx_ok ? static_cast<float>(WX_EXPR) : wx_nan;
          WX_G_EVAL1 WX_G_EVAL2 WX_G_EVAL3
        }
        const bool wx_full = wx_p0 + 4 <= wx_cnt;
#pragma unroll
        for (int o = 0; o < WX_NOUT; ++o) {
          float *out = wx_a.out_val[o];
          if (!out) continue;
          if (wx_full && (reinterpret_cast<wx_u64>(out) & 15ull) == 0ull) {
            typedef float v4f __attribute__((ext_vector_type(4)));
            const v4f v = {wx_val[o][0], wx_val[o][1], wx_val[o][2], wx_val[o][3]};
            ::wx::st_sel<WX_GATHER_NT_STORE != 0>(reinterpret_cast<v4f *>(out + wx_p0), v);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (wx_p0 + e < wx_cnt) out[wx_p0 + e] = wx_val[o][e];
          }
        }
        if (wx_a.out_rows) {
          wx_i64 *out = wx_a.out_rows + wx_p0;
          const wx_i64 b = wx_a.out_row_base;
          if (wx_full && wx_rows16) {
            typedef long long v2l __attribute__((ext_vector_type(2)));
            const v2l x = {(long long)(b + wx_row[wx_u][0]), (long long)(b + wx_row[wx_u][1])};
            const v2l y = {(long long)(b + wx_row[wx_u][2]), (long long)(b + wx_row[wx_u][3])};
            ::wx::st_sel<WX_GATHER_NT_STORE != 0>(reinterpret_cast<v2l *>(out), x);
            ::wx::st_sel<WX_GATHER_NT_STORE != 0>(reinterpret_cast<v2l *>(out + 2), y);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (wx_p0 + e < wx_cnt) out[e] = b + wx_row[wx_u][e];
          }
        }
      }
    }
  }
}
#endif
