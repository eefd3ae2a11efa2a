// wx_join.hip -- PK-FK equi-join: every left row matches at most one right
// row, and the result is an ordered compaction of the left table.  Two
// modules are built from it: the build module (WX_OP_JOIN_TABLE, no
// expression) and the probe (appended after wx_compact.hip in a
// WX_OP_COMPACT module whose prelude defines WX_JOIN_NOUT: the lookup and the
// hooks of the multi-output ordered compaction; wx_compact_multi.hip,
// appended after it, holds the kernels and says what each hook is).  The
// lookup itself is a block of its own that a WX_OP_JOIN_GROUP module takes too
// (wx_join_group.hip, the probe inside the grouped pass).  Every
// write to a table is a vector atomic, every read of one an ordinary vector
// load.

// ===========================================================================
#if WX_OP == WX_OP_JOIN_TABLE
// The build module: it names no expression, so one program serves every
// join.

// Smallest and largest key of the right table into the build's record (both
// words as unsigned minima: the largest key is stored complemented), and
// n_right beside them.
extern "C" __global__ __launch_bounds__(WX_JOIN_BLOCK) void wx_join_range(WxJoinRangeArgs wx_r) {
  wx_u32 lo = 0xffffffffu, nhi = 0xffffffffu;
  for (wx_i64 r = (wx_i64)blockIdx.x * WX_JOIN_BLOCK + threadIdx.x; r < wx_r.n_right;
       r += (wx_i64)gridDim.x * WX_JOIN_BLOCK) {
    const wx_u32 m = (wx_u32)wx_r.keys[r] ^ 0x80000000u;
    lo = m < lo ? m : lo;
    nhi = ~m < nhi ? ~m : nhi;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const wx_u32 a = (wx_u32)__shfl_xor((int)lo, o), b = (wx_u32)__shfl_xor((int)nhi, o);
    lo = a < lo ? a : lo;
    nhi = b < nhi ? b : nhi;
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(&wx_r.rec[0], lo);
    atomicMin(&wx_r.rec[1], nhi);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    wx_r.rec[4] = (wx_u32)(wx_u64)wx_r.n_right;
    wx_r.rec[5] = (wx_u32)((wx_u64)wx_r.n_right >> 32);
  }
}

// The first thread to meet a key twice records it (the call fails with it).
__device__ __forceinline__ void wx_join_dup(wx_u32 *rec, int key) {
  if (atomicCAS(&rec[2], 0u, 1u) == 0u) rec[3] = (wx_u32)key;
}

extern "C" __global__ __launch_bounds__(WX_JOIN_BLOCK) void wx_join_build(WxJoinBuildArgs wx_b) {
  const wx_u32 mask = (1u << wx_b.log2cap) - 1u;
  const int shift = 32 - wx_b.log2cap;
  for (wx_i64 r = (wx_i64)blockIdx.x * WX_JOIN_BLOCK + threadIdx.x; r < wx_b.n_right;
       r += (wx_i64)gridDim.x * WX_JOIN_BLOCK) {
    const int key = wx_b.keys[r];
    if (wx_b.form == WX_JOIN_FORM_DIRECT) {
      const wx_u32 d = (wx_u32)key - (wx_u32)wx_b.key_lo;
      if (d >= wx_b.span || d >= (wx_u32)WX_JOIN_DIRECT_BINS) {  // outside the range wx_join_range found
        atomicOr(&wx_b.ctrs[1], (wx_u64)WX_DEVERR_JOIN_PROBE);
        continue;
      }
      if (atomicCAS(&wx_b.rows[d], -1, (int)r) != -1) wx_join_dup(wx_b.rec, key);
      continue;
    }
    const wx_u64 mine = ((wx_u64)(wx_u32)key << 32) | (wx_u64)(wx_u32)r;
    wx_u32 h = ((wx_u32)key * WX_JOIN_HASH_MUL) >> shift;
    bool placed = false;
    for (wx_u32 i = 0; i <= mask && !placed; ++i) {
      wx_u64 seen = ~0ull;
      if (__hip_atomic_compare_exchange_strong(&wx_b.slots[h & mask], &seen, mine, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT)) {
        placed = true;
      } else if ((wx_u32)(seen >> 32) == (wx_u32)key) {
        wx_join_dup(wx_b.rec, key);
        placed = true;
      } else {
        h = (h + 1u) & mask;
      }
    }
    if (!placed) atomicOr(&wx_b.ctrs[1], (wx_u64)WX_DEVERR_JOIN_PROBE);  // the table is full: it never is at load 1/2
  }
}
#endif

// ===========================================================================
#if (WX_OP == WX_OP_COMPACT && defined(WX_JOIN_NOUT)) || defined(WX_JOIN_GROUP)
// The lookup and the right-column binding, shared by the probing compaction
// below and by the grouped pass of wx_join_group.hip (appended after this
// file in a WX_OP_JOIN_GROUP module, whose prelude defines WX_JOIN_GROUP).
//
// The prelude defines, beside the compaction's own:
//   WX_JOIN_NOUT    outputs of this launch, 1 .. WX_SELECT_MAX_OUT:
//                   WX_JOIN_EXPR0 .. WX_JOIN_EXPR3 over the columns of both tables
//   WX_JOIN_COND    optional WHERE over the columns of both tables
//   WX_JOIN_FORM    0: direct (rows[key - key_lo], kept in LDS), 1: hash
//   WX_JOIN_LEFT    0: inner, 1: left outer
//   WX_JOIN_RMASK   bit j set: output j names a right column
//   WX_JOIN_CONDR   the WHERE names a right column
//   WX_JOIN_RROW    the matched right row is staged as one more 4-byte output
//   WX_RCOLS(X)     X(name, c_type, slot) for every referenced right column
//   WX_KEY          the left key expression, evaluated once per row
//
// The kernels probe every row of a tile: rows the WHERE drops and the rows of
// the last tile past n_rows (zero-filled registers) too.  Their keys may be
// anything, so the lookup is clamped before it addresses anything: wx_hit
// says whether the key is in the table, wx_rrow is 0 when it is not, and a
// right column is loaded only under wx_hit (an unmatched row binds 0).
#if WX_JOIN_FORM == WX_JOIN_FORM_HASH
// Linear probing from the home slot; the slot index is masked at every step.
// At load <= 1/2 an empty slot ends the walk; the walk is bounded by the
// capacity all the same, and a bound that is reached raises the error bit.
// The table is re-read by every row and stays in L2: plain loads.
#define WX_JOIN_LOOKUP()                                                             \
  bool wx_hit = false, wx_end = false;                                               \
  int wx_rrow = 0;                                                                   \
  {                                                                                  \
    wx_u32 wx_h = ((wx_u32)wx_key * WX_JOIN_HASH_MUL) >> wx_s.shift;                 \
    for (wx_u32 wx_i = 0; wx_i <= wx_s.mask && !wx_end; ++wx_i) {                    \
      const wx_u64 wx_sl = wx_s.slots[wx_h & wx_s.mask];                             \
      if (wx_sl == ~0ull) {                                                          \
        wx_end = true;                                                               \
      } else if ((wx_u32)(wx_sl >> 32) == (wx_u32)wx_key) {                          \
        wx_hit = wx_end = true;                                                      \
        wx_rrow = (int)((wx_u32)wx_sl & (wx_u32)(WX_JOIN_MAX_RIGHT - 1));            \
      } else {                                                                       \
        wx_h = (wx_h + 1u) & wx_s.mask;                                              \
      }                                                                              \
    }                                                                                \
    if (!wx_end) atomicOr(&wx_s.c.ctrs[1], (wx_u64)WX_DEVERR_JOIN_PROBE);            \
  }
#define WX_JOIN_SETUP()                              \
  const float wx_nan = __uint_as_float(0x7fc00000u); \
  (void)wx_nan;
#define WX_JOIN_LDS
#define WX_JOIN_FILL_LDS(NTHREADS)
#else
// key - key_lo in 32-bit wrap-around arithmetic: exact for every int key,
// because key_lo + span - 1 is itself an int (the largest key of the table)
#define WX_JOIN_LOOKUP()                                                             \
  const wx_u32 wx_d = (wx_u32)wx_key - (wx_u32)wx_s.key_lo;                          \
  const bool wx_in = wx_d < wx_span;                                                 \
  const int wx_jr = s_jrows[wx_in ? wx_d : 0u];                                      \
  const bool wx_hit = wx_in && wx_jr >= 0;                                           \
  const int wx_rrow = wx_hit ? (wx_jr & (WX_JOIN_MAX_RIGHT - 1)) : 0;
#define WX_JOIN_SETUP()                                      \
  const float wx_nan = __uint_as_float(0x7fc00000u);         \
  (void)wx_nan;                                              \
  const wx_u32 wx_span = wx_s.span < (wx_u32)WX_JOIN_DIRECT_BINS ? wx_s.span : (wx_u32)WX_JOIN_DIRECT_BINS;
#define WX_JOIN_LDS __shared__ int s_jrows[WX_JOIN_DIRECT_BINS];
// the table into LDS, once per workgroup (a barrier must follow)
#define WX_JOIN_FILL_LDS(NTHREADS) \
  for (int wx_i = (int)threadIdx.x; wx_i < WX_JOIN_DIRECT_BINS; wx_i += (NTHREADS)) s_jrows[wx_i] = wx_s.rows[wx_i];
#endif

// A right column bound like a streamed left one, so the lowered text
// name[idx] reads the matched row's value and one expression may mix both
// sides; no load unless the probe hit.
#define WX_JOIN_BIND_R(name, T, slot) \
  const ::wx::reg<T> name{wx_hit ? static_cast<const T *>(wx_s.rcol[slot])[wx_rrow] : static_cast<T>(0)};

#endif

// ===========================================================================
#if WX_OP == WX_OP_COMPACT && defined(WX_JOIN_NOUT)
static_assert(((unsigned)WX_JOIN_RMASK >> WX_JOIN_NOUT) == 0u, "right-column mask out of range");

// An output that names a right column is NaN for the unmatched row a LEFT
// join keeps (an INNER join keeps none: its outputs are plain).
#define WX_CM_GET(j) (wx_hit ? static_cast<float>(WX_JOIN_EXPR##j) : wx_nan)
// The expressions and the WHERE take over the names the shared kernels
// evaluate (the single-output kernels of wx_compact.hip, compiled before this
// file, bind no right column: they saw a constant and no condition).
#undef WX_EXPR
#define WX_EXPR WX_JOIN_EXPR0
#define WX_EXPR1 WX_JOIN_EXPR1
#define WX_EXPR2 WX_JOIN_EXPR2
#define WX_EXPR3 WX_JOIN_EXPR3
#undef WX_EVAL_COND
#ifdef WX_JOIN_COND
#define WX_EVAL_COND() static_cast<bool>(WX_JOIN_COND)
#else
#define WX_EVAL_COND() true
#endif

// The hooks of wx_compact_multi.hip's two kernels.  A row is probed once,
// whatever the number of outputs, before its WHERE is evaluated, so the
// condition may name right columns and the keep bit follows the probe:
// INNER keeps hit && cond; LEFT keeps cond, which counts as false for an
// unmatched row when it names a right column.
#define WX_CM_NOUT WX_JOIN_NOUT
#define WX_CM_ARGS WxJoinArgs
#if WX_JOIN_LEFT
#define WX_CM_MASK WX_JOIN_RMASK
#else
#define WX_CM_MASK 0
#endif
#define WX_CM_ROW()                            \
  const int wx_key = static_cast<int>(WX_KEY); \
  WX_JOIN_LOOKUP()                             \
  WX_RCOLS(WX_JOIN_BIND_R)
#if WX_JOIN_LEFT && !WX_JOIN_CONDR
#define WX_CM_KEEP() true
#else
#define WX_CM_KEEP() wx_hit
#endif
#if WX_JOIN_RROW
#define WX_CM_NSTAGE (WX_JOIN_NOUT + 1)
#define WX_CM_XEVAL() wx_val[WX_JOIN_NOUT][wx_g][wx_e] = __int_as_float(wx_hit ? wx_rrow : -1);
#endif
#define WX_CM_SETUP() WX_JOIN_SETUP()
#define WX_CM_LDS WX_JOIN_LDS
#define WX_CM_FILL_LDS(NTHREADS) WX_JOIN_FILL_LDS(NTHREADS)
#define WX_CM_DEEP wx_join_compact_deep
#define WX_CM_TICKET wx_join_compact_ticket
#endif
