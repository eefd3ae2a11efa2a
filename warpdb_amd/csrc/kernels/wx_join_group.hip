// wx_join_group.hip -- JOIN under GROUP BY: the left table is streamed once,
// every row is looked up in the right table's direct or hash table and the
// kept rows are added into wx_group_multi's LDS window + general-key hash, so
// nothing is written per row.  Concatenated after wx_common.hip,
// wx_group_window.hip (the accumulator layout, wx_gm_hash_add and
// wx_group_multi_finalize), wx_group_multi.hip (WX_UNROLL), wx_join.hip (the lookup and the right-column
// binding) and wx_join_group_args.h.
#if WX_OP == WX_OP_JOIN_GROUP
// The prelude defines, beside wx_group_multi's (WX_NOUT 1 .. 4, WX_EXPR ..
// WX_EXPR3, WX_GM_SUMS, WX_GM_MMS, WX_COND):
//   WX_KEY          the left join key, over the left columns
//   WX_GKEY         the group key, over the columns of both tables
//   WX_JOIN_FORM    0: direct (rows[key - key_lo], kept in LDS), 1: hash
//   WX_JOIN_CONDR   the WHERE names a right column
//   WX_RCOLS(X)     X(name, c_type, slot) for every referenced right column
// A row is kept when idx < n_rows && hit && cond (an INNER join).  When the
// WHERE names no right column it is evaluated first and only the passing rows
// are probed; else every row is probed, the rows of the last quad past n_rows
// (zero-filled registers) too, and the lookup's clamp protects them.
#if !defined(WX_JOIN_FORM) || !defined(WX_JOIN_CONDR) || !defined(WX_GKEY)
#error "wx_join_group needs its form, its WHERE flag and its group key"
#endif

namespace wxjg {
constexpr int BLOCK = WX_JG_BLOCK(wxgm::NS, wxgm::NQ, WX_JOIN_FORM);
constexpr int LDS_BYTES = WX_JG_LDS_BYTES(wxgm::NS, wxgm::NQ, WX_JOIN_FORM);
static_assert(LDS_BYTES * WX_JG_PER_CU(wxgm::NS, wxgm::NQ, WX_JOIN_FORM) <= WX_JG_LDS_LIMIT,
              "the window and the direct table of every resident workgroup fit the LDS");
}  // namespace wxjg

#undef WX_LBLOCK
#define WX_LBLOCK (wxjg::BLOCK)
extern "C" __global__ __launch_bounds__(WX_JG_BLOCK(wxgm::NS, wxgm::NQ, WX_JOIN_FORM)) void wx_join_group(
    WxJoinGroupArgs wx_s) {
  const WxGroupMultiArgs &wx_a = wx_s.g;
  // [NS][W] f64 sums | [W] u32 counts | [NQ][W] u32 minima | [NQ][W] u32 maxima, as wx_group_multi
  __shared__ __attribute__((aligned(16))) unsigned char wx_lds[WX_GM_LDS_BYTES(wxgm::NS, wxgm::NQ)];
  WX_JOIN_LDS
  double *const wx_s_sum = reinterpret_cast<double *>(wx_lds);
  wx_u32 *const wx_s_cnt = reinterpret_cast<wx_u32 *>(wx_lds + (wx_u64)wxgm::NS * WX_GWIN * 8);
  wx_u32 *const wx_s_min = wx_s_cnt + WX_GWIN;
  wx_u32 *const wx_s_max = wx_s_min + (wx_u64)wxgm::NQ * WX_GWIN;
  for (int i = threadIdx.x; i < WX_GWIN; i += wxjg::BLOCK) {
    wx_s_cnt[i] = 0u;
#pragma unroll
    for (int p = 0; p < wxgm::NS; ++p) wx_s_sum[p * WX_GWIN + i] = 0.0;
#pragma unroll
    for (int p = 0; p < wxgm::NQ; ++p) {
      wx_s_min[p * WX_GWIN + i] = 0xffffffffu;
      wx_s_max[p * WX_GWIN + i] = 0u;
    }
  }
  WX_JOIN_FILL_LDS(wxjg::BLOCK)
  __syncthreads();
  WX_JOIN_SETUP()
  bool wx_lead_on = false;  // this batch's first rows had a bin shared by many lanes
  WX_STRIDE_LOOP_BEGIN
  // the row's group key and values, set when it is kept
  int wx_gk = 0;
  float wx_v[WX_NOUT] = {};
#if WX_JOIN_CONDR
  bool wx_pass;
  {
    const int wx_key = static_cast<int>(WX_KEY);
    WX_JOIN_LOOKUP()
    WX_RCOLS(WX_JOIN_BIND_R)
    wx_pass = idx < wx_a.n_rows && wx_hit && WX_EVAL_COND();
    if (wx_pass) {
      const float wx_t[WX_NOUT] = {WX_GM_VALS};
      wx_gk = static_cast<int>(WX_GKEY);
#pragma unroll
      for (int j = 0; j < WX_NOUT; ++j) wx_v[j] = wx_t[j];
    }
  }
#else
  bool wx_pass = idx < wx_a.n_rows && WX_EVAL_COND();
  if (wx_pass) {
    const int wx_key = static_cast<int>(WX_KEY);
    WX_JOIN_LOOKUP()
    WX_RCOLS(WX_JOIN_BIND_R)
    wx_pass = wx_hit;
    if (wx_hit) {
      const float wx_t[WX_NOUT] = {WX_GM_VALS};
      wx_gk = static_cast<int>(WX_GKEY);
#pragma unroll
      for (int j = 0; j < WX_NOUT; ++j) wx_v[j] = wx_t[j];
    }
  }
#endif
#if WX_GROUP_LEAD && WX_GM_MMS == 0
  // The skewed-key wave-combined add of wx_group_multi: grouping by a
  // dimension attribute of a few values puts many lanes of a wave on one bin.
  // Sum-only builds; full waves only.
  if ((wx_u == 0 && wx_e == 0) || wx_lead_on) {
    const wx_u32 wx_lb = wx_pass ? (wx_u32)(wx_gk - wx_a.acc.key_lo) : 0xffffffffu;
    const wx_u32 wx_b0 = (wx_u32)__builtin_amdgcn_readfirstlane((int)wx_lb);
    const wx_u64 wx_m = __builtin_amdgcn_ballot_w64(wx_lb == wx_b0 && wx_b0 < (wx_u32)WX_GWIN);
    const bool wx_shared = __builtin_popcountll(wx_m) >= WX_GROUP_LEAD;
    if (wx_u == 0 && wx_e == 0) wx_lead_on = wx_shared;
    if (wx_shared && __builtin_amdgcn_read_exec() == ~0ull) {
      const bool wx_mine = wx_lb == wx_b0;
      const bool wx_first = (threadIdx.x & 63) == __builtin_ctzll(wx_m);
#pragma unroll
      for (int j = 0; j < WX_NOUT; ++j) {
        const double wx_t = wx::wave_total_f64(wx_mine ? (double)wx_v[j] : 0.0);
        if (wx_first) atomicAdd(&wx_s_sum[wxgm::plane(wxgm::SUMS, j) * WX_GWIN + wx_b0], wx_t);
      }
      if (wx_first) atomicAdd(&wx_s_cnt[wx_b0], (wx_u32)__builtin_popcountll(wx_m));
      wx_pass = wx_pass && !wx_mine;
    }
  }
#endif
  if (wx_pass) {
    const wx_u32 wx_bin = (wx_u32)(wx_gk - wx_a.acc.key_lo);
    if (wx_bin < (wx_u32)WX_GWIN) {
      atomicAdd(&wx_s_cnt[wx_bin], 1u);
#pragma unroll
      for (int j = 0; j < WX_NOUT; ++j) {
        if (wxgm::has(wxgm::SUMS, j)) atomicAdd(&wx_s_sum[wxgm::plane(wxgm::SUMS, j) * WX_GWIN + wx_bin], (double)wx_v[j]);
        if (wxgm::has(wxgm::MMS, j)) {
          const wx_u32 wx_o = wx::f2ord(wx_v[j]);  // NaN -> 0: skipped
          if (wx_o != 0u) {
            atomicMin(&wx_s_min[wxgm::plane(wxgm::MMS, j) * WX_GWIN + wx_bin], wx_o);
            atomicMax(&wx_s_max[wxgm::plane(wxgm::MMS, j) * WX_GWIN + wx_bin], wx_o);
          }
        }
      }
    } else {
      wx_gm_hash_add(wx_a.acc, wx_gk, wx_v);
    }
  }
  WX_STRIDE_LOOP_END
  __syncthreads();
  // the non-empty bins to the global accumulators: one atomic per bin, plane
  // and workgroup
  for (int i = threadIdx.x; i < WX_GWIN; i += wxjg::BLOCK) {
    const wx_u32 c = wx_s_cnt[i];
    if (c) {
      atomicAdd(&wx_a.acc.win_cnt[i], (wx_u64)c);
#pragma unroll
      for (int p = 0; p < wxgm::NS; ++p) atomicAdd(&wx_a.acc.win_sum[p * WX_GWIN + i], wx_s_sum[p * WX_GWIN + i]);
#pragma unroll
      for (int p = 0; p < wxgm::NQ; ++p)
        if (wx_s_max[p * WX_GWIN + i] != 0u) {
          atomicMin(&wx_a.acc.win_min[p * WX_GWIN + i], wx_s_min[p * WX_GWIN + i]);
          atomicMax(&wx_a.acc.win_max[p * WX_GWIN + i], wx_s_max[p * WX_GWIN + i]);
        }
    }
  }
}
#undef WX_LBLOCK
#define WX_LBLOCK WX_BLOCK
#endif
