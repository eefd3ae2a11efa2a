// wx_group_multi.hip -- GROUP BY over several value expressions in one pass:
// the stream of a table into the LDS key window + general-key hash of
// wx_group.hip with one count per bin and one accumulator plane per requested
// aggregate (concatenated after wx_common.hip, wx_block.hip,
// wx_group_multi_args.h and wx_group_window.hip, which has the general-key
// add and the finalize)

// ===========================================================================
#if WX_OP == WX_OP_GROUP_MULTI || defined(WX_JOIN_GROUP)
// (A WX_OP_JOIN_GROUP module, whose prelude defines WX_JOIN_GROUP, streams
// with wx_join_group.hip's kernel at this geometry.)
#ifndef WX_UNROLL
#define WX_UNROLL 2  // row quads per thread per span, as wx_group_sum
#endif

#if WX_OP == WX_OP_GROUP_MULTI
namespace wxgm {
constexpr int BLOCK = WX_GM_BLOCK(NS, NQ);
constexpr int LDS_BYTES = WX_GM_LDS_BYTES(NS, NQ);
}  // namespace wxgm

#undef WX_LBLOCK
#define WX_LBLOCK (wxgm::BLOCK)
extern "C" __global__ __launch_bounds__(WX_GM_BLOCK(wxgm::NS, wxgm::NQ)) void wx_group_multi(WxGroupMultiArgs wx_a) {
  // [NS][W] f64 sums | [W] u32 counts | [NQ][W] u32 minima | [NQ][W] u32 maxima
  __shared__ __attribute__((aligned(16))) unsigned char wx_lds[wxgm::LDS_BYTES];
  double *const wx_s_sum = reinterpret_cast<double *>(wx_lds);
  wx_u32 *const wx_s_cnt = reinterpret_cast<wx_u32 *>(wx_lds + (wx_u64)wxgm::NS * WX_GWIN * 8);
  wx_u32 *const wx_s_min = wx_s_cnt + WX_GWIN;
  wx_u32 *const wx_s_max = wx_s_min + (wx_u64)wxgm::NQ * WX_GWIN;
  for (int i = threadIdx.x; i < WX_GWIN; i += wxgm::BLOCK) {
    wx_s_cnt[i] = 0u;
#pragma unroll
    for (int p = 0; p < wxgm::NS; ++p) wx_s_sum[p * WX_GWIN + i] = 0.0;
#pragma unroll
    for (int p = 0; p < wxgm::NQ; ++p) {
      wx_s_min[p * WX_GWIN + i] = 0xffffffffu;
      wx_s_max[p * WX_GWIN + i] = 0u;
    }
  }
  __syncthreads();
  bool wx_lead_on = false;  // this batch's first rows had a bin shared by many lanes
  WX_STRIDE_LOOP_BEGIN
  bool wx_pass = idx < wx_a.n_rows && WX_EVAL_COND();
#if WX_GROUP_LEAD && WX_GM_MMS == 0
  // The skewed-key wave-combined add of wx_group_sum (its comment has the
  // measurements), one DPP total per summed value for the lanes that share
  // the first lane's bin.  Sum-only builds; full waves only.
  if ((wx_u == 0 && wx_e == 0) || wx_lead_on) {
    const wx_u32 wx_lb = wx_pass ? (wx_u32)(static_cast<int>(WX_KEY) - wx_a.acc.key_lo) : 0xffffffffu;
    const wx_u32 wx_b0 = (wx_u32)__builtin_amdgcn_readfirstlane((int)wx_lb);
    const wx_u64 wx_m = __builtin_amdgcn_ballot_w64(wx_lb == wx_b0 && wx_b0 < (wx_u32)WX_GWIN);
    const bool wx_shared = __builtin_popcountll(wx_m) >= WX_GROUP_LEAD;
    if (wx_u == 0 && wx_e == 0) wx_lead_on = wx_shared;
    if (wx_shared && __builtin_amdgcn_read_exec() == ~0ull) {
      const bool wx_mine = wx_lb == wx_b0;
      const float wx_lv[WX_NOUT] = {WX_GM_VALS};
      const bool wx_first = (threadIdx.x & 63) == __builtin_ctzll(wx_m);
#pragma unroll
      for (int j = 0; j < WX_NOUT; ++j) {
        const double wx_t = wx::wave_total_f64(wx_mine ? (double)wx_lv[j] : 0.0);
        if (wx_first) atomicAdd(&wx_s_sum[wxgm::plane(wxgm::SUMS, j) * WX_GWIN + wx_b0], wx_t);
      }
      if (wx_first) atomicAdd(&wx_s_cnt[wx_b0], (wx_u32)__builtin_popcountll(wx_m));
      wx_pass = wx_pass && !wx_mine;
    }
  }
#endif
  if (wx_pass) {
    const int wx_key = static_cast<int>(WX_KEY);
    const float wx_v[WX_NOUT] = {WX_GM_VALS};
    const wx_u32 wx_bin = (wx_u32)(wx_key - wx_a.acc.key_lo);
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
      wx_gm_hash_add(wx_a.acc, wx_key, wx_v);
    }
  }
  WX_STRIDE_LOOP_END
  __syncthreads();
  // the non-empty bins to the global accumulators: one atomic per bin, plane
  // and workgroup
  for (int i = threadIdx.x; i < WX_GWIN; i += wxgm::BLOCK) {
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
#endif
