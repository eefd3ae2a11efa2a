// wx_group_multi.hip -- GROUP BY over several value expressions in one pass:
// the LDS key window + general-key hash of wx_group.hip with one count per
// bin and one accumulator plane per requested aggregate, and their finalize
// (concatenated after wx_common.hip and wx_group_multi_args.h)

// ===========================================================================
#if WX_OP == WX_OP_GROUP_MULTI || defined(WX_JOIN_GROUP)
// (A WX_OP_JOIN_GROUP module, whose prelude defines WX_JOIN_GROUP, takes the
// accumulator layout, the general-key add and the finalize from here; its
// streaming kernel is wx_join_group.hip's, and it may carry a single value.)
// WX_NOUT value expressions (WX_EXPR, WX_EXPR1 .. WX_EXPR3) of the rows of one
// GROUP BY: the key column is read, the condition evaluated and the bin found
// once per row.  Two compile-time masks say what a build carries: bit j of
// WX_GM_SUMS when value j is summed, bit j of WX_GM_MMS when it has a MIN /
// MAX.  There are no NULLs, so every aggregate of a group sees the same rows:
// one count per bin serves all values.  Semantics per value are
// wx_group_sum's: sums of (float) values in double, NaN skipped by MIN / MAX
// (order-mapped u32, 0 = NaN).
#if !defined(WX_NOUT) || WX_NOUT < 1 || WX_NOUT > WX_GM_MAX || (WX_NOUT < 2 && !defined(WX_JOIN_GROUP))
#error "wx_group_multi takes 2 to 4 value expressions (one is wx_group_sum)"
#endif
#if !defined(WX_GM_SUMS) || !defined(WX_GM_MMS)
#error "wx_group_multi needs its sum and min/max masks"
#endif
#if ((WX_GM_SUMS | WX_GM_MMS) != (1 << WX_NOUT) - 1)
#error "every value of wx_group_multi carries a SUM or a MIN / MAX, and no mask bit lies beyond the values"
#endif

#define WX_GWIN WX_GROUP_WINDOW
#ifndef WX_UNROLL
#define WX_UNROLL 2  // row quads per thread per span, as wx_group_sum
#endif
#define WX_HSORT_MAX WX_GROUP_HSORT_MAX
#ifndef WX_GROUP_LEAD
#define WX_GROUP_LEAD 16  // lanes of a wave on one window bin from which they add once (0: off)
#endif

#if WX_NOUT == 1
#define WX_GM_VALS static_cast<float>(WX_EXPR)
#elif WX_NOUT == 2
#define WX_GM_VALS static_cast<float>(WX_EXPR), static_cast<float>(WX_EXPR1)
#elif WX_NOUT == 3
#define WX_GM_VALS static_cast<float>(WX_EXPR), static_cast<float>(WX_EXPR1), static_cast<float>(WX_EXPR2)
#else
#define WX_GM_VALS \
  static_cast<float>(WX_EXPR), static_cast<float>(WX_EXPR1), static_cast<float>(WX_EXPR2), static_cast<float>(WX_EXPR3)
#endif

namespace wxgm {
constexpr int popc(unsigned m) { return m ? (int)(m & 1u) + popc(m >> 1) : 0; }
constexpr unsigned SUMS = WX_GM_SUMS, MMS = WX_GM_MMS;
constexpr int NS = popc(SUMS), NQ = popc(MMS);
constexpr bool has(unsigned mask, int j) { return ((mask >> j) & 1u) != 0u; }
// the accumulator plane of value j: the set bits of the mask below it
constexpr int plane(unsigned mask, int j) { return popc(mask & ((1u << j) - 1u)); }
constexpr int BLOCK = WX_GM_BLOCK(NS, NQ);
constexpr int LDS_BYTES = WX_GM_LDS_BYTES(NS, NQ);
__device__ __forceinline__ float mm_out(wx_u32 m, bool is_min) {
  return (is_min ? m == 0xffffffffu : m == 0u) ? __uint_as_float(0x7fc00000u) : wx::ord2f(m);
}
}  // namespace wxgm

// A key outside the window: the slot is claimed by CAS exactly as
// wx_group_sum's wx_hash_add claims it, then the count and each plane.
__device__ __forceinline__ void wx_gm_hash_add(const WxGroupMultiArgs &a, int key, const float (&v)[WX_NOUT]) {
  const wx_u64 tag = (wx_u64)(wx_u32)key | (1ull << 32);
  const wx_u64 hcap = (wx_u64)a.hmask + 1ull;
  wx_u32 h = ((wx_u32)key * 2654435761u) & a.hmask;
  for (wx_u32 probe = 0; probe <= a.hmask; ++probe) {
    wx_u64 cur = wx::ld_agent(&a.h_tag[h]);
    if (cur == 0ull) {
      const wx_u64 prev = atomicCAS(&a.h_tag[h], 0ull, tag);
      if (prev == 0ull) {
        const wx_u64 u = __hip_atomic_fetch_add(&a.ctrs[0], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a.h_used[u] = h;
        cur = tag;
      } else {
        cur = prev;
      }
    }
    if (cur == tag) {
      atomicAdd(&a.h_cnt[h], 1ull);
#pragma unroll
      for (int j = 0; j < WX_NOUT; ++j) {
        if (wxgm::has(wxgm::SUMS, j)) atomicAdd(&a.h_sum[wxgm::plane(wxgm::SUMS, j) * hcap + h], (double)v[j]);
        if (wxgm::has(wxgm::MMS, j)) {
          const wx_u32 o = wx::f2ord(v[j]);  // NaN -> 0: skipped
          if (o != 0u) {
            atomicMin(&a.h_min[wxgm::plane(wxgm::MMS, j) * hcap + h], o);
            atomicMax(&a.h_max[wxgm::plane(wxgm::MMS, j) * hcap + h], o);
          }
        }
      }
      return;
    }
    h = (h + 1) & a.hmask;
  }
  atomicOr(reinterpret_cast<unsigned int *>(&a.ctrs[1]), WX_DEVERR_CAPACITY);
}

#if WX_OP == WX_OP_GROUP_MULTI
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
    const wx_u32 wx_lb = wx_pass ? (wx_u32)(static_cast<int>(WX_KEY) - wx_a.key_lo) : 0xffffffffu;
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
    const wx_u32 wx_bin = (wx_u32)(wx_key - wx_a.key_lo);
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
      wx_gm_hash_add(wx_a, wx_key, wx_v);
    }
  }
  WX_STRIDE_LOOP_END
  __syncthreads();
  // the non-empty bins to the global accumulators: one atomic per bin, plane
  // and workgroup
  for (int i = threadIdx.x; i < WX_GWIN; i += wxgm::BLOCK) {
    const wx_u32 c = wx_s_cnt[i];
    if (c) {
      atomicAdd(&wx_a.win_cnt[i], (wx_u64)c);
#pragma unroll
      for (int p = 0; p < wxgm::NS; ++p) atomicAdd(&wx_a.win_sum[p * WX_GWIN + i], wx_s_sum[p * WX_GWIN + i]);
#pragma unroll
      for (int p = 0; p < wxgm::NQ; ++p)
        if (wx_s_max[p * WX_GWIN + i] != 0u) {
          atomicMin(&wx_a.win_min[p * WX_GWIN + i], wx_s_min[p * WX_GWIN + i]);
          atomicMax(&wx_a.win_max[p * WX_GWIN + i], wx_s_max[p * WX_GWIN + i]);
        }
    }
  }
}

#undef WX_LBLOCK
#define WX_LBLOCK WX_BLOCK
#endif

// One 1024-thread block, as wx_group_finalize: sort the general-key entries
// (in LDS, or read them pre-sorted), merge with the dense window in
// ascending key order, write the keys, the counts and each requested plane,
// and return every accumulator touched to its idle value -- the count window,
// the table and the counter word are wx_group_sum's too.
#define WX_GMF_BLOCK 1024
static_assert(WX_GWIN == 2 * WX_GMF_BLOCK, "two window bins per finalize thread");
extern "C" __global__ __launch_bounds__(WX_GMF_BLOCK) void wx_group_multi_finalize(WxGroupMultiFinArgs a) {
  __shared__ wx_u64 s_ent[WX_HSORT_MAX];  // (key ^ sign) << 32 | used-list position
  __shared__ wx_u32 s_wtot[WX_GMF_BLOCK / 64];
  __shared__ wx_i64 s_nlo;
  constexpr int NT = WX_GMF_BLOCK;
  constexpr int BPT = WX_GWIN / NT;
  const int tid = threadIdx.x;
  const wx_u64 hcap = (wx_u64)a.hmask + 1ull;
  const wx_i64 n_hash = (wx_i64)a.ctrs[0];
  const bool presorted = a.sorted != nullptr;
  const bool too_many = n_hash > WX_HSORT_MAX && !presorted;
  if (too_many) {
    if (tid == 0) atomicOr(reinterpret_cast<unsigned int *>(&a.ctrs[1]), WX_DEVERR_UNSUPPORTED);
  }
  const wx_i64 nh = too_many ? 0 : n_hash;
  int npad = 1;
  while (!presorted && npad < nh) npad <<= 1;
#define WX_ENT(i) (presorted ? a.sorted[(i)] : s_ent[(i)])
  const int b0 = tid * BPT;
  wx_u64 wc[BPT];
#pragma unroll
  for (int h = 0; h < BPT; ++h) wc[h] = a.win_cnt[b0 + h];
  for (int i = tid; !presorted && i < npad; i += NT) {
    wx_u64 e = ~0ull;
    if (i < nh) {
      const wx_u32 slot = a.h_used[i];
      const wx_u32 key = (wx_u32)a.h_tag[slot];
      e = ((wx_u64)(key ^ 0x80000000u) << 32) | (wx_u32)i;
    }
    s_ent[i] = e;
  }
  __syncthreads();
  for (int k = 2; !presorted && k <= npad; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < npad; i += NT) {
        const int p = i ^ j;
        if (p > i) {
          const wx_u64 x = s_ent[i], y = s_ent[p];
          const bool up = (i & k) == 0;
          if ((x > y) == up) { s_ent[i] = y; s_ent[p] = x; }
        }
      }
      __syncthreads();
    }
  // number of hash keys below the window (binary search in key order)
  if (tid == 0) {
    wx_i64 lo = 0, hi = nh;
    while (lo < hi) {
      const wx_i64 mid = (lo + hi) >> 1;
      if ((int)((wx_u32)(WX_ENT(mid) >> 32) ^ 0x80000000u) < a.key_lo) lo = mid + 1;
      else hi = mid;
    }
    s_nlo = lo;
  }
  __syncthreads();
  const wx_i64 nlo = s_nlo;
  // dense window compaction (ascending bins): wave scan + wave totals
  const int lane = tid & 63, wave = tid >> 6;
  wx_u32 f = 0u;
#pragma unroll
  for (int h = 0; h < BPT; ++h) f += wc[h] ? 1u : 0u;
  wx_u32 incl = f;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const wx_u32 t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  if (lane == 63) s_wtot[wave] = incl;
  __syncthreads();
  wx_u32 wbase = 0, wsum = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const wx_u32 v = s_wtot[w];
    wbase += (w < wave) ? v : 0u;
    wsum += v;
  }
  {
    wx_i64 pos = nlo + wbase + incl - f;
#pragma unroll
    for (int h = 0; h < BPT; ++h) {
      const int b = b0 + h;
      const wx_u64 c = wc[h];
      if (!c) continue;
      const bool out = pos < a.capacity;
      if (out) {
        a.out_keys[pos] = a.key_lo + b;
        a.out_counts[pos] = (wx_i64)c;
      }
      a.win_cnt[b] = 0ull;
#pragma unroll
      for (int j = 0; j < WX_NOUT; ++j) {
        if (wxgm::has(wxgm::SUMS, j)) {
          double *const acc = &a.win_sum[wxgm::plane(wxgm::SUMS, j) * WX_GWIN + b];
          if (out && a.out_sums[j]) a.out_sums[j][pos] = *acc;
          *acc = 0.0;
        }
        if (wxgm::has(wxgm::MMS, j)) {
          wx_u32 *const mn = &a.win_min[wxgm::plane(wxgm::MMS, j) * WX_GWIN + b];
          wx_u32 *const mx = &a.win_max[wxgm::plane(wxgm::MMS, j) * WX_GWIN + b];
          if (out && a.out_mins[j]) a.out_mins[j][pos] = wxgm::mm_out(*mn, true);
          if (out && a.out_maxs[j]) a.out_maxs[j][pos] = wxgm::mm_out(*mx, false);
          *mn = 0xffffffffu;
          *mx = 0u;
        }
      }
      ++pos;
    }
  }
  const wx_i64 out_pos = nlo + wsum;
  // hash entries: below-window ones first, the rest after the window
  for (wx_i64 i = tid; i < nh; i += NT) {
    const wx_u64 e = WX_ENT(i);
    const wx_u32 slot = a.h_used[(wx_u32)e];
    const wx_i64 pos = (i < nlo) ? i : out_pos + (i - nlo);
    if (pos < a.capacity) {
      a.out_keys[pos] = (int)((wx_u32)(e >> 32) ^ 0x80000000u);
      a.out_counts[pos] = (wx_i64)a.h_cnt[slot];
#pragma unroll
      for (int j = 0; j < WX_NOUT; ++j) {
        if (wxgm::has(wxgm::SUMS, j) && a.out_sums[j])
          a.out_sums[j][pos] = a.h_sum[wxgm::plane(wxgm::SUMS, j) * hcap + slot];
        if (wxgm::has(wxgm::MMS, j)) {
          if (a.out_mins[j]) a.out_mins[j][pos] = wxgm::mm_out(a.h_min[wxgm::plane(wxgm::MMS, j) * hcap + slot], true);
          if (a.out_maxs[j]) a.out_maxs[j][pos] = wxgm::mm_out(a.h_max[wxgm::plane(wxgm::MMS, j) * hcap + slot], false);
        }
      }
    }
  }
  __syncthreads();
  const wx_i64 total = out_pos + (nh - nlo);
  // return the general-key table to its clean state
  for (wx_i64 i = tid; i < n_hash; i += NT) {
    const wx_u32 slot = a.h_used[i];
    a.h_tag[slot] = 0ull;
    a.h_cnt[slot] = 0ull;
#pragma unroll
    for (int p = 0; p < wxgm::NS; ++p) a.h_sum[p * hcap + slot] = 0.0;
#pragma unroll
    for (int p = 0; p < wxgm::NQ; ++p) {
      a.h_min[p * hcap + slot] = 0xffffffffu;
      a.h_max[p * hcap + slot] = 0u;
    }
  }
  if (tid == 0) {
    a.ctrs[0] = 0ull;
    *a.n_groups_out = too_many ? -1 : total;
    if (total > a.capacity) atomicOr(reinterpret_cast<unsigned int *>(&a.ctrs[1]), WX_DEVERR_CAPACITY);
  }
#undef WX_ENT
}
#endif
