// wx_group_window.hip -- what the multi-value GROUP BY (wx_group_multi.hip) and
// the JOIN under GROUP BY (wx_join_group.hip) share beside their streaming
// kernels: the build checks, the wxgm constants, the general-key add and the
// finalize over the LDS key window + general-key hash.  Concatenated after
// wx_common.hip, wx_block.hip and wx_group_multi_args.h, ahead of
// wx_group_multi.hip.  (wx_group_sum of wx_group.hip is the NS = 1, NQ <= 1
// case with the same LDS layout; its text is pinned, so it keeps its copy.)

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
__device__ __forceinline__ float mm_out(wx_u32 m, bool is_min) {
  return (is_min ? m == 0xffffffffu : m == 0u) ? __uint_as_float(0x7fc00000u) : wx::ord2f(m);
}
}  // namespace wxgm

// A key outside the window: the slot is claimed by CAS exactly as
// wx_group_sum's wx_hash_add claims it, then the count and each plane.
__device__ __forceinline__ void wx_gm_hash_add(const WxGroupPlanes &a, int key, const float (&v)[WX_NOUT]) {
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
  const wx_u64 hcap = (wx_u64)a.acc.hmask + 1ull;
  const wx_i64 n_hash = (wx_i64)a.acc.ctrs[0];
  const bool presorted = a.sorted != nullptr;
  const bool too_many = n_hash > WX_HSORT_MAX && !presorted;
  if (too_many) {
    if (tid == 0) atomicOr(reinterpret_cast<unsigned int *>(&a.acc.ctrs[1]), WX_DEVERR_UNSUPPORTED);
  }
  const wx_i64 nh = too_many ? 0 : n_hash;
  int npad = 1;
  while (!presorted && npad < nh) npad <<= 1;
#define WX_ENT(i) (presorted ? a.sorted[(i)] : s_ent[(i)])
  const int b0 = tid * BPT;
  wx_u64 wc[BPT];
#pragma unroll
  for (int h = 0; h < BPT; ++h) wc[h] = a.acc.win_cnt[b0 + h];
  for (int i = tid; !presorted && i < npad; i += NT) {
    wx_u64 e = ~0ull;
    if (i < nh) {
      const wx_u32 slot = a.acc.h_used[i];
      const wx_u32 key = (wx_u32)a.acc.h_tag[slot];
      e = ((wx_u64)(key ^ 0x80000000u) << 32) | (wx_u32)i;
    }
    s_ent[i] = e;
  }
  __syncthreads();
  WX_BITONIC_LDS(s_ent, npad, tid, NT, !presorted)
  // number of hash keys below the window (binary search in key order)
  if (tid == 0) {
    wx_i64 lo = 0, hi = nh;
    while (lo < hi) {
      const wx_i64 mid = (lo + hi) >> 1;
      if ((int)((wx_u32)(WX_ENT(mid) >> 32) ^ 0x80000000u) < a.acc.key_lo) lo = mid + 1;
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
        a.out_keys[pos] = a.acc.key_lo + b;
        a.out_counts[pos] = (wx_i64)c;
      }
      a.acc.win_cnt[b] = 0ull;
#pragma unroll
      for (int j = 0; j < WX_NOUT; ++j) {
        if (wxgm::has(wxgm::SUMS, j)) {
          double *const acc = &a.acc.win_sum[wxgm::plane(wxgm::SUMS, j) * WX_GWIN + b];
          if (out && a.out_sums[j]) a.out_sums[j][pos] = *acc;
          *acc = 0.0;
        }
        if (wxgm::has(wxgm::MMS, j)) {
          wx_u32 *const mn = &a.acc.win_min[wxgm::plane(wxgm::MMS, j) * WX_GWIN + b];
          wx_u32 *const mx = &a.acc.win_max[wxgm::plane(wxgm::MMS, j) * WX_GWIN + b];
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
    const wx_u32 slot = a.acc.h_used[(wx_u32)e];
    const wx_i64 pos = (i < nlo) ? i : out_pos + (i - nlo);
    if (pos < a.capacity) {
      a.out_keys[pos] = (int)((wx_u32)(e >> 32) ^ 0x80000000u);
      a.out_counts[pos] = (wx_i64)a.acc.h_cnt[slot];
#pragma unroll
      for (int j = 0; j < WX_NOUT; ++j) {
        if (wxgm::has(wxgm::SUMS, j) && a.out_sums[j])
          a.out_sums[j][pos] = a.acc.h_sum[wxgm::plane(wxgm::SUMS, j) * hcap + slot];
        if (wxgm::has(wxgm::MMS, j)) {
          if (a.out_mins[j]) a.out_mins[j][pos] = wxgm::mm_out(a.acc.h_min[wxgm::plane(wxgm::MMS, j) * hcap + slot], true);
          if (a.out_maxs[j]) a.out_maxs[j][pos] = wxgm::mm_out(a.acc.h_max[wxgm::plane(wxgm::MMS, j) * hcap + slot], false);
        }
      }
    }
  }
  __syncthreads();
  const wx_i64 total = out_pos + (nh - nlo);
  // return the general-key table to its clean state
  for (wx_i64 i = tid; i < n_hash; i += NT) {
    const wx_u32 slot = a.acc.h_used[i];
    a.acc.h_tag[slot] = 0ull;
    a.acc.h_cnt[slot] = 0ull;
#pragma unroll
    for (int p = 0; p < wxgm::NS; ++p) a.acc.h_sum[p * hcap + slot] = 0.0;
#pragma unroll
    for (int p = 0; p < wxgm::NQ; ++p) {
      a.acc.h_min[p * hcap + slot] = 0xffffffffu;
      a.acc.h_max[p * hcap + slot] = 0u;
    }
  }
  if (tid == 0) {
    a.acc.ctrs[0] = 0ull;
    *a.n_groups_out = too_many ? -1 : total;
    if (total > a.capacity) atomicOr(reinterpret_cast<unsigned int *>(&a.acc.ctrs[1]), WX_DEVERR_CAPACITY);
  }
#undef WX_ENT
}
