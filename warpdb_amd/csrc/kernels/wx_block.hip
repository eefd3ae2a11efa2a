// wx_block.hip -- workgroup-wide building blocks of the GROUP BY kernels.
// Concatenated after wx_common.hip for the util, multi-value GROUP BY and
// grouped-join modules only: every other module's text stays what it was.

// s[0 .. npad) ascending by the in-LDS bitonic network (wx_u64 *s; npad a
// power of two; written and fenced by the caller), by a workgroup of NT
// threads of which this one is tid; every step ends behind a barrier.  `on`
// is workgroup-uniform: false skips the sort and its barriers.  (A macro and
// not a function: as an inlined function the same loops compile to other
// registers and compares than the two copies this replaces,
// profiles/group_window_refactor.txt.)
#define WX_BITONIC_LDS(s, npad, tid, NT, on)                                   \
  for (int wx_k = 2; (on) && wx_k <= (npad); wx_k <<= 1)                       \
    for (int wx_j = wx_k >> 1; wx_j > 0; wx_j >>= 1) {                         \
      for (int wx_i = (tid); wx_i < (npad); wx_i += (NT)) {                    \
        const int wx_p = wx_i ^ wx_j;                                          \
        if (wx_p > wx_i) {                                                     \
          const wx_u64 wx_x = (s)[wx_i], wx_y = (s)[wx_p];                     \
          const bool wx_up = (wx_i & wx_k) == 0;                               \
          if ((wx_x > wx_y) == wx_up) { (s)[wx_i] = wx_y; (s)[wx_p] = wx_x; } \
        }                                                                      \
      }                                                                        \
      __syncthreads();                                                         \
    }
