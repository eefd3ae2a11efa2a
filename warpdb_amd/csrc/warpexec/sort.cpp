// sort.cpp -- the util module and the sorts: LSD radix (wx_radix.hip) and
// the bitonic network (wx_util.hip).
#include "wx_host.hpp"

namespace wx {

std::shared_ptr<Module> util_module(int dev, bool load, const std::string &more) {
  return get_module(dev, util_spec(more), load);
}

// Radix tile geometry (workgroup size x keys per lane), measured per kind
// in one process per A/B (profiles/r05/ab_sort_geometry.txt): keys alone
// 1024 x 32 (one 147 KB workgroup per CU; 10.75-11.3 ms per 1e9 keys against
// 11.45 for round 4's 512 x 32, whose two workgroups per CU walk twice the
// look-back chains; with the permutation ahead of the look-back and plain
// stores 8.67 ms, ab_sort_split_store.txt) with three predecessor words per
// look-back round -- the util module's default; key + payload 512 x 28 (one
// 120 KB workgroup per CU, 18.5 ms per 1e9 pairs against 20.8 for 512 x 20;
// 512 x 32 spills, 23.5) with four, a module of its own.  A diagnostic build
// may set WX_RS_BLOCK / WX_RS_ITEMS in $WARPDB_EXTRA_DEFINES; the host reads
// them back from there so its tile count matches the kernel's.  rs_geometry
// returns the extra defines of the module with the kernels.
// The in-wave ranking by one returning LDS add per key (WX_RS_RANK_ATOMIC)
// is stable only because the LDS returns same-address results in ascending
// lane order -- observed and tested on gfx950, not documented.  Any other
// target builds the peer-mask ranking (WX_RS_RANK_ATOMIC=0) until its own
// heavy-tie sort tests pass with the atomic form ($WARPDB_RS_RANK_ATOMIC=1
// forces it, =0 forbids it: a test hook for both forms).
std::string rs_rank_extra(const std::string &arch) {
  const std::string f = env_or("WARPDB_RS_RANK_ATOMIC", "");
  if (f == "1") return "";
  if (f == "0" || arch.compare(0, 6, "gfx950") != 0) return ",WX_RS_RANK_ATOMIC=0";
  return "";
}

// The part of rs_geometry that needs no device: items x block of the key
// (or key + payload) tile, the define list's overrides applied and checked.
void rs_tile_shape(bool pairs, int *items, int *block) {
  const std::string extra = env_or("WARPDB_EXTRA_DEFINES", "");
  *items = define_value(extra, "WX_RS_ITEMS", pairs ? 28 : WX_RS_ITEMS);
  *block = define_value(extra, "WX_RS_BLOCK", pairs ? 512 : WX_RS_BLOCK);
  if (*block < 256 || *block > 1024 || *block % 64) fail(WX_ERR_INVALID, "WX_RS_BLOCK must be 256..1024, a multiple of 64");
  if (*items < 1 || *items > 64) fail(WX_ERR_INVALID, "WX_RS_ITEMS must be 1..64");
}

std::string rs_geometry(bool pairs, int *items, int *block, const std::string &arch) {
  rs_tile_shape(pairs, items, block);
  const std::string rank = rs_rank_extra(arch);
  if (!pairs) return rank;
  return ",WX_RS_ITEMS=" + std::to_string(*items) + ",WX_RS_BLOCK=" + std::to_string(*block) +
         ",WX_RS_LBW=4" + rank;
}

// Ascending sort of npad (a power of two >= WX_SORT_LDS) 64-bit keys in
// place: LDS passes for spans up to WX_SORT_LDS, global passes above.
void bitonic_u64(int dev, wx_u64 *keys, int64_t npad, hipStream_t s) {
  auto mod = util_module(dev, true, "");
  DeviceState &d = device_state(dev, true);
  const unsigned lds_blocks = (unsigned)(npad / WX_SORT_LDS);
  WxSortPassArgs q;
  q.keys = keys;
  q.npad = npad;
  q.k = 2;
  q.j = WX_SORT_LDS;
  launch(mod->fn("wx_bitonic_lds"), lds_blocks, &q, s);
  for (int64_t k = 2 * WX_SORT_LDS; k <= npad; k <<= 1) {
    for (int64_t j = k >> 1; j >= WX_SORT_LDS; j >>= 1) {
      WxSortPassArgs gp;
      gp.keys = keys;
      gp.npad = npad;
      gp.k = k;
      gp.j = j;
      launch(mod->fn("wx_bitonic_global"), grid_for(npad, d.cus, 8), &gp, s);
    }
    WxSortPassArgs lp;
    lp.keys = keys;
    lp.npad = npad;
    lp.k = k;
    lp.j = k;
    launch(mod->fn("wx_bitonic_lds"), lds_blocks, &lp, s);
  }
}

// Stable LSD radix sort (wx_radix_hist + up to four wx_radix_tile_*):
// `d_a` holds float values (kind 0) or int keys (kind 1, `d_v` their float
// payload); the sorted result ends in the caller's buffers.
// `src0` (keys only, nullable): the first pass reads the keys from there
// instead of `d_a` (ORDER BY a bare column: the column itself, no projection
// copy); `src0` is never written and the result still ends in `d_a`.
void radix_sort(void *d_a, float *d_v, int64_t count, int kind, int32_t ascending, const wx_launch &L, Workspace &w,
                hipStream_t s, int64_t limit, const void *src0, void **res_k, float **res_v, const float *src_v) {
  if (src0 == d_a) src0 = nullptr;
  const void *in_k = src0 ? src0 : d_a;
  int items = 0, rs_block = 0;
  const std::string more = rs_geometry(d_v != nullptr, &items, &rs_block, device_state(L.device, true).arch);
  const int64_t rs_tile = (int64_t)items * rs_block;
  auto mod = util_module(L.device, true, more);
  DeviceState &d = device_state(L.device, true);
  const bool timed = (L.flags & WX_F_TIME) != 0;
  // [0, 1024): the four digit histograms; [1024, 2048): digit bases;
  // [2048]: a float key was NaN or -0.0 (the general order map is needed)
  ensure(w, w.rs_hist, 2 * 1024 * 4 + 256, false);
  wx_u32 *hist = static_cast<wx_u32 *>(w.rs_hist.p), *bases = hist + 1024;
  WX_HIP(hipMemsetAsync(hist, 0, 1024 * 4, s));
  WX_HIP(hipMemsetAsync(hist + 2048, 0, 4, s));
  WxRadixHistArgs h;
  h.src = static_cast<const wx_u32 *>(in_k);
  h.n = count;
  h.hist = hist;
  h.aligned = aligned16(in_k) ? 1 : 0;
  const std::string hname = std::string("wx_radix_hist_") + (kind == 0 ? "f_" : "i_") + (ascending ? "a" : "d");
  // one 1024-thread workgroup per CU (128 KB of counters)
  launch(mod->fn(hname.c_str()), grid_for((count + 15) / 16 / 4, d.cus, 1), &h, s, timed, 1024);
  std::vector<wx_u32> hh(1025), base(1024);
  WX_HIP(hipMemcpyAsync(hh.data(), hist, 1024 * 4, hipMemcpyDeviceToHost, s));
  WX_HIP(hipMemcpyAsync(hh.data() + 1024, hist + 2048, 4, hipMemcpyDeviceToHost, s));
  WX_HIP(hipStreamSynchronize(s));
  // float keys with no NaN and no -0.0: the tile kernels' plain order flip
  // (same order, 2 ops instead of 9 per digit; $WARPDB_RS_PLAIN=0 turns it off)
  const bool plain = kind == 0 && hh[1024] == 0 && env_or("WARPDB_RS_PLAIN", "1") != "0";
  bool skip[4];
  for (int p = 0; p < 4; ++p) {
    uint64_t run = 0;
    skip[p] = false;
    for (int dg = 0; dg < 256; ++dg) {
      base[p * 256 + dg] = (wx_u32)run;
      run += hh[p * 256 + dg];
      if ((int64_t)hh[p * 256 + dg] == count) skip[p] = true;  // one digit for every key: identity pass
    }
    if ((int64_t)run != count)
      fail(WX_ERR_INTERNAL, "radix histogram does not add up (digit " + std::to_string(p) + ": " +
                                std::to_string(run) + " of " + std::to_string(count) + " keys)");
  }
  WX_HIP(hipMemcpyAsync(bases, base.data(), 1024 * 4, hipMemcpyHostToDevice, s));
  const int64_t n_tiles = (count + rs_tile - 1) / rs_tile;
  const size_t status_bytes = (size_t)n_tiles * 256 * 8;
  void *old_status = w.rs_status.p;
  ensure(w, w.rs_status, status_bytes, true);
  if (w.rs_status.p != old_status) w.rs_epoch = 0;  // fresh, zeroed words
  // [2 * pass]: ticket, abort; words 16..47: diagnostic look-back statistics;
  // words 64..191: diagnostic phase times (u64, 8 per pass)
  ensure(w, w.rs_ctl, 1024, false);
  WX_HIP(hipMemsetAsync(w.rs_ctl.p, 0, 1024, s));
  ensure(w, w.rs_tmp_k, (size_t)count * 4, false);
  if (d_v) ensure(w, w.rs_tmp_v, (size_t)count * 4, false);
  void *cur_k = const_cast<void *>(in_k), *alt_k = w.rs_tmp_k.p;
  // src_v (with d_v): the first executed pass reads the payload from there
  // instead of d_v, and the passes then ping-pong between the scratch and d_v
  // (src_v is never written)
  void *cur_v = d_v && src_v ? const_cast<float *>(src_v) : d_v, *alt_v = d_v ? w.rs_tmp_v.p : nullptr;
  // One kernel per (payload, key kind, direction): the key map is compiled
  // in.  One workgroup per tile, tiles in ticket order.
  const std::string kname = std::string("wx_radix_tile_") + (d_v ? "kv_" : "k_") +
                            (kind == 0 ? (plain ? "fp_" : "f_") : "i_") + (ascending ? "a" : "d");
  hipFunction_t fn = mod->fn(kname.c_str());
  const unsigned grid = (unsigned)n_tiles;  // one tile per workgroup (persistent workgroups measured 3.3x slower)
  // ORDER BY .. LIMIT: only the first `limit` keys of the sorted order are
  // wanted.  They all lie in the top-digit buckets up to the one holding
  // rank limit - 1 (cumulative count `head`); one stable pass on the top
  // digit moves those buckets, in order, to the front, and only that head
  // is sorted in full.  Worth it when the head is a small part of the array.
  int64_t head = count;
  if (limit >= 0 && limit < count && !skip[3]) {
    int64_t run = 0;
    for (int dg = 0; dg < 256 && run < std::max<int64_t>(limit, 1); ++dg) run += hh[3 * 256 + dg];
    if (run <= count / 4) head = run;
  }
  const bool partial = head < count;
  if (src0) {  // ping-pong between d_a and the scratch so that the last executed pass writes d_a
    int executed = 0;
    for (int p = partial ? 3 : 0; p < 4; ++p) executed += skip[p] ? 0 : 1;
    alt_k = executed % 2 ? d_a : w.rs_tmp_k.p;
  }
  for (int p = partial ? 3 : 0; p < 4; ++p) {
    if (skip[p]) continue;
    if (++w.rs_epoch > WX_RS_EPOCHS) {  // epoch numbers exhausted: clear every word once
      WX_HIP(hipMemsetAsync(w.rs_status.p, 0, w.rs_status.bytes, s));
      w.rs_epoch = 1;
    }
    WxRadixPassArgs a;
    a.src_k = static_cast<const wx_u32 *>(cur_k);
    a.dst_k = static_cast<wx_u32 *>(alt_k);
    a.src_v = static_cast<const wx_u32 *>(cur_v);
    a.dst_v = static_cast<wx_u32 *>(alt_v);
    a.digit_base = bases + p * 256;
    a.status = static_cast<wx_u64 *>(w.rs_status.p);
    a.ctl = static_cast<wx_u32 *>(w.rs_ctl.p) + 2 * p;
    a.err = reinterpret_cast<wx_u32 *>(static_cast<wx_u64 *>(w.ctrs.p) + 1);
    a.lbd = static_cast<wx_u64 *>(w.ctrs.p) + WX_LBD_BASE;
    a.n = count;
    a.shift = 8 * p;
    a.kind = kind;
    a.ascending = ascending ? 1 : 0;
    a.epoch = w.rs_epoch;
    // lane 0's digit group ranked by one ballot (a few-valued digit -- the
    // exponent byte of uniform floats, ~60 % on one value -- would serialize
    // the ranking's LDS adds on one counter).  On every pass: ranking by the
    // plain LDS add on the passes without a skewed digit ($WARPDB_RS_LEAD=auto:
    // where no digit holds > 1/16 of the keys) measured slower, keys 12.37 vs
    // 12.24 ms per 1e9, pairs 18.02 vs 18.05 (profiles/r03/abl_sort_plain_lead.txt)
    uint32_t top = 0;
    for (int dg = 0; dg < 256; ++dg) top = std::max<uint32_t>(top, hh[p * 256 + dg]);
    const std::string lead_env = env_or("WARPDB_RS_LEAD", "1");
    a.lead = lead_env == "1" ? 1 : lead_env == "0" ? 0 : ((int64_t)top * 16 > count ? 1 : 0);
    launch(fn, grid, &a, s, timed, (unsigned)rs_block);
    cur_k = alt_k;
    alt_k = cur_k == d_a ? w.rs_tmp_k.p : d_a;  // never src0
    const bool from_src_v = d_v && src_v && cur_v == src_v;
    std::swap(cur_v, alt_v);
    if (from_src_v) alt_v = d_v;  // never src_v
  }
  if (partial) {  // the head, still in input order within each bucket, then a full sort of it
    if (cur_k != d_a) WX_HIP(hipMemcpyAsync(d_a, cur_k, (size_t)head * 4, hipMemcpyDeviceToDevice, s));
    if (d_v) WX_HIP(hipMemcpyAsync(d_v, cur_v, (size_t)head * 4, hipMemcpyDeviceToDevice, s));
    WX_HIP(hipStreamSynchronize(s));  // `base` (pageable) must outlive its copy
    radix_sort(d_a, d_v, head, kind, ascending, L, w, s);
    return;
  }
  if (res_k) {  // the caller reads the sorted keys (and payload) wherever the last pass left them
    *res_k = cur_k;
    if (res_v) *res_v = static_cast<float *>(cur_v);
  } else {
    if (cur_k != d_a) WX_HIP(hipMemcpyAsync(d_a, cur_k, (size_t)count * 4, hipMemcpyDeviceToDevice, s));
    // (the payload's ping-pong need not end where the keys' does once either starts from a source)
    if (d_v && cur_v != d_v) WX_HIP(hipMemcpyAsync(d_v, cur_v, (size_t)count * 4, hipMemcpyDeviceToDevice, s));
  }
  WX_HIP(hipStreamSynchronize(s));  // `base` (pageable) must outlive its copy; the legacy sorts are synchronous
}

// Stable sort of `count` 4-byte payloads by a 32-bit rank: LSD radix sort,
// or the bitonic network with WARPDB_SORT=bitonic (comparison runs only).
void do_sort(void *d_a, float *d_v, int64_t count, int kind, int32_t ascending, const wx_launch *Lp,
             int64_t limit, const void *src) {
  const wx_launch L = launch_of(Lp);
  if (count < 0 || count > 0xffffffffll) fail(WX_ERR_INVALID, "bad element count");
  if (src == d_a) src = nullptr;
  if (!src && (count <= 1 || limit == 0)) return;
  if (count == 0) return;
  if (!d_a) fail(WX_ERR_INVALID, "null buffer");
  Op op(L);
  if (src && (count <= 1 || limit == 0 || env_or("WARPDB_SORT", "radix") == "bitonic")) {
    // nothing to sort, or the bitonic network (in place): the keys first
    WX_HIP(hipMemcpyAsync(d_a, src, (size_t)count * 4, hipMemcpyDeviceToDevice, op.s));
    WX_HIP(hipStreamSynchronize(op.s));  // synchronous like every sort entry point
    src = nullptr;
  }
  if (count <= 1 || limit == 0) return;
  if (env_or("WARPDB_SORT", "radix") != "bitonic") {
    radix_sort(d_a, d_v, count, kind, ascending, L, op.w, op.s, limit, src);
    if (L.flags & WX_F_SYNC) check_errors(op.w);
    return;
  }
  auto mod = util_module(L.device, true);
  int64_t npad = WX_SORT_LDS;
  while (npad < count) npad <<= 1;
  ensure(op.w, op.w.sort_keys, (size_t)npad * 8, false);
  ensure(op.w, op.w.sort_copy_a, (size_t)count * 4, false);
  WX_HIP(hipMemcpyAsync(op.w.sort_copy_a.p, d_a, (size_t)count * 4, hipMemcpyDeviceToDevice, op.s));
  if (d_v) {
    ensure(op.w, op.w.sort_copy_v, (size_t)count * 4, false);
    WX_HIP(hipMemcpyAsync(op.w.sort_copy_v.p, d_v, (size_t)count * 4, hipMemcpyDeviceToDevice, op.s));
  }
  WxSortPrepArgs p;
  p.src = op.w.sort_copy_a.p;
  p.keys = static_cast<wx_u64 *>(op.w.sort_keys.p);
  p.n = count;
  p.npad = npad;
  p.kind = kind;
  p.ascending = ascending ? 1 : 0;
  launch(mod->fn("wx_sort_prep"), grid_for(npad, op.d.cus, 8), &p, op.s);
  bitonic_u64(L.device, p.keys, npad, op.s);
  WxSortApplyArgs ap;
  ap.keys = p.keys;
  ap.n = count;
  ap.src_a = op.w.sort_copy_a.p;
  ap.dst_a = d_a;
  ap.src_v = d_v ? static_cast<const float *>(op.w.sort_copy_v.p) : nullptr;
  ap.dst_v = d_v;
  launch(mod->fn("wx_sort_apply"), grid_for(count, op.d.cus, 8), &ap, op.s);
  if (L.flags & WX_F_SYNC) check_errors(op.w);
}

}  // namespace wx
