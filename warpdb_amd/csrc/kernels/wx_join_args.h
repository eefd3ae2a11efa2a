// wx_join_args.h -- argument blocks of the PK-FK equi-join (wx_join.hip).
// Shared by the host runtime and the device templates like wx_args.h and
// wx_select_args.h, which must come first (WxCompactArgs, WX_SELECT_MAX_OUT,
// WX_SELECT_LDS_BUDGET).  Plain C++ only.
#ifndef WX_JOIN_ARGS_H
#define WX_JOIN_ARGS_H

#define WX_OP_JOIN_TABLE 9        // after wx_window_args.h's WX_OP_WINDOW_TABLE 8: wx_join_range + wx_join_build
#define WX_JOIN_DIRECT_BINS 4096  // direct form: the widest key span of a rows[key - min] table (16 KiB of LDS)
#define WX_JOIN_MAX_RIGHT (1 << 26)  // right rows: a row fits the low word of a slot and never reads as empty
#define WX_JOIN_MIN_LOG2CAP 6     // hash form: at least 64 slots
#define WX_JOIN_BLOCK 256         // wx_join_range / wx_join_build workgroup size
#define WX_JOIN_HASH_MUL 0x9E3779B1u
#define WX_JOIN_FORM_DIRECT 0
#define WX_JOIN_FORM_HASH 1
// device error bit (beside WX_DEVERR_* of wx_args.h): a probe or an insertion
// walked the whole hash table without meeting an empty slot, or the build met
// a key outside the range wx_join_range found
#define WX_DEVERR_JOIN_PROBE 16u

// A staged row costs 4 B per output, 4 B more when the matched right row is
// written, and a 2-byte tile-local offset, in two stage buffers; the direct
// form keeps its table in LDS beside them.
#define WX_JOIN_TABLE_BYTES (WX_JOIN_DIRECT_BINS * 4)
#define WX_JOIN_ROW_BYTES(nout, rrow) (2 * (4 * ((nout) + ((rrow) ? 1 : 0)) + 2))

// The record of a build, 32 bytes the host reads with one copy.  The host
// fills [0..1] with all-ones and the rest with zero before wx_join_range.
//   [0] smallest key, [1] ~(largest key), both as key ^ 0x80000000 (unsigned order)
//   [2] claim of the duplicate report, [3] one duplicated key
//   [4..5] n_right
#define WX_JOIN_REC_WORDS 8

struct WxJoinRangeArgs {
  const int *keys;  // [n_right] the right table's key column
  wx_i64 n_right;
  wx_u32 *rec;      // [WX_JOIN_REC_WORDS]
};

// wx_join_build: row r of the right table into rows[key - key_lo] (direct
// form; [WX_JOIN_DIRECT_BINS] prefilled with -1) or into the open-addressing
// table (hash form; [1 << log2cap] slots {key << 32 | row} prefilled with
// all-ones, home slot (u32(key) * WX_JOIN_HASH_MUL) >> (32 - log2cap), linear
// probing).  A key met twice is reported in rec[2..3].
struct WxJoinBuildArgs {
  const int *keys;
  wx_i64 n_right;
  int *rows;
  wx_u64 *slots;
  wx_u32 *rec;
  wx_u64 *ctrs;  // the workspace counters: [1] error bits
  int key_lo;
  wx_u32 span;   // direct form: keys lie in [key_lo, key_lo + span)
  int log2cap;
  int form;
};

// One launch of the probing compaction: up to WX_SELECT_MAX_OUT outputs over
// the columns of both tables.  out_val[nout] is the matched right row's
// output (int32 written through the float stage, -1 for an unmatched row)
// when the module stages it.  Every lookup is clamped: the direct form checks
// the span before it indexes, the hash form masks the slot, and a right
// column is read only at the row of a hit.
struct WxJoinArgs {
  WxCompactArgs c;  // the left table's columns, row ids, status words, counters, count (out_val unused)
  float *out_val[WX_SELECT_MAX_OUT + 1];  // each nullable
  const void *rcol[WX_MAX_COLS];          // the referenced right columns (WX_RCOLS slots)
  const int *rows;      // direct form
  const wx_u64 *slots;  // hash form
  int key_lo;
  wx_u32 span;
  wx_u32 mask;          // hash form: slots - 1
  int shift;            // hash form: 32 - log2cap
};

#endif  // WX_JOIN_ARGS_H
