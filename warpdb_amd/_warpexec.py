"""ctypes binding of the C ABI in include/warpexec.h (libwarpexec.so).

This is the Python side of the drop-in boundary: every function here is a
thin call into the native library with raw device pointers.  Device memory
comes from torch tensors (``tensor.data_ptr()``) and the stream from
``torch.cuda.current_stream().cuda_stream``; torch is plumbing only.

The library is loaded from the package directory (built in-tree by
``make -C warpdb_amd``).  There is no fallback: if the library is missing,
``load()`` raises.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libwarpexec.so")

WX_OK = 0
WX_ERR_INVALID = 1
WX_ERR_COMPILE = 2
WX_ERR_DEVICE = 3
WX_ERR_CAPACITY = 4
WX_ERR_UNSUPPORTED = 5
WX_ERR_INTERNAL = 6

INT32, INT64, FLOAT32, FLOAT64, STRING = 0, 1, 2, 3, 4

F_SYNC = 1
F_NO_CUSTOM = 2
F_TIME = 4
F_F64_COUNTS = 8  # reduce_sum: count written as a double (one f64 all-reduce combines shards)
F_ROW_ORDER = 16  # group_sum / group_agg: sums folded in row order (bit-identical to the reference's fold)

GROUP_WINDOW_BINS = 2048
GROUP_EXCHANGE_DOUBLES = 2 * GROUP_WINDOW_BINS + 1  # [sums | counts as f64 | out-of-window groups]
GROUP_EXCHANGE_MAX_SLOTS = 1024
GROUP_SLOT_MAX = 4096  # n_slots * slot_groups bound
GROUP_NEEDS_MERGE = -2  # wx_group_combine_slots: some shard's out-of-window groups did not fit its slot
TOPK_MAX = 32
TOPK_RECORD_BYTES = TOPK_MAX * 16 + 8  # wx_topk_record: keys f32[32] | vals f32[32] | rows i64[32] | count i64
TOPK_MERGE_MAX = 4096  # n_records * k bound


def group_slots_doubles(n_slots: int, slot_groups: int) -> int:
    """WX_GROUP_SLOTS_DOUBLES: the one-collective GROUP BY exchange buffer."""
    return GROUP_EXCHANGE_DOUBLES + n_slots * (1 + 3 * slot_groups)


def group_list_layout(cap: int):
    """WX_GROUP_LIST_*: (record bytes, sums offset, counts offset) of one
    shard's group list record (int64 count | int32 keys[cap] padded to 8 B |
    f64 sums[cap] | int64 counts[cap])."""
    sums_off = 8 + 8 * ((cap + 1) // 2)
    counts_off = sums_off + 8 * cap
    return counts_off + 8 * cap, sums_off, counts_off

MODE_DENSE = 0
MODE_DENSE_FILL = 1
MODE_COMPACT = 2
MAX_OUTPUTS = 4
GROUP_MAX_VALUES = 4  # WX_GROUP_MAX_VALUES  # WX_MAX_OUTPUTS: expressions of one project_filter_multi call
WIN_SUM, WIN_AVG, WIN_COUNT, WIN_MIN, WIN_MAX = 0, 1, 2, 3, 4  # wx_window_item.agg
JOIN_INNER, JOIN_LEFT = 0, 1  # wx_join_select's join_type
JOIN_DIRECT, JOIN_HASH = 0, 1  # the form of a join's table (wx_join_plan)
GW_GROUP_SUM, GW_GROUP_MULTI, GW_JOIN_GROUP = 0, 1, 2  # wx_group_window_geometry's family
JOIN_DIRECT_BINS = 4096  # widest key span of the direct form
JOIN_MAX_RIGHT = 1 << 26  # most rows of a right table

OP_DENSE, OP_COMPACT, OP_SUM, OP_GROUP, OP_TOPK, OP_UTIL = 0, 1, 2, 3, 4, 5

EXPORTED_SYMBOLS = (
    "wx_project_filter",
    "wx_project_filter_multi",
    "wx_prepare_multi",
    "wx_select_tile_rows",
    "wx_compact_last_launch",
    "wx_gather_multi",
    "wx_prepare_gather",
    "wx_gather_tile_rows",
    "wx_select_ordered",
    "wx_reduce_sum",
    "wx_reduce_stats",
    "wx_group_sum",
    "wx_group_agg",
    "wx_group_agg_multi",
    "wx_prepare_group_multi",
    "wx_window_select",
    "wx_prepare_window",
    "wx_window_tile_rows",
    "wx_join_select",
    "wx_prepare_join",
    "wx_join_tile_rows",
    "wx_join_plan",
    "wx_join_hash_slot",
    "wx_join_group_agg",
    "wx_prepare_join_group",
    "wx_join_group_geometry",
    "wx_group_partials",
    "wx_group_combine",
    "wx_group_partials_slots",
    "wx_group_combine_slots",
    "wx_group_merge_lists",
    "wx_topk_merge",
    "wx_order_head",
    "wx_head_merge",
    "wx_cast",
    "wx_topk",
    "wx_topk_plan",
    "wx_group_part_geometry",
    "wx_group_part_passes",
    "wx_group_rows_geometry",
    "wx_group_rows_last_call",
    "wx_group_rows_last_values",
    "wx_group_window_geometry",
    "wx_group_table_slots",
    "wx_group_hash_slot",
    "wx_sort_pairs",
    "wx_sort_float",
    "wx_sort_float_from",
    "wx_sort_by_key",
    "wx_sort_float_limit",
    "wx_sort_by_key_limit",
    "wx_sort_tile_keys",
    "wx_sort_hist_span_keys",
    "wx_fill_synthetic",
    "wx_prepare",
    "wx_check",
    "wx_timing_read",
    "wx_timing_read_device",
    "wx_cache_stats",
    "wx_shutdown",
    "wx_abi_version",
)


class WxCol(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("dtype", ctypes.c_int32), ("d_ptr", ctypes.c_void_p)]


class WxTable(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_int64), ("n_cols", ctypes.c_int32), ("cols", ctypes.POINTER(WxCol))]


class WxStats(ctypes.Structure):
    _fields_ = [("sum", ctypes.c_double), ("count", ctypes.c_int64), ("min", ctypes.c_float),
                ("max", ctypes.c_float)]


class WxWindowItem(ctypes.Structure):
    _fields_ = [("val_expr", ctypes.c_char_p), ("agg", ctypes.c_int32)]


class WxTopkGeometry(ctypes.Structure):
    _fields_ = [("grid", ctypes.c_int64), ("span_rows", ctypes.c_int64), ("max_batches", ctypes.c_int64),
                ("seed_grid", ctypes.c_int64), ("seed_stride_rows", ctypes.c_int64)]


class WxGroupPartGeometry(ctypes.Structure):
    _fields_ = [(f, ctypes.c_int64) for f in (
        "tile_rows", "n_tiles", "grid", "tiles_per_wg", "n_part", "part_keys", "chunk_rows", "target_items",
        "work_cap", "dir_chunk", "agg_tiles_per_sweep")]


class WxGroupWindowGeometry(ctypes.Structure):
    _fields_ = [(f, ctypes.c_int64) for f in (
        "block_threads", "span_rows", "grid", "max_batches", "window_keys", "hsort_max", "lead")]


class WxGroupRowsGeometry(ctypes.Structure):
    _fields_ = [(f, ctypes.c_int64) for f in (
        "tile_rows", "span_bins", "count_span_rows", "fold_block_values", "fold_blocks_ahead", "fold_small",
        "starts_chunk", "rle_wave_rows", "xf_chunk", "xf_big", "sample_rows")]


class WxGroupRowsRecord(ctypes.Structure):
    _fields_ = [(f, ctypes.c_int64) for f in (
        "route", "why", "ranges", "tiles", "n_values", "big_groups", "big_chunks")]


# wx_group_rows_record.route / .why
RO_ROUTE_NONE, RO_ROUTE_DIRECT, RO_ROUTE_ORDINARY_SPAN, RO_ROUTE_GENERAL_RUNS, RO_ROUTE_GENERAL_ORDINARY = range(5)
RO_WHY_NONE, RO_WHY_RECENT_MISS, RO_WHY_NO_SAMPLE, RO_WHY_OUTSIDE, RO_WHY_WIDE, RO_WHY_NOT_TRIED = range(6)


class WxCompactGeometry(ctypes.Structure):
    _fields_ = [(f, ctypes.c_int64) for f in ("tile_rows", "n_tiles", "grid", "deep")]


class WxLaunch(ctypes.Structure):
    _fields_ = [
        ("device", ctypes.c_int32),
        ("stream", ctypes.c_void_p),
        ("custom_src", ctypes.c_char_p),
        ("flags", ctypes.c_uint32),
    ]


class WarpExecError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(message)
        self.status = status


_lib = None


def load() -> ctypes.CDLL:
    """Load libwarpexec.so (after torch, so both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            f"{LIB_PATH} is missing: build it with `make -C warpdb_amd` (no CPU fallback exists)"
        )
    try:  # share torch's libamdhip64/libhiprtc when torch is present
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    P, I32, I64, U64, D = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double
    S, E = ctypes.c_size_t, ctypes.c_char_p
    T, L = ctypes.POINTER(WxTable), ctypes.POINTER(WxLaunch)
    pI64, pD = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
    sig = {
        "wx_project_filter": [T, E, E, L, I32, P, P, I32, I64, P, pI64, E, S],
        "wx_project_filter_multi": [T, ctypes.POINTER(E), I32, E, L, I32, ctypes.POINTER(P), P, I32, I64, P, pI64, E,
                                    S],
        "wx_prepare_multi": [T, ctypes.POINTER(E), I32, E, L, E, S],
        "wx_gather_multi": [T, ctypes.POINTER(E), I32, P, I32, I64, I64, P, L, ctypes.POINTER(P), P, I64, E, S],
        "wx_prepare_gather": [T, ctypes.POINTER(E), I32, L, E, S],
        "wx_select_ordered": [T, ctypes.POINTER(E), I32, E, E, I32, I64, L, I64, ctypes.POINTER(P), P, P, I64, P, pI64,
                              E, S],
        "wx_reduce_sum": [T, E, E, L, P, pD, pI64, E, S],
        "wx_reduce_stats": [T, E, E, L, P, ctypes.POINTER(WxStats), E, S],
        "wx_group_sum": [T, E, E, E, L, I32, I64, P, P, P, P, pI64, E, S],
        "wx_group_agg": [T, E, E, E, L, I32, I64, P, P, P, P, P, P, pI64, E, S],
        "wx_group_agg_multi": [T, ctypes.POINTER(E), I32, E, E, L, I32, I64, P, ctypes.POINTER(P), P,
                               ctypes.POINTER(P), ctypes.POINTER(P), P, pI64, E, S],
        "wx_prepare_group_multi": [T, ctypes.POINTER(E), I32, ctypes.c_uint32, ctypes.c_uint32, E, E, L, E, S],
        "wx_window_select": [T, ctypes.POINTER(E), I32, ctypes.POINTER(WxWindowItem), I32, E, E, L, I32, I64,
                             ctypes.POINTER(P), P, I32, I64, P, pI64, E, S],
        "wx_prepare_window": [T, ctypes.POINTER(E), I32, ctypes.POINTER(WxWindowItem), I32, E, E, L, I32, E, S],
        "wx_join_select": [T, T, E, E, I32, ctypes.POINTER(E), I32, E, L, ctypes.POINTER(P), P, I32, I64, P, P, pI64, E,
                           S],
        "wx_prepare_join": [T, T, E, E, I32, ctypes.POINTER(E), I32, E, L, I32, I32, E, S],
        "wx_join_plan": [I64, I32, I32, ctypes.POINTER(I32), ctypes.POINTER(I32), E, S],
        "wx_join_group_agg": [T, T, E, E, I32, ctypes.POINTER(E), I32, E, E, L, I32, I64, P, ctypes.POINTER(P), P,
                              ctypes.POINTER(P), ctypes.POINTER(P), P, pI64, E, S],
        "wx_prepare_join_group": [T, T, E, E, I32, ctypes.POINTER(E), I32, ctypes.c_uint32, ctypes.c_uint32, E, E, L,
                                  I32, E, S],
        "wx_join_group_geometry": [I32, I32, I32, ctypes.POINTER(I32), ctypes.POINTER(I32), ctypes.POINTER(I32), E, S],
        "wx_group_partials": [T, E, E, E, L, I32, P, I64, P, P, P, P, pI64, E, S],
        "wx_group_combine": [P, I32, P, P, P, I64, L, I64, P, P, P, P, pI64, E, S],
        "wx_group_partials_slots": [T, E, E, E, L, I32, P, I32, I32, I32, I64, P, P, P, P, pI64, E, S],
        "wx_group_combine_slots": [P, I32, I32, I32, L, I64, P, P, P, P, pI64, E, S],
        "wx_topk_merge": [P, I32, I32, I32, L, P, P, P, P, pI64, E, S],
        "wx_order_head": [T, E, E, E, I64, I32, L, I64, P, I64, E, S],
        "wx_head_merge": [P, I32, I64, I64, I32, L, P, P, P, P, pI64, E, S],
        "wx_group_merge_lists": [P, I32, I64, P, I32, L, I64, P, P, P, P, pI64, E, S],
        "wx_cast": [P, I32, P, I32, I64, L, E, S],
        "wx_topk": [T, E, E, E, I32, I32, L, I64, P, P, P, P, pI64, E, S],
        "wx_topk_plan": [I64, I32, I32, L, ctypes.POINTER(WxTopkGeometry), E, S],
        "wx_group_part_geometry": [I64, I64, I32, L, ctypes.POINTER(WxGroupPartGeometry), E, S],
        "wx_group_part_passes": [L, pI64, E, S],
        "wx_group_rows_geometry": [ctypes.POINTER(WxGroupRowsGeometry), E, S],
        "wx_group_rows_last_call": [L, ctypes.POINTER(WxGroupRowsRecord), E, S],
        "wx_group_rows_last_values": [L, P, I64, pI64, E, S],
        "wx_group_window_geometry": [I64, I32, I32, I32, I32, I32, L, ctypes.POINTER(WxGroupWindowGeometry), E, S],
        "wx_group_table_slots": [L, pI64, E, S],
        "wx_compact_last_launch": [L, ctypes.POINTER(WxCompactGeometry), E, S],
        "wx_sort_pairs": [P, P, I64, I32, L, E, S],
        "wx_sort_float": [P, I64, I32, L, E, S],
        "wx_sort_float_from": [P, P, I64, I32, L, E, S],
        "wx_sort_by_key": [P, P, I64, I32, L, E, S],
        "wx_sort_float_limit": [P, I64, I64, I32, L, E, S],
        "wx_sort_by_key_limit": [P, P, I64, I64, I32, L, E, S],
        "wx_fill_synthetic": [P, I32, I64, U64, I32, D, D, I64, L, E, S],
        "wx_prepare": [T, I32, E, E, E, I32, L, E, S, E, S],
        "wx_check": [L, E, S],
        "wx_timing_read": [pD, pI64, E, S],
        "wx_timing_read_device": [I32, pD, pI64, E, S],
    }
    for name, argtypes in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = ctypes.c_int
    lib.wx_cache_stats.argtypes = [pI64, pI64]
    lib.wx_cache_stats.restype = None
    lib.wx_shutdown.argtypes = []
    lib.wx_shutdown.restype = None
    lib.wx_select_tile_rows.argtypes = [I32]
    lib.wx_select_tile_rows.restype = ctypes.c_int32
    lib.wx_window_tile_rows.argtypes = [I32, I32, I32]
    lib.wx_window_tile_rows.restype = ctypes.c_int32
    lib.wx_join_tile_rows.argtypes = [I32, I32, I32]
    lib.wx_join_tile_rows.restype = ctypes.c_int32
    lib.wx_join_hash_slot.argtypes = [I32, I32]
    lib.wx_join_hash_slot.restype = ctypes.c_int32
    lib.wx_group_hash_slot.argtypes = [I32, I64]
    lib.wx_group_hash_slot.restype = ctypes.c_int32
    lib.wx_gather_tile_rows.argtypes = [I32]
    lib.wx_gather_tile_rows.restype = ctypes.c_int32
    lib.wx_sort_tile_keys.argtypes = [I32]
    lib.wx_sort_tile_keys.restype = ctypes.c_int32
    lib.wx_sort_hist_span_keys.argtypes = []
    lib.wx_sort_hist_span_keys.restype = ctypes.c_int32
    lib.wx_abi_version.argtypes = []
    lib.wx_abi_version.restype = ctypes.c_int32
    _lib = lib
    return lib


def _enc(s: Optional[str]) -> Optional[bytes]:
    return None if s is None else s.encode()


def _check(status: int, err) -> None:
    if status != WX_OK:
        raise WarpExecError(status, err.value.decode(errors="replace"))


@dataclass
class Column:
    name: str
    dtype: int
    ptr: int  # device address


class Table:
    """A wx_table over caller-owned device columns (kept alive by `owners`)."""

    def __init__(self, n_rows: int, columns: Sequence[Column], owners: Sequence[object] = ()):
        self.n_rows = int(n_rows)
        self.columns = list(columns)
        self._owners = list(owners)
        self._names = [c.name.encode() for c in self.columns]
        self._cols = (WxCol * max(1, len(self.columns)))()
        for i, c in enumerate(self.columns):
            self._cols[i] = WxCol(self._names[i], c.dtype, c.ptr)
        self.c = WxTable(self.n_rows, len(self.columns), self._cols)

    @classmethod
    def from_tensors(cls, **cols) -> "Table":
        import torch

        dmap = {torch.int32: INT32, torch.int64: INT64, torch.float32: FLOAT32, torch.float64: FLOAT64}
        n = None
        out = []
        for name, t in cols.items():
            if n is None:
                n = t.numel()
            if t.numel() != n:
                raise ValueError("columns differ in length")
            if not t.is_contiguous():
                raise ValueError(f"column {name} is not contiguous")
            out.append(Column(name, dmap[t.dtype], t.data_ptr()))
        return cls(n or 0, out, owners=list(cols.values()))


def make_launch(device: int = 0, stream: int = 0, custom_src: Optional[str] = None, flags: int = 0) -> WxLaunch:
    L = WxLaunch(device, stream or None, _enc(custom_src), flags)
    L._keep = custom_src  # noqa: SLF001 - keep the bytes object alive
    return L


def _err():
    return ctypes.create_string_buffer(8192)


def project_filter(table: Table, expr: str, cond: Optional[str], launch: WxLaunch, mode: int,
                   out_vals: int = 0, out_idx: int = 0, idx_bytes: int = 8, row_base: int = 0,
                   d_count: int = 0, want_count: bool = False) -> Optional[int]:
    lib = load()
    err = _err()
    h = ctypes.c_int64(-1)
    st = lib.wx_project_filter(ctypes.byref(table.c), _enc(expr), _enc(cond), ctypes.byref(launch), mode,
                               out_vals or None, out_idx or None, idx_bytes, row_base, d_count or None,
                               ctypes.byref(h) if want_count else None, err, len(err))
    _check(st, err)
    return h.value if want_count else None


def _expr_array(exprs: Sequence[Optional[str]]):
    return (ctypes.c_char_p * max(1, len(exprs)))(*[_enc(e) for e in exprs])


def project_filter_multi(table: Table, exprs: Sequence[str], cond: Optional[str], launch: WxLaunch,
                         d_out_vals: Sequence[int], d_out_idx: int = 0, idx_bytes: int = 8, row_base: int = 0,
                         d_count: int = 0, want_count: bool = False, mode: int = MODE_COMPACT) -> Optional[int]:
    """len(exprs) outputs of one filtered result in one pass (ordered
    compaction): d_out_vals[j] (0 = not wanted) receives expression j of the
    passing rows, d_out_idx their row ids.  A shorter d_out_vals is padded
    with nulls."""
    lib = load()
    err = _err()
    h = ctypes.c_int64(-1)
    outs = list(d_out_vals) + [0] * (len(exprs) - len(d_out_vals))
    ptrs = (ctypes.c_void_p * max(1, len(outs)))(*[p or None for p in outs])
    st = lib.wx_project_filter_multi(ctypes.byref(table.c), _expr_array(exprs), len(exprs), _enc(cond),
                                     ctypes.byref(launch), mode, ptrs, d_out_idx or None, idx_bytes, row_base,
                                     d_count or None, ctypes.byref(h) if want_count else None, err, len(err))
    _check(st, err)
    return h.value if want_count else None


def prepare_multi(table: Table, exprs: Sequence[str], cond: Optional[str] = None,
                  launch: Optional[WxLaunch] = None) -> None:
    """Compile the module project_filter_multi would use (no GPU needed)."""
    lib = load()
    err = _err()
    L = launch or make_launch()
    _check(lib.wx_prepare_multi(ctypes.byref(table.c), _expr_array(exprs), len(exprs), _enc(cond), ctypes.byref(L),
                                err, len(err)), err)


def select_tile_rows(n_exprs: int) -> int:
    """Rows per compaction tile of an n_exprs-output call (0: out of range)."""
    return int(load().wx_select_tile_rows(n_exprs))


def compact_last_launch(launch: WxLaunch) -> WxCompactGeometry:
    """What the last ordered compaction on the launch's (device, stream)
    launched: .tile_rows, .n_tiles, .grid, .deep (1: the pipelined kernel).
    Host numbers; all zero before any launch and after an empty table."""
    lib = load()
    err = _err()
    out = WxCompactGeometry()
    _check(lib.wx_compact_last_launch(ctypes.byref(launch), ctypes.byref(out), err, len(err)), err)
    return out


def gather_multi(table: Table, exprs: Sequence[str], d_rows: int, idx_bytes: int, count: int, launch: WxLaunch,
                 d_out_vals: Sequence[int], d_out_rows: int = 0, row_base: int = 0, out_row_base: int = 0,
                 d_count: int = 0) -> None:
    """len(exprs) expressions at `count` row ids (d_rows, int32 or int64 by
    idx_bytes; row = id - row_base): d_out_vals[j] (0 = not wanted) receives
    expression j, d_out_rows out_row_base + row.  d_count (device int64)
    bounds the count on the device.  A shorter d_out_vals is padded with
    nulls."""
    lib = load()
    err = _err()
    outs = list(d_out_vals) + [0] * (len(exprs) - len(d_out_vals))
    ptrs = (ctypes.c_void_p * max(1, len(outs)))(*[p or None for p in outs])
    _check(lib.wx_gather_multi(ctypes.byref(table.c), _expr_array(exprs), len(exprs), d_rows or None, idx_bytes,
                               row_base, count, d_count or None, ctypes.byref(launch), ptrs, d_out_rows or None,
                               out_row_base, err, len(err)), err)


def prepare_gather(table: Table, exprs: Sequence[str], launch: Optional[WxLaunch] = None) -> None:
    """Compile the module gather_multi would use (no GPU needed)."""
    lib = load()
    err = _err()
    L = launch or make_launch()
    _check(lib.wx_prepare_gather(ctypes.byref(table.c), _expr_array(exprs), len(exprs), ctypes.byref(L), err,
                                 len(err)), err)


def gather_tile_rows(n_exprs: int) -> int:
    """Output positions per workgroup iteration of an n_exprs-output gather (0: out of range)."""
    return int(load().wx_gather_tile_rows(n_exprs))


def select_ordered(table: Table, exprs: Sequence[str], cond: Optional[str], order_expr: Optional[str],
                   descending: bool, limit: int, launch: WxLaunch, d_out_vals: Sequence[int], d_out_keys: int = 0,
                   d_out_rows: int = 0, capacity: int = 0, row_base: int = 0, d_count: int = 0,
                   want_count: bool = True) -> Optional[int]:
    """ORDER BY order_expr [DESC] [LIMIT limit] (limit < 0: all) over
    len(exprs) expressions (0 .. 16) of the rows passing cond: the first
    min(limit, passing) keys, global rows and values, `capacity` entries per
    output (0 = not wanted).  On WX_ERR_CAPACITY the raised error carries the
    needed count in `.count`."""
    lib = load()
    err = _err()
    h = ctypes.c_int64(-1)
    outs = list(d_out_vals) + [0] * (len(exprs) - len(d_out_vals))
    ptrs = (ctypes.c_void_p * max(1, len(outs)))(*[p or None for p in outs])
    st = lib.wx_select_ordered(ctypes.byref(table.c), _expr_array(exprs), len(exprs), _enc(cond), _enc(order_expr),
                               1 if descending else 0, limit, ctypes.byref(launch), row_base, ptrs,
                               d_out_keys or None, d_out_rows or None, capacity, d_count or None,
                               ctypes.byref(h) if want_count else None, err, len(err))
    try:
        _check(st, err)
    except WarpExecError as e:
        e.count = h.value
        raise
    return h.value if want_count else None


def reduce_sum(table: Table, expr: str, cond: Optional[str], launch: WxLaunch, d_out: int = 0,
               want_host: bool = True):
    lib = load()
    err = _err()
    s, c = ctypes.c_double(0), ctypes.c_int64(0)
    st = lib.wx_reduce_sum(ctypes.byref(table.c), _enc(expr), _enc(cond), ctypes.byref(launch), d_out or None,
                           ctypes.byref(s) if want_host else None, ctypes.byref(c) if want_host else None,
                           err, len(err))
    _check(st, err)
    return (s.value, c.value) if want_host else None


def group_sum(table: Table, val_expr: str, key_expr: str, cond: Optional[str], launch: WxLaunch,
              key_window_lo: int, capacity: int, d_keys: int, d_sums: int, d_counts: int,
              d_n_groups: int = 0, want_count: bool = True) -> Optional[int]:
    lib = load()
    err = _err()
    h = ctypes.c_int64(-1)
    st = lib.wx_group_sum(ctypes.byref(table.c), _enc(val_expr), _enc(key_expr), _enc(cond),
                          ctypes.byref(launch), key_window_lo, capacity, d_keys or None, d_sums or None,
                          d_counts or None, d_n_groups or None, ctypes.byref(h) if want_count else None,
                          err, len(err))
    try:
        _check(st, err)
    except WarpExecError as e:
        e.count = h.value  # on WX_ERR_CAPACITY: the number of groups found
        raise
    return h.value if want_count else None


def reduce_stats(table: Table, expr: str, cond: Optional[str], launch: WxLaunch, d_out: int = 0,
                 want_host: bool = True):
    """(sum, count, min, max) of (float)expr WHERE cond; MIN / MAX skip NaN, NaN when empty."""
    lib = load()
    err = _err()
    h = WxStats()
    st = lib.wx_reduce_stats(ctypes.byref(table.c), _enc(expr), _enc(cond), ctypes.byref(launch), d_out or None,
                             ctypes.byref(h) if want_host else None, err, len(err))
    _check(st, err)
    return (h.sum, h.count, h.min, h.max) if want_host else None


def group_agg(table: Table, val_expr: str, key_expr: str, cond: Optional[str], launch: WxLaunch,
              key_window_lo: int, capacity: int, d_keys: int, d_sums: int, d_counts: int, d_mins: int = 0,
              d_maxs: int = 0, d_n_groups: int = 0, want_count: bool = True) -> Optional[int]:
    lib = load()
    err = _err()
    h = ctypes.c_int64(-1)
    st = lib.wx_group_agg(ctypes.byref(table.c), _enc(val_expr), _enc(key_expr), _enc(cond),
                          ctypes.byref(launch), key_window_lo, capacity, d_keys or None, d_sums or None,
                          d_counts or None, d_mins or None, d_maxs or None, d_n_groups or None,
                          ctypes.byref(h) if want_count else None, err, len(err))
    try:
        _check(st, err)
    except WarpExecError as e:
        e.count = h.value  # on WX_ERR_CAPACITY: the number of groups found
        raise
    return h.value if want_count else None


def _ptr_array(ptrs: Optional[Sequence[int]], n: int):
    """n device pointers (0 = null), or None for a null array."""
    if ptrs is None:
        return None
    full = list(ptrs) + [0] * (n - len(ptrs))
    return (ctypes.c_void_p * max(1, len(full)))(*[p or None for p in full])


def group_agg_multi(table: Table, val_exprs: Sequence[str], key_expr: str, cond: Optional[str], launch: WxLaunch,
                    key_window_lo: int, capacity: int, d_keys: int, d_counts: int,
                    d_sums: Optional[Sequence[int]] = None, d_mins: Optional[Sequence[int]] = None,
                    d_maxs: Optional[Sequence[int]] = None, d_n_groups: int = 0,
                    want_count: bool = True) -> Optional[int]:
    """GROUP BY over len(val_exprs) value expressions in one pass: d_sums[j] /
    d_mins[j] / d_maxs[j] (0 = not wanted; a shorter or missing list is padded
    with nulls) receive value j's aggregates, d_keys / d_counts the groups.
    On WX_ERR_CAPACITY the raised error carries the found count in `.count`."""
    lib = load()
    err = _err()
    h = ctypes.c_int64(-1)
    n = len(val_exprs)
    st = lib.wx_group_agg_multi(ctypes.byref(table.c), _expr_array(val_exprs), n, _enc(key_expr), _enc(cond),
                                ctypes.byref(launch), key_window_lo, capacity, d_keys or None,
                                _ptr_array(d_sums, n), d_counts or None, _ptr_array(d_mins, n), _ptr_array(d_maxs, n),
                                d_n_groups or None, ctypes.byref(h) if want_count else None, err, len(err))
    try:
        _check(st, err)
    except WarpExecError as e:
        e.count = h.value
        raise
    return h.value if want_count else None


def prepare_group_multi(table: Table, val_exprs: Sequence[str], sum_mask: int, minmax_mask: int, key_expr: str,
                        cond: Optional[str] = None, launch: Optional[WxLaunch] = None) -> None:
    """Compile the module group_agg_multi would use for the values summed
    (bit j of sum_mask) and min/maxed (bit j of minmax_mask); no GPU needed."""
    lib = load()
    err = _err()
    L = launch or make_launch()
    _check(lib.wx_prepare_group_multi(ctypes.byref(table.c), _expr_array(val_exprs), len(val_exprs), sum_mask,
                                      minmax_mask, _enc(key_expr), _enc(cond), ctypes.byref(L), err, len(err)), err)


def _window_items(items: Sequence[Tuple[Optional[str], int]]):
    return (WxWindowItem * max(1, len(items)))(*[WxWindowItem(_enc(e), int(a)) for e, a in items])


def window_select(table: Table, exprs: Sequence[str], items: Sequence[Tuple[Optional[str], int]], part_expr: str,
                  cond: Optional[str], launch: WxLaunch, d_out_vals: Sequence[int], key_window_lo: int = 0,
                  group_capacity: int = 4096, d_out_idx: int = 0, idx_bytes: int = 8, row_base: int = 0,
                  d_count: int = 0, want_count: bool = False) -> Optional[int]:
    """Plain expressions and window items (value expression, WIN_* aggregate)
    OVER (PARTITION BY part_expr) of the rows cond keeps, in row order:
    d_out_vals[j] (0 = not wanted) receives output j, plain expressions
    first; a shorter list is padded with nulls."""
    lib = load()
    err = _err()
    h = ctypes.c_int64(-1)
    n_out = len(exprs) + len(items)
    outs = list(d_out_vals) + [0] * (n_out - len(d_out_vals))
    ptrs = (ctypes.c_void_p * max(1, len(outs)))(*[p or None for p in outs])
    st = lib.wx_window_select(ctypes.byref(table.c), _expr_array(exprs), len(exprs), _window_items(items), len(items),
                              _enc(part_expr), _enc(cond), ctypes.byref(launch), key_window_lo, group_capacity, ptrs,
                              d_out_idx or None, idx_bytes, row_base, d_count or None,
                              ctypes.byref(h) if want_count else None, err, len(err))
    _check(st, err)
    return h.value if want_count else None


def prepare_window(table: Table, exprs: Sequence[str], items: Sequence[Tuple[Optional[str], int]], part_expr: str,
                   cond: Optional[str] = None, launch: Optional[WxLaunch] = None, search: bool = False) -> None:
    """Compile the modules window_select would use, in the dense or the search form (no GPU needed)."""
    lib = load()
    err = _err()
    L = launch or make_launch()
    _check(lib.wx_prepare_window(ctypes.byref(table.c), _expr_array(exprs), len(exprs), _window_items(items),
                                 len(items), _enc(part_expr), _enc(cond), ctypes.byref(L), 1 if search else 0, err,
                                 len(err)), err)


def window_tile_rows(n_outputs: int, n_items: int, search: bool = False) -> int:
    """Rows per tile of one broadcast launch (0: out of range)."""
    return int(load().wx_window_tile_rows(n_outputs, n_items, int(search)))


def join_select(left: Table, right: Table, left_key_expr: str, right_key_col: str, exprs: Sequence[str],
                cond: Optional[str], launch: WxLaunch, d_out_vals: Sequence[int], join_type: int = JOIN_INNER,
                d_out_idx: int = 0, idx_bytes: int = 8, row_base: int = 0, d_out_right_row: int = 0,
                d_count: int = 0, want_count: bool = False) -> Optional[int]:
    """PK-FK equi-join: the rows of `left` that cond keeps, each looked up in
    `right` by (int)left_key_expr == right_key_col, in left row order.
    d_out_vals[j] (0 = not wanted) receives expression j (over the columns of
    both tables), d_out_idx the left row ids, d_out_right_row (int32) the
    matched right rows (-1: none, a LEFT join).  A shorter d_out_vals is
    padded with nulls."""
    lib = load()
    err = _err()
    h = ctypes.c_int64(-1)
    outs = list(d_out_vals) + [0] * (len(exprs) - len(d_out_vals))
    ptrs = (ctypes.c_void_p * max(1, len(outs)))(*[p or None for p in outs])
    st = lib.wx_join_select(ctypes.byref(left.c), ctypes.byref(right.c), _enc(left_key_expr), _enc(right_key_col),
                            join_type, _expr_array(exprs), len(exprs), _enc(cond), ctypes.byref(launch), ptrs,
                            d_out_idx or None, idx_bytes, row_base, d_out_right_row or None, d_count or None,
                            ctypes.byref(h) if want_count else None, err, len(err))
    _check(st, err)
    return h.value if want_count else None


def prepare_join(left: Table, right: Table, left_key_expr: str, right_key_col: str, exprs: Sequence[str],
                 cond: Optional[str] = None, launch: Optional[WxLaunch] = None, join_type: int = JOIN_INNER,
                 with_right_row: bool = False, form: int = JOIN_HASH) -> None:
    """Compile the modules join_select would use, in the direct or the hash form (no GPU needed)."""
    lib = load()
    err = _err()
    L = launch or make_launch()
    _check(lib.wx_prepare_join(ctypes.byref(left.c), ctypes.byref(right.c), _enc(left_key_expr), _enc(right_key_col),
                               join_type, _expr_array(exprs), len(exprs), _enc(cond), ctypes.byref(L),
                               1 if with_right_row else 0, form, err, len(err)), err)


def join_tile_rows(n_outputs: int, form: int = JOIN_HASH, with_right_row: bool = False) -> int:
    """Rows per tile of one probe launch (0: out of range)."""
    return int(load().wx_join_tile_rows(n_outputs, form, int(with_right_row)))


def join_plan(n_right: int, key_min: int, key_max: int) -> Tuple[int, int]:
    """(form, log2 capacity) of the table join_select builds for n_right keys in [key_min, key_max]."""
    lib = load()
    err = _err()
    form, log2cap = ctypes.c_int32(-1), ctypes.c_int32(-1)
    _check(lib.wx_join_plan(n_right, key_min, key_max, ctypes.byref(form), ctypes.byref(log2cap), err, len(err)), err)
    return form.value, log2cap.value


def join_hash_slot(key: int, log2_capacity: int) -> int:
    """The home slot the kernels use for `key` in a table of 1 << log2_capacity slots."""
    return int(load().wx_join_hash_slot(key, log2_capacity))


def join_group_agg(left: Table, right: Table, left_key_expr: str, right_key_col: str, val_exprs: Sequence[str],
                   group_key_expr: str, cond: Optional[str], launch: WxLaunch, key_window_lo: int, capacity: int,
                   d_keys: int, d_counts: int, d_sums: Optional[Sequence[int]] = None,
                   d_mins: Optional[Sequence[int]] = None, d_maxs: Optional[Sequence[int]] = None,
                   d_n_groups: int = 0, want_count: bool = True, join_type: int = JOIN_INNER) -> Optional[int]:
    """JOIN under GROUP BY: group_agg_multi over the rows join_select (INNER)
    keeps, in one pass; values, group key and cond are over the columns of
    both tables.  Outputs as in group_agg_multi; on WX_ERR_CAPACITY the raised
    error carries the found count in `.count`."""
    lib = load()
    err = _err()
    h = ctypes.c_int64(-1)
    n = len(val_exprs)
    st = lib.wx_join_group_agg(ctypes.byref(left.c), ctypes.byref(right.c), _enc(left_key_expr), _enc(right_key_col),
                               join_type, _expr_array(val_exprs), n, _enc(group_key_expr), _enc(cond),
                               ctypes.byref(launch), key_window_lo, capacity, d_keys or None, _ptr_array(d_sums, n),
                               d_counts or None, _ptr_array(d_mins, n), _ptr_array(d_maxs, n), d_n_groups or None,
                               ctypes.byref(h) if want_count else None, err, len(err))
    try:
        _check(st, err)
    except WarpExecError as e:
        e.count = h.value
        raise
    return h.value if want_count else None


def prepare_join_group(left: Table, right: Table, left_key_expr: str, right_key_col: str, val_exprs: Sequence[str],
                       sum_mask: int, minmax_mask: int, group_key_expr: str, cond: Optional[str] = None,
                       launch: Optional[WxLaunch] = None, form: int = JOIN_HASH,
                       join_type: int = JOIN_INNER) -> None:
    """Compile the modules join_group_agg would use for these masks, in the direct or the hash form (no GPU needed)."""
    lib = load()
    err = _err()
    L = launch or make_launch()
    _check(lib.wx_prepare_join_group(ctypes.byref(left.c), ctypes.byref(right.c), _enc(left_key_expr),
                                     _enc(right_key_col), join_type, _expr_array(val_exprs), len(val_exprs), sum_mask,
                                     minmax_mask, _enc(group_key_expr), _enc(cond), ctypes.byref(L), form, err,
                                     len(err)), err)


def join_group_geometry(n_sums: int, n_minmax: int, form: int = JOIN_HASH) -> Tuple[int, int, int]:
    """(threads per workgroup, workgroups per CU, LDS bytes per workgroup) of the grouped pass over a join."""
    lib = load()
    err = _err()
    block, per_cu, lds = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
    _check(lib.wx_join_group_geometry(n_sums, n_minmax, form, ctypes.byref(block), ctypes.byref(per_cu),
                                      ctypes.byref(lds), err, len(err)), err)
    return block.value, per_cu.value, lds.value


def group_partials(table: Table, val_expr: str, key_expr: str, cond: Optional[str], launch: WxLaunch,
                   key_window_lo: int, d_window: int, capacity: int, d_keys: int, d_sums: int, d_counts: int,
                   d_n_extra: int = 0, want_count: bool = False) -> Optional[int]:
    """Per-shard GROUP BY partials in the exchange layout (include/warpexec.h)."""
    lib = load()
    err = _err()
    h = ctypes.c_int64(-1)
    st = lib.wx_group_partials(ctypes.byref(table.c), _enc(val_expr), _enc(key_expr), _enc(cond),
                               ctypes.byref(launch), key_window_lo, d_window, capacity, d_keys or None,
                               d_sums or None, d_counts or None, d_n_extra or None,
                               ctypes.byref(h) if want_count else None, err, len(err))
    _check(st, err)
    return h.value if want_count else None


def group_combine(d_window: int, key_window_lo: int, d_x_keys: int, d_x_sums: int, d_x_counts: int, n_extra: int,
                  launch: WxLaunch, capacity: int, d_keys: int, d_sums: int, d_counts: int, d_n_groups: int = 0,
                  want_count: bool = False) -> Optional[int]:
    """Final groups from a combined exchange window + combined out-of-window groups."""
    lib = load()
    err = _err()
    h = ctypes.c_int64(-1)
    st = lib.wx_group_combine(d_window, key_window_lo, d_x_keys or None, d_x_sums or None, d_x_counts or None,
                              n_extra, ctypes.byref(launch), capacity, d_keys or None, d_sums or None,
                              d_counts or None, d_n_groups or None, ctypes.byref(h) if want_count else None,
                              err, len(err))
    _check(st, err)
    return h.value if want_count else None


def group_partials_slots(table: Table, val_expr: str, key_expr: str, cond: Optional[str], launch: WxLaunch,
                         key_window_lo: int, d_exchange: int, n_slots: int, slot: int, slot_groups: int,
                         capacity: int, d_keys: int, d_sums: int, d_counts: int, d_n_extra: int = 0,
                         want_count: bool = False) -> Optional[int]:
    """Per-shard GROUP BY partials in the one-collective exchange layout
    (window + this shard's slot, zeros in the others; include/warpexec.h)."""
    lib = load()
    err = _err()
    h = ctypes.c_int64(-1)
    st = lib.wx_group_partials_slots(ctypes.byref(table.c), _enc(val_expr), _enc(key_expr), _enc(cond),
                                     ctypes.byref(launch), key_window_lo, d_exchange, n_slots, slot, slot_groups,
                                     capacity, d_keys or None, d_sums or None, d_counts or None, d_n_extra or None,
                                     ctypes.byref(h) if want_count else None, err, len(err))
    _check(st, err)
    return h.value if want_count else None


def group_combine_slots(d_exchange: int, n_slots: int, slot_groups: int, key_window_lo: int, launch: WxLaunch,
                        capacity: int, d_keys: int, d_sums: int, d_counts: int, d_n_groups: int = 0,
                        want_count: bool = False) -> Optional[int]:
    """Final groups from a combined one-collective exchange buffer; the count
    is GROUP_NEEDS_MERGE (-2) when a shard's slot overflowed, -1 when a
    shard's general-key table did."""
    lib = load()
    err = _err()
    h = ctypes.c_int64(-1)
    st = lib.wx_group_combine_slots(d_exchange, n_slots, slot_groups, key_window_lo, ctypes.byref(launch), capacity,
                                    d_keys or None, d_sums or None, d_counts or None, d_n_groups or None,
                                    ctypes.byref(h) if want_count else None, err, len(err))
    _check(st, err)
    return h.value if want_count else None


def group_merge_lists(d_lists: int, n_lists: int, list_capacity: int, d_window: int, key_window_lo: int,
                      launch: WxLaunch, capacity: int, d_keys: int, d_sums: int, d_counts: int, d_n_groups: int = 0,
                      want_count: bool = False) -> Optional[int]:
    """Final groups from n_lists gathered group list records (device; see
    group_list_layout), merged with the combined window d_window (0: none).
    The count is -1 when a list's count was negative or above list_capacity."""
    lib = load()
    err = _err()
    h = ctypes.c_int64(-1)
    st = lib.wx_group_merge_lists(d_lists or None, n_lists, list_capacity, d_window or None, key_window_lo,
                                  ctypes.byref(launch), capacity, d_keys or None, d_sums or None, d_counts or None,
                                  d_n_groups or None, ctypes.byref(h) if want_count else None, err, len(err))
    _check(st, err)
    return h.value if want_count else None


def topk_merge(d_records: int, n_records: int, k: int, descending: bool, launch: WxLaunch, d_keys: int = 0,
               d_idx: int = 0, d_vals: int = 0, d_count: int = 0, want_count: bool = False) -> Optional[int]:
    """Global top-K from n_records wx_topk_record candidate records (device)."""
    lib = load()
    err = _err()
    h = ctypes.c_int64(-1)
    st = lib.wx_topk_merge(d_records or None, n_records, k, 1 if descending else 0, ctypes.byref(launch),
                           d_keys or None, d_idx or None, d_vals or None, d_count or None,
                           ctypes.byref(h) if want_count else None, err, len(err))
    _check(st, err)
    return h.value if want_count else None


def head_record_bytes(cap: int) -> int:
    """WX_HEAD_RECORD_BYTES: count i64 | keys f32[cap] | vals f32[cap] | rows i64[cap]."""
    return 8 + 16 * cap


def order_head(table: Table, order_expr: str, cond: Optional[str], select_expr: Optional[str], limit: int,
               descending: bool, launch: WxLaunch, d_record: int, cap: int, row_base: int = 0) -> None:
    """This shard's ORDER BY .. LIMIT head of any length into a head record (synchronous)."""
    lib = load()
    err = _err()
    _check(lib.wx_order_head(ctypes.byref(table.c), _enc(order_expr), _enc(cond), _enc(select_expr), limit,
                             1 if descending else 0, ctypes.byref(launch), row_base, d_record or None, cap, err,
                             len(err)), err)


def head_merge(d_records: int, n_records: int, cap: int, limit: int, descending: bool, launch: WxLaunch,
               d_keys: int = 0, d_rows: int = 0, d_vals: int = 0, d_count: int = 0) -> int:
    """The global head of n_records head records (device); returns its length."""
    lib = load()
    err = _err()
    h = ctypes.c_int64(-1)
    _check(lib.wx_head_merge(d_records or None, n_records, cap, limit, 1 if descending else 0, ctypes.byref(launch),
                             d_keys or None, d_rows or None, d_vals or None, d_count or None, ctypes.byref(h), err,
                             len(err)), err)
    return h.value


def cast(d_src: int, src_dtype: int, d_dst: int, dst_dtype: int, n: int, launch: WxLaunch) -> None:
    lib = load()
    err = _err()
    _check(lib.wx_cast(d_src or None, src_dtype, d_dst or None, dst_dtype, n, ctypes.byref(launch), err, len(err)),
           err)


def topk(table: Table, order_expr: str, cond: Optional[str], select_expr: Optional[str], k: int, descending: bool,
         launch: WxLaunch, d_keys: int = 0, d_idx: int = 0, d_vals: int = 0, row_base: int = 0,
         d_count: int = 0, want_count: bool = True) -> Optional[int]:
    lib = load()
    err = _err()
    h = ctypes.c_int64(-1)
    st = lib.wx_topk(ctypes.byref(table.c), _enc(order_expr), _enc(cond), _enc(select_expr), k,
                     1 if descending else 0, ctypes.byref(launch), row_base, d_keys or None, d_idx or None,
                     d_vals or None, d_count or None, ctypes.byref(h) if want_count else None, err, len(err))
    _check(st, err)
    return h.value if want_count else None


def topk_plan(n_rows: int, k: int, cus: int = 0, launch: Optional[WxLaunch] = None) -> WxTopkGeometry:
    """The launch plan wx_topk follows under the current WARPDB_EXTRA_DEFINES:
    .grid, .span_rows, .max_batches (of the workgroup that runs the most),
    .seed_grid (0: no seed pass), .seed_stride_rows.  cus > 0 names the
    device's compute units (no device needed); otherwise the launch's device."""
    lib = load()
    err = _err()
    out = WxTopkGeometry()
    _check(lib.wx_topk_plan(n_rows, k, cus, ctypes.byref(launch) if launch is not None else None, ctypes.byref(out),
                            err, len(err)), err)
    return out


def group_part_geometry(n_rows: int, key_span: int, cus: int = 0,
                        launch: Optional[WxLaunch] = None) -> WxGroupPartGeometry:
    """The launch geometry of one range-partitioned GROUP BY pass under the
    current WARPDB_EXTRA_DEFINES (WX_GP_GRID, WX_GP_DIRCH): .tile_rows,
    .n_tiles, .grid, .tiles_per_wg, .n_part, .part_keys, .chunk_rows,
    .target_items, .work_cap, .dir_chunk, .agg_tiles_per_sweep.  cus > 0 names
    the device's compute units (no device needed); otherwise the launch's device."""
    lib = load()
    err = _err()
    out = WxGroupPartGeometry()
    _check(lib.wx_group_part_geometry(n_rows, key_span, cus, ctypes.byref(launch) if launch is not None else None,
                                      ctypes.byref(out), err, len(err)), err)
    return out


def group_part_passes(launch: WxLaunch) -> int:
    """Partitioned GROUP BY passes completed so far on the launch's (device,
    stream): a host counter, read before and after a call to see its route."""
    lib = load()
    err = _err()
    n = ctypes.c_int64(-1)
    _check(lib.wx_group_part_passes(ctypes.byref(launch), ctypes.byref(n), err, len(err)), err)
    return n.value


def group_rows_geometry() -> WxGroupRowsGeometry:
    """The sizes the row-order GROUP BY works in (no device needed):
    .tile_rows, .span_bins, .count_span_rows, .fold_block_values,
    .fold_blocks_ahead, .fold_small, .starts_chunk, .rle_wave_rows, .xf_chunk,
    .xf_big, .sample_rows."""
    lib = load()
    err = _err()
    out = WxGroupRowsGeometry()
    _check(lib.wx_group_rows_geometry(ctypes.byref(out), err, len(err)), err)
    return out


def group_rows_last_call(launch: WxLaunch) -> WxGroupRowsRecord:
    """What the last F_ROW_ORDER call on the launch's (device, stream) did:
    .route (RO_ROUTE_*), .why (RO_WHY_*: why not the direct span path),
    .ranges, .tiles, .n_values, .big_groups, .big_chunks.  Host numbers; all
    zero before any such call, after a failed one and after one without groups
    from the ordinary call.  WARPDB_RO_RANGES=<n> caps .ranges."""
    lib = load()
    err = _err()
    out = WxGroupRowsRecord()
    _check(lib.wx_group_rows_last_call(ctypes.byref(launch), ctypes.byref(out), err, len(err)), err)
    return out


def group_rows_last_values(launch: WxLaunch, d_out: int, capacity: int) -> int:
    """Copy the last F_ROW_ORDER call's row-ordered values (key-major, row
    order within a key) into d_out (device, `capacity` floats) on the launch's
    stream; returns their number.  Valid until the next call on that stream."""
    lib = load()
    err = _err()
    n = ctypes.c_int64(-1)
    _check(lib.wx_group_rows_last_values(ctypes.byref(launch), d_out or None, capacity, ctypes.byref(n), err,
                                         len(err)), err)
    return n.value


def group_window_geometry(n_rows: int, n_sums: int, n_minmax: int, family: int = GW_GROUP_SUM,
                          join_form: int = JOIN_HASH, cus: int = 0,
                          launch: Optional[WxLaunch] = None) -> WxGroupWindowGeometry:
    """The launch geometry of the streaming kernel of an LDS-window GROUP BY
    (family GW_GROUP_SUM / GW_GROUP_MULTI / GW_JOIN_GROUP) under the current
    WARPDB_EXTRA_DEFINES (WX_GROUP_GRID, WX_UNROLL, WX_GROUP_LEAD):
    .block_threads, .span_rows, .grid, .max_batches (of the workgroup that
    runs the most), .window_keys, .hsort_max, .lead.  cus > 0 names the
    device's compute units (no device needed); otherwise the launch's device."""
    lib = load()
    err = _err()
    out = WxGroupWindowGeometry()
    _check(lib.wx_group_window_geometry(n_rows, n_sums, n_minmax, family, join_form, cus,
                                        ctypes.byref(launch) if launch is not None else None, ctypes.byref(out), err,
                                        len(err)), err)
    return out


def group_table_slots(launch: WxLaunch) -> int:
    """Slots of the general-key table of the launch's (device, stream) as it
    stands (a host number; 0 before the first GROUP BY there)."""
    lib = load()
    err = _err()
    n = ctypes.c_int64(-1)
    _check(lib.wx_group_table_slots(ctypes.byref(launch), ctypes.byref(n), err, len(err)), err)
    return n.value


def group_hash_slot(key: int, slots: int) -> int:
    """The home slot the kernels use for `key` in a general-key table of `slots` slots (-1: not a power of two)."""
    return int(load().wx_group_hash_slot(key, slots))


def sort_pairs(d_keys: int, d_vals: int, count: int, ascending: bool, launch: WxLaunch) -> None:
    lib = load()
    err = _err()
    _check(lib.wx_sort_pairs(d_keys, d_vals, count, 1 if ascending else 0, ctypes.byref(launch), err, len(err)), err)


def sort_float(d_vals: int, count: int, ascending: bool, launch: WxLaunch) -> None:
    lib = load()
    err = _err()
    _check(lib.wx_sort_float(d_vals, count, 1 if ascending else 0, ctypes.byref(launch), err, len(err)), err)


def sort_by_key(d_keys: int, d_vals: int, count: int, ascending: bool, launch: WxLaunch) -> None:
    lib = load()
    err = _err()
    _check(lib.wx_sort_by_key(d_keys, d_vals, count, 1 if ascending else 0, ctypes.byref(launch), err, len(err)), err)


def sort_float_from(d_src: int, d_dst: int, count: int, ascending: bool, launch: WxLaunch) -> None:
    """Sorted copy of d_src's float keys into d_dst (d_src is not written)."""
    lib = load()
    err = _err()
    _check(lib.wx_sort_float_from(d_src, d_dst, count, 1 if ascending else 0, ctypes.byref(launch), err, len(err)),
           err)


def sort_float_limit(d_vals: int, count: int, limit: int, ascending: bool, launch: WxLaunch) -> None:
    lib = load()
    err = _err()
    _check(lib.wx_sort_float_limit(d_vals, count, limit, 1 if ascending else 0, ctypes.byref(launch), err, len(err)),
           err)


def sort_by_key_limit(d_keys: int, d_vals: int, count: int, limit: int, ascending: bool, launch: WxLaunch) -> None:
    lib = load()
    err = _err()
    _check(lib.wx_sort_by_key_limit(d_keys, d_vals, count, limit, 1 if ascending else 0, ctypes.byref(launch), err,
                                    len(err)), err)


def sort_tile_keys(with_payload) -> int:
    """Keys per radix sort tile, of the key sorts or (with_payload) of the key + payload sorts (0: invalid geometry)."""
    return int(load().wx_sort_tile_keys(1 if with_payload else 0))


def sort_hist_span_keys() -> int:
    """Keys per workgroup iteration of the sort's histogram pass."""
    return int(load().wx_sort_hist_span_keys())


def fill_synthetic(d_ptr: int, dtype: int, n: int, seed: int, kind: int, lo: float, hi: float,
                   launch: WxLaunch, row_base: int = 0) -> None:
    lib = load()
    err = _err()
    _check(lib.wx_fill_synthetic(d_ptr, dtype, n, seed, kind, lo, hi, row_base, ctypes.byref(launch), err,
                                 len(err)), err)


def prepare(table: Optional[Table], op: int, expr: Optional[str] = None, cond: Optional[str] = None,
            aux: Optional[str] = None, k: int = 0, launch: Optional[WxLaunch] = None,
            want_source: bool = False) -> Optional[str]:
    lib = load()
    err = _err()
    src = ctypes.create_string_buffer(1 << 20) if want_source else None
    L = launch or make_launch()
    st = lib.wx_prepare(ctypes.byref(table.c) if table is not None else None, op, _enc(expr), _enc(cond),
                        _enc(aux), k, ctypes.byref(L), src, len(src) if src is not None else 0, err, len(err))
    _check(st, err)
    return src.value.decode() if want_source else None


def check(launch: WxLaunch) -> None:
    lib = load()
    err = _err()
    _check(lib.wx_check(ctypes.byref(launch), err, len(err)), err)


def timing_read(device: Optional[int] = None):
    """(total ms, launches) of the unread WX_F_TIME launches of the process
    (of `device` only, when given)."""
    lib = load()
    err = _err()
    ms, n = ctypes.c_double(0), ctypes.c_int64(0)
    if device is None:
        _check(lib.wx_timing_read(ctypes.byref(ms), ctypes.byref(n), err, len(err)), err)
    else:
        _check(lib.wx_timing_read_device(device, ctypes.byref(ms), ctypes.byref(n), err, len(err)), err)
    return ms.value, n.value


def cache_stats():
    lib = load()
    c, h = ctypes.c_int64(0), ctypes.c_int64(0)
    lib.wx_cache_stats(ctypes.byref(c), ctypes.byref(h))
    return c.value, h.value
