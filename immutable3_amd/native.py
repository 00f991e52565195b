"""ctypes binding of libimm3.so (include/imm3.h) -- the only way the host side reaches the GPU.

There is no CPU fallback: if the shared library is missing, or no HIP device is present, the
calls raise.  The oracle under oracle/ is never imported from here.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
import weakref
from typing import List, Optional, Sequence

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", "libimm3.so")

# CodecType (core/src/main/scala/immutabledb/codec/Codec.scala:21-24)
PFOR_INT, DENSE_INT, DENSE_TINYINT, DENSE_STRING = 0, 1, 2, 3
SNAPPY_INT, SNAPPY_TINYINT, SNAPPY_STRING = 16, 17, 18   # extension: blocks as SnappyCodec.encode writes them
INT_CODECS, TINYINT_CODECS = (DENSE_INT, PFOR_INT, SNAPPY_INT), (DENSE_TINYINT, SNAPPY_TINYINT)
# SelectCondition (core/src/main/scala/immutabledb/Query.scala:3-9)
MATCH, NOTMATCH, EQ, GT, LT, NOOP = 0, 1, 2, 3, 4, 5
# extension (include/imm3.h: IMM3_STR_RANGE): a closed byte-order range on a string column; operand (lo, hi), each 0 .. width bytes,
# lo padded with 0x00 and hi with 0xFF
STR_RANGE = 6
# extension (include/imm3.h: IMM3_INT_IN): an IN-list on an int32 / int8 column; operand: the integers (each an int32), any order
INT_IN = 7
INT_IN_MAX_VALUES = 1 << 24   # IMM3_INT_IN_MAX_VALUES
INT_LIST_I8, INT_LIST_ARGS, INT_LIST_LDS, INT_LIST_GLOBAL = 0, 1, 2, 3   # plan_int_list_form (csrc/imm3_int_list_plan.h: IntListForm)
# extension (include/imm3.h: IMM3_INT_IN_SET): membership in a device-resident set built from other queries' selections -- IN
# (sub-query); operand: an IntSet of the same context
INT_IN_SET = 8
# operators of a select tree's postfix program (include/imm3.h: IMM3_EXPR_AND / IMM3_EXPR_OR / IMM3_EXPR_NOT); values >= 0 are leaf
# indices.  NOT pops one operand and pushes its complement (-4: -3 stays the unknown operator it has always been)
EXPR_AND, EXPR_OR, EXPR_NOT = -1, -2, -4
EXPR_FORM_TILE, EXPR_FORM_GENERIC = 0, 1
# how every "this tree does not fit a table" refusal of the _table_expr entry points begins (include/imm3.h: IMM3_TABLE_TREE_REFUSED)
TABLE_TREE_REFUSED = "a select tree over a table takes "
# how every "this view does not fit the device's order" refusal of imm3_comm_merge_groups_view begins (include/imm3.h:
# IMM3_MERGE_VIEW_REFUSED): the caller merges with merge_groups_wide and orders on the host
MERGE_VIEW_REFUSED = "a view of merged groups takes "

OK = 0
ERR_UNSUPPORTED_CONDITION, ERR_UNSUPPORTED_VECTOR, ERR_NO_CODEC, ERR_LAYOUT, ERR_ARG, ERR_DEVICE, ERR_STATE = 1, 2, 3, 4, 5, 6, 7

# every symbol include/imm3.h declares (tests check the library exports all of them)
EXPORTS = [
    "imm3_abi_version", "imm3_last_error", "imm3_device_count",
    "imm3_ctx_create", "imm3_ctx_destroy", "imm3_ctx_sync", "imm3_ctx_stream",
    "imm3_ctx_capture_begin", "imm3_ctx_capture_end", "imm3_graph_launch", "imm3_graph_destroy",
    "imm3_segment_create", "imm3_segment_create_async", "imm3_segment_wait", "imm3_segment_wrap_device", "imm3_segment_destroy", "imm3_segment_bytes",
    "imm3_table_create", "imm3_table_destroy", "imm3_query_create_table", "imm3_query_create_table_agg",
    "imm3_query_segment_starts", "imm3_query_locate_rows",
    "imm3_query_create", "imm3_query_create_agg", "imm3_query_group_count", "imm3_query_fetch_groups", "imm3_query_agg_shape",
    "imm3_query_fetch_group_strings", "imm3_query_destroy", "imm3_query_reserve_rows", "imm3_query_set_order", "imm3_query_set_group_order",
    "imm3_query_set_group_filter",
    "imm3_query_create_agg_wide", "imm3_query_create_table_agg_wide", "imm3_query_fetch_group_keys",
    "imm3_query_create_expr", "imm3_query_create_agg_expr", "imm3_query_create_table_expr", "imm3_query_create_table_agg_expr",
    "imm3_query_run", "imm3_query_run_select", "imm3_query_run_count", "imm3_query_sync", "imm3_query_join_count", "imm3_query_log_counts",
    "imm3_query_layout", "imm3_query_batches", "imm3_query_count", "imm3_query_bitmap",
    "imm3_query_row_count", "imm3_query_fetch_rows", "imm3_query_device_ptr",
    "imm3_comm_unique_id", "imm3_comm_create", "imm3_comm_create_all", "imm3_comm_destroy", "imm3_comm_info",
    "imm3_comm_sync", "imm3_comm_join", "imm3_comm_allreduce_u64", "imm3_comm_allreduce_count", "imm3_comm_allreduce_count_all", "imm3_comm_merge_groups", "imm3_comm_merge_groups_all",
    "imm3_comm_merge_groups_wide", "imm3_comm_merge_groups_wide_all", "imm3_comm_merge_ordered", "imm3_comm_merge_ordered_all",
    "imm3_comm_merge_groups_view", "imm3_comm_merge_groups_view_all",
    "imm3_pfor_encode_bound", "imm3_pfor_encode_block", "imm3_pfor_encode_column",
    "imm3_snappy_encode_bound", "imm3_snappy_encode_block",
    "imm3_int_set_create", "imm3_int_set_destroy", "imm3_int_set_info", "imm3_int_set_values",
]
# include/imm3_diag.h: measurement / tuning hooks, not part of the drop-in boundary
DIAG_EXPORTS = [
    "imm3_ctx_timing_enable", "imm3_ctx_timing_reset", "imm3_ctx_timing_mask", "imm3_ctx_timing_collect", "imm3_ctx_set_tuning",
    "imm3_ctx_measure_read_gbps", "imm3_ctx_devclock_enable", "imm3_ctx_devclock_collect", "imm3_ctx_devclock_raw", "imm3_query_plan",
    "imm3_ctx_inject_fault", "imm3_ctx_debug_device_lock", "imm3_plan_predict", "imm3_comm_debug_standin", "imm3_plan_limit_scan",
    "imm3_plan_table_limit", "imm3_plan_string_route", "imm3_plan_string_range_route", "imm3_plan_limit_chunks", "imm3_plan_distinct_capacity",
    "imm3_plan_int_list_table", "imm3_plan_int_list_form", "imm3_plan_int_list_probe",
    "imm3_plan_hi16_bounds", "imm3_plan_hi16_class", "imm3_plan_hi16_span_ok", "imm3_plan_hi16_eligible",
    "imm3_query_agg_form", "imm3_query_hi16_refined", "imm3_segment_hi16_plane", "imm3_query_expr_form", "imm3_expr_normalize", "imm3_query_group_order_path",
    "imm3_query_group_filter_stats", "imm3_group_filter_check", "imm3_comm_merge_view_path", "imm3_merge_view_plan_json",
    "imm3_plan_int_set_scratch_slots", "imm3_int_set_create_capped", "imm3_int_set_table",
]
COMM_ID_BYTES = 128
# imm3_query_device_ptr ids of an ordered query's arrays (include/imm3.h)
PTR_ORDER_ROW_INDEX, PTR_ORDER_ROW_COUNT, PTR_ORDER_COLUMN = 0x1000, 0x1001, 0x2000
# ORDER BY over groups (include/imm3.h: imm3_query_set_group_order; include/imm3_diag.h: imm3_query_group_order_path)
GROUP_ORDER_GROUP_COL, GROUP_ORDER_AGG = 0, 1
GROUP_ORDER_KEY_MAX_WIDTH = 12
ORDER_MAX_KEYS = 4             # IMM3_ORDER_MAX_KEYS: keys of an order, of rows and of groups alike
GROUP_ORDER_NONE, GROUP_ORDER_SMALL, GROUP_ORDER_RADIX_FULL, GROUP_ORDER_RADIX_SELECT = 0, 1, 2, 3
GROUP_ORDER_SMALL_MAX = 2048   # groups the one-work-group launch takes (csrc/imm3_internal.h: kGroupOrderSmall)
# HAVING (include/imm3.h: imm3_query_set_group_filter): a leaf's `agg` for the group's selected-row count; the leaf record
GROUP_FILTER_COUNT = -1
GROUP_FILTER_MAX_LEAVES, GROUP_FILTER_MAX_PROG = 8, 32
GROUP_FILTER_LEAF = np.dtype([("agg", "<i4"), ("average", "<i4"), ("cond", "<i4"), ("value", "<i8")], align=True)
TV_I32_SCAN = 26               # tuning variant: int32 range predicates scan the column itself, no high-half plane (csrc/imm3_handles.h)
TV_GROUP_ORDER_RADIX = 25      # tuning variant: an ordered aggregation takes the radix path whatever its group count
TV_ORDER_FULL_SORT, TV_ORDER_SELECT_ALWAYS = 23, 24   # tuning variants (csrc/imm3_handles.h): an ordered query with a limit always sorts every row / always selects


def group_filter_arrays(leaves: Sequence[tuple], prog: Sequence[int]):
    """imm3_query_set_group_filter's two arrays (never empty: the pointers stay valid)"""
    ls = np.zeros(max(len(leaves), 1), GROUP_FILTER_LEAF)
    for i, (agg, average, cond, value) in enumerate(leaves):
        ls[i] = (int(agg), 1 if average else 0, int(cond), int(value))
    pg = np.array(list(prog) or [0], dtype=np.int32)
    return ls, pg


def group_filter_check(agg_kinds: Sequence[int], agg_col_kinds: Sequence[int], leaves: Sequence[tuple], prog: Sequence[int], group=None, is_agg: bool = True):
    """imm3_group_filter_check (include/imm3_diag.h): the entry point's argument checks on plain values, no device.  group = (count,
    [values]): also the program's answer on that one group, by the evaluator the kernels run.  Raises Imm3Error as the call would."""
    ak = np.array(list(agg_kinds) or [0], dtype=np.int32)
    ck = np.array(list(agg_col_kinds) or [0], dtype=np.int32)
    ls, pg = group_filter_arrays(leaves, prog)
    kept = C.c_int32(-1)
    cv = None
    if group is not None:
        cv = np.zeros(5, np.int64)
        cv[0] = int(group[0])
        cv[1: 1 + len(group[1])] = [int(v) for v in group[1]]
    _check(load().imm3_group_filter_check(1 if is_agg else 0, ak.ctypes.data, ck.ctypes.data, len(agg_kinds), ls.ctypes.data, len(leaves), pg.ctypes.data, len(prog),
                                          cv.ctypes.data if cv is not None else None, C.byref(kept)))
    return None if group is None else bool(kept.value)


class Imm3Error(Exception):
    """The reference's `throw new Exception(msg)` as surfaced by the C ABI (status + message)."""

    def __init__(self, code: int, msg: str):
        super().__init__(msg)
        self.code = code
        self.msg = msg


class CColumn(C.Structure):
    _fields_ = [
        ("codec", C.c_int32),
        ("width", C.c_int32),
        ("dat", C.c_void_p),
        ("dat_bytes", C.c_uint64),
        ("block_offsets", C.c_void_p),
        ("n_offsets", C.c_int32),
    ]


class CSelect(C.Structure):
    _fields_ = [
        ("column", C.c_int32),
        ("cond", C.c_int32),
        ("value", C.c_double),
        ("match_bytes", C.c_void_p),
        ("match_lens", C.c_void_p),
        ("n_match", C.c_int32),
    ]


class CGroupView(C.Structure):
    """imm3_group_view (include/imm3.h): a view of merged groups -- filter, then order, then limit"""
    _fields_ = [
        ("order", C.c_void_p),
        ("n_order", C.c_int32),
        ("leaves", C.c_void_p),
        ("n_leaves", C.c_int32),
        ("prog", C.c_void_p),
        ("n_prog", C.c_int32),
        ("limit", C.c_int64),
    ]


def group_view(order: Sequence[tuple] = (), leaves: Sequence[tuple] = (), prog: Sequence[int] = (), limit: int = 0):
    """(CGroupView, the arrays it points into -- keep them alive as long as the view): order as set_group_order's keys, leaves / prog
    as set_group_filter's"""
    ks = np.array([[int(k), int(i), 1 if d else 0] for (k, i, d) in order] or [[0, 0, 0]], dtype=np.int32)
    ls, pg = group_filter_arrays(leaves, prog)
    v = CGroupView(ks.ctypes.data, len(order), ls.ctypes.data, len(leaves), pg.ctypes.data, len(prog), int(limit))
    return v, (ks, ls, pg)


def merge_view_plan(group_kinds: Sequence[int], group_widths: Sequence[int], agg_kinds: Sequence[int], agg_col_kinds: Sequence[int], agg_col_widths: Sequence[int],
                    largest_segment_index: int, order: Sequence[tuple] = (), leaves: Sequence[tuple] = (), prog: Sequence[int] = (), limit: int = 0) -> dict:
    """imm3_merge_view_plan_json (include/imm3_diag.h): the host-only plan of a view of merged groups on plain values, no device --
    {"seg_bytes", "user_bytes", "key_bytes", "canonical_bytes", "hash"}.  Column kinds: 0 = int32, 1 = int8, 2 = string.  Raises
    Imm3Error as imm3_comm_merge_groups_view would (a bad key or leaf; the refusal that begins with MERGE_VIEW_REFUSED)."""
    import json
    arrs = [np.array(list(a) or [0], dtype=np.int32) for a in (group_kinds, group_widths, agg_kinds, agg_col_kinds, agg_col_widths)]
    v, keep = group_view(order, leaves, prog, limit)
    buf = C.create_string_buffer(512)
    _check(load().imm3_merge_view_plan_json(len(group_kinds), arrs[0].ctypes.data, arrs[1].ctypes.data, len(agg_kinds), arrs[2].ctypes.data, arrs[3].ctypes.data,
                                            arrs[4].ctypes.data, C.byref(v), int(largest_segment_index), buf, 512, None))
    del keep
    return json.loads(buf.value.decode())


_lib = None


def load() -> C.CDLL:
    """Load libimm3.so; fail loudly when the HIP extension has not been built.
    Note for hosts that also use PyTorch-ROCm in the same process: import torch BEFORE the first call of this function.
    torch bundles its own HIP runtime; the runtime loaded first serves the process, a second instance sees no GPU."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("IMM3_LIB_PATH", LIB_PATH)   # development only: A/B an older build of the SAME library on one box
    if not os.path.exists(path):
        raise ImportError(
            f"{LIB_PATH} is missing: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C immutable3_amd/csrc). "
            "The immutable3 GPU path has no CPU fallback."
        )
    L = C.CDLL(path)
    if path != LIB_PATH:   # an older build lacks the newer entry points: bind what is there
        class _Tolerant:
            def __init__(self, lib):
                object.__setattr__(self, "_lib", lib)

            def __getattr__(self, name):
                try:
                    return getattr(object.__getattribute__(self, "_lib"), name)
                except AttributeError:
                    class _Missing:
                        argtypes = restype = None
                    return _Missing()
        L = _Tolerant(L)
    vp, i32, i64, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
    P = C.POINTER
    L.imm3_abi_version.restype = C.c_int
    L.imm3_last_error.restype = C.c_char_p
    L.imm3_device_count.argtypes = [P(C.c_int)]
    L.imm3_ctx_create.argtypes = [C.c_int, vp, P(vp)]
    L.imm3_ctx_destroy.argtypes = [vp]
    L.imm3_ctx_sync.argtypes = [vp]
    L.imm3_ctx_stream.argtypes = [vp, P(vp)]
    L.imm3_ctx_capture_begin.argtypes = [vp]
    L.imm3_ctx_capture_end.argtypes = [vp, P(vp)]
    L.imm3_graph_launch.argtypes = [vp]
    L.imm3_graph_destroy.argtypes = [vp]
    L.imm3_segment_create.argtypes = [vp, P(CColumn), i32, P(vp)]
    L.imm3_segment_wrap_device.argtypes = [vp, P(CColumn), i32, P(vp)]
    L.imm3_segment_create_async.argtypes = [vp, P(CColumn), i32, P(vp)]
    L.imm3_segment_wait.argtypes = [vp]
    L.imm3_segment_destroy.argtypes = [vp]
    L.imm3_segment_bytes.argtypes = [vp, P(u64)]
    L.imm3_query_create.argtypes = [vp, vp, vp, i32, P(CSelect), i32, vp, i32, i64, i32, P(vp)]
    L.imm3_query_create_agg.argtypes = [vp, vp, vp, i32, P(CSelect), i32, vp, i32, vp, i32, i32, P(vp)]
    L.imm3_table_create.argtypes = [vp, P(vp), i32, P(vp)]
    L.imm3_table_destroy.argtypes = [vp]
    L.imm3_query_create_table.argtypes = [vp, vp, vp, i32, P(CSelect), i32, vp, i32, i64, i32, P(vp)]
    L.imm3_query_create_table_agg.argtypes = [vp, vp, vp, i32, P(CSelect), i32, vp, i32, vp, i32, i32, P(vp)]
    L.imm3_query_segment_starts.argtypes = [vp, P(i32), vp, vp]
    L.imm3_query_locate_rows.argtypes = [vp, vp, u64, vp, vp]
    L.imm3_query_group_count.argtypes = [vp, P(C.c_uint32)]
    L.imm3_query_fetch_groups.argtypes = [vp, vp, vp, vp, vp, C.c_uint32]
    L.imm3_query_fetch_group_strings.argtypes = [vp, i32, vp, C.c_uint32]
    L.imm3_query_create_agg_wide.argtypes = [vp, vp, vp, i32, P(CSelect), i32, vp, i32, vp, i32, i32, P(vp)]
    L.imm3_query_create_table_agg_wide.argtypes = [vp, vp, vp, i32, P(CSelect), i32, vp, i32, vp, i32, i32, P(vp)]
    L.imm3_query_fetch_group_keys.argtypes = [vp, vp, C.c_uint32]
    L.imm3_query_create_expr.argtypes = [vp, vp, vp, i32, P(CSelect), i32, vp, i32, vp, i32, i64, i32, P(vp)]
    L.imm3_query_create_agg_expr.argtypes = [vp, vp, vp, i32, P(CSelect), i32, vp, i32, vp, i32, vp, i32, i32, P(vp)]
    L.imm3_query_create_table_expr.argtypes = L.imm3_query_create_expr.argtypes
    L.imm3_query_create_table_agg_expr.argtypes = L.imm3_query_create_agg_expr.argtypes
    L.imm3_query_expr_form.argtypes = [vp, P(i32)]
    L.imm3_expr_normalize.argtypes = [vp, vp, i32, P(CSelect), i32, vp, i32, vp, i64, P(i64)]
    L.imm3_query_destroy.argtypes = [vp]
    L.imm3_query_reserve_rows.argtypes = [vp, u64]
    L.imm3_query_set_order.argtypes = [vp, vp, i32, i64]
    L.imm3_query_set_group_order.argtypes = [vp, vp, i32, i64]
    L.imm3_query_group_order_path.argtypes = [vp, P(i32)]
    L.imm3_query_set_group_filter.argtypes = [vp, vp, i32, vp, i32]
    L.imm3_query_group_filter_stats.argtypes = [vp, P(u64), P(u64)]
    L.imm3_group_filter_check.argtypes = [i32, vp, vp, i32, vp, i32, vp, i32, vp, P(i32)]
    L.imm3_query_run.argtypes = [vp]
    L.imm3_query_run_select.argtypes = [vp]
    L.imm3_query_run_count.argtypes = [vp]
    L.imm3_query_sync.argtypes = [vp]
    L.imm3_query_join_count.argtypes = [vp]
    L.imm3_query_log_counts.argtypes = [vp, vp, C.c_uint64]
    L.imm3_query_layout.argtypes = [vp, P(i32), P(i64), P(i64)]
    L.imm3_query_batches.argtypes = [vp, vp, vp, vp]
    L.imm3_query_count.argtypes = [vp, P(u64)]
    L.imm3_query_bitmap.argtypes = [vp, vp, i64]
    L.imm3_query_row_count.argtypes = [vp, P(u64)]
    L.imm3_query_fetch_rows.argtypes = [vp, vp, P(vp), u64]
    L.imm3_query_device_ptr.argtypes = [vp, i32, P(vp)]
    L.imm3_ctx_timing_enable.argtypes = [vp, i32]
    L.imm3_ctx_timing_reset.argtypes = [vp]
    L.imm3_ctx_timing_mask.argtypes = [vp, C.c_uint32]
    L.imm3_ctx_timing_collect.argtypes = [vp, i32, vp, i32, P(i32)]
    L.imm3_ctx_set_tuning.argtypes = [vp, i32, i32]
    L.imm3_ctx_measure_read_gbps.argtypes = [vp, u64, i32, P(C.c_double)]
    L.imm3_ctx_devclock_enable.argtypes = [vp, i32]
    L.imm3_ctx_devclock_collect.argtypes = [vp, vp, i32, P(i32)]
    L.imm3_query_plan.argtypes = [vp, vp, i32]
    L.imm3_query_agg_form.argtypes = [vp, P(i32)]
    L.imm3_query_agg_shape.argtypes = [vp, P(i32), P(i32), P(i32)]
    L.imm3_ctx_inject_fault.argtypes = [vp, i32, i32, C.c_uint32]
    L.imm3_ctx_debug_device_lock.argtypes = [vp, u64, P(u64)]
    L.imm3_ctx_devclock_raw.argtypes = [vp, i32, vp, i32]
    L.imm3_comm_unique_id.argtypes = [vp]
    L.imm3_comm_create.argtypes = [vp, i32, i32, vp, P(vp)]
    L.imm3_comm_create_all.argtypes = [P(vp), i32, P(vp)]
    L.imm3_comm_destroy.argtypes = [vp]
    L.imm3_comm_info.argtypes = [vp, P(i32), P(i32)]
    L.imm3_comm_sync.argtypes = [vp]
    L.imm3_comm_join.argtypes = [vp]
    L.imm3_comm_allreduce_u64.argtypes = [vp, vp, u64]
    L.imm3_comm_debug_standin.argtypes = [vp, i32, C.c_uint32]
    L.imm3_comm_allreduce_count.argtypes = [vp, P(vp), i32, vp, P(u64)]
    L.imm3_comm_allreduce_count_all.argtypes = [P(vp), i32, P(P(vp)), P(i32), P(u64)]
    L.imm3_comm_merge_groups.argtypes = [vp, P(vp), vp, i32, vp, vp, vp, vp, C.c_uint32, P(C.c_uint32)]
    L.imm3_comm_merge_groups_all.argtypes = [P(vp), i32, P(P(vp)), P(vp), P(i32), vp, vp, vp, vp, C.c_uint32, P(C.c_uint32)]
    L.imm3_comm_merge_groups_wide.argtypes = [vp, P(vp), vp, i32, vp, vp, vp, vp, P(vp), C.c_uint32, P(C.c_uint32)]
    L.imm3_comm_merge_groups_wide_all.argtypes = [P(vp), i32, P(P(vp)), P(vp), P(i32), vp, vp, vp, vp, P(vp), C.c_uint32, P(C.c_uint32)]
    L.imm3_comm_merge_groups_view.argtypes = [vp, P(vp), vp, i32, P(CGroupView), vp, vp, vp, vp, P(vp), C.c_uint32, P(C.c_uint32), P(u64)]
    L.imm3_comm_merge_groups_view_all.argtypes = [P(vp), i32, P(P(vp)), P(vp), P(i32), P(CGroupView), vp, vp, vp, vp, P(vp), C.c_uint32, P(C.c_uint32), P(u64)]
    L.imm3_comm_merge_view_path.argtypes = [vp, P(i32)]
    L.imm3_merge_view_plan_json.argtypes = [i32, vp, vp, i32, vp, vp, vp, P(CGroupView), C.c_uint32, vp, i64, P(i64)]
    L.imm3_comm_merge_ordered.argtypes = [vp, P(vp), vp, i32, i64, vp, vp, P(vp), u64, P(u64)]
    L.imm3_comm_merge_ordered_all.argtypes = [P(vp), i32, P(P(vp)), P(vp), P(i32), i64, vp, vp, P(vp), u64, P(u64)]
    L.imm3_int_set_create.argtypes = [vp, P(vp), vp, i32, P(vp)]
    L.imm3_int_set_create_capped.argtypes = [vp, P(vp), vp, i32, i64, P(vp)]
    L.imm3_int_set_destroy.argtypes = [vp]
    L.imm3_int_set_info.argtypes = [vp, P(i64), P(i32), P(i32), P(i32)]
    L.imm3_int_set_values.argtypes = [vp, vp, i64]
    L.imm3_int_set_table.argtypes = [vp, vp, i64, P(i64), P(i32), P(i32), vp, P(i32)]
    L.imm3_plan_int_set_scratch_slots.argtypes = [i64, i32, i32, i64]
    for name in EXPORTS + DIAG_EXPORTS:
        fn = getattr(L, name)
        if name not in ("imm3_last_error", "imm3_pfor_encode_bound", "imm3_snappy_encode_bound"):
            fn.restype = C.c_int
    L.imm3_plan_int_set_scratch_slots.restype = C.c_int64
    L.imm3_snappy_encode_bound.restype = C.c_uint64
    L.imm3_snappy_encode_bound.argtypes = [C.c_uint64]
    L.imm3_snappy_encode_block.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.imm3_pfor_encode_bound.restype = C.c_uint64
    L.imm3_pfor_encode_bound.argtypes = [C.c_int32]
    L.imm3_pfor_encode_block.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.imm3_pfor_encode_column.argtypes = [C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]
    _lib = L
    return L


def _check(rc: int):
    if rc != OK:
        msg = load().imm3_last_error()
        raise Imm3Error(rc, msg.decode() if msg else f"imm3 error {rc}")


def pfor_encode_block(values) -> bytes:
    """PFORCodecInt.encode (core/codec/PFORCodec.scala:19-31) of one block of int32 values (host code)."""
    v = np.ascontiguousarray(values, dtype=np.int32)
    cap = load().imm3_pfor_encode_bound(v.size)
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_uint64(0)
    _check(load().imm3_pfor_encode_block(v.ctypes.data, v.size, out.ctypes.data, cap, C.byref(n)))
    return out[:n.value].tobytes()


def pfor_encode_column(values, block_rows: int):
    """A whole int32 column as SegmentWriter would write it with a PFOR_INT codec: (.dat bytes, blockOffset table)."""
    v = np.ascontiguousarray(values, dtype=np.int32)
    nb = (v.size + block_rows - 1) // block_rows
    cap = v.size * 4 + nb * (load().imm3_pfor_encode_bound(0) + 4 * (block_rows // 32 + 4)) + 64
    out = np.empty(cap, dtype=np.uint8)
    offs = np.zeros(nb + 1, dtype=np.int32)
    n = C.c_uint64(0)
    _check(load().imm3_pfor_encode_column(v.ctypes.data, v.size, block_rows, out.ctypes.data, cap, offs.ctypes.data, C.byref(n)))
    return out[:n.value].copy(), offs


def snappy_encode_block(raw) -> bytes:
    """SnappyCodec.encode (core/codec/SnappyCodec.scala:15-27) of one block's raw value bytes (host code)."""
    a = np.frombuffer(bytes(raw), dtype=np.uint8) if not isinstance(raw, np.ndarray) else np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    cap = load().imm3_snappy_encode_bound(a.size)
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_uint64(0)
    _check(load().imm3_snappy_encode_block(a.ctypes.data, a.size, out.ctypes.data, cap, C.byref(n)))
    return out[:n.value].tobytes()


def device_count() -> int:
    n = C.c_int(0)
    rc = load().imm3_device_count(C.byref(n))
    if rc != OK:
        return 0
    return n.value


class Context:
    """imm3_ctx: device id + HIP stream."""

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        """stream: a hipStream_t as an int (e.g. torch.cuda.Stream().cuda_stream), or None to let the library create its
        own non-blocking stream.  0 -- what torch reports for its default stream -- cannot be named through the C ABI
        (NULL means "create one"), and silently getting a private stream is how work ends up unordered: refuse it."""
        if stream is not None and int(stream) == 0:
            raise ValueError("stream 0 is HIP's legacy default stream and cannot be passed to imm3_ctx_create; pass None "
                             "(library-owned stream) or a real stream such as torch.cuda.Stream().cuda_stream")
        self._h = C.c_void_p()
        _check(load().imm3_ctx_create(device, C.c_void_p(int(stream)) if stream is not None else None, C.byref(self._h)))
        self.device = device
        # handles created on this context; closed before the context itself (they hold raw pointers into it)
        self._children = weakref.WeakSet()
        self._children_mu = threading.Lock()   # a context may be shared by threads (include/imm3.h, "Threading")

    def _adopt(self, child):
        with self._children_mu:
            self._children.add(child)

    def sync(self):
        _check(load().imm3_ctx_sync(self._h))

    @property
    def stream(self) -> int:
        s = C.c_void_p()
        _check(load().imm3_ctx_stream(self._h, C.byref(s)))
        return s.value or 0

    def capture(self) -> "_Capture":
        """`with ctx.capture() as cap: q0.run(); q1.run()` records the runs (nothing executes); `cap.graph.launch()`
        then enqueues all of their kernels with one call (imm3_ctx_capture_begin / _end, a hipGraph)."""
        return _Capture(self)

    def set_tuning(self, filter_variant: int = 0, grid_blocks: int = 0):
        _check(load().imm3_ctx_set_tuning(self._h, filter_variant, grid_blocks))

    def inject_fault(self, work_group: int = -1, span: int = -1, max_polls: int = 0):
        """Tools' build only (imm3_diag.h): work-group `work_group` of every single-pass launch never announces its `span`-th span;
        look-back waits give up after `max_polls` polls.  (-1, -1, 0) switches it off."""
        _check(load().imm3_ctx_inject_fault(self._h, work_group, span, max_polls))

    def debug_device_lock(self, value: int) -> int:
        """Overwrites the device's single-pass ticket word (0 = free); returns what it held (imm3_diag.h)."""
        prev = C.c_uint64(0)
        _check(load().imm3_ctx_debug_device_lock(self._h, value, C.byref(prev)))
        return prev.value

    def measure_read_gbps(self, nbytes: int = 400_000_000, iters: int = 30) -> float:
        g = C.c_double(0.0)
        _check(load().imm3_ctx_measure_read_gbps(self._h, nbytes, iters, C.byref(g)))
        return g.value

    def devclock_enable(self, max_launches: int):
        _check(load().imm3_ctx_devclock_enable(self._h, max_launches))

    def devclock_collect(self, cap: int = 65536) -> np.ndarray:
        out = np.zeros(cap, dtype=np.float32)
        n = C.c_int32(0)
        _check(load().imm3_ctx_devclock_collect(self._h, out.ctypes.data, cap, C.byref(n)))
        return out[: min(n.value, cap)]

    def devclock_raw(self, launch: int, n: int = 8192) -> np.ndarray:
        out = np.zeros(n, dtype=np.uint64)
        _check(load().imm3_ctx_devclock_raw(self._h, launch, out.ctypes.data, n))
        return out

    def timing_enable(self, max_records: int):
        _check(load().imm3_ctx_timing_enable(self._h, max_records))

    def timing_mask(self, kernel_mask: int):
        _check(load().imm3_ctx_timing_mask(self._h, kernel_mask))

    def timing_reset(self):
        _check(load().imm3_ctx_timing_reset(self._h))

    def timing_collect(self, kernel_id: int, cap: int = 65536) -> np.ndarray:
        out = np.zeros(cap, dtype=np.float32)
        n = C.c_int32(0)
        _check(load().imm3_ctx_timing_collect(self._h, kernel_id, out.ctypes.data, cap, C.byref(n)))
        return out[: min(n.value, cap)]

    def close(self):
        if self._h:
            # The C ABI allows any destruction order (handles are reference counted); closing dependants first simply
            # returns their device memory now instead of when the garbage collector gets to them.
            with self._children_mu:
                kids = list(self._children)
            for kind in (Graph, Comm, DeviceQuery, IntSet, DeviceTable, DeviceSegment):   # graphs, comms, queries -> sets -> tables -> segments
                for k in kids:
                    if isinstance(k, kind):
                        k.close()
            load().imm3_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Graph:
    """imm3_graph: a recorded sequence of query runs."""

    def __init__(self, ctx: Context, handle):
        self.ctx = ctx
        self._h = handle
        ctx._adopt(self)

    def launch(self):
        _check(load().imm3_graph_launch(self._h))

    def close(self):
        if self._h:
            load().imm3_graph_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Capture:
    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.graph: Optional[Graph] = None

    def __enter__(self):
        _check(load().imm3_ctx_capture_begin(self.ctx._h))
        return self

    def __exit__(self, exc_type, exc, tb):
        h = C.c_void_p()
        rc = load().imm3_ctx_capture_end(self.ctx._h, C.byref(h))
        if exc_type is None:
            _check(rc)
            self.graph = Graph(self.ctx, h)
        elif rc == OK:                       # the body failed: drop what was recorded, let its exception through
            load().imm3_graph_destroy(h)
        return False


def _ccolumns(cols):
    """cols: sequence of (codec, width, dat (np.uint8 array or int device ptr), dat_bytes, offsets int32 array)"""
    arr = (CColumn * len(cols))()
    keep = []
    for i, (codec, width, dat, nbytes, offsets) in enumerate(cols):
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        keep.append(offsets)
        arr[i].codec = codec
        arr[i].width = width
        if isinstance(dat, (int, np.integer)):
            arr[i].dat = int(dat)
        else:
            dat = np.ascontiguousarray(dat).view(np.uint8).reshape(-1)
            keep.append(dat)
            arr[i].dat = dat.ctypes.data if dat.size else None
        arr[i].dat_bytes = int(nbytes)
        arr[i].block_offsets = offsets.ctypes.data if offsets.size else None
        arr[i].n_offsets = int(offsets.size)
    return arr, keep


class DeviceSegment:
    """imm3_segment: all columns of one segment id, resident in HBM."""

    def __init__(self, ctx: Context, cols, wrap_device: bool = False, async_copy: bool = False):
        """async_copy: imm3_segment_create_async -- returns once the copies are enqueued on the context's copy stream; the
        host arrays are kept alive here until wait() (or the first close)."""
        self.ctx = ctx
        self.ncols = len(cols)
        arr, keep = _ccolumns(cols)
        self._h = C.c_void_p()
        fn = load().imm3_segment_wrap_device if wrap_device else (load().imm3_segment_create_async if async_copy else load().imm3_segment_create)
        _check(fn(ctx._h, arr, len(cols), C.byref(self._h)))
        ctx._adopt(self)
        self._keep = keep if (wrap_device or async_copy) else None
        self.widths = [c[1] for c in cols]
        self.codecs = [c[0] for c in cols]

    @property
    def device_bytes(self) -> int:
        n = C.c_uint64(0)
        _check(load().imm3_segment_bytes(self._h, C.byref(n)))
        return n.value

    def hi16_plane(self, col: int, rows: int):
        """imm3_segment_hi16_plane -- (state, (min half, max half), plane or None) of a DENSE_INT column's 16-bit high-half plane."""
        L = load()
        L.imm3_segment_hi16_plane.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.c_void_p]
        out = np.zeros(max(rows, 1), np.int16)
        state = C.c_int32(0)
        mm = np.zeros(2, np.int32)
        _check(L.imm3_segment_hi16_plane(self._h, col, out.ctypes.data, rows, C.byref(state), mm.ctypes.data))
        return state.value, (int(mm[0]), int(mm[1])), (out[:rows] if state.value == 1 else None)

    def wait(self):
        """The copies of an async_copy segment have consumed the host buffers."""
        _check(load().imm3_segment_wait(self._h))

    def close(self):
        if self._h:
            load().imm3_segment_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


AGG_COUNT, AGG_MIN, AGG_MAX, AGG_SUM = 0, 1, 2, 3
# include/imm3.h: IMM3_AGG_COUNT_DISTINCT -- the number of distinct values of the column among the group's selected rows (int32, int8,
# strings of 1 .. 4 bytes); 5, not 4: kinds 4 and 9 stay "Unknown Aggregate type"
AGG_COUNT_DISTINCT = 5
# kernel ids of Context.timing_collect (include/imm3_diag.h): the mark pass of a COUNT_DISTINCT aggregate, the clear of its pair set
KERNEL_DISTINCT_MARK, KERNEL_DISTINCT_CLEAR = 10, 11
# the aggregation's kernel forms (csrc/imm3_internal.h: AggForm; DeviceQuery.agg_form, tuning 100 + form)
AGG_FORM_LANES, AGG_FORM_LANES_WIDE, AGG_FORM_DIRECT, AGG_FORM_TILE, AGG_FORM_GENERAL = 0, 1, 2, 3, 4
GROUP_KEY_MAX_WIDTH = 256  # include/imm3.h: IMM3_GROUP_KEY_MAX_WIDTH (DeviceQuery(..., wide_keys=True))
TV_AGG_WEAK_HASH = 18      # tuning variant: wide group keys hash to 3 bits (csrc/imm3_handles.h)
TV_NO_LIMIT_CHUNKS = 14    # tuning variant: a `limit` never stops the scan -- the whole segment / table in one launch (csrc/imm3_handles.h)
# csrc/imm3_internal.h: kTableLimitClaimTiles -- a table query with a limit scans in runs of this many virtual tiles, claimed in
# ascending order by the work-groups of one launch, until the finished runs hold `limit` rows; kFinishLimitTiles -- the word of the
# finish block (DeviceQuery.device_ptr(1), u64 words) that then says how many tiles were scanned
TABLE_LIMIT_CLAIM_TILES = 32
FINISH_LIMIT_TILES = 12


class DeviceTable:
    """imm3_table: all segments of one table as one scan unit (one launch over the tile table)."""

    def __init__(self, ctx: Context, segs: Sequence[DeviceSegment]):
        self.ctx, self.segs = ctx, list(segs)
        arr = (C.c_void_p * len(self.segs))(*[s._h for s in self.segs])
        self._h = C.c_void_p()
        _check(load().imm3_table_create(ctx._h, arr, len(self.segs), C.byref(self._h)))
        ctx._adopt(self)
        self.widths, self.codecs = self.segs[0].widths, self.segs[0].codecs

    def close(self):
        if self._h:
            load().imm3_table_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RawIntList:
    """An INT_IN operand handed to the library as it stands: n_match and the values' buffer (None: a null match_bytes) -- for callers
    that hold the leaf's fields themselves, and for the tests of its argument checks."""

    def __init__(self, n_match: int, values=None):
        self.n_match, self.values = int(n_match), values


class RawIntSet:
    """An INT_IN_SET operand handed to the library as it stands: n_match and the handle (None: a null match_bytes) -- for the tests
    of the leaf's argument checks."""

    def __init__(self, n_match: int, int_set=None):
        self.n_match, self.int_set = int(n_match), int_set


class IntSet:
    """imm3_int_set: the distinct values one column takes among the rows a query selects, united over [(query, column), ...] --
    built on the device and kept there (imm3_int_set_create).  `column` indexes the query's used columns.  The operand of an
    INT_IN_SET leaf, (col, INT_IN_SET, int_set), in any number of queries of the same context; they keep it alive, so close() may
    come before they run.  max_values: the diagnostic creator with a lower cap on the distinct values (imm3_diag.h)."""

    def __init__(self, ctx: Context, sources: Sequence[tuple], max_values: Optional[int] = None):
        self.ctx = ctx
        srcs = list(sources)
        hs = (C.c_void_p * max(1, len(srcs)))(*[(q._h if q is not None else None) for q, _ in srcs])
        cols = np.array([int(c) for _, c in srcs] or [0], dtype=np.int32)
        self._h = C.c_void_p()
        if max_values is None:
            _check(load().imm3_int_set_create(ctx._h, hs, cols.ctypes.data, len(srcs), C.byref(self._h)))
        else:
            _check(load().imm3_int_set_create_capped(ctx._h, hs, cols.ctypes.data, len(srcs), int(max_values), C.byref(self._h)))
        ctx._adopt(self)

    def info(self):
        """(n_values, min, max, form): the distinct values, their extremes (0, 0 when empty), the INT_LIST_* form an int32 consumer probes"""
        n, lo, hi, form = C.c_int64(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _check(load().imm3_int_set_info(self._h, C.byref(n), C.byref(lo), C.byref(hi), C.byref(form)))
        return int(n.value), int(lo.value), int(hi.value), int(form.value)

    def values(self) -> np.ndarray:
        """the values, ascending, each once (copied from the device, sorted on the host)"""
        n = self.info()[0]
        out = np.zeros(max(n, 1), dtype=np.int32)
        _check(load().imm3_int_set_values(self._h, out.ctypes.data, n))
        return out[:n]

    def table(self):
        """imm3_diag.h: imm3_int_set_table -- (slots int32[], empty, max_probe, set256 uint32[8], host_route)"""
        n_slots, empty, max_probe, host = C.c_int64(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        set256 = np.zeros(8, np.uint32)
        _check(load().imm3_int_set_table(self._h, None, 0, C.byref(n_slots), C.byref(empty), C.byref(max_probe), set256.ctypes.data, C.byref(host)))
        slots = np.zeros(max(n_slots.value, 1), dtype=np.int32)
        if n_slots.value:
            _check(load().imm3_int_set_table(self._h, slots.ctypes.data, slots.size, C.byref(n_slots), C.byref(empty), C.byref(max_probe), set256.ctypes.data, C.byref(host)))
        return slots[: n_slots.value], int(empty.value), int(max_probe.value), set256, bool(host.value)

    def close(self):
        if self._h:
            load().imm3_int_set_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def plan_int_set_scratch_slots(selected_rows: int, lo: int, hi: int, cap: int = INT_IN_MAX_VALUES) -> int:
    """include/imm3_diag.h: imm3_plan_int_set_scratch_slots -- the slots of the scratch table an IntSet build inserts into; a pure
    function, no device needed."""
    return int(load().imm3_plan_int_set_scratch_slots(selected_rows, lo, hi, cap))


def _cselects(sels):
    """(CSelect array, the numpy buffers it points into) for [(column, cond, operand)]"""
    cs = (CSelect * max(1, len(sels)))()
    keep = []
    for i, (col, cond, operand) in enumerate(sels):
        cs[i].column = col
        cs[i].cond = cond
        cs[i].value = 0.0
        cs[i].n_match = 0
        if cond in (MATCH, NOTMATCH, STR_RANGE):   # (STR_RANGE: the two bounds travel as Match's values do)
            vals = [bytes(v) for v in (operand or [])]
            blob = np.frombuffer(b"".join(vals) or b"\0", dtype=np.uint8).copy()
            lens = np.array([len(v) for v in vals] or [0], dtype=np.int32)
            keep += [blob, lens]
            cs[i].match_bytes = blob.ctypes.data
            cs[i].match_lens = lens.ctypes.data
            cs[i].n_match = len(vals)
        elif cond == INT_IN and isinstance(operand, RawIntList):   # the leaf's fields as given (the library's own checks)
            blob = None if operand.values is None else np.array(list(operand.values) or [0], dtype="<i4")
            keep.append(blob)
            cs[i].match_bytes = None if blob is None else blob.ctypes.data
            cs[i].match_lens = None
            cs[i].n_match = operand.n_match
        elif cond == INT_IN_SET:   # the handle itself travels in match_bytes
            raw = operand if isinstance(operand, RawIntSet) else RawIntSet(1, operand)
            keep.append(raw.int_set)   # (the library retains the set; this keeps the Python object from closing it mid-call)
            cs[i].match_bytes = None if raw.int_set is None else raw.int_set._h
            cs[i].match_lens = None
            cs[i].n_match = raw.n_match
        elif cond == INT_IN:   # 4-byte little-endian values; no lengths
            vals = [int(v) for v in (operand if operand is not None else [])]
            if any(not -(1 << 31) <= v < (1 << 31) for v in vals):
                raise ValueError("an IntIn value is outside int32")
            blob = np.array(vals or [0], dtype="<i4")
            keep.append(blob)
            cs[i].match_bytes = blob.ctypes.data
            cs[i].match_lens = None
            cs[i].n_match = len(vals)
        elif operand is not None:
            cs[i].value = float(operand)
    return cs, keep


def plan_table_limit(table=1, tree=0, limit=10, count_in_scan=1, single_tile_pass=1, whole=0, count_log_on=0, count_only=0,
                     filter_variant=0, n_tiles=1 << 20, grid=512) -> int:
    """include/imm3_diag.h: imm3_plan_table_limit -- the library's own decision whether a table query with a limit runs the one
    launch that stops at the limit (1) or the whole select (0); a pure function, no device needed."""
    L = load()
    L.imm3_plan_table_limit.argtypes = [C.c_int32, C.c_int32, C.c_int64] + [C.c_int32] * 6 + [C.c_int64, C.c_int32]
    return int(L.imm3_plan_table_limit(table, tree, limit, count_in_scan, single_tile_pass, whole, count_log_on, count_only,
                                       filter_variant, n_tiles, grid))


def plan_limit_chunks(n_tiles: int) -> list:
    """include/imm3_diag.h: imm3_plan_limit_chunks -- the chunk ends (in tiles, ascending, the last one n_tiles) of a limit scan over
    a segment of n_tiles tiles; a pure function, no device needed."""
    L = load()
    L.imm3_plan_limit_chunks.argtypes = [C.c_int64, C.c_void_p, C.c_int32]
    ends = np.zeros(32, dtype=np.int64)
    n = int(L.imm3_plan_limit_chunks(n_tiles, ends.ctypes.data, 32))
    return [int(e) for e in ends[:n]]


def plan_string_route(width: int, n_match: int = 1) -> int:
    """include/imm3_diag.h: imm3_plan_string_route -- the kernel a string Match goes to on a uniform layout: 0 the tile kernel,
    1 k_filter_str_rows, 2 the word-at-a-time kernel (what a table refuses); a pure function, no device needed."""
    L = load()
    L.imm3_plan_string_route.argtypes = [C.c_int32, C.c_int32]
    return int(L.imm3_plan_string_route(width, n_match))


def plan_string_range_route(width: int) -> int:
    """include/imm3_diag.h: imm3_plan_string_range_route -- the kernel a STR_RANGE leaf goes to on a uniform layout: 1 the string
    pass (k_filter_str_range: widths 4, 8, ... 256), 2 the word-at-a-time kernel (what a table refuses), -1 outside 1 .. 256."""
    L = load()
    L.imm3_plan_string_range_route.argtypes = [C.c_int32]
    return int(L.imm3_plan_string_range_route(width))


def plan_int_list_form(width: int, n: int) -> int:
    """include/imm3_diag.h: imm3_plan_int_list_form -- the form of k_filter_int_list a folded IMM3_INT_IN list of n values takes on a
    column of `width` bytes: INT_LIST_I8 / _ARGS / _LDS / _GLOBAL, -1 for a bad argument; a pure function, no device needed."""
    L = load()
    L.imm3_plan_int_list_form.argtypes = [C.c_int32, C.c_int64]
    return int(L.imm3_plan_int_list_form(width, n))


# the 16-bit high-half plane (include/imm3_diag.h, csrc/imm3_hi16_plan.h)
HI16_FAIL, HI16_PASS, HI16_UNDECIDED = 0, 1, 2
HI16_MIN_SPAN = 64
HI16_FLAGS = ("table", "tree", "ragged", "dense_int", "has_list", "stages", "chunked", "has_plane", "pinned_i32")


def plan_hi16_bounds(lo: int, hi: int):
    """imm3_plan_hi16_bounds -- (possible_first, possible_count, certain_first, certain_count) of [lo, hi] over the halves v >> 16."""
    L = load()
    L.imm3_plan_hi16_bounds.argtypes = [C.c_int32, C.c_int32, C.c_void_p]
    out = np.zeros(4, np.uint32)
    _check(L.imm3_plan_hi16_bounds(lo, hi, out.ctypes.data))
    return tuple(int(x) for x in out)


def plan_hi16_class(lo: int, hi: int, half: int) -> int:
    """imm3_plan_hi16_class -- HI16_FAIL / HI16_PASS / HI16_UNDECIDED for a row whose half (v >> 16) is `half`."""
    L = load()
    L.imm3_plan_hi16_class.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    return int(L.imm3_plan_hi16_class(lo, hi, half))


def plan_hi16_span_ok(min_half: int, max_half: int) -> bool:
    L = load()
    L.imm3_plan_hi16_span_ok.argtypes = [C.c_int32, C.c_int32]
    return bool(L.imm3_plan_hi16_span_ok(min_half, max_half))


def plan_hi16_eligible(n_i32=1, n_i8=0, n_s2=0, **facts) -> bool:
    """imm3_plan_hi16_eligible -- does a tile pass's int32 predicate scan the plane; facts: the names of HI16_FLAGS."""
    L = load()
    L.imm3_plan_hi16_eligible.argtypes = [C.c_uint32, C.c_int32, C.c_int32, C.c_int32]
    flags = 0
    for name, on in facts.items():
        flags |= (1 << HI16_FLAGS.index(name)) if on else 0
    return bool(L.imm3_plan_hi16_eligible(flags, n_i32, n_i8, n_s2))


def plan_int_list_table(values):
    """include/imm3_diag.h: imm3_plan_int_list_table -- (slots int32[], empty, max_probe): the open-addressing table query creation
    builds for these int32 values; a pure function, no device needed."""
    L = load()
    L.imm3_plan_int_list_table.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    v = np.ascontiguousarray(np.asarray(values, dtype=np.int32))
    n_slots, empty, max_probe = C.c_int64(0), C.c_int32(0), C.c_int32(0)
    vp = v.ctypes.data if v.size else None
    _check(L.imm3_plan_int_list_table(vp, v.size, None, 0, C.byref(n_slots), C.byref(empty), C.byref(max_probe)))
    slots = np.zeros(n_slots.value, dtype=np.int32)
    _check(L.imm3_plan_int_list_table(vp, v.size, slots.ctypes.data, slots.size, C.byref(n_slots), C.byref(empty), C.byref(max_probe)))
    return slots, int(empty.value), int(max_probe.value)


def plan_int_list_probe(slots, empty: int, max_probe: int, v: int) -> int:
    """include/imm3_diag.h: imm3_plan_int_list_probe -- the kernels' bounded probe on the host: 1 found, 0 not, -1 bad table."""
    L = load()
    L.imm3_plan_int_list_probe.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32]
    s = np.ascontiguousarray(np.asarray(slots, dtype=np.int32))
    return int(L.imm3_plan_int_list_probe(s.ctypes.data, s.size, empty, max_probe, v))


def plan_distinct_capacity(rows: int, key_bytes: int, width: int) -> int:
    """include/imm3_diag.h: imm3_plan_distinct_capacity -- the entries of a COUNT_DISTINCT aggregate's pair set: the power of two at
    or above 2 x min(rows, min(rows, 256^key_bytes) x 256^width), at least 1024; -1 above 2^28 (creation refuses), -2 for a bad
    argument; a pure function, no device needed."""
    L = load()
    L.imm3_plan_distinct_capacity.argtypes = [C.c_int64, C.c_int32, C.c_int32]
    L.imm3_plan_distinct_capacity.restype = C.c_int64
    return int(L.imm3_plan_distinct_capacity(rows, key_bytes, width))


def expr_normalize(col_codecs: Sequence[int], col_widths: Sequence[int], leaves: Sequence[tuple], prog: Sequence[int]):
    """The normal form of a select tree (include/imm3_diag.h: imm3_expr_normalize), no device needed: a list of terms, each a list
    of {"col", "lo", "hi"} / {"col", "match": [bytes]} / {"col", "not_match": [bytes]} (a negated IN-list: every value but these)
    -- the selection is the OR of the terms, a term the AND of its predicates; [[]] selects every row, [] none."""
    import json
    cs, keep = _cselects(leaves)
    cc = np.array(list(col_codecs) or [0], dtype=np.int32)
    cw = np.array(list(col_widths) or [0], dtype=np.int32)
    pg = np.array(list(prog) or [0], dtype=np.int32)
    need = C.c_int64(0)
    args = (cc.ctypes.data, cw.ctypes.data, len(col_codecs), cs, len(leaves), pg.ctypes.data, len(prog))
    _check(load().imm3_expr_normalize(*args, None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value)
    _check(load().imm3_expr_normalize(*args, C.cast(buf, C.c_void_p), need.value, None))
    terms = json.loads(buf.value.decode())
    for t in terms:
        for p in t:
            for key in ("match", "not_match"):
                if key in p:
                    p[key] = [bytes.fromhex(h) for h in p[key]]
    return terms


class DeviceQuery:
    """imm3_query: ScanOp -> SelectOp* -> ProjectOp (or ProjectAggOp when `aggs` is given) over one device segment."""

    def __init__(self, ctx: Context, seg: DeviceSegment, used_cols: Sequence[int],
                 sels: Sequence[tuple], proj: Sequence[int] = (), limit: int = 0, table_block_size: int = 1024,
                 group_cols: Optional[Sequence[int]] = None, aggs: Optional[Sequence[tuple]] = None,
                 wide_keys: bool = False, expr: Optional[Sequence[int]] = None):
        """wide_keys: an aggregation through the _wide entry points (group keys of up to GROUP_KEY_MAX_WIDTH bytes).
        expr: a select TREE -- `sels` are its leaves and `expr` the postfix program over them (leaf indices, EXPR_AND, EXPR_OR,
        EXPR_NOT): the _expr entry points, which honour OR and NOT (a DeviceTable: the _table_expr ones -- ERR_ARG when the tree does not fit the one
        table launch).  Without it `sels` is a conjunction."""
        self.ctx, self.seg = ctx, seg
        self.used_cols = list(used_cols)
        self.proj = list(proj)
        self.group_cols = list(group_cols or [])
        self.aggs = list(aggs) if aggs is not None else None
        self.expr = list(expr) if expr is not None else None
        used = np.array(self.used_cols or [0], dtype=np.int32)
        pj = np.array(self.proj or [0], dtype=np.int32)
        cs, keep = _cselects(sels)
        self._h = C.c_void_p()
        self.is_table = isinstance(seg, DeviceTable)
        if self.expr is not None:
            create = load().imm3_query_create_table_expr if self.is_table else load().imm3_query_create_expr
            create_agg = load().imm3_query_create_table_agg_expr if self.is_table else load().imm3_query_create_agg_expr
            pg = np.array(self.expr or [0], dtype=np.int32)
            if self.aggs is not None:
                gc = np.array(self.group_cols or [0], dtype=np.int32)
                ag = np.array([[k, c] for (k, c) in self.aggs] or [[0, 0]], dtype=np.int32)
                _check(create_agg(ctx._h, seg._h, used.ctypes.data, len(self.used_cols), cs, len(sels),
                                  pg.ctypes.data, len(self.expr), gc.ctypes.data, len(self.group_cols),
                                  ag.ctypes.data, len(self.aggs), table_block_size, C.byref(self._h)))
            else:
                _check(create(ctx._h, seg._h, used.ctypes.data, len(self.used_cols), cs, len(sels),
                              pg.ctypes.data, len(self.expr), pj.ctypes.data, len(self.proj), limit,
                              table_block_size, C.byref(self._h)))
            self._finish_init(ctx, seg)
            return
        create = load().imm3_query_create_table if self.is_table else load().imm3_query_create
        if wide_keys:
            create_agg = load().imm3_query_create_table_agg_wide if self.is_table else load().imm3_query_create_agg_wide
        else:
            create_agg = load().imm3_query_create_table_agg if self.is_table else load().imm3_query_create_agg
        if self.aggs is not None:
            gc = np.array(self.group_cols or [0], dtype=np.int32)
            ag = np.array([[k, c] for (k, c) in self.aggs] or [[0, 0]], dtype=np.int32)
            _check(create_agg(ctx._h, seg._h, used.ctypes.data, len(self.used_cols), cs, len(sels),
                                                gc.ctypes.data, len(self.group_cols), ag.ctypes.data, len(self.aggs),
                                                table_block_size, C.byref(self._h)))
        else:
            _check(create(ctx._h, seg._h, used.ctypes.data, len(self.used_cols), cs, len(sels),
                          pj.ctypes.data, len(self.proj), limit, table_block_size, C.byref(self._h)))
        self._finish_init(ctx, seg)

    def _finish_init(self, ctx, seg):
        ctx._adopt(self)
        nb, tw, nr = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        _check(load().imm3_query_layout(self._h, C.byref(nb), C.byref(tw), C.byref(nr)))
        self.n_batches, self.total_words, self.n_rows = nb.value, tw.value, nr.value
        self.proj_widths = [seg.widths[self.used_cols[j]] for j in self.proj]
        self.proj_codecs = [seg.codecs[self.used_cols[j]] for j in self.proj]

    def batches(self):
        nb = max(self.n_batches, 1)
        size = np.zeros(nb, np.int32)
        oid = np.zeros(nb, np.int32)
        woff = np.zeros(nb, np.int64)
        _check(load().imm3_query_batches(self._h, size.ctypes.data, oid.ctypes.data, woff.ctypes.data))
        return size[: self.n_batches], oid[: self.n_batches], woff[: self.n_batches]

    def segment_starts(self):
        """(first_batch int32[n_seg+1], first_word int64[n_seg+1])"""
        n = C.c_int32(0)
        _check(load().imm3_query_segment_starts(self._h, C.byref(n), None, None))
        fb = np.zeros(n.value + 1, np.int32)
        fw = np.zeros(n.value + 1, np.int64)
        _check(load().imm3_query_segment_starts(self._h, C.byref(n), fb.ctypes.data, fw.ctypes.data))
        return fb, fw

    def locate_rows(self, row_index: np.ndarray):
        """virtual row ids of a table query -> (segment uint32[n], row-in-segment uint32[n])"""
        row_index = np.ascontiguousarray(row_index, dtype=np.uint32)
        seg = np.zeros(max(row_index.size, 1), np.uint32)
        row = np.zeros(max(row_index.size, 1), np.uint32)
        _check(load().imm3_query_locate_rows(self._h, row_index.ctypes.data, row_index.size, seg.ctypes.data, row.ctypes.data))
        return seg[: row_index.size], row[: row_index.size]

    def reserve_rows(self, rows: int):
        _check(load().imm3_query_reserve_rows(self._h, rows))

    def set_order(self, keys: Sequence[tuple], limit: int = 0):
        """ORDER BY (imm3_query_set_order): keys = [(index into the SELECT list, descending)], most significant first; limit > 0: the
        first `limit` rows of the ordered result.  Before the first run; row_count / fetch_rows then answer in that order."""
        ks = np.array([[int(p), 1 if d else 0] for (p, d) in keys] or [[0, 0]], dtype=np.int32)
        _check(load().imm3_query_set_order(self._h, ks.ctypes.data, len(keys), int(limit)))

    def set_group_order(self, keys: Sequence[tuple], limit: int = 0):
        """ORDER BY over groups (imm3_query_set_group_order): keys = [(GROUP_ORDER_GROUP_COL | GROUP_ORDER_AGG, index, descending)], most
        significant first; limit > 0: the first `limit` groups of the order.  Before or after runs; the group getters then answer in
        that order.  No keys: first-seen order again."""
        ks = np.array([[int(k), int(i), 1 if d else 0] for (k, i, d) in keys] or [[0, 0, 0]], dtype=np.int32)
        _check(load().imm3_query_set_group_order(self._h, ks.ctypes.data, len(keys), int(limit)))

    def group_order_path(self) -> int:
        """The path the last ordered settle took: GROUP_ORDER_NONE / _SMALL / _RADIX_FULL / _RADIX_SELECT (include/imm3_diag.h)."""
        p = C.c_int32(0)
        _check(load().imm3_query_group_order_path(self._h, C.byref(p)))
        return p.value

    def set_group_filter(self, leaves: Sequence[tuple], prog: Sequence[int]):
        """HAVING (imm3_query_set_group_filter): leaves = [(agg index | GROUP_FILTER_COUNT, average, GT | LT | EQ, int value)], prog =
        postfix over leaf indices with EXPR_AND / EXPR_OR / EXPR_NOT.  Before or after runs; the group getters then answer over the
        groups the program keeps -- filter, then order, then limit.  No leaves and no program: the filter is removed."""
        ls, pg = group_filter_arrays(leaves, prog)
        _check(load().imm3_query_set_group_filter(self._h, ls.ctypes.data, len(leaves), pg.ctypes.data, len(prog)))

    def group_filter_stats(self):
        """(groups the device's filter evaluated, groups it kept) of the last settled view; zeros without a filter or a current view"""
        gi, gk = C.c_uint64(0), C.c_uint64(0)
        _check(load().imm3_query_group_filter_stats(self._h, C.byref(gi), C.byref(gk)))
        return gi.value, gk.value

    def run(self):
        _check(load().imm3_query_run(self._h))

    def run_select(self):
        _check(load().imm3_query_run_select(self._h))

    def run_count(self):
        """ScanOp -> SelectOp* for the count alone: a single-launch chain stores no bitmap."""
        _check(load().imm3_query_run_count(self._h))

    def sync(self):
        _check(load().imm3_query_sync(self._h))

    def join_count(self):
        _check(load().imm3_query_join_count(self._h))

    def log_counts(self, device_ptr: int, capacity: int):
        """Every later run stores its selected-row count at device_ptr[k] (uint64, k = runs since this call)."""
        _check(load().imm3_query_log_counts(self._h, C.c_void_p(device_ptr), C.c_uint64(capacity)))

    def count(self) -> int:
        n = C.c_uint64(0)
        _check(load().imm3_query_count(self._h, C.byref(n)))
        return n.value

    def bitmap(self) -> np.ndarray:
        out = np.zeros(max(self.total_words, 1), dtype=np.uint64)
        _check(load().imm3_query_bitmap(self._h, out.ctypes.data, self.total_words))
        return out[: self.total_words]

    def row_count(self) -> int:
        n = C.c_uint64(0)
        _check(load().imm3_query_row_count(self._h, C.byref(n)))
        return n.value

    def fetch_rows(self):
        """(row_index uint32[n], [per projected column uint8[n, width]])"""
        n = self.row_count()
        cap = max(n, 1)
        idx = np.zeros(cap, dtype=np.uint32)
        cols = [np.zeros((cap, w), dtype=np.uint8) for w in self.proj_widths]
        ptrs = (C.c_void_p * max(1, len(cols)))(*[c.ctypes.data for c in cols])
        _check(load().imm3_query_fetch_rows(self._h, idx.ctypes.data, ptrs, n))
        return idx[:n], [c[:n] for c in cols]

    def fetch_groups(self):
        """(keys uint64[g], first_row uint32[g], counts uint64[g], vals int64[g, n_aggs]) in first-seen order."""
        n = C.c_uint32(0)
        _check(load().imm3_query_group_count(self._h, C.byref(n)))
        g = n.value
        na = max(1, len(self.aggs or []))
        keys = np.zeros(max(g, 1), np.uint64)
        first = np.zeros(max(g, 1), np.uint32)
        counts = np.zeros(max(g, 1), np.uint64)
        vals = np.zeros((max(g, 1), na), np.int64)
        _check(load().imm3_query_fetch_groups(self._h, keys.ctypes.data, first.ctypes.data, counts.ctypes.data, vals.ctypes.data, g))
        return keys[:g], first[:g], counts[:g], vals[:g, : len(self.aggs or [])]

    def fetch_group_strings(self, j: int) -> np.ndarray:
        """The exact value of string MAX aggregate j per group: uint8[g, width], groups in fetch_groups' order."""
        n = C.c_uint32(0)
        _check(load().imm3_query_group_count(self._h, C.byref(n)))
        g = n.value
        col = self.aggs[j][1] if self.aggs is not None and 0 <= j < len(self.aggs) else 0
        width = self.seg.widths[self.used_cols[col]] if 0 <= col < len(self.used_cols) else 1
        out = np.zeros((max(g, 1), width), np.uint8)
        _check(load().imm3_query_fetch_group_strings(self._h, j, out.ctypes.data, g))
        return out[:g]

    def fetch_group_keys(self) -> np.ndarray:
        """Every group's packed key bytes (the group columns' raw bytes in order): uint8[g, key_bytes], fetch_groups' order."""
        n = C.c_uint32(0)
        _check(load().imm3_query_group_count(self._h, C.byref(n)))
        g = n.value
        kb = C.c_int32(0)
        _check(load().imm3_query_agg_shape(self._h, None, None, C.byref(kb)))
        out = np.zeros((max(g, 1), max(kb.value, 1)), np.uint8)
        _check(load().imm3_query_fetch_group_keys(self._h, out.ctypes.data, g))
        return out[:g, : kb.value]

    def plan(self) -> dict:
        """How the library planned this query (include/imm3_diag.h: imm3_query_plan)."""
        v = np.zeros(15, np.int64)
        _check(load().imm3_query_plan(self._h, v.ctypes.data, 15))
        return {"single_pass": bool(v[0]), "P": int(v[1]), "grid": int(v[2]), "spans": int(v[3]), "records": bool(v[4]),
                "rec_dwords": int(v[5]), "ran_single_pass": bool(v[6]), "run_syncs": int(v[7]),
                "abandoned_runs": int(v[8]), "busy_runs": int(v[9]), "limit_gather_gave_up": int(v[10]),
                "order_select_runs": int(v[11]), "order_full_runs": int(v[12]), "order_launches": int(v[13]),
                "hi16_plane": bool(v[14])}

    def hi16_refined(self) -> bool:
        """imm3_query_hi16_refined -- has a full tile of a plane scan compared full values since the last call (reads and clears)."""
        L = load()
        L.imm3_query_hi16_refined.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        r = C.c_int32(0)
        _check(L.imm3_query_hi16_refined(self._h, C.byref(r)))
        return bool(r.value)

    def agg_form(self) -> int:
        """The kernel form (AGG_FORM_*) of this aggregation's last launch, -1 before the first (include/imm3_diag.h)."""
        f = C.c_int32(-1)
        _check(load().imm3_query_agg_form(self._h, C.byref(f)))
        return f.value

    def expr_form(self) -> int:
        """The kernel form of a select tree's last select launch: EXPR_FORM_TILE, EXPR_FORM_GENERIC, -1 when none ran."""
        f = C.c_int32(-1)
        _check(load().imm3_query_expr_form(self._h, C.byref(f)))
        return f.value

    def device_ptr(self, which: int) -> int:
        p = C.c_void_p()
        _check(load().imm3_query_device_ptr(self._h, which, C.byref(p)))
        return p.value or 0

    def close(self):
        if self._h:
            load().imm3_query_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def plan_predict(n_rows, pred, proj, rec_bytes, sigma, sloc, full):
    """The planner's cost model (csrc/imm3_plan.h): predicted us of plans A, B, C.  pred = [(width, n_match)], proj = [(width, is_pred)]."""
    lib = load()
    pw = (C.c_int32 * max(1, len(pred)))(*[w for w, _ in pred])
    pm = (C.c_int32 * max(1, len(pred)))(*[m for _, m in pred])
    jw = (C.c_int32 * max(1, len(proj)))(*[w for w, _ in proj])
    jp = (C.c_int32 * max(1, len(proj)))(*[1 if p else 0 for _, p in proj])
    out = (C.c_double * 3)()
    lib.imm3_plan_predict.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_void_p]
    lib.imm3_plan_predict.restype = C.c_int
    _check(lib.imm3_plan_predict(n_rows, pw, pm, len(pred), jw, jp, len(proj), rec_bytes, sigma, sloc, full, out))
    return {"A": out[0], "B": out[1], "C": out[2]}


def comm_unique_id() -> bytes:
    """imm3_comm_unique_id: rank 0 makes it, the host hands it to every rank (any channel)."""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    _check(load().imm3_comm_unique_id(buf))
    return bytes(buf)


class Comm:
    """imm3_comm: this rank's end of the RCCL communicator; the one collective of the path is the count all-reduce."""

    def __init__(self, ctx: Context, world: int, rank: int, unique_id: bytes):
        assert len(unique_id) == COMM_ID_BYTES
        self.ctx, self.world, self.rank = ctx, world, rank
        self._h = C.c_void_p()
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        _check(load().imm3_comm_create(ctx._h, world, rank, buf, C.byref(self._h)))
        ctx._adopt(self)

    @classmethod
    def create_all(cls, ctxs: Sequence[Context]) -> List["Comm"]:
        """Single-process flavour (ncclCommInitAll): one context per device, one Comm per context."""
        n = len(ctxs)
        harr = (C.c_void_p * n)(*[c._h for c in ctxs])
        out = (C.c_void_p * n)()
        _check(load().imm3_comm_create_all(harr, n, out))
        comms = []
        for i, c in enumerate(ctxs):
            o = cls.__new__(cls)
            o.ctx, o.world, o.rank, o._h = c, n, i, C.c_void_p(out[i])
            c._adopt(o)
            comms.append(o)
        return comms

    def sync(self):
        _check(load().imm3_comm_sync(self._h))

    def join(self):
        """The context's stream waits (stream side) for the last collective."""
        _check(load().imm3_comm_join(self._h))

    def debug_standin(self, work_groups: int, spin_us: int):
        """Tools' build: a kernel with RCCL's footprint in front of every count all-reduce (include/imm3_diag.h)."""
        _check(load().imm3_comm_debug_standin(self._h, work_groups, spin_us))

    def allreduce_u64(self, device_ptr: int, n: int):
        _check(load().imm3_comm_allreduce_u64(self._h, C.c_void_p(device_ptr), n))

    def allreduce_count(self, queries: Sequence["DeviceQuery"], device_out: int = 0, wait: bool = True) -> Optional[int]:
        """Sum of the queries' selected-row counts over all ranks.  wait=False only enqueues (device_out receives it)."""
        qs = (C.c_void_p * max(1, len(queries)))(*[q._h for q in queries])
        host = C.c_uint64(0)
        _check(load().imm3_comm_allreduce_count(self._h, qs, len(queries), C.c_void_p(device_out) if device_out else None,
                                                C.byref(host) if wait else None))
        return host.value if wait else None

    def merge_groups(self, queries: Sequence["DeviceQuery"], segment_index: Sequence[int]):
        """ProjectAggregateQueueOp across segments and ranks: (keys uint64[g], first uint64[g] = segment << 32 | row, counts uint64[g],
        vals int64[g, n_aggs]) in first-seen order; every rank gets the whole table."""
        qs = (C.c_void_p * max(1, len(queries)))(*[q._h for q in queries])
        seg = np.ascontiguousarray(segment_index, dtype=np.int32)
        na = max(1, len(queries[0].aggs or [])) if queries else 1
        n = C.c_uint32(0)
        _check(load().imm3_comm_merge_groups(self._h, qs, seg.ctypes.data, len(queries), None, None, None, None, 0, C.byref(n)))
        g = n.value
        keys, first, counts = np.zeros(max(g, 1), np.uint64), np.zeros(max(g, 1), np.uint64), np.zeros(max(g, 1), np.uint64)
        vals = np.zeros((max(g, 1), na), np.int64)
        _check(load().imm3_comm_merge_groups(self._h, qs, seg.ctypes.data, len(queries), keys.ctypes.data, first.ctypes.data, counts.ctypes.data,
                                             vals.ctypes.data, g, C.byref(n)))
        return keys[:g], first[:g], counts[:g], vals[:g]

    @staticmethod
    def merge_groups_all(comms: Sequence["Comm"], queries_per_comm: Sequence[Sequence["DeviceQuery"]], segments_per_comm: Sequence[Sequence[int]]):
        """Single-process flavour of merge_groups: one Comm per context -- create_all's (one context per device) or a world-of-one Comm per
        context, several on one device included: only a Comm's context is read --, each with its queries and their segment indices."""
        n = len(comms)
        carr = (C.c_void_p * n)(*[c._h for c in comms])
        qarrs = [(C.c_void_p * max(1, len(qs)))(*[q._h for q in qs]) for qs in queries_per_comm]
        qq = (C.POINTER(C.c_void_p) * n)(*[C.cast(a, C.POINTER(C.c_void_p)) for a in qarrs])
        segs = [np.ascontiguousarray(s, dtype=np.int32) for s in segments_per_comm]
        ss = (C.c_void_p * n)(*[s.ctypes.data if s.size else None for s in segs])
        nq = (C.c_int32 * n)(*[len(qs) for qs in queries_per_comm])
        na = max(1, len(next(q for qs in queries_per_comm for q in qs).aggs or []))
        g = C.c_uint32(0)
        _check(load().imm3_comm_merge_groups_all(carr, n, qq, ss, nq, None, None, None, None, 0, C.byref(g)))
        m = g.value
        keys, first, counts = np.zeros(max(m, 1), np.uint64), np.zeros(max(m, 1), np.uint64), np.zeros(max(m, 1), np.uint64)
        vals = np.zeros((max(m, 1), na), np.int64)
        _check(load().imm3_comm_merge_groups_all(carr, n, qq, ss, nq, keys.ctypes.data, first.ctypes.data, counts.ctypes.data, vals.ctypes.data, m, C.byref(g)))
        return keys[:m], first[:m], counts[:m], vals[:m]

    @staticmethod
    def _wide_buffers(q0: "DeviceQuery", g: int):
        """Result buffers of a merge by byte key, sized from imm3_query_agg_shape: (key bytes, first, counts, vals, {j: string bytes},
        the str_out pointer array)."""
        na, kb = C.c_int32(0), C.c_int32(0)
        _check(load().imm3_query_agg_shape(q0._h, None, C.byref(na), C.byref(kb)))
        n = max(g, 1)
        keys = np.zeros((n, max(kb.value, 1)), np.uint8)
        first, counts = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        vals = np.zeros((n, max(na.value, 1)), np.int64)
        strs = {}
        for j, (kind, col) in enumerate(q0.aggs or []):
            if kind == AGG_MAX and q0.seg.codecs[q0.used_cols[col]] in (DENSE_STRING, SNAPPY_STRING):
                strs[j] = np.zeros((n, q0.seg.widths[q0.used_cols[col]]), np.uint8)
        ptrs = (C.c_void_p * max(1, na.value))(*[strs[j].ctypes.data if j in strs else None for j in range(na.value)])
        return keys, first, counts, vals, strs, ptrs, na.value, kb.value

    def merge_groups_wide(self, queries: Sequence["DeviceQuery"], segment_index: Sequence[int], max_groups: Optional[int] = None):
        """merge_groups by byte key: any key width, string maxima of any width.  (key_bytes uint8[g, key_bytes], first uint64[g] =
        segment << 32 | row, counts uint64[g], vals int64[g, n_aggs], {j: uint8[g, width]} for every MAX over STRING aggregate j) in
        first-seen order; every rank gets the whole table.  max_groups: fetch only that many (the total is then the sixth item)."""
        qs = (C.c_void_p * max(1, len(queries)))(*[q._h for q in queries])
        seg = np.ascontiguousarray(segment_index, dtype=np.int32)
        n = C.c_uint32(0)
        _check(load().imm3_comm_merge_groups_wide(self._h, qs, seg.ctypes.data, len(queries), None, None, None, None, None, 0, C.byref(n)))
        g = n.value if max_groups is None else min(n.value, max_groups)
        keys, first, counts, vals, strs, ptrs, na, kb = self._wide_buffers(queries[0], g)
        _check(load().imm3_comm_merge_groups_wide(self._h, qs, seg.ctypes.data, len(queries), keys.ctypes.data, first.ctypes.data, counts.ctypes.data,
                                                  vals.ctypes.data, ptrs, g, C.byref(n)))
        out = (keys[:g, :kb], first[:g], counts[:g], vals[:g, :na], {j: b[:g] for j, b in strs.items()})
        return out if max_groups is None else out + (n.value,)

    @staticmethod
    def merge_groups_wide_all(comms: Sequence["Comm"], queries_per_comm: Sequence[Sequence["DeviceQuery"]], segments_per_comm: Sequence[Sequence[int]]):
        """Single-process flavour of merge_groups_wide: one Comm per context -- create_all's (one context per device) or a world-of-one Comm per
        context, several on one device included: only a Comm's context is read --, each with its queries and their segment indices."""
        n = len(comms)
        carr = (C.c_void_p * n)(*[c._h for c in comms])
        qarrs = [(C.c_void_p * max(1, len(qs)))(*[q._h for q in qs]) for qs in queries_per_comm]
        qq = (C.POINTER(C.c_void_p) * n)(*[C.cast(a, C.POINTER(C.c_void_p)) for a in qarrs])
        segs = [np.ascontiguousarray(s, dtype=np.int32) for s in segments_per_comm]
        ss = (C.c_void_p * n)(*[s.ctypes.data if s.size else None for s in segs])
        nq = (C.c_int32 * n)(*[len(qs) for qs in queries_per_comm])
        q0 = next(q for qs in queries_per_comm for q in qs)
        g = C.c_uint32(0)
        _check(load().imm3_comm_merge_groups_wide_all(carr, n, qq, ss, nq, None, None, None, None, None, 0, C.byref(g)))
        m = g.value
        keys, first, counts, vals, strs, ptrs, na, kb = Comm._wide_buffers(q0, m)
        _check(load().imm3_comm_merge_groups_wide_all(carr, n, qq, ss, nq, keys.ctypes.data, first.ctypes.data, counts.ctypes.data, vals.ctypes.data,
                                                      ptrs, m, C.byref(g)))
        return keys[:m, :kb], first[:m], counts[:m], vals[:m, :na], {j: b[:m] for j, b in strs.items()}

    def merge_groups_view(self, queries: Sequence["DeviceQuery"], segment_index: Sequence[int], order: Sequence[tuple] = (), leaves: Sequence[tuple] = (),
                          prog: Sequence[int] = (), limit: int = 0, max_groups: Optional[int] = None):
        """A view of the merged groups (imm3_comm_merge_groups_view): merge_groups_wide's merge, then filter (leaves / prog as
        set_group_filter's), then order (keys as set_group_order's), then limit, all on the device -- only the view's groups come
        back: (key_bytes, first, counts, vals, {j: string bytes}, n_kept) in the view's order, n_kept = the groups the filter kept
        before the limit.  With a limit (or max_groups) the call is made once, sized by it; else once for the count and once for the
        groups.  Imm3Error(ERR_ARG) whose message begins with MERGE_VIEW_REFUSED: the keys and the tie do not fit the device's order
        -- merge_groups_wide and the host's order are the way then."""
        qs = (C.c_void_p * max(1, len(queries)))(*[q._h for q in queries])
        seg = np.ascontiguousarray(segment_index, dtype=np.int32)
        view, keep = group_view(order, leaves, prog, limit)
        n, kept = C.c_uint32(0), C.c_uint64(0)
        cap = max_groups if max_groups is not None else (int(limit) if limit > 0 else None)
        if cap is None:
            _check(load().imm3_comm_merge_groups_view(self._h, qs, seg.ctypes.data, len(queries), C.byref(view), None, None, None, None, None, 0, C.byref(n), C.byref(kept)))
            cap = n.value
        keys, first, counts, vals, strs, ptrs, na, kb = self._wide_buffers(queries[0], cap)
        _check(load().imm3_comm_merge_groups_view(self._h, qs, seg.ctypes.data, len(queries), C.byref(view), keys.ctypes.data, first.ctypes.data, counts.ctypes.data,
                                                  vals.ctypes.data, ptrs, cap, C.byref(n), C.byref(kept)))
        del keep
        g = min(n.value, cap)
        return keys[:g, :kb], first[:g], counts[:g], vals[:g, :na], {j: b[:g] for j, b in strs.items()}, kept.value

    @staticmethod
    def merge_groups_view_all(comms: Sequence["Comm"], queries_per_comm: Sequence[Sequence["DeviceQuery"]], segments_per_comm: Sequence[Sequence[int]],
                              order: Sequence[tuple] = (), leaves: Sequence[tuple] = (), prog: Sequence[int] = (), limit: int = 0):
        """Single-process flavour of merge_groups_view (communicators as for merge_groups_wide_all): the merge finishes on the host,
        and so does the view, under the same rule.  Returns what merge_groups_view returns."""
        n = len(comms)
        carr = (C.c_void_p * n)(*[c._h for c in comms])
        qarrs = [(C.c_void_p * max(1, len(qs)))(*[q._h for q in qs]) for qs in queries_per_comm]
        qq = (C.POINTER(C.c_void_p) * n)(*[C.cast(a, C.POINTER(C.c_void_p)) for a in qarrs])
        segs = [np.ascontiguousarray(s, dtype=np.int32) for s in segments_per_comm]
        ss = (C.c_void_p * n)(*[s.ctypes.data if s.size else None for s in segs])
        nq = (C.c_int32 * n)(*[len(qs) for qs in queries_per_comm])
        q0 = next(q for qs in queries_per_comm for q in qs)
        view, keep = group_view(order, leaves, prog, limit)
        g, kept = C.c_uint32(0), C.c_uint64(0)
        cap = int(limit) if limit > 0 else None
        if cap is None:
            _check(load().imm3_comm_merge_groups_view_all(carr, n, qq, ss, nq, C.byref(view), None, None, None, None, None, 0, C.byref(g), C.byref(kept)))
            cap = g.value
        keys, first, counts, vals, strs, ptrs, na, kb = Comm._wide_buffers(q0, cap)
        _check(load().imm3_comm_merge_groups_view_all(carr, n, qq, ss, nq, C.byref(view), keys.ctypes.data, first.ctypes.data, counts.ctypes.data, vals.ctypes.data,
                                                      ptrs, cap, C.byref(g), C.byref(kept)))
        del keep
        m = min(g.value, cap)
        return keys[:m, :kb], first[:m], counts[:m], vals[:m, :na], {j: b[:m] for j, b in strs.items()}, kept.value

    def merge_view_path(self) -> int:
        """The path the last merge_groups_view on this communicator took: GROUP_ORDER_NONE / _SMALL / _RADIX_FULL / _RADIX_SELECT
        (include/imm3_diag.h: imm3_comm_merge_view_path)."""
        p = C.c_int32(0)
        _check(load().imm3_comm_merge_view_path(self._h, C.byref(p)))
        return p.value

    @staticmethod
    def _flat_segments(segment_index) -> np.ndarray:
        """segment_index of merge_ordered: an int per segment query, a sequence of ints per table query -> the flattened int32 array."""
        flat: List[int] = []
        for e in segment_index:
            flat.extend(int(x) for x in e) if isinstance(e, (list, tuple, np.ndarray)) else flat.append(int(e))
        return np.ascontiguousarray(flat, dtype=np.int32)

    @staticmethod
    def _ordered_buffers(q0: "DeviceQuery", n: int):
        rows = max(n, 1)
        seg, row = np.zeros(rows, np.uint32), np.zeros(rows, np.uint32)
        cols = [np.zeros((rows, w), np.uint8) for w in q0.proj_widths]
        ptrs = (C.c_void_p * max(1, len(cols)))(*[c.ctypes.data for c in cols])
        return seg, row, cols, ptrs

    def merge_ordered(self, queries: Sequence["DeviceQuery"], segment_index: Sequence, limit: int = 0, max_rows: Optional[int] = None):
        """The ordered rows (set_order) of this rank's queries and of every other rank's, merged on the device by (key, global segment,
        row) and cut to `limit` (0: all): (segment uint32[n], row uint32[n], [uint8[n, width] per SELECT-list column]); every rank
        gets the whole result.  segment_index: per query its global segment index, or for a query over a DeviceTable the global
        indices of the table's segments in table order.  max_rows: fetch only that many (the total is then the last item)."""
        qs = (C.c_void_p * max(1, len(queries)))(*[q._h for q in queries])
        flat = self._flat_segments(segment_index)
        n = C.c_uint64(0)
        if max_rows is None:
            try:                                             # one rank: its queries' rows bound the result, no call to ask for the total
                cap = sum(q.row_count() for q in queries) if self.world == 1 else None
            except (Imm3Error, AttributeError):
                cap = None                                   # (the merge itself says what is wrong with the query)
            if cap is None:
                _check(load().imm3_comm_merge_ordered(self._h, qs, flat.ctypes.data, len(queries), limit, None, None, None, 0, C.byref(n)))
                cap = n.value
            elif limit > 0:
                cap = min(cap, limit)
        else:
            cap = max_rows
        seg, row, cols, ptrs = self._ordered_buffers(queries[0], cap)
        _check(load().imm3_comm_merge_ordered(self._h, qs, flat.ctypes.data, len(queries), limit, seg.ctypes.data, row.ctypes.data, ptrs, cap, C.byref(n)))
        m = min(n.value, cap)
        out = (seg[:m], row[:m], [c[:m] for c in cols])
        return out if max_rows is None else out + (n.value,)

    @staticmethod
    def merge_ordered_all(comms: Sequence["Comm"], queries_per_comm: Sequence[Sequence["DeviceQuery"]], segments_per_comm: Sequence[Sequence], limit: int = 0):
        """Single-process flavour of merge_ordered: one Comm per context -- create_all's (one context per device) or a world-of-one Comm per
        context, several on one device included: only a Comm's context is read --, each with its queries and their segment indices."""
        n = len(comms)
        carr = (C.c_void_p * n)(*[c._h for c in comms])
        qarrs = [(C.c_void_p * max(1, len(qs)))(*[q._h for q in qs]) for qs in queries_per_comm]
        qq = (C.POINTER(C.c_void_p) * n)(*[C.cast(a, C.POINTER(C.c_void_p)) for a in qarrs])
        segs = [Comm._flat_segments(s) for s in segments_per_comm]
        ss = (C.c_void_p * n)(*[s.ctypes.data if s.size else None for s in segs])
        nq = (C.c_int32 * n)(*[len(qs) for qs in queries_per_comm])
        q0 = next(q for qs in queries_per_comm for q in qs)
        cap = sum(q.row_count() for qs in queries_per_comm for q in qs)
        if limit > 0:
            cap = min(cap, limit)
        seg, row, cols, ptrs = Comm._ordered_buffers(q0, cap)
        m = C.c_uint64(0)
        _check(load().imm3_comm_merge_ordered_all(carr, n, qq, ss, nq, limit, seg.ctypes.data, row.ctypes.data, ptrs, cap, C.byref(m)))
        k = min(m.value, cap)
        return seg[:k], row[:k], [c[:k] for c in cols]

    @staticmethod
    def allreduce_count_all(comms: Sequence["Comm"], queries_per_comm: Sequence[Sequence["DeviceQuery"]]) -> int:
        n = len(comms)
        carr = (C.c_void_p * n)(*[c._h for c in comms])
        qarrs = [(C.c_void_p * max(1, len(qs)))(*[q._h for q in qs]) for qs in queries_per_comm]
        qq = (C.POINTER(C.c_void_p) * n)(*[C.cast(a, C.POINTER(C.c_void_p)) for a in qarrs])
        nq = (C.c_int32 * n)(*[len(qs) for qs in queries_per_comm])
        host = C.c_uint64(0)
        _check(load().imm3_comm_allreduce_count_all(carr, n, qq, nq, C.byref(host)))
        return host.value

    def close(self):
        if self._h:
            load().imm3_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
