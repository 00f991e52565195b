"""GPU-backed Operator / ScanOp / SelectOp / ProjectOp / Engine -- the host-side mirror of the reference's
operator interface for the hot path (same names, argument meaning and error behaviour):

    engine/src/main/scala/immutabledb/engine/operator/Operator.scala:14-28   Operator / ColumnVectorOperator / ProjectionOperator
    engine/src/main/scala/immutabledb/engine/operator/Scan.scala:10-73       ScanOp, mkScanOp
    engine/src/main/scala/immutabledb/engine/operator/Select.scala:5-165     SelectOp, mkSelectOp
    engine/src/main/scala/immutabledb/engine/operator/Project.scala:8-81     ProjectOp, mkProjectOp
    engine/src/main/scala/immutabledb/engine/Engine.scala:85-128,158-262     getColumns / resolveSelectOps / execute / PipelineThread
    core/src/main/scala/immutabledb/DataVector.scala:15-48                   ColumnVectorBatch family

The operators are PLAN BUILDERS: composing them costs nothing, and the first `iterator` call fuses the
chain ScanOp -> SelectOp* (-> ProjectOp) of one segment into one imm3_query, i.e. one fused scan+select
kernel (+ offsets scan + compact/gather) on the segment's HBM-resident columns.  Everything that touches
data goes through the C ABI (immutable3_amd/native.py -> libimm3.so); there is no CPU evaluation path.
"""
from __future__ import annotations

import decimal
from dataclasses import dataclass
from typing import Callable, Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from . import native
from .native import Imm3Error
from .query import (STR_RANGE_CONDS, IntIn, IntInQuery, str_range_bounds)
from .query import (EQ, GT, LT, And, Avg, Count, CountDistinct, Match, Max, Min, NoOp, NoSelect, NotMatch, Or, Project, ProjectAgg,
                    Query, Select, SelectADT, SelectCondition, Sum, group_filter_leaves, order_keys)
from .schema import CodecType, Column, Row, Table
from .storage import SegmentManager


# ------------------------------------------------------------------------------------------
# vectors (core/.../DataVector.scala)
# ------------------------------------------------------------------------------------------
class BitSet:
    """scala.collection.mutable.BitSet over the uint64 words the GPU produced (bit i <-> word i>>6, bit i&63)."""

    def __init__(self, words: np.ndarray):
        self.words = words

    def contains(self, i: int) -> bool:
        w = i >> 6
        return w < self.words.size and bool((int(self.words[w]) >> (i & 63)) & 1)

    __call__ = contains
    __contains__ = contains

    @property
    def size(self) -> int:
        return int(np.unpackbits(self.words.view(np.uint8)).sum()) if self.words.size else 0

    @property
    def isEmpty(self) -> bool:
        return not self.words.any()

    def toList(self) -> List[int]:
        if not self.words.size:
            return []
        bits = np.unpackbits(self.words.view(np.uint8), bitorder="little")
        return np.flatnonzero(bits).tolist()

    def __iter__(self):
        return iter(self.toList())


@dataclass
class ColumnVector:                 # IntColumnVector / TinyIntColumnVector / StringColumnVector (:42-48)
    data: np.ndarray


class IntColumnVector(ColumnVector):
    pass


class TinyIntColumnVector(ColumnVector):
    pass


class StringColumnVector(ColumnVector):
    pass


@dataclass
class FilledColumnVectorBatch:      # DataVector.scala:24-31
    oid: int
    size: int
    columnVectors: List[ColumnVector]
    columns: List[Column]
    selected: BitSet
    selectedInUse: bool


ColumnVectorBatch = FilledColumnVectorBatch


def _decode_view(col: Column, raw: np.ndarray) -> ColumnVector:
    """DENSE_* decode is a fixed-width little-endian reinterpretation (DenseCodec.scala:37-73): a view."""
    if col.codec == CodecType.DENSE_INT:
        return IntColumnVector(raw.view("<i4"))
    if col.codec == CodecType.DENSE_TINYINT:
        return TinyIntColumnVector(raw.view(np.int8))
    if col.codec == CodecType.DENSE_STRING:
        return StringColumnVector(raw.reshape(-1, col.width))
    raise Exception(f"No implementation for {col.codec}")


# ------------------------------------------------------------------------------------------
# device-resident SegmentManager
# ------------------------------------------------------------------------------------------
class GpuSegmentManager:
    """What SegmentManager is to the reference (mmap everything once, keep it for the process lifetime,
    SegmentManager.scala:20-23), this is to the GPU path: every segment of every table staged into HBM
    once.  Segment s lives on the context `ctxs[s % len(ctxs)]` (segment-per-GPU sharding)."""

    def __init__(self, sm: SegmentManager, ctxs: Sequence[native.Context] | native.Context | None = None,
                 segment_filter: Optional[Callable[[str, int], bool]] = None):
        if ctxs is None:
            ctxs = [native.Context(0)]
        if isinstance(ctxs, native.Context):
            ctxs = [ctxs]
        self.sm = sm
        self.ctxs = list(ctxs)
        self.tables = sm.tables
        self._segs: Dict[Tuple[str, int], native.DeviceSegment] = {}
        self._tables: Dict[str, Optional[native.DeviceTable]] = {}
        self._filter = segment_filter
        self._merge_comms: Dict[int, native.Comm] = {}

    def merge_comm(self, ci: int) -> native.Comm:
        """The one-rank communicator of context `ci` that the ordered device merge runs on, made once and kept until close():
        creating one initialises RCCL, which costs far more than a merge.  (One rank: its collectives launch nothing and it
        reserves nothing on the device.)"""
        if ci not in self._merge_comms:
            self._merge_comms[ci] = native.Comm(self.ctxs[ci], 1, 0, native.comm_unique_id())
        return self._merge_comms[ci]

    def getTable(self, tableName: str) -> Table:
        return self.sm.getTable(tableName)

    def getTableSegmentCount(self, tableName: str) -> int:
        return self.sm.getTableSegmentCount(tableName)

    def ctx_of(self, segIdx: int) -> native.Context:
        return self.ctxs[segIdx % len(self.ctxs)]

    def owns(self, tableName: str, segIdx: int) -> bool:
        return self._filter is None or self._filter(tableName, segIdx)

    def device_segment(self, tableName: str, segIdx: int) -> native.DeviceSegment:
        key = (tableName, segIdx)
        if key not in self._segs:
            t = self.getTable(tableName)
            cols = []
            for c in t.columns:
                k = f"{tableName}.{c.name}"
                dat = self.sm.segments[k][segIdx]
                meta = self.sm.segmentsMeta[k][segIdx]
                cols.append((CodecType.id_of(c.codec), c.width, dat, dat.size, meta.blockOffsets))
            self._segs[key] = native.DeviceSegment(self.ctx_of(segIdx), cols)
        return self._segs[key]

    def device_table(self, tableName: str) -> Optional[native.DeviceTable]:
        """All owned segments of the table as one scan unit (imm3_table), or None when the table cannot take the
        single-launch path (ragged segments, several contexts): callers then fall back to per-segment pipelines."""
        if tableName in self._tables:
            return self._tables[tableName]
        table = None
        if len(self.ctxs) == 1:
            segs = [s for s in range(self.getTableSegmentCount(tableName)) if self.owns(tableName, s)]
            if segs:
                try:
                    table = native.DeviceTable(self.ctxs[0], [self.device_segment(tableName, s) for s in segs])
                    table.segment_ids = segs
                except Imm3Error as e:
                    if e.code != native.ERR_LAYOUT:
                        raise
        self._tables[tableName] = table
        return table

    def close(self):
        for c in self._merge_comms.values():
            c.close()
        self._merge_comms.clear()
        for t in self._tables.values():
            if t is not None:
                t.close()
        self._tables.clear()
        for s in self._segs.values():
            s.close()
        self._segs.clear()


# ------------------------------------------------------------------------------------------
# operators
# ------------------------------------------------------------------------------------------
class Operator:                      # Operator.scala:14-16
    def iterator(self):
        raise NotImplementedError

    def __iter__(self):
        return self.iterator()


class ColumnVectorOperator(Operator):  # Operator.scala:18-20
    pass


class ProjectionOperator(Operator):    # Operator.scala:26-28
    pass


class IntInSet(SelectCondition):
    """An IntInQuery whose inner query has run: membership in the device-resident set built from its selection (native.IntSet,
    IMM3_INT_IN_SET).  Made by Engine.resolve_subqueries only; every consumer query retains the set."""

    def __init__(self, int_set: "native.IntSet"):
        self.int_set = int_set

    def __repr__(self):
        return f"IntInSet({self.int_set.info()[0]} values)"


SUPPORTED_CONDS = (Match, GT, LT, EQ) + STR_RANGE_CONDS + (IntIn, IntInSet)   # what SelectOp.iterator lets through (Select.scala:17-23, and the range, integer-list and set extensions)


def _cond_spec(cond: SelectCondition, width: int = 0):
    """(native cond, operand) of one leaf; width: bytes of the leaf's column (the range forms are made for it)"""
    if isinstance(cond, STR_RANGE_CONDS):
        return native.STR_RANGE, list(str_range_bounds(cond, width))
    if isinstance(cond, IntIn):
        return native.INT_IN, list(cond.values)
    if isinstance(cond, IntInSet):
        return native.INT_IN_SET, cond.int_set
    if isinstance(cond, Match):
        return native.MATCH, [v.encode("utf-8") if isinstance(v, str) else bytes(v) for v in cond.values]
    if isinstance(cond, NotMatch):
        return native.NOTMATCH, [v.encode("utf-8") if isinstance(v, str) else bytes(v) for v in cond.values]
    if isinstance(cond, GT):
        return native.GT, cond.gt
    if isinstance(cond, LT):
        return native.LT, cond.lt
    if isinstance(cond, EQ):
        return native.EQ, cond.eq
    return native.NOOP, None


class ScanOp(ColumnVectorOperator):
    """Scan.scala:17: ScanOp(sm, segIdx, tableName, cols)."""

    def __init__(self, sm: GpuSegmentManager, segIdx: int, tableName: str, cols: Sequence[Column]):
        self.sm, self.segIdx, self.tableName, self.cols = sm, segIdx, tableName, list(cols)

    @staticmethod
    def mkScanOp(sm: GpuSegmentManager, tableName: str):       # Scan.scala:10-15
        return lambda cols, segIdx: ScanOp(sm, segIdx, tableName, cols)

    # -- plan pieces used by SelectOp / ProjectOp --
    def _table(self) -> Table:
        return self.sm.getTable(self.tableName)

    def _used_indices(self) -> List[int]:
        t = self._table()
        names = [c.name for c in t.columns]
        return [names.index(c.name) for c in self.cols]

    def _query(self, leaves, proj_names: Sequence[str] = (), limit: int = 0, expr=None) -> native.DeviceQuery:
        t = self._table()
        colnames = [c.name for c in self.cols]
        sels = []
        for (col, cond) in leaves:
            # `vec.columns...filter(_.name == col).head` (Select.scala:60): first used column of that name
            if col not in colnames:
                raise Exception("NoSuchElementException: next on empty iterator")
            code, operand = _cond_spec(cond, self.cols[colnames.index(col)].width)
            sels.append((colnames.index(col), code, operand))
        # Project.scala:32-35: vecCols maps each SELECT-list name to its position among the batch columns
        proj = []
        for name in proj_names:
            if name not in colnames:
                raise Exception(f"NoSuchElementException: key not found: {name}")
            proj.append(colnames.index(name))
        seg = self.sm.device_segment(self.tableName, self.segIdx)
        return native.DeviceQuery(seg.ctx, seg, self._used_indices(), sels, proj, limit, t.blockSize, expr=expr)

    def _pfor_decoded(self, c: Column) -> np.ndarray:
        """PFOR_INT column of this segment as the GPU decodes it (one projection without predicates), cached."""
        cache = self.__dict__.setdefault("_pfor_cache", {})
        if c.name not in cache:
            seg = self.sm.device_segment(self.tableName, self.segIdx)
            t = self._table()
            q = native.DeviceQuery(seg.ctx, seg, [[x.name for x in t.columns].index(c.name)], [], [0], 0, t.blockSize)
            q.run()
            _, cols = q.fetch_rows()
            q.close()
            raw = cols[0]
            cache[c.name] = (raw.reshape(-1).view("<i4").copy() if c.codec in CodecType.INT_CODECS else
                             raw.reshape(-1).view(np.int8).copy() if c.codec in CodecType.TINYINT_CODECS else raw.reshape(-1, c.width).copy())
        return cache[c.name]

    def _host_vectors(self, k: int, start_row: int, size: int) -> List[ColumnVector]:
        out = []
        for c in self.cols:
            if c.codec == CodecType.PFOR_INT or c.codec in CodecType.SNAPPY:   # compressed: the GPU's decode
                dec = self._pfor_decoded(c)
                if c.codec in CodecType.INT_CODECS:
                    out.append(IntColumnVector(dec[start_row:start_row + size]))
                elif c.codec in CodecType.TINYINT_CODECS:
                    out.append(TinyIntColumnVector(dec[start_row:start_row + size]))
                else:
                    out.append(StringColumnVector(dec[start_row:start_row + size]))
                continue
            dat = self.sm.sm.segments[f"{self.tableName}.{c.name}"][self.segIdx]
            out.append(_decode_view(c, np.asarray(dat[start_row * c.width: (start_row + size) * c.width])))
        return out

    def _batches(self, leaves, expr=None) -> Iterator[FilledColumnVectorBatch]:
        q = self._query(leaves, expr=expr)
        q.run_select()
        size, oid, woff = q.batches()
        words = q.bitmap()
        q.close()
        row = 0
        for k in range(q.n_batches):
            n = int(size[k])
            nw = (n + 63) // 64
            sel = BitSet(words[int(woff[k]): int(woff[k]) + nw])
            # selectedInUse = false when a SelectOp leaves the batch empty (Select.scala:44-47); ScanOp alone yields true
            in_use = (not sel.isEmpty) if leaves else True
            yield FilledColumnVectorBatch(int(oid[k]), n, self._host_vectors(k, row, n), list(self.cols), sel, in_use)
            row += n

    def iterator(self):
        return self._batches([])


class SelectOp(ColumnVectorOperator):
    """Select.scala:14: SelectOp(col, cond, op).  NotMatch / NoOp are rejected when the iterator is built (:22)."""

    def __init__(self, col: str, cond: SelectCondition, op: ColumnVectorOperator):
        self.col, self.cond, self.op = col, cond, op

    @staticmethod
    def mkSelectOp(col: str, cond: SelectCondition):            # Select.scala:5-12
        return lambda op: SelectOp(col, cond, op)

    def _chain(self):
        """-> (ScanOp, [(col, cond)] in application order: innermost SelectOp first)."""
        leaves = []
        op = self
        while isinstance(op, SelectOp):
            leaves.append((op.col, op.cond))
            op = op.op
        if not isinstance(op, ScanOp):
            raise Exception("SelectOp chain must end in a ScanOp for the fused GPU path")
        leaves.reverse()
        return op, leaves

    def iterator(self):
        scan, leaves = self._chain()
        for (_, cond) in leaves:
            if not isinstance(cond, SUPPORTED_CONDS):
                raise Exception(f"Unsupported condition: {cond}")   # Select.scala:22
        return scan._batches(leaves)


def select_program(select: SelectADT, honour_not_match: bool = False):
    """A SelectADT (Query.scala:11-15) as the leaves and the postfix program of include/imm3.h's select trees, post-order:
    ([(col, cond)], [leaf index | native.EXPR_AND | native.EXPR_OR | native.EXPR_NOT]).  NoSelect adds nothing.
    honour_not_match: a NotMatch(values) leaf is emitted as Match(values) followed by EXPR_NOT; off, it stays the NotMatch leaf
    every consumer rejects ("Unsupported condition", Select.scala:22)."""
    leaves, prog = [], []

    def rec(sel):
        if isinstance(sel, (And, Or)):
            before = len(prog)
            rec(sel.op1)
            mid = len(prog)
            rec(sel.op2)
            if mid > before and len(prog) > mid:          # (a NoSelect side adds nothing: the other side stands alone)
                prog.append(native.EXPR_AND if isinstance(sel, And) else native.EXPR_OR)
        elif isinstance(sel, Select):
            prog.append(len(leaves))
            if honour_not_match and isinstance(sel.cond, NotMatch):
                leaves.append((sel.col, Match(list(sel.cond.values))))
                prog.append(native.EXPR_NOT)
            else:
                leaves.append((sel.col, sel.cond))
    rec(select)
    return leaves, prog


def has_or(select: SelectADT) -> bool:
    return isinstance(select, Or) or (isinstance(select, And) and (has_or(select.op1) or has_or(select.op2)))


def has_not_match(select: SelectADT) -> bool:
    if isinstance(select, (And, Or)):
        return has_not_match(select.op1) or has_not_match(select.op2)
    return isinstance(select, Select) and isinstance(select.cond, NotMatch)


class SelectTreeOp(ColumnVectorOperator):
    """A whole SelectADT over a ScanOp with its AND / OR tags HONOURED -- what the reference announces and does not do
    (Engine.scala:236,266: "TODO: use AND/OR operators"; its runOps applies the leaves one after the other).  Fuses with ScanOp /
    ProjectOp / ProjectAggOp like a SelectOp chain does: one imm3 query per segment (imm3_query_create_expr).
    honour_not_match: a NotMatch leaf runs as the complement of its Match (select_program); off, it raises as in the reference."""

    def __init__(self, select: SelectADT, op: ColumnVectorOperator, honour_not_match: bool = False):
        self.select, self.op, self.honour_not_match = select, op, honour_not_match
        self.program: List[int] = []

    @staticmethod
    def mkSelectTreeOp(select: SelectADT, honour_not_match: bool = False):
        return lambda op: SelectTreeOp(select, op, honour_not_match)

    def _chain(self):
        """-> (ScanOp, [(col, cond)] in program order); the program itself is left in self.program"""
        if not isinstance(self.op, ScanOp):
            raise Exception("SelectTreeOp must sit on a ScanOp for the fused GPU path")
        leaves, self.program = select_program(self.select, self.honour_not_match)
        return self.op, leaves

    def iterator(self):
        scan, leaves = self._chain()
        for (_, cond) in leaves:
            if not isinstance(cond, SUPPORTED_CONDS):
                raise Exception(f"Unsupported condition: {cond}")   # Select.scala:22
        return scan._batches(leaves, self.program)


def _expr_of(op):
    """the program a fused launch passes on: a SelectTreeOp's (after its _chain()), None for a SelectOp chain"""
    return op.program if isinstance(op, SelectTreeOp) else None


def merge_ordered(parts, keys, limit: int = 0):
    """The host merge of per-segment ordered results: parts = [(segIdx, row_index, [typed column arrays])], keys = [(index into the
    columns, descending)].  Returns (segment int64[n], row int64[n], [column arrays]) ordered by (keys, segment, row) -- int columns as
    signed integers, string columns (uint8[n, width]) byte-wise unsigned -- and cut to `limit` rows when limit > 0."""
    parts = list(parts)
    if not parts:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), []
    seg = np.concatenate([np.full(np.asarray(ri).size, s, np.int64) for (s, ri, _) in parts])
    row = np.concatenate([np.asarray(ri).astype(np.int64) for (_, ri, _) in parts])
    cols = [np.concatenate([p[2][j] for p in parts]) for j in range(len(parts[0][2]))]
    sort_keys = []                                              # most significant first
    for (j, desc) in keys:
        c = cols[j]
        if c.ndim == 2:                                         # a string column: one key per byte
            b = c.astype(np.int16)
            sort_keys += [(255 - b[:, k]) if desc else b[:, k] for k in range(b.shape[1])]
        else:
            v = c.astype(np.int64)
            sort_keys.append(-v if desc else v)
    perm = np.lexsort(tuple([row, seg] + sort_keys[::-1]))
    if limit > 0:
        perm = perm[:limit]
    return seg[perm], row[perm], [c[perm] for c in cols]


class ProjectOp(ProjectionOperator):
    """Project.scala:17: ProjectOp(cols, op, limit = 0).  order_by -- entries (col, descending) over `cols`, most significant first -- is
    the sort the reference announces and does not have (Query.scala:27): the rows come back in that order, sorted on the device
    (imm3_query_set_order), and `limit` is applied after it."""

    def __init__(self, cols: Sequence[str], op: ColumnVectorOperator, limit: int = 0, order_by=()):
        self.cols, self.op, self.limit = list(cols), op, limit
        self.order_by = tuple(order_by)
        self.order_keys = order_keys(self.cols, self.order_by)   # (ValueError: a key outside the SELECT list)

    @staticmethod
    def mkProjectOp(cols: Sequence[str], limit: int = 0, order_by=()):       # Project.scala:8-15
        return lambda op: ProjectOp(cols, op, limit, order_by)

    def _fused(self):
        if isinstance(self.op, ScanOp):
            return self.op, []
        if isinstance(self.op, (SelectOp, SelectTreeOp)):
            return self.op._chain()
        return None

    def _open(self) -> "native.DeviceQuery":
        """The fused query of this pipeline, created, ordered when there are keys, and run; the caller fetches and closes it."""
        scan, leaves = self._fused()
        for (_, cond) in leaves:
            if not isinstance(cond, SUPPORTED_CONDS):
                raise Exception(f"Unsupported condition: {cond}")
        q = scan._query(leaves, self.cols, 0 if self.order_keys else self.limit, _expr_of(self.op))
        try:
            if self.order_keys:
                q.set_order(self.order_keys, self.limit)           # (the limit is applied behind the order: no creation-time limit)
            q.run()
        except Exception:
            q.close()
            raise
        return q

    @staticmethod
    def _typed(cols, codecs):
        """raw column bytes (uint8[n, width]) -> int32 / int8 arrays for the int codecs, strings as they are"""
        out = []
        for raw, codec in zip(cols, codecs):
            if codec in native.INT_CODECS:
                out.append(raw.reshape(-1).view("<i4"))
            elif codec in native.TINYINT_CODECS:
                out.append(raw.reshape(-1).view(np.int8))
            else:
                out.append(raw)
        return out

    def run_columns(self):
        """Fused execution; returns (row_index uint32[n], [typed numpy array per SELECT-list column])."""
        q = self._open()
        idx, cols = q.fetch_rows()
        out = self._typed(cols, q.proj_codecs)
        q.close()
        return idx, out

    def iterator(self) -> Iterator[Row]:
        if self._fused() is None:
            return self._host_iterator()
        _, cols = self.run_columns()
        return _rows_from_columns(cols)

    def _host_iterator(self) -> Iterator[Row]:
        """ProjectIterator over batches from a non-fusable upstream (e.g. a queue of batches from several
        segments, Engine.scala:190-191).  Row materialisation is Project.scala:50-63; batches without
        survivors are skipped (the reference faults on them)."""
        if self.order_keys:
            yield from self._host_ordered()
            return
        total = 0
        for vec in self.op.iterator():
            names = [c.name for c in vec.columns]
            vec_cols = [names.index(c) for c in self.cols]
            for pos in vec.selected.toList():
                if self.limit > 0 and total >= self.limit:
                    return
                yield Row(*[_value(vec.columnVectors[j].data[pos]) for j in vec_cols])
                total += 1
            if self.limit > 0 and total >= self.limit:
                return


    def _host_ordered(self) -> Iterator[Row]:
        """the same over a non-fusable upstream with an order: every row, then a stable sort by the keys"""
        rows = []
        for vec in self.op.iterator():
            names = [c.name for c in vec.columns]
            vec_cols = [names.index(c) for c in self.cols]
            for pos in vec.selected.toList():
                rows.append([vec.columnVectors[j].data[pos] for j in vec_cols])     # (raw: a string's bytes order it, not its decoding)
        rows = _stable_by_keys(rows, self.order_keys)
        for r in rows[: self.limit] if self.limit > 0 else rows:
            yield Row(*[_value(x) for x in r])


def _stable_by_keys(rows, keys):
    """rows (lists of raw values: numpy ints, uint8 arrays for strings) in (keys, arrival) order: ints compare as signed integers,
    strings byte-wise unsigned"""
    import functools

    def val(v):
        return bytes(v) if isinstance(v, np.ndarray) else int(v)

    def cmp(a, b):
        for (j, desc) in keys:
            x, y = val(a[1][j]), val(b[1][j])
            if x != y:
                return (1 if x < y else -1) if desc else (-1 if x < y else 1)
        return a[0] - b[0]
    return [r for (_, r) in sorted(enumerate(rows), key=functools.cmp_to_key(cmp))]


# ------------------------------------------------------------------------------------------
# aggregation (engine/.../operator/ProjectAggregate.scala, ProjectAggregateQueue.scala)
# ------------------------------------------------------------------------------------------
def java_double_to_string(v: float) -> str:
    """Double.toString for the integral values Max/MinDoubleAggr hold (value.toDouble of an Int / Byte)."""
    iv = int(v)
    if abs(iv) < 10 ** 7:
        return f"{iv}.0"
    digits = str(abs(iv))
    return ("-" if iv < 0 else "") + digits[0] + "." + (digits[1:].rstrip("0") or "0") + "E" + str(len(digits) - 1)


class Aggregator:                    # ProjectAggregate.scala:11-20
    kind = native.AGG_COUNT

    def __init__(self, col: str, alias: str):
        self.col, self.alias = col, alias

    def make(self):
        return type(self)(self.col, self.alias)


class CountAggr(Aggregator):         # :22-35
    kind = native.AGG_COUNT

    def __init__(self, col, alias):
        super().__init__(col, alias)
        self.counter = 0

    def set(self, n):
        self.counter = n

    def get(self):
        return self.counter

    def combine(self, other):
        self.counter += other.get()
        return self

    def repr(self):
        return str(self.counter)


class MaxDoubleAggr(Aggregator):     # :37-48
    kind = native.AGG_MAX

    def __init__(self, col, alias):
        super().__init__(col, alias)
        self.value = -1.7976931348623157e308

    def add(self, v):
        if v > self.value:
            self.value = float(v)

    def get(self):
        return self.value

    def combine(self, other):
        self.add(other.get())
        return self

    def repr(self):
        return java_double_to_string(self.value)


class MinDoubleAggr(MaxDoubleAggr):  # :50-61
    kind = native.AGG_MIN

    def __init__(self, col, alias):
        Aggregator.__init__(self, col, alias)
        self.value = 1.7976931348623157e308

    def add(self, v):
        if v < self.value:
            self.value = float(v)


class AvgDoubleAggr(Aggregator):     # :60-75
    """State (sum, counter).  The reference's sum is a BigDecimal built from Double.toString of each value.toDouble of an Int /
    Byte: an integer with scale 1, kept here as the exact int (the GPU's int64 SUM).  repr() is java.math.BigDecimal's
    divide(counter, MathContext.DECIMAL128) -- 34 digits, HALF_EVEN, an exact quotient at the preferred scale 1 -- and its
    toString (E-notation below an adjusted exponent of -6): Python's decimal implements the same arithmetic."""
    kind = native.AGG_SUM
    _DECIMAL128 = decimal.Context(prec=34, rounding=decimal.ROUND_HALF_EVEN)

    def __init__(self, col, alias):
        super().__init__(col, alias)
        self.sum = 0
        self.counter = 0

    def add(self, v):
        if float(v) != int(v):
            raise ValueError(f"AvgDoubleAggr sums integral values (value.toDouble of an Int / Byte), got {v!r}")
        self.sum += int(v)
        self.counter += 1

    def get(self):
        return (self.sum, self.counter)

    def combine(self, other):
        s, c = other.get()
        self.sum += s
        self.counter += c
        return self

    def repr(self):
        return str(self._DECIMAL128.divide(decimal.Decimal(f"{self.sum}.0"), decimal.Decimal(self.counter)))


COUNT_DISTINCT_ONE_QUERY = "count(distinct) runs as one table query only"


class CountDistinctAggr(Aggregator):
    """count(distinct col): the number of distinct values of col among the group's selected rows (IMM3_AGG_COUNT_DISTINCT; not in the
    reference).  The figure is exact because ONE query counts it over a set on the device; two figures do not add, so combine()
    raises -- OUT OF SCOPE: a getter for the sets themselves, and with it the engines' per-segment fallback."""
    kind = native.AGG_COUNT_DISTINCT

    def __init__(self, col, alias):
        super().__init__(col, alias)
        self.counter = 0

    def set(self, n):
        self.counter = int(n)

    def get(self):
        return self.counter

    def combine(self, other):
        raise Exception(COUNT_DISTINCT_ONE_QUERY + f": {self.alias!r} of two queries cannot be combined (counts of distinct values do not add)")

    def repr(self):
        return str(self.counter)


def count_distinct_route(has_count_distinct: bool, table_query: bool, owned_segments: int, device_merge: bool, n_contexts: int) -> str:
    """How Engine.execute_agg answers a statement: "table" (ONE table query: exact over all segments, HAVING / ORDER BY / LIMIT on the
    device), "segment" (the table's single owned segment as that segment's query) or "merge" (per-segment queries whose groups are
    combined -- what a statement without count(distinct) may always do).  A statement WITH one that would have to combine several
    queries' groups raises: table_query is False (no table could be built, or it refused the statement) and the segments are several,
    or merge on the device, or live on several contexts.  Decided from these facts alone: no device is asked."""
    if table_query:
        return "table"
    if not has_count_distinct:
        return "merge"
    if device_merge:
        raise Exception(COUNT_DISTINCT_ONE_QUERY + ": device_merge combines per-segment queries, and counts of distinct values do not add")
    if owned_segments > 1 and n_contexts > 1:
        raise Exception(COUNT_DISTINCT_ONE_QUERY + f": the {owned_segments} segments live on {n_contexts} contexts")
    if owned_segments > 1:
        raise Exception(COUNT_DISTINCT_ONE_QUERY + f": this rank owns {owned_segments} segments of a table it cannot run as one query")
    return "segment"


class MaxStringAggr(Aggregator):     # :79-91
    kind = native.AGG_MAX

    def __init__(self, col, alias):
        super().__init__(col, alias)
        self.value = ""

    def add(self, v):
        if self.value == "" or v > self.value:
            self.value = v

    def get(self):
        return self.value

    def combine(self, other):
        self.add(other.get())
        return self

    def repr(self):
        return self.value


def resolveProjectOp(projectAgg: ProjectAgg, table: Table):
    """Engine.resolveProjectOp (Engine.scala:130-156): Aggregate ADT -> Aggregators, default aliases
    col_max / col_min / col_count; Min over a STRING column becomes MaxStringAggr (the reference's own mapping,
    :145); Sum / Avg parse but are rejected (:152)."""
    aggs = []
    for a in projectAgg.aggs:
        if isinstance(a, Max):
            ct = table.getColumn(a.col).columnType
            aggs.append((MaxStringAggr if ct == "STRING" else MaxDoubleAggr)(a.col, a.alias or a.col + "_max"))
        elif isinstance(a, Min):
            ct = table.getColumn(a.col).columnType
            aggs.append((MaxStringAggr if ct == "STRING" else MinDoubleAggr)(a.col, a.alias or a.col + "_min"))
        elif isinstance(a, Count):
            aggs.append(CountAggr(a.col, a.alias or a.col + "_count"))
        elif isinstance(a, CountDistinct):
            aggs.append(CountDistinctAggr(a.col, a.alias or a.col + "_distinct"))
        else:
            raise Exception("Unknown Aggregate type")
    return lambda op: ProjectAggOp(aggs, op, list(projectAgg.groupBy), getattr(projectAgg, "order_by", ()), getattr(projectAgg, "limit", 0),
                                   getattr(projectAgg, "having", None))


def group_order_spec(aggs: Sequence[Aggregator], groupBy: Sequence[str], order_by):
    """ORDER BY entries (name, descending) over an aggregation's group-by columns and aliases -> [(is_agg, name, descending)].  A name
    that is neither raises ValueError naming it; so does an AvgDoubleAggr's alias (ordering by a quotient is out of scope)."""
    by_alias = {a.alias: a for a in aggs}
    out = []
    for (name, desc) in order_by:
        if name in groupBy:
            out.append((False, name, bool(desc)))
        elif name in by_alias:
            if isinstance(by_alias[name], AvgDoubleAggr):
                raise ValueError(f"order by {name!r}: ordering by an average is not supported")
            out.append((True, name, bool(desc)))
        else:
            raise ValueError(f"order by {name!r} is neither a group-by column {list(groupBy)} nor an aggregate's alias {list(by_alias)}")
    return out


class _Alias:
    """what group_filter_leaves reads of an aggregate: its alias (Aggregators carry theirs)"""

    def __init__(self, alias):
        self.alias, self.col = alias, alias


def group_filter_spec(aggs: Sequence[Aggregator], groupBy: Sequence[str], having):
    """A HAVING tree over the aggregators' aliases -> ([(alias, average, native cond, int threshold)], postfix program over the leaf
    indices with native.EXPR_AND / EXPR_OR): what filter_groups evaluates on the host and imm3_query_set_group_filter on the device.
    An AvgDoubleAggr's alias becomes an `average` leaf on its SUM.  ValueError (query.group_filter_leaves's causes, and): a
    MaxStringAggr's alias -- string maxima are not compared --, an average's threshold outside [-2^31, 2^31 - 1]."""
    by_alias = {a.alias: a for a in aggs}
    named, prog = group_filter_leaves([_Alias(a) for a in by_alias], groupBy, having)
    leaves = []
    for (alias, cond, value) in named:
        a = by_alias[alias]
        if isinstance(a, MaxStringAggr):
            raise ValueError(f"having {alias!r}: a string MAX is not compared by having")
        average = isinstance(a, AvgDoubleAggr)
        if average and not -2 ** 31 <= value <= 2 ** 31 - 1:
            raise ValueError(f"having {alias!r}: an average's threshold must lie in [-2^31, 2^31 - 1], got {value}")
        leaves.append((alias, average, {GT: native.GT, LT: native.LT, EQ: native.EQ}[cond], value))
    return leaves, [native.EXPR_AND if op == "and" else native.EXPR_OR if op == "or" else op for op in prog]


def group_filter_leaf(aggmap: dict, leaf) -> bool:
    """one leaf on one merged group, in exact integers: a count, the integral value of a Max / MinDoubleAggr, or -- an average --
    sum <cond> threshold * count (the device's rule: include/imm3.h, imm3_query_set_group_filter)"""
    alias, average, cond, value = leaf
    a = aggmap[alias]
    if isinstance(a, AvgDoubleAggr):
        lhs, rhs = int(a.sum), int(value) * int(a.counter)
    elif isinstance(a, (CountAggr, CountDistinctAggr)):
        lhs, rhs = int(a.get()), int(value)
    else:
        lhs, rhs = int(a.get()), int(value)
    return lhs > rhs if cond == native.GT else (lhs < rhs if cond == native.LT else lhs == rhs)


def filter_groups(result: Dict[str, dict], leaves, prog) -> Dict[str, dict]:
    """The host's HAVING over MERGED groups (the per-segment fallback and device_merge; the C++ mirror: host/operators.hpp
    filterGroups): the groups of `result` the program keeps, in their order.  leaves / prog: group_filter_spec's; no program: every group."""
    if not prog:
        return result
    out = {}
    for key, aggmap in result.items():
        stack = []
        for op in prog:
            if op >= 0:
                stack.append(group_filter_leaf(aggmap, leaves[op]))
            elif op == native.EXPR_NOT:
                stack.append(not stack.pop())
            else:
                y, x = stack.pop(), stack.pop()
                stack.append((x and y) if op == native.EXPR_AND else (x or y))
        if stack[-1]:
            out[key] = aggmap
    return out


def _order_bytes(v: int, nbytes: int, bias: int) -> bytes:
    return (int(v) + bias).to_bytes(nbytes, "big")


def order_groups(result: Dict[str, dict], raw_keys: Dict[str, Sequence[bytes]], group_cols: Sequence[Column], spec, limit: int = 0) -> Dict[str, dict]:
    """The host's ORDER BY over MERGED groups (the per-segment fallback and device_merge; the C++ mirror: host/operators.hpp
    orderGroups): `result` is key -> {alias: Aggregator} in merged first-arrival order, raw_keys[key] the raw bytes of the key's parts
    in the order of group_cols, spec group_order_spec's.  The normal form is the device's (include/imm3.h): signed integers biased to
    unsigned, big-endian; counts and sums as integers; strings byte-wise; a descending key complemented; ties -- all keys equal --
    in arrival order.  Cut to `limit` > 0.  Returns a new dict that iterates in the order asked for."""
    names = [c.name for c in group_cols]
    normal = []
    for arrival, (key, aggmap) in enumerate(result.items()):
        parts = []
        for (is_agg, name, desc) in spec:
            if not is_agg:
                col, raw = group_cols[names.index(name)], bytes(raw_keys[key][names.index(name)])
                if col.codec in CodecType.INT_CODECS or col.codec in CodecType.TINYINT_CODECS:
                    b = _order_bytes(int.from_bytes(raw, "little", signed=True), 8, 1 << 63)
                else:
                    b = raw
            else:
                a = aggmap[name]
                if isinstance(a, (CountAggr, CountDistinctAggr)):
                    b = _order_bytes(a.get(), 16, 0)
                elif isinstance(a, MaxStringAggr):
                    b = a.get().encode("utf-8")     # (new String(bytes) of the value: the bytes again for ASCII)
                else:                                   # Max / MinDoubleAggr: the integral value of an Int / Byte column
                    b = _order_bytes(int(a.get()), 16, 1 << 127)
            parts.append(bytes(255 - x for x in b) if desc else b)
        normal.append((tuple(parts), arrival, key))
    normal.sort(key=lambda t: (t[0], t[1]))
    if limit > 0:
        normal = normal[:limit]
    return {key: result[key] for (_, _, key) in normal}


class ProjectAggOp(Operator):
    """ProjectAggOp(aggs, op, groupBy) (ProjectAggregate.scala:125): yields (groupKey, {alias: Aggregator}) in
    first-seen order.  The whole chain of one segment runs fused on the GPU: scan+select kernel, then the LDS
    hash-aggregation kernel; group keys and aggregates come back already reduced."""

    def __init__(self, aggs: Sequence[Aggregator], op: ColumnVectorOperator, groupBy: Sequence[str], order_by=(), limit: int = 0, having=None):
        """having -- And / Or over Select(alias, GT | LT | EQ) -- keeps groups BEFORE the order and the limit: on the device when ONE
        query answers (imm3_query_set_group_filter), on the merged groups otherwise (filter_groups).
        order_by -- entries (name, descending) over the group-by columns and the aggregates' aliases -- and limit are applied by the
        device when ONE query answers (a table query: _run(ordered=True)); per-segment results are ordered after their merge
        (order_groups).  raw_keys: group key -> the raw bytes of its parts, for every group this operator has yielded."""
        self.aggs, self.op, self.groupBy = list(aggs), op, list(groupBy)
        self.order_by = tuple((str(c), bool(d)) for (c, d) in order_by)
        self.limit = int(limit)
        self.order_spec = group_order_spec(self.aggs, self.groupBy, self.order_by)   # (ValueError: an unknown name, an average)
        self.having = having
        self.filter_leaves, self.filter_prog = group_filter_spec(self.aggs, self.groupBy, having)   # (ValueError: see group_filter_spec)
        self.raw_keys: Dict[str, list] = {}

    @staticmethod
    def make(aggs, groupBy):           # ProjectAggregate.scala:116-122
        return lambda op: ProjectAggOp(aggs, op, groupBy)

    def _segment_args(self):
        """_run's arguments for this operator's own segment"""
        if isinstance(self.op, ScanOp):
            scan, leaves = self.op, []
        else:
            scan, leaves = self.op._chain()
        for (_, cond) in leaves:
            if not isinstance(cond, SUPPORTED_CONDS):
                raise Exception(f"Unsupported condition: {cond}")
        colnames = [c.name for c in scan.cols]
        # groupCols filters the BATCH columns by membership in groupBy (:135-140): batch-column order
        group_idx = [i for i, n in enumerate(colnames) if n in self.groupBy]
        by_alias = {}
        for a in self.aggs:              # aggsMap is a HashMap keyed by alias: a later duplicate replaces an earlier one
            by_alias[a.alias] = a
        aggs = list(by_alias.values())
        t = scan._table()
        sels = []
        for (col, cond) in leaves:
            code, operand = _cond_spec(cond, scan.cols[colnames.index(col)].width)
            sels.append((colnames.index(col), code, operand))
        seg = scan.sm.device_segment(scan.tableName, scan.segIdx)
        return seg, scan.cols, scan._used_indices(), sels, t.blockSize, _expr_of(self.op)

    def iterator(self):
        yield from self._run(*self._segment_args())

    def _shape(self, cols):
        """(column names, group column indices, aggregators, group widths, key wider than 8 bytes, indices of the MaxStringAggr
        over a column wider than 8 bytes) of this operator over the batch columns `cols`"""
        colnames = [c.name for c in cols]
        group_idx = [i for i, n in enumerate(colnames) if n in self.groupBy]
        by_alias = {}
        for a in self.aggs:
            by_alias[a.alias] = a
        aggs = list(by_alias.values())
        widths = [cols[i].width for i in group_idx]
        wide_strs = [j for j, a in enumerate(aggs)
                     if a.kind == native.AGG_MAX and cols[colnames.index(a.col)].columnType == "STRING" and cols[colnames.index(a.col)].width > 8]
        return colnames, group_idx, aggs, widths, sum(widths) > 8, wide_strs

    def _open(self, seg, cols, used_idx, sels, block_size, expr=None) -> native.DeviceQuery:
        """The aggregation query over seg, run and left open (the caller fetches or merges its groups, then closes it)."""
        colnames, group_idx, aggs, _, wide_key, _ = self._shape(list(cols))
        q = native.DeviceQuery(seg.ctx, seg, used_idx, sels, (), 0, block_size,
                               group_cols=group_idx, aggs=[(a.kind, colnames.index(a.col)) for a in aggs],
                               wide_keys=wide_key, expr=expr)   # a key wider than 8 bytes: the _wide entry points, the key bytes from the device
        q.run()
        return q

    def _native_order(self, cols):
        """order_spec as imm3_query_set_group_order's keys: places in the native group_cols / aggs lists of _open"""
        colnames, group_idx, aggs, _, _, _ = self._shape(list(cols))
        gnames = [colnames[i] for i in group_idx]
        aliases = [a.alias for a in aggs]
        return [(native.GROUP_ORDER_AGG, aliases.index(name), desc) if is_agg else (native.GROUP_ORDER_GROUP_COL, gnames.index(name), desc)
                for (is_agg, name, desc) in self.order_spec]

    def _order_key_bytes(self, cols) -> int:
        """the bytes order_spec's keys take in the device's normal form (include/imm3.h: imm3_query_set_group_order): a group column its
        width, COUNT 5, SUM 8, MIN / MAX its column's width"""
        by_name = {c.name: c for c in cols}
        by_alias = {a.alias: a for a in self._shape(list(cols))[2]}
        total = 0
        for (is_agg, name, _) in self.order_spec:
            if not is_agg:
                total += by_name[name].width
            else:
                a = by_alias[name]
                total += 5 if a.kind == native.AGG_COUNT else 8 if a.kind in (native.AGG_SUM, native.AGG_COUNT_DISTINCT) else by_name[a.col].width
        return total

    def _native_filter(self, cols):
        """filter_leaves as imm3_query_set_group_filter's leaves: places in the native aggs list of _open"""
        aliases = [a.alias for a in self._shape(list(cols))[2]]
        return [(aliases.index(alias), average, cond, value) for (alias, average, cond, value) in self.filter_leaves]

    def _run(self, seg, cols, used_idx, sels, block_size, expr=None, ordered=False):
        """seg: a DeviceSegment or a DeviceTable (then the groups are already merged across segments).  ordered: this query's groups are
        the whole answer -- the device orders them and cuts them to the limit (imm3_query_set_group_order)."""
        _, _, _, _, wide_key, wide_strs = self._shape(list(cols))
        q = self._open(seg, cols, used_idx, sels, block_size, expr)
        if ordered and self.filter_prog:                      # filter, then order, then limit
            q.set_group_filter(self._native_filter(cols), self.filter_prog)
        if ordered and self.order_spec:
            q.set_group_order(self._native_order(cols), self.limit)
        keys, first, counts, vals = q.fetch_groups()
        key_bytes = q.fetch_group_keys() if wide_key else None
        # a MaxStringAggr over a column wider than 8 bytes: vals hold its first 8 bytes, the exact value comes from the device
        wide = {j: q.fetch_group_strings(j) for j in wide_strs}
        q.close()
        yield from self._groups(cols, keys, key_bytes, counts, vals, wide)

    def _groups(self, cols, keys, key_bytes, counts, vals, wide):
        """(groupKey, {alias: Aggregator}) per group of the fetched (or merged) arrays: keys uint64[g] or, when key_bytes is given,
        the packed key bytes uint8[g, key width]; wide: {j: uint8[g, width]} for the string maxima wider than 8 bytes."""
        colnames, group_idx, aggs, widths, _, _ = self._shape(list(cols))

        class _S:                             # the per-row decoding below only needs `cols`
            pass
        scan = _S()
        scan.cols = list(cols)
        for g in range(counts.shape[0]):
            raw = bytes(key_bytes[g]) if key_bytes is not None else int(keys[g]).to_bytes(8, "little")
            parts, off = [], 0
            raw_parts = []
            for i, w in zip(group_idx, widths):
                parts.append(_key_part(scan.cols[i], raw[off: off + w]))
                raw_parts.append(raw[off: off + w])
                off += w
            self.raw_keys.setdefault("_".join(parts), raw_parts)
            out = {}
            for j, a in enumerate(aggs):
                na = a.make()
                if isinstance(na, CountAggr):
                    na.set(int(counts[g]))
                elif isinstance(na, CountDistinctAggr):   # the pair set's figure, an int64 in the value column
                    na.set(int(vals[g, j]))
                elif isinstance(na, AvgDoubleAggr):  # the group's exact sum; every selected row added once to the counter
                    na.sum, na.counter = int(vals[g, j]), int(counts[g])
                elif isinstance(na, MaxStringAggr) and j in wide:
                    na.value = _value(wide[j][g])     # new String(bytes)
                elif isinstance(na, MaxStringAggr):
                    w = scan.cols[colnames.index(a.col)].width
                    na.value = int(vals[g, j]).to_bytes(8, "big", signed=True)[8 - w:].decode("utf-8", errors="replace")
                else:
                    na.value = float(int(vals[g, j]))
                out[a.alias] = na
            yield "_".join(parts), out


def _key_part(col: Column, raw: bytes) -> str:
    if col.codec in CodecType.INT_CODECS:
        return str(int.from_bytes(raw, "little", signed=True))
    if col.codec in CodecType.TINYINT_CODECS:
        return str(int.from_bytes(raw, "little", signed=True))
    return raw.decode("utf-8", errors="replace")


def _value(x):
    if isinstance(x, np.ndarray):           # fixed-width string: new String(bytes) (DataType.scala:70)
        return bytes(x).decode("utf-8", errors="replace")
    return int(x)


def _rows_from_columns(cols: List[np.ndarray]) -> Iterator[Row]:
    n = cols[0].shape[0] if cols else 0
    for i in range(n):
        yield Row(*[_value(c[i]) for c in cols])


# ------------------------------------------------------------------------------------------
# Engine (the caller of the hot path; only what the path needs: planning + per-segment fan-out)
# ------------------------------------------------------------------------------------------
def _column_hash(c: Column) -> int:
    from . import scala_sets
    codec_id = CodecType.id_of(c.codec)
    return scala_sets.product_hash([scala_sets.java_string_hash(c.name), scala_sets.COLUMN_TYPE_ID[c.columnType], codec_id,
                                    scala_sets.map_hash(dict(c.dtypeAttrs))])


def getColumns(query: Query, table: Table) -> List[Column]:
    """Engine.getColumns (Engine.scala:85-106): (rec(query.select).toList ++ projectColumns).toSet.toList.
    Scala's Set1..Set4 keep insertion order, so for <= 4 distinct columns the order is first-seen order
    (SURVEY A.1 rule 3).  From the fifth distinct column on the set is an immutable.HashSet and the order is its hash
    trie's: restated in scala_sets.py (scala-library 2.12.11; unpinned at the reference boundary, pinned against the
    library's well-known Set(1 to 10) order).  The first column of the result defines the batches (Scan.scala:55); for
    aggregations the order also decides how the group key is joined (ProjectAggregate.scala:135-156)."""
    from .scala_sets import ScalaSet

    def rec(sel: SelectADT) -> ScalaSet:
        out = ScalaSet()
        if isinstance(sel, (And, Or)):                 # rec(a) ++ rec(b): b's elements, in b's order, added to a
            out = rec(sel.op1)
            for c in rec(sel.op2).to_list():
                out.add(c, _column_hash(c))
        elif isinstance(sel, Select):
            c = table.getColumn(sel.col)
            out.add(c, _column_hash(c))
        return out

    cols = ScalaSet()
    for c in rec(query.select).to_list():
        cols.add(c, _column_hash(c))
    if isinstance(query.project, Project):
        names = list(query.project.cols)
    else:                                              # ProjectAgg: aggsCols ++ groupCols (Engine.scala:96-100)
        names = [a.col for a in query.project.aggs] + list(query.project.groupBy)
    for name in names:
        c = table.getColumn(name)
        cols.add(c, _column_hash(c))
    return cols.to_list()


def resolveSelectOps(query: Query) -> List[Callable[[ColumnVectorOperator], ColumnVectorOperator]]:
    """Engine.resolveSelectOps + PipelineThread.runOps (Engine.scala:108-128, 237-245) flattened: the PTree is
    folded left-to-right, PNode(n1, n2, _) => rec(n2) o rec(n1), and the AND/OR tag is ignored."""
    def rec(sel: SelectADT):
        if isinstance(sel, (And, Or)):
            return rec(sel.op1) + rec(sel.op2)
        if isinstance(sel, Select):
            return [SelectOp.mkSelectOp(sel.col, sel.cond)]
        return []                                             # NoSelect => identity
    return rec(query.select)


class Engine:
    """Engine.execute (Engine.scala:158-197) for Project queries.  One fused pipeline per segment (the
    reference: one PipelineThread per segment, :176-180); output order across segments is unspecified in
    the reference (queue interleaving, :255) and defined here as ascending segment index."""

    def __init__(self, sm: GpuSegmentManager, honour_and_or: bool = False, device_merge: bool = False, honour_not_match: bool = False):
        """honour_and_or: a query whose select tree holds an Or runs it as a disjunction (one table launch when the table takes the
        tree, else SelectTreeOp per segment) instead of the reference's conjunction.  Off (the default) nothing changes; a tree without Or is the same either way.
        device_merge: the per-segment branches merge on the GPU instead of on the host -- execute_agg its queries' groups (one
        imm3_comm_merge_groups_wide over a one-rank communicator per context) instead of combining dicts, an ORDER BY statement its
        per-segment ordered rows (one imm3_comm_merge_ordered) instead of operators.merge_ordered's lexsort; the results are the
        same.  Off (the default) nothing changes.
        honour_not_match: a query whose select tree holds a NotMatch leaf -- which the reference's SelectOp throws on -- runs as a
        tree, whether or not it has an Or: the leaf is the complement of its Match (IMM3_EXPR_NOT), and the And / Or tags of THAT
        query are then honoured too, whatever honour_and_or says (a complement under a conjunction-for-everything has no meaning
        to preserve).  Off (the default) nothing changes: a NotMatch leaf raises "Unsupported condition", as in the reference."""
        self.sm = sm
        self.honour_and_or = honour_and_or
        self.device_merge = device_merge
        self.honour_not_match = honour_not_match
        # who applied having / order by / limit to the groups of the last device merge: "device" (imm3_comm_merge_groups_view), "host"
        # (the library refused the view: plain merge, ordered here), None (no such clause, or no device merge yet)
        self.last_merge_view = None
        # how the sub-queries (IntInQuery) of the last statement ran, outermost first: "set/table" (one table query was the set's source),
        # "set/segments" (per-segment queries were), "host" (several contexts: the inner values fetched, an IntIn leaf instead)
        self.last_subquery_paths: List[str] = []

    def lastPath(self) -> str:
        """which route the last statement's sub-queries took (`--explain`): the paths joined by ",", "" for a statement without one"""
        return ",".join(self.last_subquery_paths)

    def resolve_subqueries(self, query: Query) -> Query:
        """The statement with every IntInQuery leaf replaced by what it resolves to: the inner query's selects run (one table query
        where _table_plan takes them, else per-segment queries), ALL of them become the sources of one native.IntSet, and the leaf
        becomes IntInSet(that set) -- so the outer statement takes whichever plan it would take with an IntIn.  A segment manager
        with more than one context cannot share a set: the inner values are fetched and the leaf becomes an IntIn."""
        def holds(sel, kind):
            if isinstance(sel, (And, Or)):
                return holds(sel.op1, kind) or holds(sel.op2, kind)
            return isinstance(sel, Select) and isinstance(sel.cond, kind)
        if not holds(query.select, IntInQuery):
            if not holds(query.select, IntInSet):              # (a statement resolved already keeps what its resolution recorded)
                self.last_subquery_paths = []
            return query
        self.last_subquery_paths = []
        return Query(query.table, self._resolve_select(query.select), query.project)

    def _resolve_select(self, sel: SelectADT) -> SelectADT:
        if isinstance(sel, (And, Or)):
            return type(sel)(self._resolve_select(sel.op1), self._resolve_select(sel.op2))
        if isinstance(sel, Select) and isinstance(sel.cond, IntInQuery):
            return Select(sel.col, self._resolve_inner(sel.cond.query))
        return sel

    def _resolve_inner(self, inner: Query) -> SelectCondition:
        at = len(self.last_subquery_paths)
        self.last_subquery_paths.append("")
        inner = Query(inner.table, self._resolve_select(inner.select), inner.project)   # (sub-queries of the sub-query first)
        table = self.sm.getTable(inner.table)
        col = table.getColumn(inner.project.cols[0])
        if not (col.codec in CodecType.INT_CODECS or col.codec in CodecType.TINYINT_CODECS):
            raise Exception(f"IntInQuery: the inner column {col.name!r} is neither int32 nor int8 (Unsupported column vector)")
        if len(self.sm.ctxs) > 1:
            self.last_subquery_paths[at] = "host"
            parts = [cols[0] for (_, _, cols) in self._columns(inner)]   # (resolved above: not through resolve_subqueries again)
            vals = np.unique(np.concatenate(parts).astype(np.int64)) if parts else np.zeros(0, np.int64)
            return IntIn([int(v) for v in vals])
        sources, opened = [], []
        try:
            plan = self._table_plan(inner)
            if plan is not None:
                dt, used, used_idx, sels, prog = plan
                try:
                    q = native.DeviceQuery(dt.ctx, dt, used_idx, sels, [], 0, table.blockSize, expr=prog)
                    opened.append(q)
                    sources.append((q, [c.name for c in used].index(col.name)))
                    self.last_subquery_paths[at] = "set/table"
                except native.Imm3Error as e:
                    if not self._table_tree_refused(e, prog):
                        raise
            if not sources:
                self.last_subquery_paths[at] = "set/segments"
                for _, proj in self.pipelines(inner):
                    fused = proj._fused()
                    if fused is None:
                        raise Exception("IntInQuery: the inner query must be a fused scan / select pipeline")
                    scan, leaves = fused
                    for (_, cond) in leaves:
                        if not isinstance(cond, SUPPORTED_CONDS):
                            raise Exception(f"Unsupported condition: {cond}")
                    q = scan._query(leaves, (), 0, _expr_of(proj.op))
                    opened.append(q)
                    sources.append((q, [c.name for c in scan.cols].index(col.name)))
            if not sources:                                    # no segment at all: the empty list
                return IntIn([])
            return IntInSet(native.IntSet(self.sm.ctxs[0], sources))   # (runs every source's select chain: none has run yet)
        finally:
            for q in opened:                                   # sources are not retained
                q.close()

    def _not_tree(self, query: Query) -> bool:
        return self.honour_not_match and has_not_match(query.select)

    def _as_tree(self, query: Query) -> bool:
        return (self.honour_and_or and has_or(query.select)) or self._not_tree(query)

    def _select_ops(self, query: Query):
        """the operators between ScanOp and the projection: the reference's SelectOp chain, or one SelectTreeOp"""
        return [SelectTreeOp.mkSelectTreeOp(query.select, self._not_tree(query))] if self._as_tree(query) else resolveSelectOps(query)

    def pipelines(self, query: Query):
        table = self.sm.getTable(query.table)
        used = getColumns(query, table)
        leaves = self._select_ops(query)
        mk_scan = ScanOp.mkScanOp(self.sm, query.table)
        mk_proj = ProjectOp.mkProjectOp(list(query.project.cols), query.project.limit, getattr(query.project, "order_by", ()))
        for segIdx in range(self.sm.getTableSegmentCount(table.name)):
            if not self.sm.owns(table.name, segIdx):
                continue
            op: ColumnVectorOperator = mk_scan(used, segIdx)
            for leaf in leaves:
                op = leaf(op)
            yield segIdx, mk_proj(op)

    def _table_plan(self, query: Query):
        """(DeviceTable, used columns, their table indices, select specs, program) when the whole table can run as ONE fused launch,
        else None.  program: None for the reference's conjunction; for a tree with an Or under honour_and_or, or with a NotMatch under honour_not_match, the postfix program over
        the select specs (imm3_query_create_table_expr), which the library may still refuse (ERR_ARG: _table_tree_refused)."""
        table = self.sm.getTable(query.table)
        dt = self.sm.device_table(query.table)
        if dt is None:
            return None
        used = getColumns(query, table)
        names = [c.name for c in used]
        if self._as_tree(query):
            leaves, prog = select_program(query.select, self._not_tree(query))
        else:
            leaves, prog = [(op.col, op.cond) for op in (leaf(None) for leaf in resolveSelectOps(query))], None
        sels = []
        for (name, cond) in leaves:
            if not isinstance(cond, SUPPORTED_CONDS):
                raise Exception(f"Unsupported condition: {cond}")
            col = used[names.index(name)]
            code, operand = _cond_spec(cond, col.width)
            if code == native.STR_RANGE:
                # a table takes a range on a string column whose width is a multiple of 4, in a flat select list only
                if not (col.codec in CodecType.STRING_CODECS and prog is None and col.width % 4 == 0 and 4 <= col.width <= 256):
                    return None
            if code == native.MATCH:
                # the tile kernels take 2-byte strings with <= 8 IN-list values; a flat select list also takes any non-empty
                # IN-list on a string column whose width is a multiple of 4 (k_filter_str_rows); a tree keeps the tile kinds
                is_str = col.codec in CodecType.STRING_CODECS
                tile = is_str and col.width == 2 and 0 < len(operand) <= 8
                rows = is_str and prog is None and col.width % 4 == 0 and 4 <= col.width <= 256 and len(operand) > 0
                if not (tile or rows):
                    return None
            sels.append((names.index(name), code, operand))
        tnames = [c.name for c in table.columns]
        return dt, used, [tnames.index(n) for n in names], sels, prog

    @staticmethod
    def _table_tree_refused(e: native.Imm3Error, prog) -> bool:
        """the table refused a select TREE because it does not fit its one launch (more terms or predicate columns than it carries:
        the message prefix is the C ABI's contract, imm3.h): per-segment queries.  Any other ERR_ARG is a real argument error."""
        return prog is not None and e.code == native.ERR_ARG and e.msg.startswith(native.TABLE_TREE_REFUSED)

    def execute_agg(self, query: Query):
        """ProjectAgg queries: per-segment ProjectAggOp, then ProjectAggregateQueueOp's combine by group key
        (first arrival first; segments in ascending order).  Returns an ordered dict key -> {alias: Aggregator}.
        When the table qualifies, the whole thing is one imm3 table query (groups already merged on the GPU)."""
        query = self.resolve_subqueries(query)
        table = self.sm.getTable(query.table)
        plan = self._table_plan(query)
        if plan is not None:
            dt, used, used_idx, sels, prog = plan
            agg_op = resolveProjectOp(query.project, table)(ScanOp(self.sm, 0, query.table, used))
            try:   # ONE table query: the device orders its groups and cuts them to the limit
                return self._cut(dict(agg_op._run(dt, used, used_idx, sels, table.blockSize, prog, ordered=True)), agg_op)
            except native.Imm3Error as e:
                if not self._table_tree_refused(e, prog):
                    raise
        # count(distinct): no table query answered -- a single owned segment still does, several queries' groups cannot be combined
        owned = sum(1 for s in range(self.sm.getTableSegmentCount(table.name)) if self.sm.owns(table.name, s))
        count_distinct_route(any(isinstance(a, CountDistinct) for a in query.project.aggs), False, owned, self.device_merge, len(self.sm.ctxs))
        used = getColumns(query, table)
        leaves = self._select_ops(query)
        mk_scan = ScanOp.mkScanOp(self.sm, query.table)
        mk_agg = resolveProjectOp(query.project, table)
        if self.device_merge:
            return self._execute_agg_device_merge(table, used, leaves, mk_scan, mk_agg)
        result = {}
        raw_keys: Dict[str, list] = {}
        agg_op = None
        for segIdx in range(self.sm.getTableSegmentCount(table.name)):
            if not self.sm.owns(table.name, segIdx):
                continue
            op = mk_scan(used, segIdx)
            for leaf in leaves:
                op = leaf(op)
            agg_op = mk_agg(op)
            for key, aggmap in agg_op.iterator():
                raw_keys.setdefault(key, agg_op.raw_keys[key])
                cur = result.get(key)
                if cur is None:
                    result[key] = aggmap
                else:
                    for alias, agg in aggmap.items():
                        cur[alias] = cur[alias].combine(agg) if alias in cur else agg
        return self._order_merged(result, raw_keys, used, agg_op)

    @staticmethod
    def _cut(result: dict, agg_op) -> dict:
        """a limit without an order: the first `limit` groups in first-seen order (an ordered query was cut by whoever ordered it)"""
        if agg_op is None or agg_op.order_spec or agg_op.limit <= 0:
            return result
        return dict(list(result.items())[: agg_op.limit])

    def _order_merged(self, result: dict, raw_keys, used, agg_op) -> dict:
        """HAVING, then ORDER BY / limit over groups that were merged from per-segment results: on the host (filter_groups, order_groups)"""
        if agg_op is not None:
            result = filter_groups(result, agg_op.filter_leaves, agg_op.filter_prog)
        if agg_op is None or not agg_op.order_spec:
            return self._cut(result, agg_op)
        group_cols = [c for c in used if c.name in agg_op.groupBy]      # batch-column order: the order of a key's parts
        return order_groups(result, raw_keys, group_cols, agg_op.order_spec, agg_op.limit)

    def _execute_agg_device_merge(self, table, used, leaves, mk_scan, mk_agg):
        """execute_agg's per-segment branch with the combine on the GPU: every owned segment's aggregation query stays open, one
        merge by byte key brings their groups together (first arrival first: ascending segment, then first row), and the merged
        arrays are decoded into the same dict the host combine builds."""
        queries: Dict[int, list] = {}          # by index of the segment's context
        seg_ids: Dict[int, list] = {}
        agg_op = None
        self.last_merge_view = None
        try:
            for segIdx in range(self.sm.getTableSegmentCount(table.name)):
                if not self.sm.owns(table.name, segIdx):
                    continue
                op = mk_scan(used, segIdx)
                for leaf in leaves:
                    op = leaf(op)
                agg_op = mk_agg(op)
                ci = segIdx % len(self.sm.ctxs)
                queries.setdefault(ci, []).append(agg_op._open(*agg_op._segment_args()))
                seg_ids.setdefault(ci, []).append(segIdx)
            if agg_op is None:
                return {}
            order = sorted(queries)
            # having / order by / limit: the view of the merged groups comes from the merge itself (imm3_comm_merge_groups_view), in
            # its order and cut to its limit -- unless the library refuses the view (keys and tie beyond the order's 16 bytes): then
            # the plain merge, ordered on the host as before
            view = None
            if agg_op._order_key_bytes(used) > native.GROUP_ORDER_KEY_MAX_WIDTH or len(agg_op.order_spec) > native.ORDER_MAX_KEYS:
                # no device order takes such keys (imm3.h: four keys, 12 bytes): the host's does
                self.last_merge_view = "host"
            elif agg_op.filter_prog or agg_op.order_spec or agg_op.limit > 0:
                view = dict(order=agg_op._native_order(used), leaves=agg_op._native_filter(used), prog=agg_op.filter_prog, limit=max(agg_op.limit, 0))
            if len(order) == 1:
                comm = native.Comm(self.sm.ctxs[order[0]], 1, 0, native.comm_unique_id())
                merges = (lambda: comm.merge_groups_view(queries[order[0]], seg_ids[order[0]], **view),
                          lambda: comm.merge_groups_wide(queries[order[0]], seg_ids[order[0]]), comm.close)
            else:
                # several contexts: each one's world-of-one communicator (the _all merges use a communicator's context only).  Not
                # Comm.create_all: that is one context per DEVICE, and a manager may hold several contexts on one device.
                comms = [self.sm.merge_comm(ci) for ci in order]
                per_comm = ([queries[ci] for ci in order], [seg_ids[ci] for ci in order])
                merges = (lambda: native.Comm.merge_groups_view_all(comms, *per_comm, **view), lambda: native.Comm.merge_groups_wide_all(comms, *per_comm), lambda: None)
            try:
                merged = None
                if view is not None:
                    try:
                        merged = merges[0]()
                        self.last_merge_view = "device"
                    except native.Imm3Error as e:
                        if not (e.code == native.ERR_ARG and e.msg.startswith(native.MERGE_VIEW_REFUSED)):
                            raise
                        self.last_merge_view = "host"
                if merged is None:
                    merged = merges[1]()
            finally:
                merges[2]()
            key_bytes, _, counts, vals, strs = merged[:5]
        finally:
            for qs in queries.values():
                for q in qs:
                    q.close()
        wide = {j: strs[j] for j in agg_op._shape(list(used))[5]}
        groups = dict(agg_op._groups(used, None, key_bytes, counts, vals, wide))
        if self.last_merge_view == "device":         # already the view: decoded in the order it arrived
            return groups
        return self._order_merged(groups, agg_op.raw_keys, used, agg_op)

    def execute_table_columns(self, query: Query):
        """Project query over the whole table as ONE fused launch: (segment uint32[n], row uint32[n], [column arrays])
        in ascending (segment, row) order with the global limit applied -- or None when the table does not qualify."""
        return self._table_columns(self.resolve_subqueries(query))

    def _table_columns(self, query: Query):
        plan = self._table_plan(query)
        if plan is None:
            return None
        dt, used, used_idx, sels, prog = plan
        names = [c.name for c in used]
        proj = [names.index(n) for n in query.project.cols]
        okeys = order_keys(query.project.cols, getattr(query.project, "order_by", ()))
        try:
            q = native.DeviceQuery(dt.ctx, dt, used_idx, sels, proj, 0 if okeys else query.project.limit, self.sm.getTable(query.table).blockSize, expr=prog)
        except native.Imm3Error as e:
            if self._table_tree_refused(e, prog):
                return None
            raise
        if okeys:
            q.set_order(okeys, query.project.limit)                 # ONE ordered table query: (keys, segment, row) order, then the limit
        q.run()
        idx, cols = q.fetch_rows()
        seg, row = q.locate_rows(idx)
        out = []
        for raw, codec in zip(cols, q.proj_codecs):
            out.append(raw.reshape(-1).view("<i4") if codec in native.INT_CODECS else
                       raw.reshape(-1).view(np.int8) if codec in native.TINYINT_CODECS else raw)
        q.close()
        seg_ids = np.asarray(getattr(dt, "segment_ids", list(range(len(dt.segs)))), dtype=np.uint32)
        return seg_ids[seg] if seg.size else seg, row, out

    def execute(self, query: Query) -> Iterator[Row]:
        if isinstance(query.project, ProjectAgg):
            # ProjectAggregateQueueOp.next: Row of the aggregators' repr.  The reference lists them in the iteration
            # order of a mutable.HashMap keyed by alias (not reproduced); here: SELECT-list order.
            for _, aggmap in self.execute_agg(query).items():
                yield Row(*[a.repr() for a in aggmap.values()])
            return
        query = self.resolve_subqueries(query)                   # (once: what follows sees IntInSet / IntIn leaves)
        fused = self._table_columns(query)
        if fused is not None:
            yield from _rows_from_columns(fused[2])
            return
        limit = query.project.limit
        okeys = order_keys(query.project.cols, getattr(query.project, "order_by", ()))
        if okeys:
            # per-segment ordered queries, each with the limit (no segment contributes more), then a stable host merge by
            # (keys, segment, row)
            pipes = list(self.pipelines(query))
            if self.device_merge and pipes and all(proj._fused() is not None for _, proj in pipes):
                cols = self._execute_ordered_device_merge(pipes, limit)
            else:
                _, _, cols = merge_ordered([(segIdx, *proj.run_columns()) for segIdx, proj in pipes], okeys, limit)
            yield from _rows_from_columns(cols)
            return
        total = 0
        for _, proj in self.pipelines(query):
            for row in proj.iterator():
                if limit > 0 and total >= limit:
                    return
                yield row
                total += 1

    def _execute_ordered_device_merge(self, pipes, limit: int):
        """execute's ordered per-segment branch with the merge on the GPU: every owned segment's ordered query stays open, one
        imm3_comm_merge_ordered (one context) or _all (several) brings their rows together by (keys, segment, row) and cuts them to
        the limit; the merged columns are decoded as execute_table_columns decodes its own.  The rows operators.merge_ordered gives."""
        queries: Dict[int, list] = {}          # by index of the segment's context
        seg_ids: Dict[int, list] = {}
        try:
            for segIdx, proj in pipes:
                ci = segIdx % len(self.sm.ctxs)
                queries.setdefault(ci, []).append(proj._open())
                seg_ids.setdefault(ci, []).append(segIdx)
            order = sorted(queries)
            codecs = queries[order[0]][0].proj_codecs
            if len(order) == 1:
                _, _, cols = self.sm.merge_comm(order[0]).merge_ordered(queries[order[0]], seg_ids[order[0]], limit)
            else:
                comms = [self.sm.merge_comm(ci) for ci in order]      # (world-of-one each, as in _execute_agg_device_merge)
                _, _, cols = native.Comm.merge_ordered_all(comms, [queries[ci] for ci in order], [seg_ids[ci] for ci in order], limit)
        finally:
            for qs in queries.values():
                for q in qs:
                    q.close()
        return ProjectOp._typed(cols, codecs)

    def execute_columns(self, query: Query):
        """Columnar result per segment: [(segIdx, row_index, [column arrays])] (no Row boxing)."""
        return self._columns(self.resolve_subqueries(query))

    def _columns(self, query: Query):
        return [(segIdx, *proj.run_columns()) for segIdx, proj in self.pipelines(query)]
