"""Query ADT -- mirror of core/src/main/scala/immutabledb/Query.scala:3-46 (same names, same fields)."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional


class SelectCondition:
    pass


@dataclass(frozen=True)
class Match(SelectCondition):      # Query.scala:4
    values: tuple

    def __init__(self, values):
        object.__setattr__(self, "values", tuple(values))


@dataclass(frozen=True)
class NotMatch(SelectCondition):   # Query.scala:5 (SelectOp rejects it, Select.scala:22)
    values: tuple

    def __init__(self, values):
        object.__setattr__(self, "values", tuple(values))


@dataclass(frozen=True)
class EQ(SelectCondition):         # Query.scala:6
    eq: float


@dataclass(frozen=True)
class GT(SelectCondition):         # Query.scala:7
    gt: float


@dataclass(frozen=True)
class LT(SelectCondition):         # Query.scala:8
    lt: float


# ---- EXTENSION: byte-order ranges on a string column (include/imm3.h: IMM3_STR_RANGE).  The order is the one ORDER BY sorts by and
# the string MAX aggregate maximises by: unsigned, byte-wise, from the first byte.  Bounds are str (UTF-8) or bytes. ----
def _bytes(v) -> bytes:
    return v.encode("utf-8") if isinstance(v, str) else bytes(v)


@dataclass(frozen=True)
class StrRange(SelectCondition):   # closed: lo padded to the column's width with 0x00 <= row <= hi padded with 0xFF
    lo: bytes
    hi: bytes

    def __init__(self, lo, hi):
        object.__setattr__(self, "lo", _bytes(lo))
        object.__setattr__(self, "hi", _bytes(hi))


@dataclass(frozen=True)
class Prefix(SelectCondition):     # the rows that start with p: StrRange(p, p)
    p: bytes

    def __init__(self, p):
        object.__setattr__(self, "p", _bytes(p))


@dataclass(frozen=True)
class StrGT(SelectCondition):      # strict: row > v padded to the column's width with 0x00
    v: bytes

    def __init__(self, v):
        object.__setattr__(self, "v", _bytes(v))


@dataclass(frozen=True)
class StrLT(SelectCondition):      # strict: row < v padded to the column's width with 0x00
    v: bytes

    def __init__(self, v):
        object.__setattr__(self, "v", _bytes(v))


STR_RANGE_CONDS = (StrRange, Prefix, StrGT, StrLT)
STR_RANGE_NONE = (b"\x01", b"\x00")   # a leaf no row passes: 01 00 00 .. > 00 FF FF ..


def str_successor(v: bytes):
    """the next value of len(v) bytes in byte order (big-endian arithmetic over all the bytes), or None behind FF .. FF"""
    n = int.from_bytes(v, "big") + 1
    return None if not v or n >> (8 * len(v)) else n.to_bytes(len(v), "big")


def str_predecessor(v: bytes):
    """the value before v, or None before 00 .. 00"""
    n = int.from_bytes(v, "big")
    return None if not v or n == 0 else (n - 1).to_bytes(len(v), "big")


def str_range_bounds(cond: SelectCondition, width: int):
    """(lo, hi) of the IMM3_STR_RANGE leaf a range condition becomes on a string column of `width` bytes; the library pads lo with
    0x00 and hi with 0xFF.  StrGT(v) is from the successor of v padded with 0x00 on, StrLT(v) up to its predecessor; where there is
    none the leaf is STR_RANGE_NONE.  A bound longer than the column raises ValueError (the library refuses it too)."""
    given = {StrRange: lambda c: (c.lo, c.hi), Prefix: lambda c: (c.p, c.p), StrGT: lambda c: (c.v,), StrLT: lambda c: (c.v,)}[type(cond)](cond)
    for b in given:
        if len(b) > width:
            raise ValueError(f"string bound {b!r} is longer than the column's {width} bytes")
    if isinstance(cond, (StrRange, Prefix)):
        return given
    padded = cond.v + b"\x00" * (width - len(cond.v))
    if isinstance(cond, StrGT):
        lo = str_successor(padded)
        return STR_RANGE_NONE if lo is None else (lo, b"")
    hi = str_predecessor(padded)
    return STR_RANGE_NONE if hi is None else (b"", hi)


# ---- EXTENSION: an IN-list on an int32 / int8 column (include/imm3.h: IMM3_INT_IN): the rows whose value is one of `values`.
# Membership is exact on integers (no narrowing: a value outside an int8 column's range matches nothing); duplicates count once, an
# empty list selects no row.  Not under an Or or a NotMatch-as-NOT tree (the library refuses the program). ----
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
INT_IN_RANGE_ERROR = "integer literal out of range for an IN-list (int32): "


@dataclass(frozen=True)
class IntIn(SelectCondition):
    values: tuple

    def __init__(self, values):
        vals = []
        for v in values:
            if isinstance(v, bool) or int(v) != v:
                raise ValueError(f"IntIn takes integers, not {v!r}")
            if not INT32_MIN <= int(v) <= INT32_MAX:
                raise ValueError(INT_IN_RANGE_ERROR + str(int(v)))
            vals.append(int(v))
        object.__setattr__(self, "values", tuple(vals))


# ---- EXTENSION: IN (sub-query), the semi-join (include/imm3.h: IMM3_INT_IN_SET): the rows whose value is one the inner query's column
# takes among the rows the inner query selects.  The inner query is a plain projection of exactly ONE int32 / int8 column with a where
# tree: no aggregation, no order by, no limit (the set is the whole selection's either way; refused so that nobody reads a cut into
# it).  Uncorrelated: the inner query names its own table and nothing of the outer one.  Not under an Or or a NotMatch-as-NOT tree.
# `query` is typed loosely because Query is defined below. ----
INT_IN_QUERY_ERRORS = {
    "query": "IntInQuery takes a Query, not ",
    "agg": "IntInQuery: the inner query is an aggregation; it must be a plain projection of one column",
    "cols": "IntInQuery: the inner query must project exactly one column, not ",
    "order": "IntInQuery: the inner query has an order by; the set is its whole selection, unordered",
    "limit": "IntInQuery: the inner query has a limit; the set is its whole selection",
}


@dataclass(frozen=True)
class IntInQuery(SelectCondition):
    query: object

    def __init__(self, query):
        if not isinstance(query, Query):
            raise ValueError(INT_IN_QUERY_ERRORS["query"] + repr(query))
        if not isinstance(query.project, Project):
            raise ValueError(INT_IN_QUERY_ERRORS["agg"])
        if len(query.project.cols) != 1:
            raise ValueError(INT_IN_QUERY_ERRORS["cols"] + str(list(query.project.cols)))
        if query.project.order_by:
            raise ValueError(INT_IN_QUERY_ERRORS["order"])
        if query.project.limit != 0:
            raise ValueError(INT_IN_QUERY_ERRORS["limit"])
        object.__setattr__(self, "query", query)


@dataclass(frozen=True)
class _NoOp(SelectCondition):      # Query.scala:9
    pass


NoOp = _NoOp()


class SelectADT:
    pass


@dataclass(frozen=True)
class And(SelectADT):              # Query.scala:12
    op1: SelectADT
    op2: SelectADT


@dataclass(frozen=True)
class Or(SelectADT):               # Query.scala:13 (executed exactly like And: Engine.scala:240 ignores the tag)
    op1: SelectADT
    op2: SelectADT


@dataclass(frozen=True)
class Select(SelectADT):           # Query.scala:14
    col: str
    cond: SelectCondition


@dataclass(frozen=True)
class _NoSelect(SelectADT):        # Query.scala:15
    pass


NoSelect = _NoSelect()


class ProjectADT:
    pass


def order_keys(cols, order_by):
    """ORDER BY entries (col, descending) as places in the SELECT list `cols`: [(index, descending)].  A key that is not a
    SELECT-list column raises ValueError naming it (order keys outside the SELECT list are out of scope: include/imm3.h)."""
    cols = list(cols)
    out = []
    for (col, desc) in order_by:
        if col not in cols:
            raise ValueError(f"order by column {col!r} is not in the SELECT list {cols}")
        out.append((cols.index(col), bool(desc)))
    return out


@dataclass(frozen=True)
class Project(ProjectADT):         # Query.scala:29; order_by is the "sort" the reference announces above ProjectADT (Query.scala:27)
    cols: tuple
    limit: int = 0
    order_by: tuple = ()           # entries (col, descending), most significant first; with it `limit` is applied AFTER the order

    def __init__(self, cols, limit: int = 0, order_by=()):
        object.__setattr__(self, "cols", tuple(cols))
        object.__setattr__(self, "limit", int(limit))
        object.__setattr__(self, "order_by", tuple((str(c), bool(d)) for (c, d) in order_by))
        order_keys(self.cols, self.order_by)


@dataclass(frozen=True)
class Aggregate:                   # Query.scala:17-20
    col: str
    alias: Optional[str] = None


class Sum(Aggregate):              # Query.scala:21 (parsed, then rejected: Engine.scala:152)
    pass


class Avg(Aggregate):              # Query.scala:22
    pass


class Min(Aggregate):              # Query.scala:23
    pass


class Max(Aggregate):              # Query.scala:24
    pass


class Count(Aggregate):            # Query.scala:25
    pass


class CountDistinct(Aggregate):    # not in the reference: count(distinct col), the number of distinct values per group (IMM3_AGG_COUNT_DISTINCT)
    pass


def default_alias(agg: Aggregate) -> str:
    """the alias Engine.resolveProjectOp gives an aggregate without one (Engine.scala:130-156): <col>_max / _min / _count; a CountDistinct: <col>_distinct"""
    suffix = {Max: "max", Min: "min", Count: "count", Sum: "sum", Avg: "avg", CountDistinct: "distinct"}[type(agg)]
    return agg.alias or f"{agg.col}_{suffix}"


def group_order_names(aggs, groupBy, order_by):
    """ORDER BY entries (name, descending) of an aggregation checked against its group-by columns and its aggregates' aliases: a name
    that is neither raises ValueError naming it, and so does an average (ordering by a quotient is out of scope: include/imm3.h).  A
    name that is both a group column and an alias means the group column."""
    aliases = {default_alias(a): a for a in aggs}
    for (name, _) in order_by:
        if name in groupBy:
            continue
        if name not in aliases:
            raise ValueError(f"order by {name!r} is neither a group-by column {list(groupBy)} nor an aggregate's alias {list(aliases)}")
        if isinstance(aliases[name], Avg):
            raise ValueError(f"order by {name!r}: ordering by an average is not supported")


def group_filter_leaves(aggs, groupBy, having):
    """A HAVING tree -- And / Or over Select(name, GT | LT | EQ), name an aggregate's alias -- checked and flattened:
    ([(alias, cond class, int threshold)], postfix program over the leaf indices with "and" / "or").  ValueError names the cause: a name
    that is no alias, a group-by column (rows are filtered by the select), a condition other than GT / LT / EQ, a threshold that is no
    integer (aggregates are compared exactly in int64: include/imm3.h, imm3_query_set_group_filter).  None: ([], [])."""
    aliases = {(a.alias or default_alias(a)): a for a in aggs}
    leaves, prog = [], []

    def rec(node):
        if isinstance(node, (And, Or)):
            rec(node.op1)
            rec(node.op2)
            prog.append("and" if isinstance(node, And) else "or")
        elif isinstance(node, Select):
            if node.col in groupBy:
                raise ValueError(f"having {node.col!r}: a group-by column is filtered by the select (where), not by having")
            if node.col not in aliases:
                raise ValueError(f"having {node.col!r} is not an aggregate's alias {list(aliases)}")
            if not isinstance(node.cond, (GT, LT, EQ)):
                raise ValueError(f"having {node.col!r}: the condition must be GT, LT or EQ, not {node.cond!r}")
            v = {GT: lambda c: c.gt, LT: lambda c: c.lt, EQ: lambda c: c.eq}[type(node.cond)](node.cond)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v in (float("inf"), float("-inf")) or int(v) != v:
                raise ValueError(f"having {node.col!r}: the threshold {v!r} is not an integer (aggregates are compared exactly)")
            prog.append(len(leaves))
            leaves.append((node.col, type(node.cond), int(v)))
        else:
            raise ValueError(f"having: {node!r} is neither And, Or nor Select")

    if having is not None:
        rec(having)
    return leaves, prog


@dataclass(frozen=True)
class ProjectAgg(ProjectADT):      # Query.scala:30; order_by / limit: the "sort" of Query.scala:27 over the groups (imm3_query_set_group_order)
    aggs: tuple
    groupBy: tuple = ()
    order_by: tuple = ()           # entries (name, descending), most significant first: a group-by column or an aggregate's alias
    limit: int = 0                 # > 0: the first `limit` groups of the order (without an order: of the first-seen order)
    having: Optional[SelectADT] = None   # And / Or over Select(alias, GT | LT | EQ): the groups kept, BEFORE the order and the limit (imm3_query_set_group_filter)

    def __init__(self, aggs, groupBy=(), order_by=(), limit: int = 0, having=None):
        object.__setattr__(self, "aggs", tuple(aggs))
        object.__setattr__(self, "groupBy", tuple(groupBy))
        object.__setattr__(self, "order_by", tuple((str(c), bool(d)) for (c, d) in order_by))
        object.__setattr__(self, "limit", int(limit))
        object.__setattr__(self, "having", having)
        group_order_names(self.aggs, self.groupBy, self.order_by)
        group_filter_leaves(self.aggs, self.groupBy, self.having)


@dataclass(frozen=True)
class Query:                       # Query.scala:42-46
    table: str
    select: SelectADT
    project: ProjectADT
