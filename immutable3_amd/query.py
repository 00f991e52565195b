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


@dataclass(frozen=True)
class ProjectAgg(ProjectADT):      # Query.scala:30
    aggs: tuple
    groupBy: tuple = ()

    def __init__(self, aggs, groupBy=()):
        object.__setattr__(self, "aggs", tuple(aggs))
        object.__setattr__(self, "groupBy", tuple(groupBy))


@dataclass(frozen=True)
class Query:                       # Query.scala:42-46
    table: str
    select: SelectADT
    project: ProjectADT
