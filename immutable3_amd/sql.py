"""SQLParser -- the SQL subset of engine/src/main/scala/immutabledb/sql/SQLParser.scala:8-129 as a backtracking recursive-descent
parser with the semantics of scala-parser-combinators' JavaTokenParsers (the Python mirror of host/sql.hpp): whitespace is skipped
before every literal / regex, literals match as PREFIXES (no word boundary), alternatives are tried in order with backtracking,
parseAll must consume the whole input.

  query            := queryProjectAgg | queryProjectAggNoGroup | queryProject
  queryProject     := "select" repsep(ident, ",") "from" ident where limit
  queryProjectAgg  := "select" rep1sep(agg, ",") "from" ident where ["group" "by" rep1sep(ident, ",")]
  where            := opt("where" filter)
  filter           := "(" repsep(filter,"and") ")" | "(" repsep(filter,"or") ")"
                    | ident "=" value | ident "=" "'" value "'" | ident ">" value | ident "<" value
  limit            := opt("limit" digits)
  ident = [\\w#]+   value = [\\w0-9#]+

EXTENSION, only when the parser is asked for it -- parseAll(sql, order_by=True) -- the "sort" core/Query.scala:27 announces:
  queryProject     := "select" repsep(ident, ",") "from" ident where orderBy limit
  orderBy          := opt("order" "by" rep1sep(ident opt("asc" | "desc"), ","))
With the flag off the grammar is the reference's, and such a statement fails to parse.

EXTENSION, only when asked for -- parseAll(sql, group_order=True) -- ORDER BY and LIMIT over the groups of an aggregation:
  queryProjectAgg  := "select" rep1sep(agg, ",") "from" ident where ["group" "by" rep1sep(ident, ",")] orderBy limit
an order key being an ident (a group-by column or an alias) or an aggregate call as written in the SELECT list (`count(id)`), which
resolves to its alias (id_count).  A flag of its own, because order_by=True has always left aggregation statements to the reference's
grammar (imm3_sql's --order-by switches both on).  With the flag off such a statement fails to parse as it always has.

EXTENSION, only when asked for -- parseAll(sql, string_ranges=True) -- byte-order ranges on string columns (query.Prefix / StrGT / StrLT),
tried behind the reference's alternatives:
  filter           := ... | ident ">" "'" value "'" | ident "<" "'" value "'" | ident "like" "'" value "%" "'"
With the flag off those statements fail to parse with the message they have always given.

EXTENSION, only when asked for -- parseAll(sql, having=True) -- HAVING over the groups of an aggregation, before their order and limit:
  queryProjectAgg  := "select" rep1sep(agg, ",") "from" ident where ["group" "by" rep1sep(ident, ",")] having orderBy limit
  having           := opt("having" hfilter)
  hfilter          := "(" repsep(hfilter,"and") ")" | "(" repsep(hfilter,"or") ")" | hkey ">" value | hkey "<" value | hkey "=" value
  hkey             := ident | the aggregate call as written in the SELECT list (count(id) names id_count)
orderBy / limit follow only under their own flag (group_order).  The tree becomes ProjectAgg.having -- And / Or over Select(alias, GT |
LT | EQ) --, whose checks (query.group_filter_leaves: an unknown alias, a group-by column, a threshold that is no integer) raise
ValueError.  With the flag off the grammar and every parse-failure message are what they were.

EXTENSION, only when asked for -- parseAll(sql, count_distinct=True) -- the number of distinct values per group (query.CountDistinct),
tried in front of the reference's aggregates:
  agg              := "count" "(" "distinct" ident ")" | ...
wherever an aggregate call may stand (the SELECT list, an order key, a having key: `count(distinct age)` names age_distinct).  Literals
match as prefixes, as everywhere here, so under the flag `count(distinctx)` is count(distinct x); a column called `distinct` itself
still counts as before (no ident follows).  With the flag off the grammar is exactly what it was: `count(distinct x)` fails with
"`)' expected".

EXTENSION, only when asked for -- parseAll(sql, int_lists=True) -- IN-lists on int32 / int8 columns (query.IntIn), tried behind the
reference's alternatives (and behind the string ranges):
  filter           := ... | ident "in" "(" rep1sep(int, ",") ")"        int = -?[0-9]+
A literal outside int32 raises ValueError (query.INT_IN_RANGE_ERROR + the literal), at parse time.  With the flag off the grammar and
every parse-failure message are what they were.

EXTENSION, only when asked for -- parseAll(sql, subqueries=True) -- IN (sub-query) on int32 / int8 columns (query.IntInQuery), tried
behind everything above:
  filter           := ... | ident "in" "(" "select" ident from where ")"
The inner statement is one column, a table and an optional where tree (which may hold further sub-queries): no aggregate, no
group by, order by or limit can be spelled there.  With the flag off the grammar and every parse-failure message are what they were."""
from __future__ import annotations

import re

from . import query as Q

_WORD = re.compile(r"[A-Za-z0-9_#]+")
_DIGITS = re.compile(r"[0-9]+")
_INT = re.compile(r"-?[0-9]+")


class ParseError(Exception):
    pass


class SQLParser:
    def __init__(self, s: str, order_by: bool = False, string_ranges: bool = False, group_order: bool = False, having: bool = False,
                 count_distinct: bool = False, int_lists: bool = False, subqueries: bool = False):
        self.int_lists = int_lists
        self.subqueries = subqueries
        self.s, self.order_by, self.string_ranges, self.group_order, self.having = s, order_by, string_ranges, group_order, having
        self.count_distinct = count_distinct
        self.furthest, self.expected = 0, "`select'"

    @staticmethod
    def parseAll(sql: str, order_by: bool = False, string_ranges: bool = False, group_order: bool = False, having: bool = False,
                 count_distinct: bool = False, int_lists: bool = False, subqueries: bool = False) -> Q.Query:
        p = SQLParser(sql, order_by, string_ranges, group_order, having, count_distinct, int_lists, subqueries)
        r = p._query(0)
        if r is not None:
            q, end = r
            end = p._ws(end)
            if end == len(sql):
                return q
            raise ParseError(f"[1.{end + 1}] failure: end of input expected\n\n{sql}")
        raise ParseError(f"[1.{p.furthest + 1}] failure: {p.expected} expected\n\n{sql}")

    # ---- tokens ----
    def _ws(self, i):
        while i < len(self.s) and self.s[i].isspace():
            i += 1
        return i

    def _note(self, at, what):
        if at >= self.furthest:
            self.furthest, self.expected = at, what

    def _lit(self, i, word):
        i = self._ws(i)
        if self.s.startswith(word, i):
            return i + len(word)
        self._note(i, f"`{word}'")
        return None

    def _ident(self, i):
        i = self._ws(i)
        m = _WORD.match(self.s, i)
        if not m:
            self._note(i, "string matching regex `[\\w\\#]+'")
            return None
        return m.group(0), m.end()

    @staticmethod
    def _to_double(v: str) -> float:
        try:
            if v[-1:] in "dDfF" and v[:-1]:
                return float(v[:-1])
            return float(v)
        except ValueError:
            raise ParseError(f'NumberFormatException: For input string: "{v}"')

    # ---- filters ----
    def _filter_list(self, i, sep, is_and):
        p = self._lit(i, "(")
        if p is None:
            return None
        xs = []
        r = self._filter(p)
        if r is not None:
            xs.append(r[0])
            p = r[1]
            while True:
                t = self._lit(p, sep)
                if t is None:
                    break
                r = self._filter(t)
                if r is None:
                    break
                xs.append(r[0])
                p = r[1]
        q = self._lit(p, ")")
        if q is None:
            return None
        if not xs:
            raise ParseError("UnsupportedOperationException: tail of empty list")
        acc = xs[0]
        for x in xs[1:]:
            acc = Q.And(acc, x) if is_and else Q.Or(acc, x)
        return acc, q

    def _cmp(self, i, op):
        a = self._ident(i)
        if a is None:
            return None
        q = self._lit(a[1], op)
        if q is None:
            return None
        return a[0], q

    def _filter(self, i):
        for sep, is_and in (("and", True), ("or", False)):
            r = self._filter_list(i, sep, is_and)
            if r is not None:
                return r
        c = self._cmp(i, "=")
        if c is not None:
            v = self._ident(c[1])
            if v is not None:
                return Q.Select(c[0], Q.EQ(self._to_double(v[0]))), v[1]
            t = self._lit(c[1], "'")
            if t is not None:
                v = self._ident(t)
                if v is not None:
                    u = self._lit(v[1], "'")
                    if u is not None:
                        return Q.Select(c[0], Q.Match([v[0]])), u
        for op, mk in ((">", Q.GT), ("<", Q.LT)):
            c = self._cmp(i, op)
            if c is not None:
                v = self._ident(c[1])
                if v is not None:
                    return Q.Select(c[0], mk(self._to_double(v[0]))), v[1]
        if self.string_ranges:
            for op, mk, tail in ((">", Q.StrGT, ""), ("<", Q.StrLT, ""), ("like", Q.Prefix, "%")):
                c = self._cmp(i, op)
                t = self._lit(c[1], "'") if c is not None else None
                v = self._ident(t) if t is not None else None
                u = (self._lit(v[1], tail) if tail else v[1]) if v is not None else None
                u = self._lit(u, "'") if u is not None else None
                if u is not None:
                    return Q.Select(c[0], mk(v[0])), u
        if self.int_lists:                                     # ident "in" "(" rep1sep(int, ",") ")"
            c = self._cmp(i, "in")
            p = self._lit(c[1], "(") if c is not None else None
            r = self._int(p) if p is not None else None
            if r is not None:
                ints, p = [r[0]], r[1]
                while True:
                    t = self._lit(p, ",")
                    r = self._int(t) if t is not None else None
                    if r is None:                              # (rep1sep backtracks over a dangling separator)
                        break
                    ints.append(r[0])
                    p = r[1]
                u = self._lit(p, ")")
                if u is not None:
                    return Q.Select(c[0], Q.IntIn(ints)), u
        if self.subqueries:                                    # ident "in" "(" "select" ident from where ")"
            c = self._cmp(i, "in")
            p = self._lit(c[1], "(") if c is not None else None
            p = self._lit(p, "select") if p is not None else None
            g = self._ident(p) if p is not None else None
            f = self._from(g[1]) if g is not None else None
            if f is not None:
                w, e = self._where(f[1])
                u = self._lit(e, ")")
                if u is not None:
                    return Q.Select(c[0], Q.IntInQuery(Q.Query(f[0], w, Q.Project([g[0]])))), u
        return None

    def _int(self, i):
        """-?[0-9]+ ; a literal outside int32 is a ValueError, not a parse failure"""
        i = self._ws(i)
        m = _INT.match(self.s, i)
        if not m:
            self._note(i, "string matching regex `-?[0-9]+'")
            return None
        v = int(m.group(0))
        if not Q.INT32_MIN <= v <= Q.INT32_MAX:
            raise ValueError(Q.INT_IN_RANGE_ERROR + m.group(0))
        return v, m.end()

    def _where(self, i):
        p = self._lit(i, "where")
        if p is not None:
            r = self._filter(p)
            if r is not None:
                return r
        return Q.NoSelect, i

    def _from(self, i):
        p = self._lit(i, "from")
        return None if p is None else self._ident(p)

    def _ident_list(self, i, at_least_one):
        r = self._ident(i)
        if r is None:
            return None if at_least_one else ([], i)
        out, p = [r[0]], r[1]
        while True:
            q = self._lit(p, ",")
            r = self._ident(q) if q is not None else None
            if r is None:
                break
            out.append(r[0])
            p = r[1]
        return out, p

    def _agg(self, i):
        if self.count_distinct:                                # (the opt-in: "count" "(" "distinct" ident ")")
            p = self._lit(i, "count")
            q = self._lit(p, "(") if p is not None else None
            d = self._lit(q, "distinct") if q is not None else None
            r = self._ident(d) if d is not None else None
            t = self._lit(r[1], ")") if r is not None else None
            if t is not None:
                return Q.CountDistinct(r[0]), t
        for kw, mk in (("sum", Q.Sum), ("min", Q.Min), ("max", Q.Max), ("count", Q.Count)):
            p = self._lit(i, kw)
            q = self._lit(p, "(") if p is not None else None
            r = self._ident(q) if q is not None else None
            t = self._lit(r[1], ")") if r is not None else None
            if t is not None:
                return mk(r[0]), t
        return None

    def _select_agg(self, i):
        q = self._lit(i, "select")
        r = self._agg(q) if q is not None else None
        if r is None:
            return None
        aggs, p = [r[0]], r[1]
        while True:
            c = self._lit(p, ",")
            r = self._agg(c) if c is not None else None
            if r is None:
                break
            aggs.append(r[0])
            p = r[1]
        return aggs, p

    def _order_key(self, i, aggs):
        """ident, or -- in an aggregation -- an aggregate call, which names its alias"""
        if aggs:
            r = self._agg(i)
            if r is not None:
                return Q.default_alias(r[0]), r[1]
        return self._ident(i)

    def _hfilter(self, i):
        """hfilter: a parenthesised and-list / or-list of hfilters, or hkey (an ident or an aggregate call) > | < | = value"""
        for sep, is_and in (("and", True), ("or", False)):
            p = self._lit(i, "(")
            xs = []
            r = self._hfilter(p) if p is not None else None
            while r is not None:
                xs.append(r[0])
                p = r[1]
                t = self._lit(p, sep)
                r = self._hfilter(t) if t is not None else None
            q = self._lit(p, ")") if p is not None and xs else None
            if q is not None:
                acc = xs[0]
                for x in xs[1:]:
                    acc = Q.And(acc, x) if is_and else Q.Or(acc, x)
                return acc, q
        k = self._order_key(i, True)
        if k is None:
            return None
        for op, mk in ((">", Q.GT), ("<", Q.LT), ("=", Q.EQ)):
            q = self._lit(k[1], op)
            v = self._ident(q) if q is not None else None
            if v is not None:
                return Q.Select(k[0], mk(self._to_double(v[0]))), v[1]
        return None

    def _having(self, i):
        """opt("having" hfilter): (tree or None, position behind the clause)"""
        p = self._lit(i, "having")
        r = self._hfilter(p) if p is not None else None
        return (None, i) if r is None else r

    def _limit(self, d):
        """opt("limit" digits): (limit, position behind it)"""
        e = self._lit(d, "limit")
        if e is not None:
            m = _DIGITS.match(self.s, self._ws(e))
            if m:
                return int(m.group(0)), m.end()
        return 0, d

    def _order_by(self, i, aggs=False):
        """opt("order" "by" rep1sep(ident opt("asc" | "desc"), ",")): (keys, position behind the clause); no clause: ([], i)"""
        p = self._lit(i, "order")
        q = self._lit(p, "by") if p is not None else None
        if q is None:
            return [], i
        keys = []
        while True:
            r = self._order_key(q, aggs)
            if r is None:
                break
            name, e = r
            desc = False
            t = self._lit(e, "desc")
            if t is not None:
                desc, e = True, t
            else:
                t = self._lit(e, "asc")
                if t is not None:
                    e = t
            keys.append((name, desc))
            q = e
            t = self._lit(q, ",")
            if t is None or self._order_key(t, aggs) is None:      # (rep1sep backtracks over a dangling separator)
                break
            q = t
        return (keys, q) if keys else ([], i)

    def _query(self, i):
        a = self._select_agg(i)
        if a is not None:
            t = self._from(a[1])
            if t is not None:
                w = self._where(t[1])
                d = self._lit(w[1], "group")
                e = self._lit(d, "by") if d is not None else None
                g = self._ident_list(e, True) if e is not None else None
                groups, d = (g[0], g[1]) if g is not None else ([], w[1])
                order, limit, having = [], 0, None
                if self.having:                                    # (the opt-in, like group_order below)
                    having, d = self._having(d)
                if self.group_order:                               # (the opt-in: with it off the statement ends here, as in the reference)
                    order, d = self._order_by(d, aggs=True)
                    limit, d = self._limit(d)
                return Q.Query(t[0], w[0], Q.ProjectAgg(a[0], groups, order, limit, having)), d
        p = self._lit(i, "select")
        if p is None:
            return None
        cols = self._ident_list(p, False)
        t = self._from(cols[1])
        if t is None:
            return None
        w = self._where(t[1])
        d, order, limit = w[1], [], 0
        if self.order_by:
            order, d = self._order_by(d)
        limit, d = self._limit(d)
        return Q.Query(t[0], w[0], Q.Project(cols[0], limit, order)), d
