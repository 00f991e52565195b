"""The statement fuzz (test_stmt_fuzz_host.py, test_gpu_stmt_fuzz.py): one loader-made table in two block sizes, a seeded generator of
whole statements -- where tree, engine flags, projection or aggregation with HAVING, ORDER BY and LIMIT --, their SQL text where the
grammar can spell them, and a plain-Python reference over the list of row dicts.  Nothing here imports the engines or the library: the
reference restates the documented rules (README, include/imm3.h, the comments of operators.py) and shares no code with what it checks.

A statement is a Stmt (below): plain tuples, so that the error class -- statements whose ADT cannot even be built -- has a
representation; to_query() makes the immutable3_amd.query ADT, render() the SQL text, show() the text imm3_sql --parse-only prints."""
import json
import os
import subprocess
from dataclasses import dataclass, replace

import numpy as np

from immutable3_amd import query as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "immutable3_amd", "bin")
TABLE = "people"
N = 5_000
COLDEF = ("id:DENSE_INT,v:DENSE_INT,age:DENSE_TINYINT,state:DENSE_STRING:size=2,name:DENSE_STRING:size=8,tag:DENSE_STRING:size=5,"
          "order_no:DENSE_INT")
COLUMNS = ("id", "v", "age", "state", "name", "tag", "order_no")       # order_no: a name that begins with a keyword of the grammar
WIDTH = {"id": 4, "v": 4, "age": 1, "state": 2, "name": 8, "tag": 5, "order_no": 4}
INT_COLS = ("id", "v", "age", "order_no")
STR_COLS = ("state", "name", "tag")
COMMON_STATES = ("CA", "NY", "TX", "WA", "VA", "DC", "CT", "OH", "FL", "MA")
FIRST_ONLY, LAST_ONLY = "AA", "ZZ"                                      # states of the first / the last segment only
STATES = COMMON_STATES + (FIRST_ONLY, LAST_ONLY)
V_VALUES = (-7, -5, -4, -3, -2, -1, 0, 1, 2, 3, 4, 6, 8, 9, 12)
BLOCKS = (1024, 1000)
SEEDS = 16                                                              # the default seed set; IMM3_FUZZ_MORE adds seeds behind it
PER_SEED = 10
SEED_BASE = 20261020


class Refused(Exception):
    """the reference's verdict on a statement of the error class: both engines must refuse it before running anything"""


# ---- the table ---------------------------------------------------------------------------------------------------------------------
HIGH_NAMES = ("prefix\u00e9", "\u00f1and\u00faz", "zebra\u20ac")          # 8 bytes each in UTF-8, with bytes >= 0x80: behind the stem, in front, at the end


def pools():
    """(names, tags): 30 names of 8 bytes, half of them behind the 6-byte prefix `prefix`; 10 tags of 5 bytes.  Three names carry bytes
    >= 0x80 (valid UTF-8, so that they pass the CSV, the loader and both engines' decoding unchanged): strings are ordered, maximised
    and range-tested as UNSIGNED bytes, and a signed-char comparison anywhere would put these names before `a` instead of behind `z`."""
    rng = np.random.default_rng(SEED_BASE)
    letters = "abcdefghijklmnopqrstuvwxyz"
    names = set(HIGH_NAMES)
    assert all(len(n.encode()) == 8 for n in names)
    while len(names) < 15:
        names.add("prefix" + "".join(letters[i] for i in rng.integers(0, 26, size=2)))
    while len(names) < 30:
        names.add("".join(letters[i] for i in rng.integers(0, 26, size=8)))
    tags = set()
    alnum = letters + letters.upper() + "0123456789"
    while len(tags) < 10:
        tags.add("".join(alnum[i] for i in rng.integers(0, len(alnum), size=5)))
    return sorted(names), sorted(tags)


NAMES, TAGS = pools()


def make_rows():
    """the 5000 row dicts, in load order.  id: unique, 700 of them negative; v: 15 values around 0; age: -3 .. 3 and a few -128 / 127;
    state: 10 codes everywhere, AA in the first 1500 rows only, ZZ in the last 700 only; every string exactly as wide as its column"""
    rng = np.random.default_rng(SEED_BASE + 1)
    ids = (rng.permutation(N) - 700).tolist()
    v = [V_VALUES[i] for i in rng.integers(0, len(V_VALUES), size=N)]
    age = rng.integers(-3, 4, size=N).tolist()
    for k, i in enumerate(rng.choice(N, size=12, replace=False).tolist()):
        age[i] = -128 if k % 2 else 127
    state = [COMMON_STATES[i] for i in rng.integers(0, len(COMMON_STATES), size=N)]
    for i in rng.choice(1500, size=40, replace=False).tolist():
        state[i] = FIRST_ONLY
    for i in (N - 700 + rng.choice(700, size=40, replace=False)).tolist():
        state[i] = LAST_ONLY
    name = [NAMES[i] for i in rng.integers(0, len(NAMES), size=N)]
    tag = [TAGS[i] for i in rng.integers(0, len(TAGS), size=N)]
    order_no = rng.integers(0, 60, size=N).tolist()
    return [{"id": ids[i], "v": v[i], "age": age[i], "state": state[i], "name": name[i], "tag": tag[i], "order_no": order_no[i]} for i in range(N)]


def make_tables(base):
    """(rows, {block size: data directory}, {block size: rows per segment}): the same rows loaded by bin/imm3_loader in blocks of 1024
    (a table takes them) and of 1000 (it does not), two blocks to a segment"""
    rows = make_rows()
    csv = os.path.join(str(base), "people.csv")
    with open(csv, "w", encoding="utf-8") as f:
        f.write(",".join(COLUMNS) + "\n")
        for r in rows:
            f.write(",".join(str(r[c]) for c in COLUMNS) + "\n")
    dirs, seg_rows = {}, {}
    for block in BLOCKS:
        d = os.path.join(str(base), f"data{block}")
        os.mkdir(d)
        p = subprocess.run([os.path.join(BIN, "imm3_loader"), "-t", TABLE, "-c", COLDEF, "-d", d, "-i", csv, "--block-size", str(block), "--segment-size", "2"],
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        dirs[block] = d
        seg_rows[block] = segment_rows(d)
    return rows, dirs, seg_rows


def segment_rows(d):
    """rows per segment, read from the id column's block tables (4 bytes a row)"""
    out = []
    while os.path.exists(os.path.join(d, TABLE, f"id_{len(out)}.meta")):
        with open(os.path.join(d, TABLE, f"id_{len(out)}.meta")) as f:
            out.append(int(json.load(f)["blockOffset"][-1]) // 4)
    return out


# ---- statements --------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Stmt:
    """kind: "project" | "agg".  where: None, ("and" | "or", a, b) or ("leaf", col, op, operand) with op one of > < = (an int), in /
    notin (a tuple of strings), range (lo, hi), prefix, sgt, slt (a string).  having: None, ("and" | "or", a, b) or (alias, op, number).
    aggs: (kind, col) with kind count / min / max / sum / avg.  order_by: (name, descending).  error: None, or what makes both engines
    refuse the statement."""
    kind: str
    where: object = None
    honour_and_or: bool = False
    honour_not_match: bool = False
    cols: tuple = ()
    aggs: tuple = ()
    group: tuple = ()
    having: object = None
    order_by: tuple = ()
    limit: int = 0
    error: object = None


RANGE_OPS = ("range", "prefix", "sgt", "slt")


def leaves_of(t):
    if t is None:
        return []
    return [t] if t[0] == "leaf" else leaves_of(t[1]) + leaves_of(t[2])


def has_or(t):
    return t is not None and t[0] != "leaf" and (t[0] == "or" or has_or(t[1]) or has_or(t[2]))


def as_tree(s):
    """the where clause runs with its And / Or tags honoured: an Or under honour_and_or, or a NotMatch under honour_not_match (which
    honours the tags of that statement whatever honour_and_or says); else it is the reference's conjunction of every leaf"""
    return (s.honour_and_or and has_or(s.where)) or (s.honour_not_match and any(l[2] == "notin" for l in leaves_of(s.where)))


def used_columns(s):
    """the batch columns, first mention first: the where tree's in leaf order, the SELECT list's or the aggregates', the group-by's"""
    out = []
    for c in [l[1] for l in leaves_of(s.where)] + (list(s.cols) if s.kind == "project" else [c for (_, c) in s.aggs] + list(s.group)):
        if c not in out:
            out.append(c)
    return out


def alias_of(agg):
    return f"{agg[1]}_{agg[0]}"


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def narrowed(col, x):
    """an integer threshold as the column's type holds it (Select.scala: `gt.toInt` on an Int column, `gt.toByte` on a TinyInt one): on
    the int8 column the low 8 bits, signed -- age > 128 is age > -128, age > -129 is age > 127"""
    return (x + 128) % 256 - 128 if col == "age" else x


def leaf_holds(leaf, r):
    _, col, op, x = leaf
    v = r[col]
    if op in (">", "<", "="):
        x = narrowed(col, x)
    if op == ">":
        return v > x
    if op == "<":
        return v < x
    if op == "=":
        return v == x
    if op == "in":
        return v in x                                                  # whole values: one of another length matches nothing
    if op == "notin":
        return v not in x
    b, w = v.encode(), WIDTH[col]
    if op == "range":                                                  # closed; lo padded with 0x00, hi with 0xFF
        return x[0].encode().ljust(w, b"\x00") <= b <= x[1].encode().ljust(w, b"\xff")
    if op == "prefix":
        return b.startswith(x.encode())
    pad = x.encode().ljust(w, b"\x00")                                 # strict, against the value padded with 0x00
    return b > pad if op == "sgt" else b < pad


def tree_holds(t, r):
    if t[0] == "leaf":
        return leaf_holds(t, r)
    return (tree_holds(t[1], r) and tree_holds(t[2], r)) if t[0] == "and" else (tree_holds(t[1], r) or tree_holds(t[2], r))


def check_where(s):
    ls = leaves_of(s.where)
    if any(l[2] == "notin" for l in ls) and not s.honour_not_match:
        raise Refused("NotMatch with the flag off: Unsupported condition")
    if as_tree(s) and any(l[2] in RANGE_OPS for l in ls):
        raise Refused("a string range in a tree that runs with OR / NOT (include/imm3.h: out of scope)")


def keep_mask(rows, s):
    """[bool per row]: the where clause as the engine flags make it run"""
    check_where(s)
    if s.where is None:
        return [True] * len(rows)
    if as_tree(s):
        return [tree_holds(s.where, r) for r in rows]
    ls = leaves_of(s.where)                                            # every Or is an And: the conjunction of all the leaves
    return [all(leaf_holds(l, r) for l in ls) for r in rows]


def _order_value(v):
    return v.encode() if isinstance(v, str) else v


def _agg_is_string(agg):
    return agg[0] in ("min", "max") and agg[1] in STR_COLS


def check_project(s):
    for (name, _) in s.order_by:
        if name not in s.cols:
            raise Refused(f"order key {name} outside the SELECT list")


def check_agg(s):
    for a in s.aggs:
        if a[0] in ("sum", "avg"):
            raise Refused("Sum / Avg through the Engine: Unknown Aggregate type")
    aliases = {alias_of(a): a for a in s.aggs}
    for (name, _) in s.order_by:
        if name not in s.group and name not in aliases:
            raise Refused(f"order key {name} is neither a group column nor an alias")

    def rec(h):
        if h[0] in ("and", "or"):
            rec(h[1])
            rec(h[2])
            return
        if h[0] in s.group or h[0] not in aliases:
            raise Refused(f"having {h[0]}: not an aggregate's alias")
        if _agg_is_string(aliases[h[0]]):
            raise Refused(f"having {h[0]}: a string maximum is not compared")
        if int(h[2]) != h[2]:
            raise Refused(f"having {h[0]}: the threshold {h[2]} is no integer")
    if s.having is not None:
        rec(s.having)


def having_holds(h, g):
    if h[0] in ("and", "or"):
        a, b = having_holds(h[1], g), having_holds(h[2], g)
        return (a and b) if h[0] == "and" else (a or b)
    v = g[h[0]]
    return v > h[2] if h[1] == ">" else (v < h[2] if h[1] == "<" else v == h[2])


def all_groups(rows, s, keep=None):
    """([(key label, {alias: value}, {group column: value}, first row)]) in first-seen order, before HAVING.  count counts rows; max is
    the maximum -- of the bytes, for a string column; min on a string column is that string MAXIMUM too (resolveProjectOp: "Min over a
    STRING column becomes MaxStringAggr (the reference's own mapping)"), under the alias <col>_min."""
    keep = keep_mask(rows, s) if keep is None else keep
    gcols = [c for c in used_columns(s) if c in s.group]
    groups, order = {}, []
    for i, r in enumerate(rows):
        if not keep[i]:
            continue
        key = "_".join(str(r[c]) for c in gcols)
        g = groups.get(key)
        if g is None:
            g = groups[key] = ({}, {c: r[c] for c in gcols}, i)
            order.append(key)
        vals = g[0]
        for a in s.aggs:
            alias, x = alias_of(a), r[a[1]]
            if a[0] == "count":
                vals[alias] = vals.get(alias, 0) + 1
            elif alias not in vals:
                vals[alias] = x
            elif a[0] == "max" or isinstance(x, str):
                vals[alias] = max(vals[alias], x, key=_order_value)
            else:
                vals[alias] = min(vals[alias], x)
    return [(k, groups[k][0], groups[k][1], groups[k][2]) for k in order]


def expected(rows, s, keep=None):
    """What the statement returns.  A projection: [tuple of values] -- the survivors in ascending (segment, row), i.e. load order, or,
    ordered, after one stable sort per key from the least significant up (ints signed, strings as bytes, so ties stay in (segment,
    row)); then the limit.  An aggregation: [(key label, {alias: value})] -- the groups in first-seen order, the ones HAVING keeps,
    the stable sorts, the limit (without an order it cuts the first-seen order).  Raises Refused for the error class."""
    if s.kind == "project":
        check_project(s)
        keep = keep_mask(rows, s) if keep is None else keep
        out = [tuple(r[c] for c in s.cols) for i, r in enumerate(rows) if keep[i]]
        for (name, desc) in reversed(s.order_by):
            j = s.cols.index(name)
            out.sort(key=lambda t: _order_value(t[j]), reverse=desc)
        return out[: s.limit] if s.limit > 0 else out
    check_agg(s)
    groups = all_groups(rows, s, keep)
    if s.having is not None:
        groups = [g for g in groups if having_holds(s.having, g[1])]
    for (name, desc) in reversed(s.order_by):
        groups.sort(key=lambda g: _order_value(g[2][name] if name in g[2] else g[1][name]), reverse=desc)
    if s.limit > 0:
        groups = groups[: s.limit]
    return [(g[0], g[1]) for g in groups]


def java_double(v):
    """Double.toString of the integral value a numeric MIN / MAX holds (below 10^7: no exponent)"""
    assert abs(int(v)) < 10 ** 7
    return f"{int(v)}.0"


def rows_text(s, want):
    """the Row(...) lines both engines print: a projection's values as they are; an aggregation's aggregators in SELECT-list order --
    counts as integers, string maxima as they are, numeric minima / maxima as Double.toString"""
    if s.kind == "project":
        return ["Row(" + ",".join(str(x) for x in t) + ")" for t in want]
    out = []
    for (_, m) in want:
        xs = [str(m[alias_of(a)]) if a[0] == "count" or _agg_is_string(a) else java_double(m[alias_of(a)]) for a in s.aggs]
        out.append("Row(" + ",".join(xs) + ")")
    return out


# ---- which launch a statement gets -------------------------------------------------------------------------------------------------
def predict_path(s, block, contexts=1):
    """"table" (one launch over all segments), "segments" (per-segment queries and a merge) or "either", from the documented rules:
    ragged blocks and several contexts have no table; a table takes Match on a 2-byte column with 1 .. 8 values (flat list or tree), on
    a width that is a multiple of 4 in a flat list only, and a string range on such a width in a flat list only -- so nothing on the
    5-byte tag; a tree must fit the tile form, which is predicted only where an upper bound of its normal form is plain to see:
    terms (a leaf 1, Or the sum, And the product) <= 8, <= 3 predicate columns, exclusion lists that cannot grow past 8."""
    if block != 1024 or contexts > 1:
        return "segments"
    ls = leaves_of(s.where)
    tree = as_tree(s)
    for (_, col, op, x) in ls:
        if op in ("in", "notin"):
            if col == "state":
                if not 0 < len(x) <= 8:
                    return "segments"
            elif WIDTH[col] % 4 or tree:
                return "segments"
        elif op in RANGE_OPS and (WIDTH[col] % 4 or tree):
            return "segments"
    if not tree:
        return "table"

    def terms(t):
        return 1 if t[0] == "leaf" else (terms(t[1]) + terms(t[2]) if t[0] == "or" else terms(t[1]) * terms(t[2]))
    excluded = sum(len(l[3]) for l in ls if l[2] == "notin")
    if terms(s.where) <= 8 and len({l[1] for l in ls}) <= 3 and excluded <= 8:
        return "table"
    return "either"


# ---- ADT, SQL text, the text imm3_sql --parse-only prints ----------------------------------------------------------------------------
def _select_adt(t):
    if t is None:
        return Q.NoSelect
    if t[0] != "leaf":
        return (Q.And if t[0] == "and" else Q.Or)(_select_adt(t[1]), _select_adt(t[2]))
    _, col, op, x = t
    cond = {">": lambda: Q.GT(float(x)), "<": lambda: Q.LT(float(x)), "=": lambda: Q.EQ(float(x)), "in": lambda: Q.Match(list(x)),
            "notin": lambda: Q.NotMatch(list(x)), "range": lambda: Q.StrRange(x[0], x[1]), "prefix": lambda: Q.Prefix(x),
            "sgt": lambda: Q.StrGT(x), "slt": lambda: Q.StrLT(x)}[op]()
    return Q.Select(col, cond)


def _having_adt(h):
    if h is None:
        return None
    if h[0] in ("and", "or"):
        return (Q.And if h[0] == "and" else Q.Or)(_having_adt(h[1]), _having_adt(h[2]))
    return Q.Select(h[0], {">": Q.GT, "<": Q.LT, "=": Q.EQ}[h[1]](float(h[2])))


def to_query(s):
    """the immutable3_amd.query ADT; for some statements of the error class the constructors themselves refuse (ValueError)"""
    if s.kind == "project":
        return Q.Query(TABLE, _select_adt(s.where), Q.Project(list(s.cols), s.limit, s.order_by))
    mk = {"count": Q.Count, "min": Q.Min, "max": Q.Max, "sum": Q.Sum, "avg": Q.Avg}
    return Q.Query(TABLE, _select_adt(s.where), Q.ProjectAgg([mk[k](c) for (k, c) in s.aggs], list(s.group), s.order_by, s.limit, _having_adt(s.having)))


def _where_sql(t, top=True):
    if t[0] != "leaf":
        a, b = _where_sql(t[1], False), _where_sql(t[2], False)
        return None if a is None or b is None else f"({a} {t[0]} {b})"
    _, col, op, x = t
    if op in (">", "<", "="):
        return f"{col} {op} {x}" if x >= 0 else None                   # (a value is [\w#]+: no sign)
    if op == "in" and len(x) == 1 and x[0].isascii():                  # (a value is [A-Za-z0-9_#]+)
        return f"{col} = '{x[0]}'"
    if op in ("prefix", "sgt", "slt") and x.isascii():
        return {"prefix": f"{col} like '{x}%'", "sgt": f"{col} > '{x}'", "slt": f"{col} < '{x}'"}[op]
    return None                                                        # IN-lists, NotMatch and closed ranges have no spelling


def _having_sql(h):
    if h[0] in ("and", "or"):
        a, b = _having_sql(h[1]), _having_sql(h[2])
        return None if a is None or b is None else f"({a} {h[0]} {b})"
    return f"{h[0]} {h[1]} {h[2]}" if h[2] >= 0 and int(h[2]) == h[2] else None     # (a value is [\w#]+: no sign, no point)


def render(s):
    """the statement as SQL for the parsers with every extension flag on, or None where the grammar cannot spell it"""
    if s.kind == "project":
        sql = "select " + ", ".join(s.cols) + " from " + TABLE
    else:
        if any(k == "avg" for (k, _) in s.aggs):
            return None
        sql = "select " + ", ".join(f"{k}({c})" for (k, c) in s.aggs) + " from " + TABLE
    if s.where is not None:
        w = _where_sql(s.where)
        if w is None:
            return None
        sql += " where " + w
    if s.kind == "agg":
        if s.group:
            sql += " group by " + ", ".join(s.group)
        if s.having is not None:
            h = _having_sql(s.having)
            if h is None:
                return None
            sql += " having " + h
    if s.order_by:
        sql += " order by " + ", ".join(f"{n} {'desc' if d else 'asc'}" for (n, d) in s.order_by)
    if s.limit > 0:
        sql += f" limit {s.limit}"
    return sql


def _show_select(t):
    if t is None:
        return "NoSelect"
    if t[0] != "leaf":
        return f"{'And' if t[0] == 'and' else 'Or'}({_show_select(t[1])},{_show_select(t[2])})"
    _, col, op, x = t
    cond = {">": f"GT({x})", "<": f"LT({x})", "=": f"EQ({x})", "prefix": f"Prefix({x})", "sgt": f"StrGT({x})", "slt": f"StrLT({x})"}.get(op)
    if op == "in":
        cond = "Match(List(" + ", ".join(x) + "))"
    return f"Select({col},{cond})"


def _show_having(h):
    if h[0] in ("and", "or"):
        return f"{'And' if h[0] == 'and' else 'Or'}({_show_having(h[1])},{_show_having(h[2])})"
    return "Select(" + h[0] + "," + {">": "GT", "<": "LT", "=": "EQ"}[h[1]] + "(" + str(h[2]) + "))"


def show(s):
    """the Query(...) line of imm3_sql --parse-only for a spellable statement"""
    order = "List(" + ", ".join(f"({n},{'desc' if d else 'asc'})" for (n, d) in s.order_by) + ")"
    if s.kind == "project":
        p = "Project(List(" + ", ".join(s.cols) + ")," + str(s.limit) + ("," + order if s.order_by else "") + ")"
    else:
        p = "ProjectAgg(List(" + ", ".join(f"{k.capitalize()}({c},None)" for (k, c) in s.aggs) + "),List(" + ", ".join(s.group) + ")"
        if s.order_by or s.limit > 0 or s.having is not None:
            p += "," + order + "," + str(s.limit) + (",Some(" + _show_having(s.having) + ")" if s.having is not None else "")
        p += ")"
    return f"Query({TABLE},{_show_select(s.where)},{p})"


# ---- the generator -----------------------------------------------------------------------------------------------------------------
class Data:
    """what the generator reads of the rows: per int column its candidate thresholds -- quantiles, the value below the minimum and
    the one above the maximum --, and the row count"""

    def __init__(self, rows):
        self.rows = rows
        self.lo, self.hi, self.quant = {}, {}, {}
        for c in INT_COLS:
            xs = sorted(r[c] for r in rows)
            self.lo[c], self.hi[c] = xs[0], xs[-1]
            self.quant[c] = [xs[0] - 1] + [xs[int(q * (len(xs) - 1))] for q in (0.02, 0.1, 0.25, 0.5, 0.75, 0.9, 0.98)] + [xs[-1] + 1]


def _pick(rng, xs, p=None):
    return xs[int(rng.choice(len(xs), p=p))]


def _int_leaf(rng, data, col, spell=False):
    """spell: a threshold the grammar can write (its values carry no sign)"""
    xs = [x for x in data.quant[col] if x >= 0] if spell else data.quant[col]
    op = _pick(rng, (">", "<", "="), (0.4, 0.4, 0.2))
    if op == "=" and col == "id":                                      # (one row at the most: rarely)
        op = ">"
    inner = [x for x in xs if data.lo[col] <= x <= data.hi[col]]
    return ("leaf", col, op, int(_pick(rng, xs if rng.random() < 0.15 or not inner else inner)))


def _match_leaf(rng, col, negate=False, n=None):
    if col == "state":
        n = n or _pick(rng, (1, 2, 8, 9, 12), (0.3, 0.25, 0.15, 0.2, 0.1))
        pool = list(STATES) + ["QQ", "XY"]                               # (two codes the data does not have)
        vals = [pool[i] for i in rng.choice(len(pool), size=n, replace=False)]
    else:
        pool = (NAMES if col == "name" else TAGS) + ["zzzzzzzz"[: WIDTH[col]], "q"]   # (an absent value, and one of another length)
        vals = [pool[i] for i in rng.choice(len(pool), size=n or int(rng.integers(1, 4)), replace=False)]
    return ("leaf", col, "notin" if negate else "in", tuple(vals))


def _range_leaf(rng, col, spell=False):
    pool = NAMES if col == "name" else TAGS
    a, b = sorted(pool[i] for i in rng.choice(len(pool), size=2, replace=False))
    op = _pick(rng, RANGE_OPS[1:] if spell else RANGE_OPS)
    if op == "range":
        return ("leaf", col, op, (a[: int(rng.integers(1, WIDTH[col] + 1))], b[: int(rng.integers(1, WIDTH[col] + 1))]))
    if op == "prefix":
        return ("leaf", col, op, "prefix"[: int(rng.integers(1, 7))] if col == "name" and rng.random() < 0.6 else a[: int(rng.integers(1, 4))])
    return ("leaf", col, op, a[: int(rng.integers(1, WIDTH[col] + 1))])


def _tree(rng, leaves, p_or):
    """a random binary tree over the leaves in their order (at most 4: at most 3 levels of And / Or)"""
    if len(leaves) == 1:
        return leaves[0]
    k = int(rng.integers(1, len(leaves)))
    return ("or" if rng.random() < p_or else "and", _tree(rng, leaves[:k], p_or), _tree(rng, leaves[k:], p_or))


def _where(rng, data, theme, wide="name"):
    """(tree or None, honour_and_or, honour_not_match); wide: the string column the range theme's first leaf is on"""
    if theme == "none":
        return None, bool(rng.random() < 0.5), False
    if theme in ("nothing", "everything"):
        col = _pick(rng, ("id", "v", "order_no"))                      # (not the int8 column: a threshold past its range wraps)
        leaf = ("leaf", col, ">", data.hi[col] + 1 if theme == "nothing" else data.lo[col] - 1)
        if rng.random() < 0.5:                                         # under a conjunction the verdict is the same
            other = ("leaf", "state", "in", tuple(STATES)) if theme == "everything" else _int_leaf(rng, data, _pick(rng, INT_COLS))
            return ("and", leaf, other), bool(rng.random() < 0.5), False
        return leaf, False, False
    int_cols = [INT_COLS[i] for i in rng.choice(len(INT_COLS), size=2, replace=False)]
    spell = theme not in ("not", "inlist") and rng.random() < 0.7           # keep to what the grammar can spell
    n = _pick(rng, (1, 2, 3, 4), (0.3, 0.4, 0.2, 0.1))
    leaves = []
    for k in range(n):
        kind = _pick(rng, ("int", "state", "not", "str", "range"), {"tree": (0.55, 0.3, 0.15, 0, 0), "not": (0.45, 0.15, 0.4, 0, 0),
                                                                      "inlist": (0.3, 0.7, 0, 0, 0), "range": (0.4, 0.1, 0, 0.1, 0.4),
                                                                      "flat": (0.45, 0.25, 0, 0.15, 0.15)}[theme])
        if theme == "range" and k == 0:
            kind = "range"
        if theme == "not" and k == 0:
            kind = "not"
        if theme == "inlist" and k == 0:
            leaves.append(_match_leaf(rng, "state", n=_pick(rng, (9, 12))))
        elif kind == "int":
            leaves.append(_int_leaf(rng, data, _pick(rng, int_cols), spell))
        elif kind in ("state", "not"):
            leaves.append(_match_leaf(rng, "state", negate=kind == "not", n=1 if spell else None))
        else:
            col = wide if theme == "range" and k == 0 else ("name" if rng.random() < 0.55 else "tag")
            if any(l[1] in ("name", "tag") for l in leaves):               # (one wide string column per where clause: the column budget)
                col = next(l[1] for l in leaves if l[1] in ("name", "tag"))
            leaves.append(_match_leaf(rng, col, n=1 if spell else None) if kind == "str" else _range_leaf(rng, col, spell))
    t = _tree(rng, leaves, {"tree": 0.6, "not": 0.4, "inlist": 0.3, "range": 0.5, "flat": 0.0}[theme])
    hnm = any(l[2] == "notin" for l in leaves)
    hao = bool(rng.random() < 0.6)
    if any(l[2] in RANGE_OPS for l in leaves):                          # a range never runs in a program with OR / NOT: its Or runs as And
        hao = False
    return t, hao, hnm


def _limit(rng, kept):
    return max(0, int(_pick(rng, (0, 1, 10, kept - 1, kept, kept + 3))))


def _project(rng, data, s, ordered):
    used = used_columns(s)
    room = 4 - len(used)
    fresh = [c for c in COLUMNS if c not in used]
    k = int(rng.integers(0 if used else 1, room + 1))
    cols = [fresh[i] for i in rng.choice(len(fresh), size=k, replace=False)] + [c for c in used if rng.random() < 0.5]
    if not cols:
        cols = [used[0]]
    cols = [cols[i] for i in rng.permutation(len(cols))][:4]
    order = []
    if ordered:
        width = 0
        for c in [cols[i] for i in rng.permutation(len(cols))][: int(rng.integers(1, 5))]:
            if width + WIDTH[c] <= 16:
                order.append((c, bool(rng.random() < 0.5)))
                width += WIDTH[c]
        if not order:
            order = [(cols[0], False)]
        if order[0][0] == "id" and len(cols) > 1 and rng.random() < 0.8:   # (a unique first key leaves the others nothing to decide)
            order = order[1:] + order[:1] if len(order) > 1 else [(next(c for c in cols if c != "id"), False)]
    s = replace(s, cols=tuple(cols), order_by=tuple(order))
    return replace(s, limit=_limit(rng, sum(keep_mask(data.rows, s))))


def _order_width(s, name):
    """a group-order key's normalised width (include/imm3.h): a group column's width; COUNT 5; MIN / MAX its column's width"""
    if name in s.group:
        return WIDTH[name]
    a = next(a for a in s.aggs if alias_of(a) == name)
    return 5 if a[0] == "count" else WIDTH[a[1]]


def _aggregation(rng, data, s, theme):
    used = used_columns(s)
    room = 4 - len(used)
    gpool = ("state", "age", "v", "name")
    if theme == "many":
        group = _pick(rng, (("name", "v"), ("state", "v"), ("name", "age"), ("v", "name"), ("name", "state")))
    elif theme == "one":
        group = ()
    else:
        ng = _pick(rng, (0, 1, 2), (0.1, 0.6, 0.3))
        group = tuple(gpool[i] for i in rng.choice(len(gpool), size=ng, replace=False))
        if ng and rng.random() < 0.5:
            group = ("state",) + tuple(c for c in group if c != "state")[: ng - 1]
    group = tuple(group)
    while len(set(used) | set(group)) > 4:
        group = group[:-1]
    aggs = []
    for _ in range(int(rng.integers(1, 5))):
        a = (_pick(rng, ("count", "min", "max"), (0.4, 0.25, 0.35)), _pick(rng, COLUMNS))
        if a[1] == "tag" and a[0] != "count":
            a = ("count", a[1])
        if a not in aggs and len(set(used) | set(group) | {x[1] for x in aggs} | {a[1]}) <= 4:
            aggs.append(a)
    have = list(dict.fromkeys(list(used) + list(group) + [c for (_, c) in aggs]))
    if not aggs or (theme.startswith("having") and not any(a[0] == "count" for a in aggs) and len(aggs) < 4):
        aggs.append(("count", "id" if len(have) < 4 or "id" in have else have[0]))
    s = replace(s, aggs=tuple(aggs), group=group)
    base = all_groups(data.rows, s)
    having = None
    numeric = [a for a in aggs if not _agg_is_string(a)]
    if numeric and theme in ("having", "having-none", "having-all") or (numeric and rng.random() < 0.3):
        def hleaf():
            a = _pick(rng, numeric)
            vals = sorted(g[1][alias_of(a)] for g in base) or [0]
            med = vals[len(vals) // 2]
            if theme == "having-none":
                return (alias_of(a), ">", vals[-1] + 1)
            if theme == "having-all":
                return (alias_of(a), ">", vals[0] - 1)
            return (alias_of(a), _pick(rng, (">", "<", "=")), int(med + _pick(rng, (-1, 0, 0, 1))))
        shape = _pick(rng, (1, 2, 3), (0.5, 0.3, 0.2))
        if theme in ("having-none", "having-all"):
            having = hleaf() if shape == 1 else ("and", hleaf(), hleaf())
        elif shape == 1:
            having = hleaf()
        elif shape == 2:
            having = (_pick(rng, ("and", "or")), hleaf(), hleaf())
        else:
            having = (_pick(rng, ("and", "or")), (_pick(rng, ("and", "or")), hleaf(), hleaf()), hleaf())
    s = replace(s, having=having)
    order = []
    if rng.random() < (0.75 if theme != "one" else 0.3):
        names = list(group) + [alias_of(a) for a in aggs]
        width = 0
        for name in [names[i] for i in rng.permutation(len(names))][: int(rng.integers(1, 4))]:
            if width + _order_width(s, name) <= 12:
                order.append((name, bool(rng.random() < 0.5)))
                width += _order_width(s, name)
    s = replace(s, order_by=tuple(order))
    return replace(s, limit=_limit(rng, len(expected(data.rows, replace(s, limit=0)))))


ERRORS = ("sum", "avg", "notmatch-off", "order-outside", "having-group-column", "having-string-max", "having-fraction", "or-with-range")


def _error(rng, data, which):
    """one statement of the error class: a sound statement with the one thing both engines refuse"""
    leaf = _int_leaf(rng, data, "v", spell=True)
    if which in ("sum", "avg"):
        return Stmt("agg", leaf, aggs=(("count", "id"), (which, "age")), group=("state",), error=which)
    if which == "notmatch-off":
        return Stmt(_pick(rng, ("project", "agg")), ("and", leaf, _match_leaf(rng, "state", negate=True, n=2)), honour_and_or=True, cols=("id", "state"),
                    aggs=(("count", "id"),), group=("state",), error=which)
    if which == "order-outside":
        return Stmt("project", leaf, cols=("id", "state"), order_by=(("age", False),), limit=10, error=which)
    if which == "having-group-column":
        return Stmt("agg", leaf, aggs=(("count", "id"),), group=("age",), having=("age", ">", 0), error=which)
    if which == "having-string-max":
        return Stmt("agg", leaf, aggs=(("count", "id"), ("max", "name")), group=("state",), having=("name_max", ">", 3), error=which)
    if which == "having-fraction":
        return Stmt("agg", leaf, aggs=(("count", "id"),), group=("state",), having=("id_count", ">", 2.5), error=which)
    return Stmt("project", ("or", leaf, ("leaf", "name", "prefix", "prefix")), honour_and_or=True, cols=("id", "name"), error=which)


# one seed's ten statements: (projection or aggregation, the where clause's theme, the rest's theme)
THEMES = (("project", "tree", "plain"), ("project", "flat", "ordered"), ("agg", "flat", "having"), ("agg", "not", "free"),
          ("project", "range", "ordered"), ("agg", "tree", "many"), ("*", "extreme", "*"), ("project", "inlist", "ordered"),
          ("error", "", ""), ("agg", "none", "having-edge"))


def statements(seed, data):
    """the statements of one seed"""
    rng = np.random.default_rng([SEED_BASE, seed])
    out = []
    for i in range(PER_SEED):
        kind, wtheme, rest = THEMES[i % len(THEMES)]
        if kind == "error":
            out.append(_error(rng, data, ERRORS[seed % len(ERRORS)]))
            continue
        if wtheme == "extreme":
            wtheme = ("nothing", "everything")[seed % 2]
            kind, rest = (("project", "ordered"), ("agg", "free"), ("agg", "one"), ("project", "plain"))[(seed // 2) % 4]
        if rest == "having-edge":
            rest = ("having-none", "having-all")[seed % 2]
            wtheme = ("none", "flat", "tree", "none")[seed % 4]
        if (kind, wtheme, rest) == ("agg", "not", "free") and seed % 4 == 3:
            rest = "one"
        where, hao, hnm = _where(rng, data, wtheme, ("name", "tag")[seed % 2])
        s = Stmt(kind, where, honour_and_or=hao, honour_not_match=hnm)
        out.append(_project(rng, data, s, rest == "ordered") if kind == "project" else _aggregation(rng, data, s, rest))
    return out


# ---- the second witness: numpy over column arrays -------------------------------------------------------------------------------------
def column_arrays(rows):
    return {c: np.array([r[c] if c in INT_COLS else r[c].encode() for r in rows], dtype=np.int64 if c in INT_COLS else f"S{WIDTH[c]}") for c in COLUMNS}


def np_mask(arrs, s):
    """keep_mask's answer from whole-column comparisons"""
    def leaf(l):
        _, col, op, x = l
        a, w = arrs[col], WIDTH[col]
        if op in (">", "<", "="):
            if col == "age":
                x = int(np.array(x, np.int64).astype(np.int8))       # (the cast wraps as toByte does)
            return a > x if op == ">" else (a < x if op == "<" else a == x)
        if op in ("in", "notin"):
            m = np.isin(a, np.array([v.encode() for v in x if len(v.encode()) == w] or [b""], dtype=f"S{w}"))
            return ~m if op == "notin" else m
        if op == "range":
            return (a >= np.bytes_(x[0].encode())) & (a <= np.bytes_(x[1].encode().ljust(w, b"\xff")))
        if op == "prefix":
            return np.char.startswith(a, x.encode())
        return a > np.bytes_(x.encode()) if op == "sgt" else a < np.bytes_(x.encode())

    def rec(t):
        if t[0] == "leaf":
            return leaf(t)
        return (rec(t[1]) & rec(t[2])) if t[0] == "and" else (rec(t[1]) | rec(t[2]))
    n = arrs["id"].shape[0]
    if s.where is None:
        return np.ones(n, bool)
    if as_tree(s):
        return rec(s.where)
    m = np.ones(n, bool)
    for l in leaves_of(s.where):
        m &= leaf(l)
    return m


def np_groups(arrs, s, mask):
    """all_groups' (label, values) pairs from numpy: group codes by np.unique, first-seen order by each group's first row, counts by
    bincount, minima / maxima by ufunc.at (strings through the rank of their sorted distinct values)"""
    idx = np.flatnonzero(mask)
    if idx.size == 0:
        return []
    gcols = [c for c in used_columns(s) if c in s.group]
    code = np.zeros(idx.size, np.int64)
    for c in gcols:
        u, inv = np.unique(arrs[c][idx], return_inverse=True)
        code = code * len(u) + inv
    _, first, inv = np.unique(code, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    out_vals = {}
    for a in s.aggs:
        col = arrs[a[1]][idx]
        if a[0] == "count":
            out_vals[alias_of(a)] = np.bincount(inv, minlength=first.size).tolist()
            continue
        u, rank = np.unique(col, return_inverse=True)
        if a[0] == "max" or a[1] in STR_COLS:
            best = np.full(first.size, -1, np.int64)
            np.maximum.at(best, inv, rank)
        else:
            best = np.full(first.size, len(u), np.int64)
            np.minimum.at(best, inv, rank)
        out_vals[alias_of(a)] = [x.decode() if isinstance(x, bytes) else int(x) for x in u[best].tolist()]
    out = []
    for g in order.tolist():
        r = idx[first[g]]
        label = "_".join(arrs[c][r].decode() if c in STR_COLS else str(int(arrs[c][r])) for c in gcols)
        out.append((label, {k: v[g] for k, v in out_vals.items()}))
    return out
