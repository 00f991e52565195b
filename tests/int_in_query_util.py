"""What the IN (sub-query) suites share (test_int_in_query_host.py, test_gpu_int_in_query.py): a second table beside the statement
fuzz's `people` (tests/stmt_fuzz_util.py) -- `orders`, whose `cust` refers to people.id and whose `qty` is an int8 --, statements with
sub-query leaves, their plain-Python reference over the row dicts, and their spelling as a Query ADT and as SQL.

A statement is (table, leaves, cols, limit); a leaf is (col, op, operand) with op one of > < = (an int), match (a list of strings),
in (a list of ints) or inq -- operand (inner table, inner column, inner leaves): the rows whose `col` is a value the inner column takes
among the inner table's rows that pass the inner leaves (a conjunction, like the outer ones)."""
import os
import subprocess

import numpy as np

import stmt_fuzz_util as F
from immutable3_amd import query as Q

ORDERS = "orders"
N_ORDERS = 3_000
ORDERS_COLDEF = "order_id:DENSE_INT,cust:DENSE_INT,qty:DENSE_TINYINT,region:DENSE_STRING:size=2"
ORDERS_COLUMNS = ("order_id", "cust", "qty", "region")
INT8_COLS = ("age", "qty")
INT_COLS = {F.TABLE: ("id", "v", "age", "order_no"), ORDERS: ("order_id", "cust", "qty")}
STR_COL = {F.TABLE: "state", ORDERS: "region"}
# (outer column, inner table, inner column) whose values have something in common
RELATED = {F.TABLE: (("id", ORDERS, "cust"), ("age", ORDERS, "qty"), ("v", ORDERS, "qty"), ("order_no", ORDERS, "qty"), ("id", F.TABLE, "id")),
           ORDERS: (("cust", F.TABLE, "id"), ("qty", F.TABLE, "age"), ("qty", F.TABLE, "v"), ("order_id", ORDERS, "order_id"))}


def make_orders():
    """3000 orders: cust is a people.id for nine in ten (ids repeat), else an id nobody has; qty -128 .. 127 clustered around 0"""
    rng = np.random.default_rng(F.SEED_BASE + 7)
    cust = (rng.integers(0, F.N, size=N_ORDERS) - 700)
    miss = rng.random(N_ORDERS) < 0.1
    cust[miss] = 9_000 + rng.integers(0, 50, size=int(miss.sum()))
    qty = rng.integers(-6, 7, size=N_ORDERS)
    qty[rng.choice(N_ORDERS, size=10, replace=False)] = [-128, 127] * 5
    region = [F.COMMON_STATES[i] for i in rng.integers(0, 4, size=N_ORDERS)]
    return [{"order_id": 100_000 + i, "cust": int(cust[i]), "qty": int(qty[i]), "region": region[i]} for i in range(N_ORDERS)]


def load_orders(base, dirs):
    """`orders` loaded beside `people` into every data directory of F.make_tables, in the same block sizes"""
    rows = make_orders()
    csv = os.path.join(str(base), "orders.csv")
    with open(csv, "w", encoding="utf-8") as f:
        f.write(",".join(ORDERS_COLUMNS) + "\n")
        for r in rows:
            f.write(",".join(str(r[c]) for c in ORDERS_COLUMNS) + "\n")
    for block, d in dirs.items():
        p = subprocess.run([os.path.join(F.BIN, "imm3_loader"), "-t", ORDERS, "-c", ORDERS_COLDEF, "-d", d, "-i", csv, "--block-size", str(block), "--segment-size", "2"],
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
    return rows


# ---- the reference: plain Python over the row dicts --------------------------------------------------------------------------------
def narrowed(col, x):
    return (x + 128) % 256 - 128 if col in INT8_COLS else x


def inner_values(db, operand, cache=None):
    table, col, leaves = operand
    cache = {} if cache is None else cache                      # (a sub-query of the sub-query is evaluated once, not once per row)
    return {r[col] for r in db[table] if all(holds(db, l, r, cache) for l in leaves)}


def holds(db, leaf, r, cache=None):
    col, op, x = leaf
    if op == "inq":
        key = repr(x)
        if cache is not None and key in cache:
            return r[col] in cache[key]
        vals = inner_values(db, x, cache)
        if cache is not None:
            cache[key] = vals
        return r[col] in vals
    if op == "in":
        return r[col] in set(x)
    if op == "match":
        return r[col] in x
    t = narrowed(col, x)
    return r[col] > t if op == ">" else (r[col] < t if op == "<" else r[col] == t)


def expected(db, stmt):
    table, leaves, cols, limit = stmt
    cache = {}
    keep = [r for r in db[table] if all(holds(db, l, r, cache) for l in leaves)]
    return [tuple(r[c] for c in cols) for r in (keep[:limit] if limit else keep)]


# ---- the statement as a Query ADT and as SQL ---------------------------------------------------------------------------------------
def _select(leaves):
    def cond(op, x):
        if op == "inq":
            return Q.IntInQuery(Q.Query(x[0], _select(x[2]), Q.Project([x[1]])))
        return {"in": lambda: Q.IntIn(x), "match": lambda: Q.Match(x), ">": lambda: Q.GT(float(x)), "<": lambda: Q.LT(float(x)), "=": lambda: Q.EQ(float(x))}[op]()
    if not leaves:
        return Q.NoSelect
    sel = Q.Select(leaves[0][0], cond(*leaves[0][1:]))
    for (col, op, x) in leaves[1:]:
        sel = Q.And(sel, Q.Select(col, cond(op, x)))
    return sel


def to_query(stmt):
    table, leaves, cols, limit = stmt
    return Q.Query(table, _select(leaves), Q.Project(cols, limit, ()))


def _where(leaves):
    """the where clause, or None when the grammar cannot spell a leaf (a signed threshold, a Match of several values, an empty list)"""
    parts = []
    for (col, op, x) in leaves:
        if op == "inq":
            inner = _where(x[2])
            if inner is None:
                return None
            parts.append(f"{col} in (select {x[1]} from {x[0]}{inner})")
        elif op == "in":
            if not x:
                return None
            parts.append(f"{col} in ({', '.join(str(v) for v in x)})")
        elif op == "match":
            if len(x) != 1:
                return None
            parts.append(f"{col} = '{x[0]}'")
        else:
            if x < 0:
                return None
            parts.append(f"{col} {op} {x}")
    if not parts:
        return ""
    return " where " + (parts[0] if len(parts) == 1 else "(" + " and ".join(parts) + ")")


def to_sql(stmt):
    table, leaves, cols, limit = stmt
    where = _where(leaves)
    if where is None:
        return None
    return f"select {', '.join(cols)} from {table}{where}" + (f" limit {limit}" if limit else "")


# ---- the statements: a dozen fixed ones, then a seeded fuzz --------------------------------------------------------------------------
def fixed_statements():
    P, O = F.TABLE, ORDERS
    return [
        (O, [("cust", "inq", (P, "id", [("state", "match", ["CA"])]))], ["order_id", "cust"], 0),                       # the issue's statement
        (O, [("cust", "inq", (P, "id", [("state", "match", ["CA"]), ("age", ">", 0)])), ("qty", ">", 2)], ["order_id", "qty"], 0),
        (O, [("cust", "inq", (P, "id", []))], ["order_id"], 7),                                                          # an inner query that selects every row
        (O, [("cust", "inq", (P, "id", [("v", ">", 100)]))], ["order_id"], 0),                                           # ... and one that selects nothing
        (P, [("id", "inq", (O, "cust", [("qty", ">", 5)]))], ["id", "state"], 0),                                        # the other way round
        (P, [("id", "inq", (O, "cust", [("region", "match", ["NY"])])), ("id", ">", 1000), ("id", "<", 1200)], ["id"], 0),   # folded with an interval
        (P, [("id", "inq", (O, "cust", [])), ("id", ">", 8000)], ["id"], 0),                                             # an interval above every person's id: nobody
        (P, [("age", "inq", (O, "qty", [("order_id", "<", 100_400)]))], ["id", "age"], 50),                              # int8 probes an int8 set
        (P, [("age", "inq", (O, "cust", [("cust", "<", 200)]))], ["id", "age"], 0),                                      # int8 probes an int32 set: only -128 .. 127 match
        (P, [("order_no", "inq", (O, "qty", [("qty", ">", 0)]))], ["id", "order_no"], 20),                               # int32 probes an int8 set (at most 8 values: the short form)
        (O, [("cust", "inq", (P, "id", [("id", "inq", (O, "cust", [("qty", "=", 127)]))]))], ["order_id", "cust"], 0),   # a sub-query in the sub-query
        (O, [("cust", "inq", (P, "id", [("state", "match", ["TX"])])), ("order_id", "inq", (O, "order_id", [("qty", "<", 0)]))], ["order_id"], 0),   # two sets, two columns
    ]


def draw(rng, db):
    """one fuzzed statement: an outer table, one or two sub-query leaves on its int columns, further plain leaves, a SELECT list, a limit"""
    def plain(table, n):
        out = []
        for _ in range(n):
            r = rng.random()
            if r < 0.75:
                col = str(rng.choice(INT_COLS[table]))
                span = {"id": (-700, 4300), "cust": (-700, 4300), "order_id": (100_000, 103_000)}.get(col, (-5, 60))
                out.append((col, str(rng.choice([">", "<", "="])), int(rng.integers(*span))))
            else:
                out.append((STR_COL[table], "match", [str(rng.choice(F.COMMON_STATES[:5]))]))
        return out
    table = str(rng.choice([F.TABLE, ORDERS]))
    leaves = []
    for _ in range(int(rng.integers(1, 3))):
        if rng.random() < 0.8:                                  # columns whose values meet; else any pair (mostly nothing in common)
            col, inner_table, inner_col = RELATED[table][int(rng.integers(0, len(RELATED[table])))]
        else:
            inner_table = str(rng.choice([F.TABLE, ORDERS]))
            col, inner_col = str(rng.choice(INT_COLS[table])), str(rng.choice(INT_COLS[inner_table]))
        leaves.append((col, "inq", (inner_table, inner_col, plain(inner_table, int(rng.integers(0, 3))))))
    leaves += plain(table, int(rng.integers(0, 3)))
    leaves = [leaves[int(i)] for i in rng.permutation(len(leaves))]
    cols = [str(c) for c in rng.choice(INT_COLS[table], size=int(rng.integers(1, 3)), replace=False)]
    return table, leaves, cols, int(rng.choice([0, 0, 3, 50]))


def one_set_per_column(stmt):
    """the library refuses a second list or set on a column that has a set leaf (include/imm3.h): the fuzz leaves such draws out"""
    cols = [l[0] for l in stmt[1] if l[1] in ("inq", "in")]
    return len(cols) == len(set(cols))


def fuzz_statements(db, n=50, seed=20262):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        st = draw(rng, db)
        if one_set_per_column(st):
            out.append(st)
    return out
