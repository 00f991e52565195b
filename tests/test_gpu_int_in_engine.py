"""GPU suite: IntIn above the C ABI.  200 seeded statements -- one or two IN-lists of 0 .. 40 values on the int32 / int8 columns of the
statement fuzz's table (tests/stmt_fuzz_util.py: 5000 rows, three segments), about half the values present, beside optional GT / LT /
EQ / Match leaves, a SELECT list and a limit -- through the Python Engine over blocks of 1024 (ONE table query) and of 1000 (ragged:
per-segment queries through the word-at-a-time kernel), against plain Python over the row dicts; EVERY statement the grammar can spell
through host/operators.hpp's Engine as well (tests/native/int_in_batch.cpp: one child process per block size), and four of them through
imm3_sql --int-lists itself.  The GROUP BY form and the refusal of a list under an honoured OR go through both paths too."""
import os
import subprocess

import numpy as np
import pytest

import stmt_fuzz_util as F
from immutable3_amd import query as Q

pytestmark = pytest.mark.gpu
INT_COLS = ("id", "v", "age", "order_no")


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    rows, dirs, _ = F.make_tables(tmp_path_factory.mktemp("int_in_engine"))
    return rows, dirs


@pytest.fixture(scope="module")
def managers(tables):
    from immutable3_amd.operators import GpuSegmentManager
    from immutable3_amd.storage import SegmentManager
    _, dirs = tables
    one, ragged = GpuSegmentManager(SegmentManager(dirs[1024])), GpuSegmentManager(SegmentManager(dirs[1000]))
    assert one.device_table(F.TABLE) is not None and ragged.device_table(F.TABLE) is None
    yield {"table": one, "per segment": ragged}
    one.close()
    ragged.close()


def draw(rng, rows):
    """(leaves [(col, op, operand)], SELECT list, limit)"""
    leaves = []
    for _ in range(int(rng.integers(1, 3))):
        col = str(rng.choice(INT_COLS))
        k = int(rng.integers(0, 41))
        vals = []
        for _ in range(k):
            if rng.random() < 0.5:
                vals.append(int(rows[int(rng.integers(0, len(rows)))][col]))
            else:
                vals.append(int(rng.choice([-(1 << 31), (1 << 31) - 1, -129, 128, 5000 + int(rng.integers(0, 900)), -701 - int(rng.integers(0, 900))])))
        leaves.append((col, "in", vals))
    for _ in range(int(rng.integers(0, 3))):
        r = rng.random()
        if r < 0.7:
            col = str(rng.choice(INT_COLS))
            leaves.append((col, str(rng.choice([">", "<", "="])), int(rng.integers(-5, 60) if col != "id" else rng.integers(-700, 4300))))
        else:
            leaves.append(("state", "match", [str(s) for s in rng.choice(F.STATES, size=int(rng.integers(1, 4)), replace=False)]))
    leaves = [leaves[int(i)] for i in rng.permutation(len(leaves))]
    cols = [str(c) for c in rng.choice(INT_COLS, size=int(rng.integers(1, 4)), replace=False)]
    return leaves, cols, int(rng.choice([0, 0, 3, 50]))


def holds(leaf, r):
    col, op, x = leaf
    if op == "in":
        return r[col] in set(x)
    if op == "match":
        return r[col] in x
    t = F.narrowed(col, x)
    return r[col] > t if op == ">" else (r[col] < t if op == "<" else r[col] == t)


def to_query(leaves, cols, limit):
    def cond(op, x):
        return {"in": lambda: Q.IntIn(x), "match": lambda: Q.Match(x), ">": lambda: Q.GT(float(x)), "<": lambda: Q.LT(float(x)), "=": lambda: Q.EQ(float(x))}[op]()
    sel = Q.Select(leaves[0][0], cond(*leaves[0][1:]))
    for (col, op, x) in leaves[1:]:
        sel = Q.And(sel, Q.Select(col, cond(op, x)))
    return Q.Query(F.TABLE, sel, Q.Project(cols, limit, ()))


def to_sql(leaves, cols, limit):
    def one(col, op, x):
        if op == "in":
            return f"{col} in ({', '.join(str(v) for v in x)})" if x else None
        if op == "match":
            return f"{col} = '{x[0]}'" if len(x) == 1 else None
        return f"{col} {op} {x}" if x >= 0 else None                    # (the grammar's value has no sign)
    parts = [one(*l) for l in leaves]
    if any(p is None for p in parts):
        return None
    where = parts[0] if len(parts) == 1 else "(" + " and ".join(parts) + ")"
    return f"select {', '.join(cols)} from {F.TABLE} where {where}" + (f" limit {limit}" if limit else "")


def statements(rows):
    rng = np.random.default_rng(20261)
    return [draw(rng, rows) for _ in range(200)]


def expected(rows, leaves, cols, limit):
    keep = [r for r in rows if all(holds(l, r) for l in leaves)]
    return [tuple(r[c] for c in cols) for r in (keep[:limit] if limit else keep)]


def test_python_engine_table_plan_and_per_segment(tables, managers):
    from immutable3_amd.operators import Engine
    rows, _ = tables
    selected = 0
    for k, (leaves, cols, limit) in enumerate(statements(rows)):
        want = expected(rows, leaves, cols, limit)
        selected += bool(want)
        q = to_query(leaves, cols, limit)
        for name, gsm in managers.items():
            engine = Engine(gsm)
            assert [tuple(r) for r in engine.execute(q)] == want, (k, name, leaves, cols, limit)
            assert (engine.execute_table_columns(q) is not None) == (name == "table"), (k, name)
    assert selected >= 60                                               # (the lists do select rows)


def test_group_by_and_the_refusal_under_an_honoured_or(tables, managers):
    from immutable3_amd.operators import Engine
    rows, _ = tables
    ids = [r["id"] for r in rows[::7]] + [99999]
    want = {}
    for r in rows:
        if r["id"] in set(ids) and r["age"] > -2:
            c, m = want.get(r["state"], (0, None))
            want[r["state"]] = (c + 1, r["v"] if m is None else max(m, r["v"]))
    sel = Q.And(Q.Select("id", Q.IntIn(ids)), Q.Select("age", Q.GT(-2.0)))
    for name, gsm in managers.items():
        got = Engine(gsm).execute_agg(Q.Query(F.TABLE, sel, Q.ProjectAgg([Q.Count("id"), Q.Max("v")], ["state"])))
        plain = {k: tuple(a.get() for a in m.values()) for k, m in got.items()}
        assert {k: (int(c), int(v)) for k, (c, v) in plain.items()} == want, name
        tree = Q.Or(Q.Select("id", Q.IntIn([1, 2])), Q.Select("age", Q.GT(2.0)))
        assert [tuple(r) for r in Engine(gsm).execute(Q.Query(F.TABLE, tree, Q.Project(["id"], 0, ())))] == \
            [(r["id"],) for r in rows if r["id"] in (1, 2) and r["age"] > 2]   # the reference's conjunction: OR ignored
        with pytest.raises(Exception, match="IMM3_INT_IN"):               # honoured: the program has an OR and a list
            list(Engine(gsm, honour_and_or=True).execute(Q.Query(F.TABLE, tree, Q.Project(["id"], 0, ()))))


def test_cpp_engine_every_spellable_statement_and_imm3_sql(tables, tmp_path):
    rows, dirs = tables
    spellable = [(s, to_sql(*s)) for s in statements(rows)]
    spellable = [(s, sql) for (s, sql) in spellable if sql is not None]
    assert len(spellable) >= 40
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, lib = str(tmp_path / "int_in_batch"), os.path.join(root, "immutable3_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O0", os.path.join(root, "tests", "native", "int_in_batch.cpp"), "-o", exe, "-L", lib, "-limm3", f"-Wl,-rpath,{lib}"])
    listing = tmp_path / "statements.sql"
    listing.write_text("".join(sql + "\n" for _, sql in spellable))
    for block in F.BLOCKS:
        p = subprocess.run([exe, dirs[block], str(listing)], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (block, p.returncode, p.stdout[-1500:], p.stderr[-1500:])
        got, cur = {}, None
        for ln in p.stdout.splitlines():
            if ln.startswith("== "):
                k, head = ln[3:].split(" ", 1)
                cur = got.setdefault(int(k), (head, []))
            else:
                cur[1].append(ln)
        assert sorted(got) == list(range(1, len(spellable) + 1))
        for k, ((leaves, cols, limit), sql) in enumerate(spellable):
            head, lines = got[k + 1]
            assert lines == ["Row(" + ",".join(str(x) for x in t) + ")" for t in expected(rows, leaves, cols, limit)], (block, sql)
            assert head.startswith("path: one table query" if block == 1024 else "path: per-segment queries"), (block, sql, head)
    picked = [x for x in spellable if expected(rows, *x[0])][:3] + [x for x in spellable if not expected(rows, *x[0])][:1]
    assert len(picked) == 4
    for n, ((leaves, cols, limit), sql) in enumerate(picked):
        block = F.BLOCKS[n % 2]
        want = ["Row(" + ",".join(str(x) for x in t) + ")" for t in expected(rows, leaves, cols, limit)]
        p = subprocess.run([os.path.join(F.BIN, "imm3_sql"), "--int-lists", "--explain", "-q", sql, "-d", dirs[block]], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and p.stdout.splitlines() == want, (sql, block, p.stdout[-1500:], p.stderr[-1500:])
        assert ("path: one table query" in p.stderr) == (block == 1024), (sql, p.stderr)
    off = subprocess.run([os.path.join(F.BIN, "imm3_sql"), "-q", picked[0][1], "-d", dirs[1024]], capture_output=True, text=True, timeout=120)
    assert off.returncode == 1 and "failure:" in off.stdout               # without the switch the statement does not parse
