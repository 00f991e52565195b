"""GPU suite: IN (sub-query) above the C ABI.  A dozen fixed statements and 50 seeded ones over two tables (tests/int_in_query_util.py:
`people`, 5000 rows, and `orders`, 3000 rows whose `cust` refers to people.id) through the Python Engine -- blocks of 1024 (the inner
selects AND the outer statement as table queries), blocks of 1000 (ragged: per-segment queries on both sides) and two contexts (no
set can be shared: the inner values fetched, an IntIn leaf instead) --, through host/operators.hpp's Engine (tests/native/
int_in_query_batch.cpp: one child process per block size) and, the fixed ones in both block sizes, through imm3_sql --subqueries itself; against plain Python
over the row dicts.  The aggregation form, execute_columns and the refusals go through the Python engine too."""
import os
import subprocess

import pytest

import int_in_query_util as U
import stmt_fuzz_util as F
from immutable3_amd import native
from immutable3_amd import query as Q

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    base = tmp_path_factory.mktemp("int_in_query")
    people, dirs, _ = F.make_tables(base)
    orders = U.load_orders(base, dirs)
    return {F.TABLE: people, U.ORDERS: orders}, dirs


@pytest.fixture(scope="module")
def managers(tables):
    from immutable3_amd.operators import GpuSegmentManager
    from immutable3_amd.storage import SegmentManager
    _, dirs = tables
    one, ragged = GpuSegmentManager(SegmentManager(dirs[1024])), GpuSegmentManager(SegmentManager(dirs[1000]))
    two = GpuSegmentManager(SegmentManager(dirs[1024]), [native.Context(0), native.Context(0)])
    assert one.device_table(F.TABLE) is not None and one.device_table(U.ORDERS) is not None and ragged.device_table(F.TABLE) is None
    yield {"table": one, "per segment": ragged, "two contexts": two}
    for m in (one, ragged, two):
        m.close()
    for c in two.ctxs:
        c.close()


ROUTE = {"table": "set/table", "per segment": "set/segments", "two contexts": "host"}


def statements(db):
    return U.fixed_statements() + U.fuzz_statements(db)


def test_python_engine_three_routes(tables, managers):
    """(fails without the feature: there is no IntInQuery)"""
    from immutable3_amd.operators import Engine
    db, _ = tables
    selected = nothing = 0
    for k, st in enumerate(statements(db)):
        want = U.expected(db, st)
        selected += bool(want)
        nothing += not want
        q = U.to_query(st)
        n_sub = repr(st).count("'inq'")
        for name, gsm in managers.items():
            engine = Engine(gsm)
            assert [tuple(r) for r in engine.execute(q)] == want, (k, name, st)
            assert engine.lastPath() == ",".join([ROUTE[name]] * n_sub), (k, name, engine.lastPath())
            if name != "two contexts":
                assert (engine.execute_table_columns(q) is not None) == (name == "table"), (k, name)
    assert selected >= 20 and nothing >= 5                                  # (the sub-queries do select rows, and some select none)


def test_the_fixed_statements_say_what_they_claim(tables):
    db, _ = tables
    fixed = U.fixed_statements()
    assert U.expected(db, fixed[0]) and len(U.expected(db, fixed[2])) == 7
    assert U.inner_values(db, fixed[2][1][0][2]) == {r["id"] for r in db[F.TABLE]}           # selects every row
    assert U.inner_values(db, fixed[3][1][0][2]) == set() and U.expected(db, fixed[3]) == []   # selects nothing
    assert U.expected(db, fixed[6]) == [] and U.expected(db, fixed[5]) and U.expected(db, fixed[8]) and U.expected(db, fixed[10])
    assert len(U.inner_values(db, fixed[9][1][0][2])) <= 8


def test_aggregation_columns_and_refusals(tables, managers):
    from immutable3_amd.operators import Engine
    db, _ = tables
    inner = Q.Query(F.TABLE, Q.Select("state", Q.Match(["CA"])), Q.Project(["id"]))
    sel = Q.And(Q.Select("cust", Q.IntInQuery(inner)), Q.Select("qty", Q.GT(-3.0)))
    ca = {r["id"] for r in db[F.TABLE] if r["state"] == "CA"}
    keep = [r for r in db[U.ORDERS] if r["cust"] in ca and r["qty"] > -3]
    want = {}
    for r in keep:
        c, m = want.get(r["region"], (0, None))
        want[r["region"]] = (c + 1, r["qty"] if m is None else max(m, r["qty"]))
    for name, gsm in managers.items():
        got = Engine(gsm).execute_agg(Q.Query(U.ORDERS, sel, Q.ProjectAgg([Q.Count("order_id"), Q.Max("qty")], ["region"])))
        assert {k: (int(m["order_id_count"].get()), int(m["qty_max"].get())) for k, m in got.items()} == want, name
        parts = Engine(gsm).execute_columns(Q.Query(U.ORDERS, sel, Q.Project(["order_id"])))
        assert [int(v) for (_, _, cols) in parts for v in cols[0]] == [r["order_id"] for r in keep], name
    gsm = managers["table"]
    tree = Q.Or(Q.Select("cust", Q.IntInQuery(inner)), Q.Select("qty", Q.GT(2.0)))
    assert [tuple(r) for r in Engine(gsm).execute(Q.Query(U.ORDERS, tree, Q.Project(["order_id"])))] == \
        [(r["order_id"],) for r in db[U.ORDERS] if r["cust"] in ca and r["qty"] > 2]          # the reference's conjunction: OR ignored
    with pytest.raises(Exception, match="IMM3_INT_IN_SET"):                                  # honoured: the program has an OR and a set
        list(Engine(gsm, honour_and_or=True).execute(Q.Query(U.ORDERS, tree, Q.Project(["order_id"]))))
    two = Q.And(Q.Select("cust", Q.IntInQuery(inner)), Q.Select("cust", Q.IntIn([1, 2, 3])))
    with pytest.raises(Exception, match="takes no other"):
        list(Engine(gsm).execute(Q.Query(U.ORDERS, two, Q.Project(["order_id"]))))
    text = Q.Query(F.TABLE, Q.NoSelect, Q.Project(["state"]))
    with pytest.raises(Exception, match="neither int32 nor int8"):
        list(Engine(gsm).execute(Q.Query(U.ORDERS, Q.Select("cust", Q.IntInQuery(text)), Q.Project(["order_id"]))))


def test_cpp_engine_and_imm3_sql(tables, tmp_path):
    db, dirs = tables
    spellable = [(s, U.to_sql(s)) for s in statements(db)]
    spellable = [(s, sql) for (s, sql) in spellable if sql is not None]
    assert len(spellable) >= 30
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, lib = str(tmp_path / "int_in_query_batch"), os.path.join(root, "immutable3_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O0", os.path.join(root, "tests", "native", "int_in_query_batch.cpp"), "-o", exe, "-L", lib, "-limm3", f"-Wl,-rpath,{lib}"])
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
        for k, (st, sql) in enumerate(spellable):
            head, lines = got[k + 1]
            assert lines == ["Row(" + ",".join(str(x) for x in t) + ")" for t in U.expected(db, st)], (block, sql)
            n_sub = sql.count("(select ")
            route = "set/table" if block == 1024 else "set/segments"
            assert head.startswith("path: one table query" if block == 1024 else "path: per-segment queries"), (block, sql, head)
            assert head.endswith("; sub-queries: " + ",".join([route] * n_sub)), (block, sql, head)


@pytest.mark.parametrize("block", F.BLOCKS)
def test_imm3_sql_every_fixed_statement(tables, block):
    """the CLI itself -- its switch, its row output and its --explain line -- over every fixed statement, one process each"""
    db, dirs = tables
    exe = os.path.join(F.BIN, "imm3_sql")
    fixed = [(st, U.to_sql(st)) for st in U.fixed_statements()]
    assert all(sql is not None for _, sql in fixed) and len(fixed) == 12
    route = "set/table" if block == 1024 else "set/segments"
    for st, sql in fixed:
        want = ["Row(" + ",".join(str(x) for x in t) + ")" for t in U.expected(db, st)]
        p = subprocess.run([exe, "--int-lists", "--subqueries", "--explain", "-q", sql, "-d", dirs[block]], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and p.stdout.splitlines() == want, (sql, block, p.stdout[-1500:], p.stderr[-1500:])
        path = [ln for ln in p.stderr.splitlines() if ln.startswith("path: ")]
        assert len(path) == 1 and path[0].startswith("path: one table query" if block == 1024 else "path: per-segment queries"), (sql, p.stderr)
        assert path[0].endswith("; sub-queries: " + ",".join([route] * sql.count("(select "))), (sql, p.stderr)
    off = subprocess.run([exe, "--int-lists", "-q", fixed[0][1], "-d", dirs[block]], capture_output=True, text=True, timeout=120)
    assert off.returncode == 1 and "failure:" in off.stdout                  # without the switch the statement does not parse
