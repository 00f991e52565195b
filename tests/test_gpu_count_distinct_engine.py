"""GPU suite: count(distinct f) through the engines, over the committed tables under tests/golden (read only): test_100 -- one segment,
so ONE query answers -- through the Python Engine, the C++ Engine behind imm3_sql and its --count-distinct flag, each against plain
Python over the rows; quirk_25 -- three segments that do not make a table -- for the refusal, device_merge=True included."""
import os
import subprocess

import pytest

from immutable3_amd import synth
from immutable3_amd.sql import SQLParser

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "immutable3_amd", "bin")
REFUSAL = "count(distinct) runs as one table query only"


def rows_100():
    t = synth.test_100()
    return [{"id": int(t["id"][i]), "age": int(t["age"][i]), "state": bytes(t["state"][i]).decode()} for i in range(100)]


# (sql, where, group column, distinct column, having threshold, order: "figure" | the group column, limit)
STATEMENTS = [
    ("select count(distinct age), count(id) from test_100 where id > 10 group by state having count(distinct age) > 12 "
     "order by count(distinct age) desc, state limit 4", lambda r: r["id"] > 10, "state", "age", 12, "figure", 4),
    ("select count(distinct state), count(id) from test_100 group by age having state_distinct > 1 order by age desc limit 5",
     lambda r: True, "age", "state", 1, "age", 5),
]


def expected(where, group, col, t, order, limit):
    """[(group value, figure, count)] in the statement's order, in plain Python"""
    groups = {}
    for r in rows_100():
        if where(r):
            groups.setdefault(r[group], []).append(r)
    out = [(k, len(set(r[col] for r in rs)), len(rs)) for k, rs in groups.items()]
    every = len(out)
    out = [g for g in out if g[1] > t]
    assert 0 < len(out) < every                   # the having keeps some groups and drops some
    out.sort(key=(lambda g: (-g[1], g[0])) if order == "figure" else (lambda g: -g[0]))
    return out[:limit]


def test_the_second_statement_has_figures_that_differ_from_the_counts_of_other_groups():
    want = expected(*STATEMENTS[1][1:])
    assert want and all(f == 2 and c == 2 for (_, f, c) in want)      # (ages shared by two rows of different states)


@pytest.mark.parametrize("case", range(len(STATEMENTS)))
def test_python_engine(case):
    from immutable3_amd.operators import CountDistinctAggr, Engine, GpuSegmentManager
    from immutable3_amd.storage import SegmentManager
    sql, where, group, col, t, order, limit = STATEMENTS[case]
    want = expected(where, group, col, t, order, limit)
    q = SQLParser.parseAll(sql, group_order=True, having=True, count_distinct=True)
    gsm = GpuSegmentManager(SegmentManager(GOLDEN))
    try:
        for device_merge in (False, True):        # ONE query answers: device_merge has nothing to merge
            res = Engine(gsm, device_merge=device_merge).execute_agg(q)
            assert [(k, m[f"{col}_distinct"].get(), m["id_count"].get()) for k, m in res.items()] == [(str(k), f, c) for (k, f, c) in want]
            assert all(isinstance(m[f"{col}_distinct"], CountDistinctAggr) and m[f"{col}_distinct"].repr() == str(m[f"{col}_distinct"].get()) for m in res.values())
        rows = [tuple(r) for r in Engine(gsm).execute(q)]
        assert rows == [(str(f), str(c)) for (_, f, c) in want]
    finally:
        gsm.close()


def run_sql(sql, *flags):
    return subprocess.run([os.path.join(BIN, "imm3_sql"), *flags, "--explain", "-q", sql, "-d", GOLDEN], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("case", range(len(STATEMENTS)))
def test_cpp_engine_behind_the_cli(case):
    sql, where, group, col, t, order, limit = STATEMENTS[case]
    want = expected(where, group, col, t, order, limit)
    r = run_sql(sql, "--count-distinct", "--having", "--order-by")
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == [f"Row({f},{c})" for (_, f, c) in want]
    assert "path: one table query" in r.stderr
    r = run_sql(sql, "--having", "--order-by")            # without the flag: the parse failure it has always been
    assert r.returncode != 0 and "`)' expected" in (r.stdout + r.stderr)


def test_several_segments_are_refused():
    from immutable3_amd.operators import Engine, GpuSegmentManager
    from immutable3_amd.storage import SegmentManager
    sql = "select count(distinct age), count(id) from quirk_25 group by state"
    q = SQLParser.parseAll(sql, count_distinct=True)
    gsm = GpuSegmentManager(SegmentManager(GOLDEN))
    try:
        assert gsm.device_table("quirk_25") is None and gsm.getTableSegmentCount("quirk_25") == 3
        for device_merge in (True, False):
            with pytest.raises(Exception) as e:
                Engine(gsm, device_merge=device_merge).execute_agg(q)
            assert str(e.value).startswith(REFUSAL), str(e.value)
        # the same statement without the new aggregate still runs per segment
        plain = SQLParser.parseAll("select count(age), count(id) from quirk_25 group by state")
        assert sum(m["id_count"].get() for m in Engine(gsm, device_merge=True).execute_agg(plain).values()) == 25
    finally:
        gsm.close()
    r = run_sql(sql, "--count-distinct")
    assert r.returncode != 0 and REFUSAL in (r.stdout + r.stderr)
