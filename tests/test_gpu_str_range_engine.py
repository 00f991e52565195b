"""GPU suite, end to end: a stored 3-segment table through the Python Engine, the C++ Engine (imm3_sql --string-ranges) and their
SQL spellings of a string range -- `like 'p%'`, `> 'v'`, `< 'v'` -- alone, with `and`, `order by` and `limit`, and under a group-by.
Expected rows are the reference's (rows compared as Python bytes)."""
import os
import subprocess

import numpy as np
import pytest

from immutable3_amd.sql import SQLParser

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "immutable3_amd", "bin")
NAMES = ["Joanna", "Jo", "Jonas", "John", "Mary", "M", "Zed", "Adam", "Moe", "Lz", "Zz", "Jn", "Jp"]
SHAPE = [(2 * 1024 + 1, [1024, 1024, 1]), (1024, [1024]), (1500, [1024, 476])]


@pytest.fixture(scope="module")
def people(tmp_path_factory):
    """id int32, name 8 bytes (the names padded with '0', a character the grammar's value token takes), code 3 bytes, age int8"""
    from immutable3_amd.schema import CodecType, Column, Table, TableIO
    from immutable3_amd.storage import write_segment_arrays
    d = str(tmp_path_factory.mktemp("people"))
    t = Table("people", [Column.make("id", CodecType.DENSE_INT), Column.make("name", CodecType.DENSE_STRING, {"size": "8"}),
                         Column.make("code", CodecType.DENSE_STRING, {"size": "3"}), Column.make("age", CodecType.DENSE_TINYINT)], 1024)
    TableIO.store(d, t)
    rng = np.random.default_rng(808)
    pool = np.frombuffer(b"".join(n.encode().ljust(8, b"0") for n in NAMES), dtype=np.uint8).reshape(-1, 8)
    rows = []
    for s, (n, br) in enumerate(SHAPE):
        ids = (np.arange(n) + s * 10 ** 5).astype(np.int32)
        names = pool[rng.integers(0, len(NAMES), size=n)].copy()
        codes = rng.integers(97, 100, size=(n, 3)).astype(np.uint8)
        ages = rng.integers(0, 100, size=n).astype(np.int8)
        write_segment_arrays(d, t, s, {"id": ids, "name": names, "code": codes, "age": ages}, block_rows=br)
        rows += [(int(ids[r]), bytes(names[r]), bytes(codes[r]), int(ages[r])) for r in range(n)]
    return d, rows


def run_sql(sql, data_dir, *flags):
    r = subprocess.run([os.path.join(BIN, "imm3_sql"), "--string-ranges", "--explain", *flags, "-q", sql, "-d", data_dir], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    paths = [line[len("path: "):] for line in r.stderr.splitlines() if line.startswith("path: ")]
    return r.stdout.splitlines(), paths[0] if paths else None


def pad0(v, width):
    return v.encode().ljust(width, b"\x00")


CASES = [
    # (where clause, predicate over (id, name, code, age), runs as one table query)
    ("name like 'Jo%'", lambda r: r[1].startswith(b"Jo"), True),
    ("name > 'M'", lambda r: r[1] > pad0("M", 8), True),
    ("name < 'M'", lambda r: r[1] < pad0("M", 8), True),
    ("(name > 'Jo' and name < 'Mary0000')", lambda r: pad0("Jo", 8) < r[1] < b"Mary0000", True),
    ("(name like 'M%' and age > 50)", lambda r: r[1].startswith(b"M") and r[3] > 50, True),
    ("(name like 'J%' and name = 'John0000')", lambda r: r[1] == b"John0000", True),
    ("code like 'ab%'", lambda r: r[2].startswith(b"ab"), False),          # a 3-byte column: per-segment queries
    ("(code > 'b' and name like 'Z%')", lambda r: r[2] > b"b\x00\x00" and r[1].startswith(b"Z"), False),
]


@pytest.mark.parametrize("where,pred,one_table", CASES)
def test_both_engines_and_the_cli(people, where, pred, one_table):
    from immutable3_amd.operators import Engine, GpuSegmentManager
    from immutable3_amd.storage import SegmentManager
    d, rows = people
    keep = [r for r in rows if pred(r)]
    assert 0 < len(keep) < len(rows)
    by_name = sorted(keep, key=lambda r: (r[1], r[0]))          # ids ascend with (segment, row)
    statements = [
        (f"select id, name from people where {where}", [(r[0], r[1].decode()) for r in keep], False),
        (f"select id, name from people where {where} limit 7", [(r[0], r[1].decode()) for r in keep[:7]], False),
        (f"select name, id from people where {where} order by name limit 9", [(r[1].decode(), r[0]) for r in by_name[:9]], True),
    ]
    gsm = GpuSegmentManager(SegmentManager(d))
    try:
        eng = Engine(gsm)
        for sql, want, ordered in statements:
            q = SQLParser.parseAll(sql, order_by=True, string_ranges=True)
            assert [tuple(r) for r in eng.execute(q)] == want, sql
            assert (eng._table_plan(q) is not None) == one_table
            got, path = run_sql(sql, d, "--order-by")
            assert got == ["Row(" + ",".join(str(x) for x in w) + ")" for w in want], sql
            if not ordered:
                assert (path == "one table query") == one_table and (one_table or path.startswith("per-segment queries")), (sql, path)
        # under a group-by: count per name
        gsql = f"select count(id) from people where {where} group by name"
        counts = {}
        for r in keep:
            counts[r[1].decode()] = counts.get(r[1].decode(), 0) + 1
        got = eng.execute_agg(SQLParser.parseAll(gsql, string_ranges=True))
        assert {k: [a.get() for a in m.values()] for k, m in got.items()} == {k: [c] for k, c in counts.items()} and list(got) == list(counts)
        rows_g, _ = run_sql(gsql, d)
        assert rows_g == [f"Row({c})" for c in counts.values()]
    finally:
        gsm.close()


def test_flag_off_the_cli_refuses_the_spellings(people):
    d, _ = people
    r = subprocess.run([os.path.join(BIN, "imm3_sql"), "-q", "select id from people where name like 'Jo%'", "-d", d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "failure:" in r.stdout
