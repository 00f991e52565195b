"""imm3_sql --order-by end to end on tests/golden/test_100: SQL text -> parser -> ordered table query on the GPU -> rows, against
tests/order_util.py's rows; and the same statement without the flag, which fails to parse as it always has."""
import os
import subprocess

import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_TINYINT, GT, LT, RawColumn
import order_util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "immutable3_amd", "bin", "imm3_sql")
GOLDEN = os.path.join(ROOT, "tests", "golden")
SQL = "select id, age from test_100 where (age > 18 and age < 30) order by age desc limit 10"


def expected_rows(order_by, limit):
    from immutable3_amd import synth
    t = synth.test_100()
    cols = [RawColumn(DENSE_TINYINT, 1, t["age"], [100]).npcol(), RawColumn(DENSE_INT, 4, t["id"], [100]).npcol()]   # used = [age, id]
    _, vals = order_util.expected(cols, [DENSE_TINYINT, DENSE_INT], [(0, GT, 18.0), (0, LT, 30.0)], [1, 0], order_by, limit)
    ids, ages = vals[0].view("<i4").reshape(-1), vals[1].view(np.int8).reshape(-1)
    return [f"Row({i},{a})" for i, a in zip(ids.tolist(), ages.tolist())]


def test_order_by_rows():
    p = subprocess.run([BIN, "--order-by", "-q", SQL, "-d", GOLDEN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    want = expected_rows([(1, True)], 10)
    assert p.stdout.splitlines() == want and len(want) == 10
    assert want[0] == "Row(54,29)"                                       # age 29 first; the two-key form below breaks its ties by id
    p = subprocess.run([BIN, "--order-by", "-q", SQL.replace("age desc", "age desc, id desc").replace("limit 10", ""), "-d", GOLDEN],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.splitlines() == expected_rows([(1, True), (0, True)], 0)


def test_without_the_flag_the_statement_does_not_parse():
    p = subprocess.run([BIN, "-q", SQL, "-d", GOLDEN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and p.stdout.startswith("[1.60] failure: end of input expected"), p.stdout
