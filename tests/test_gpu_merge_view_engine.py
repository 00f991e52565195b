"""GPU suite: views of merged groups through Engine.execute_agg.  The loader-made rows of test_gpu_group_order_engine.py with a 12-byte
name, as three segments that no table query answers: spread over two contexts (blocks of 1024 rows; the single-process merge) and
ragged on one context (blocks of 1000 rows; the one-rank merge, its view on the device).  Statements with having / order by / limit
through Engine(device_merge=True) -- the merge's own view, Engine.last_merge_view == "device" -- and device_merge=False -- the host's
filter_groups / order_groups -- must give equal dicts in equal order, equal to the plain-Python expectation over the rows.  A 12-byte
order key leaves no room for the segment byte of the tie: the library refuses the view and the engine orders on the host."""
import os
import subprocess

import pytest

from immutable3_amd import Count, Max, Min, NoSelect, ProjectAgg, Query, native
from test_gpu_group_filter_engine import adt, expected
from test_gpu_group_order_engine import BIN, as_plain, make_rows

pytestmark = pytest.mark.gpu

# (aggregates as (kind, column), group by, having as nested tuples or None, order by, limit)
EVERY = ("id_count", ">", 0)
CASES = [
    ([("count", "id"), ("max", "age")], ["state"], ("id_count", ">", 420), [("id_count", True)], 3),
    ([("count", "id"), ("min", "id")], ["state", "age"], ("and", ("id_count", ">", 55), ("id_min", "<", 0)), [("age", True), ("id_count", False)], 7),
    ([("count", "id"), ("min", "id"), ("max", "id")], ["state"],
     ("or", ("and", ("id_max", "<", 4895), ("id_count", ">", 420)), ("or", ("id_max", "=", 4899), ("id_count", "<", 400))), [("state", True)], 0),
    ([("max", "name"), ("count", "id")], ["state"], ("id_count", ">", 410), [("id_count", True), ("state", False)], 0),     # a wide string MAX rides along
    ([("count", "id")], ["state"], ("id_count", ">", 400), [], 4),                                                          # a limit without an order
    ([("count", "id"), ("max", "age")], ["state"], None, [("age_max", False), ("state", True)], 5),                         # no having: ties on age_max
]
HOST_CASE = ([("max", "name"), ("count", "id")], ["state"], ("id_count", ">", 410), [("name_max", True)], 0)                # 12 + 1 + 4 > 16


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    rows = make_rows()
    for r in rows:
        r["name"] = f"{r['name']}-{r['state']}x"                       # 8 + 4 = 12 bytes
    base = tmp_path_factory.mktemp("merge_view")
    csv = base / "people.csv"
    with open(csv, "w") as f:
        f.write("id,state,name,age\n")
        for r in rows:
            f.write(f"{r['id']},{r['state']},{r['name']},{r['age']}\n")
    dirs = {}
    for block in (1024, 1000):
        d = base / f"data{block}"
        d.mkdir()
        p = subprocess.run([os.path.join(BIN, "imm3_loader"), "-t", "people", "-c", "id:DENSE_INT,state:DENSE_STRING:size=2,name:DENSE_STRING:size=12,age:DENSE_TINYINT",
                            "-d", str(d), "-i", str(csv), "--block-size", str(block), "--segment-size", "2"], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        dirs[block] = str(d)
    return rows, dirs


def mk_query(aggs, group, having, order_by, limit):
    mk = {"count": Count, "max": Max, "min": Min}
    return Query("people", NoSelect, ProjectAgg([mk[k](c) for (k, c) in aggs], group, order_by, limit, having=adt(having) if having else None))


def both_engines(dirs, block, n_ctx, case):
    """(device_merge=True's result, its last_merge_view, device_merge=False's result) as plain lists"""
    from immutable3_amd.operators import Engine, GpuSegmentManager
    from immutable3_amd.storage import SegmentManager
    ctxs = [native.Context(0) for _ in range(n_ctx)]
    gsm = GpuSegmentManager(SegmentManager(dirs[block]), ctxs)
    try:
        assert gsm.getTableSegmentCount("people") == 3 and gsm.device_table("people") is None
        dev = Engine(gsm, device_merge=True)
        got = dev.execute_agg(mk_query(*case))
        host = Engine(gsm, device_merge=False)
        return as_plain(got), dev.last_merge_view, as_plain(host.execute_agg(mk_query(*case))), host.last_merge_view
    finally:
        gsm.close()
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("block,n_ctx", [(1024, 2), (1000, 1)], ids=["two contexts", "one context"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_the_view_of_the_merge_is_what_the_host_gives(tables, case, block, n_ctx):
    rows, dirs = tables
    aggs, group, having, order_by, limit = CASES[case]
    want = expected(rows, aggs, group, having or EVERY, order_by, limit)
    assert len(want) > 1
    got, who, host, host_who = both_engines(dirs, block, n_ctx, CASES[case])
    assert who == "device" and host_who is None
    assert got == host and got == want


def test_a_twelve_byte_order_key_is_refused_and_ordered_on_the_host(tables):
    rows, dirs = tables
    aggs, group, having, order_by, limit = HOST_CASE
    want = expected(rows, aggs, group, having, order_by, limit)
    assert len(want) > 1
    for block, n_ctx in ((1024, 2), (1000, 1)):
        got, who, host, _ = both_engines(dirs, block, n_ctx, HOST_CASE)
        assert who == "host" and got == host and got == want
