"""GPU suite: ORDER BY over groups through Engine.execute_agg, over a loader-made table of three small segments.  The ordered table query
(blocks of 1024 rows: the table takes the query), the per-segment fallback (blocks of 1000 rows: no uniform layout, no table) and
device_merge=True must return the same ordered groups; a limit cuts after the order.  The expectation is plain Python: the groups in
first-seen order, then one stable sort per key from the least significant one up."""
import os
import subprocess

import numpy as np
import pytest

from immutable3_amd import Count, Max, Min, NoSelect, ProjectAgg, Query, Select
from immutable3_amd.query import GT
from test_gpu_agg_wide_key import STATES, name_pool

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "immutable3_amd", "bin")
N = 5_000

# (aggregates as (kind, column), group by, order by, limit)
CASES = [
    ([("count", "id"), ("max", "age")], ["state"], [("id_count", True)], 5),
    ([("count", "id"), ("max", "age")], ["state"], [("age_max", True), ("state", False)], 0),
    ([("count", "id"), ("min", "id")], ["state", "age"], [("age", True), ("id_count", False)], 7),
    ([("max", "name"), ("count", "id")], ["state"], [("name_max", True)], 0),
    ([("count", "id"), ("max", "age")], ["state"], [("age_max", False)], 3),       # few distinct maxima: ties in first-seen order
    ([("count", "id")], ["state"], [], 4),                                          # a limit without an order: first-seen order, cut
]


def make_rows():
    rng = np.random.default_rng(77)
    st = [bytes(s).decode() for s in STATES[rng.integers(0, 12, size=N)]]
    names = [bytes(s).decode() for s in name_pool(rng, 30, 8)[rng.integers(0, 30, size=N)]]
    ages = rng.integers(-3, 4, size=N).tolist()
    return [{"id": i - 100, "state": st[i], "name": names[i], "age": ages[i]} for i in range(N)]


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """{block size: data directory} of the same 5000 rows: 1024 (three segments a table takes), 1000 (three segments it does not)"""
    rows = make_rows()
    base = tmp_path_factory.mktemp("group_order")
    csv = base / "people.csv"
    with open(csv, "w") as f:
        f.write("id,state,name,age\n")
        for r in rows:
            f.write(f"{r['id']},{r['state']},{r['name']},{r['age']}\n")
    dirs = {}
    for block in (1024, 1000):
        d = base / f"data{block}"
        d.mkdir()
        p = subprocess.run([os.path.join(BIN, "imm3_loader"), "-t", "people", "-c", "id:DENSE_INT,state:DENSE_STRING:size=2,name:DENSE_STRING:size=8,age:DENSE_TINYINT",
                            "-d", str(d), "-i", str(csv), "--block-size", str(block), "--segment-size", "2"], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        dirs[block] = str(d)
    return rows, dirs


def expected(rows, aggs, group, order_by, limit, keep=lambda r: True, batch_cols=("id", "state", "name", "age")):
    """[(group key, {alias: value})] in the order asked for.  The key joins the group columns in BATCH-column order -- Engine.getColumns:
    the aggregates' columns, then the group-by columns, first mention first."""
    used = []
    for c in [c for (_, c) in aggs] + list(group):
        if c not in used:
            used.append(c)
    gcols = [c for c in used if c in group]
    groups = {}
    for r in rows:
        if not keep(r):
            continue
        key = "_".join(str(r[c]) for c in gcols)
        g = groups.setdefault(key, {"__cols": {c: r[c] for c in gcols}})
        for (kind, c) in aggs:
            alias = f"{c}_{kind}"
            if kind == "count":
                g[alias] = g.get(alias, 0) + 1
            elif kind == "max":
                g[alias] = max(g.get(alias, r[c]), r[c])
            else:
                g[alias] = min(g.get(alias, r[c]), r[c])
    order = list(groups)
    for (name, desc) in reversed(order_by):             # stable sorts from the least significant key up; reverse=True keeps ties in place
        order.sort(key=lambda k: groups[k]["__cols"][name] if name in groups[k]["__cols"] else groups[k][name], reverse=desc)
    if limit > 0:
        order = order[:limit]
    return [(k, {a: v for a, v in groups[k].items() if a != "__cols"}) for k in order]


def mk_query(aggs, group, order_by, limit, select=NoSelect):
    mk = {"count": Count, "max": Max, "min": Min}
    return Query("people", select, ProjectAgg([mk[k](c) for (k, c) in aggs], group, order_by, limit))


def as_plain(result):
    return [(k, {a: (x.get() if not isinstance(x.get(), float) else int(x.get())) for a, x in m.items()}) for k, m in result.items()]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_three_paths_agree(tables, case):
    from immutable3_amd.operators import Engine, GpuSegmentManager
    from immutable3_amd.storage import SegmentManager
    rows, dirs = tables
    aggs, group, order_by, limit = CASES[case]
    want = expected(rows, aggs, group, order_by, limit)
    assert len(want) > 1
    for block, device_merge in ((1024, False), (1000, False), (1000, True)):
        gsm = GpuSegmentManager(SegmentManager(dirs[block]))
        try:
            assert gsm.getTableSegmentCount("people") == 3
            assert (gsm.device_table("people") is not None) == (block == 1024)
            got = Engine(gsm, device_merge=device_merge).execute_agg(mk_query(aggs, group, order_by, limit))
            assert as_plain(got) == want, (block, device_merge)
        finally:
            gsm.close()


def test_with_a_select_and_without_clauses(tables):
    from immutable3_amd.operators import Engine, GpuSegmentManager
    from immutable3_amd.storage import SegmentManager
    rows, dirs = tables
    aggs, group = [("count", "id"), ("max", "age")], ["state"]
    for block in (1024, 1000):
        gsm = GpuSegmentManager(SegmentManager(dirs[block]))
        try:
            got = Engine(gsm).execute_agg(mk_query(aggs, group, [("id_count", True), ("state", True)], 6, Select("age", GT(0))))
            assert as_plain(got) == expected(rows, aggs, group, [("id_count", True), ("state", True)], 6, keep=lambda r: r["age"] > 0), block
            plain = Engine(gsm).execute_agg(mk_query(aggs, group, [], 0))       # no clause: first-seen order, every group, as always
            assert as_plain(plain) == expected(rows, aggs, group, [], 0), block
        finally:
            gsm.close()


def test_two_contexts_on_one_device_merge_on_the_device(tables):
    """Several contexts need not mean several devices.  With device_merge=True the Engine's several-context branch used to ask for one
    communicator per DEVICE (Comm.create_all), which refuses two contexts on one device; it now takes each context's own world-of-one
    communicator.  The segments alternate between the contexts, so every group and every tie crosses them.  (Pinned from the statement
    fuzz, test_gpu_stmt_fuzz.py, configuration d.)"""
    from immutable3_amd import native
    from immutable3_amd.operators import Engine, GpuSegmentManager
    from immutable3_amd.query import Project
    from immutable3_amd.storage import SegmentManager
    rows, dirs = tables
    ctxs = [native.Context(0) for _ in range(2)]
    gsm = GpuSegmentManager(SegmentManager(dirs[1024]), ctxs)
    try:
        assert gsm.device_table("people") is None                      # no table over several contexts: per-segment queries
        aggs, group, order_by, limit = CASES[2]
        got = Engine(gsm, device_merge=True).execute_agg(mk_query(aggs, group, order_by, limit))
        assert as_plain(got) == expected(rows, aggs, group, order_by, limit)
        q = Query("people", NoSelect, Project(["age", "id"], 7, [("age", True)]))
        want = sorted(((r["age"], r["id"]) for r in rows), key=lambda t: -t[0])[:7]       # stable: ties in (segment, row)
        assert [tuple(r) for r in Engine(gsm, device_merge=True).execute(q)] == want
    finally:
        gsm.close()
        for c in ctxs:
            c.close()
