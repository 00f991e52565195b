"""ORDER BY through the Python Engine on the GPU: one ordered table query when the table takes the query, per-segment ordered queries
and the stable host merge when it does not, and ProjectOp over a non-fusable upstream (the host sort) -- against numpy over the
segments' arrays: lexsort by the keys, then (segment, row)."""
import numpy as np
import pytest

from immutable3_amd import GT, LT, And, Project, Query, Row, Select
from immutable3_amd import synth
from immutable3_amd.schema import TableIO
from immutable3_amd.storage import SegmentManager, write_segment_arrays

pytestmark = pytest.mark.gpu
ROWS = (2049, 1024, 3000)


def make_table(path, name, block_size):
    t = synth.table_schema(name, block_size)
    TableIO.store(str(path), t)
    allc = []
    for s, n in enumerate(ROWS):
        age = synth.uniform_below(700 + s, n, 100, np.int8)
        age[:30] = 25
        age[-30:] = 25                                                    # equal keys on both sides of every segment boundary
        cols = {"id": np.random.default_rng(800 + s).integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64).astype(np.int32),
                "age": age, "state": synth.state_codes(900 + s, n)}
        write_segment_arrays(str(path), t, s, cols)
        allc.append(cols)
    return allc


def expected(allc, order_by, limit):
    """rows (id, state bytes, age) of `select id, state, age where age > 18 and age < 30 order by ...`, plus (segment, row)"""
    seg = np.concatenate([np.full(c["id"].size, s) for s, c in enumerate(allc)])
    row = np.concatenate([np.arange(c["id"].size) for c in allc])
    ids, age, st = (np.concatenate([c[k] for c in allc]) for k in ("id", "age", "state"))
    keep = np.flatnonzero((age > 18) & (age < 30))
    keys = []
    for col, desc in order_by:                                            # most significant first
        vs = [st[keep, 0].astype(np.int64), st[keep, 1].astype(np.int64)] if col == "state" else [(ids if col == "id" else age)[keep].astype(np.int64)]
        keys += [-v if desc else v for v in vs]
    perm = keep[np.lexsort(tuple([row[keep], seg[keep]] + keys[::-1]))]
    perm = perm[:limit] if limit > 0 else perm
    return seg[perm], row[perm], [Row(int(ids[i]), bytes(st[i]).decode(), int(age[i])) for i in perm]


CASES = [([("age", True)], 0), ([("age", True)], 10), ([("state", False), ("age", True)], 100), ([("id", True)], 7), ([("age", False), ("id", False)], 0)]
WHERE = And(Select("age", GT(18)), Select("age", LT(30)))


@pytest.mark.parametrize("block_size,table_path", [(1024, True), (1000, False)])
def test_engine_execute_ordered(tmp_path, block_size, table_path):
    """block size 1024: the table is one scan unit, one ordered table query; block size 1000 (blocks that are no multiple of 64 rows):
    no device table, so per-segment ordered queries, each with the limit, and the host merge."""
    from immutable3_amd.operators import Engine, GpuSegmentManager
    allc = make_table(tmp_path, "to", block_size)
    g = GpuSegmentManager(SegmentManager(str(tmp_path)))
    try:
        assert (g.device_table("to") is not None) == table_path
        for order_by, limit in CASES:
            q = Query("to", WHERE, Project(["id", "state", "age"], limit, order_by))
            wseg, wrow, wrows = expected(allc, order_by, limit)
            assert list(Engine(g).execute(q)) == wrows, (order_by, limit)
            fused = Engine(g).execute_table_columns(q)
            assert (fused is not None) == table_path
            if fused is not None:
                assert fused[0].tolist() == wseg.tolist() and fused[1].tolist() == wrow.tolist()
        # without an order nothing changes: ascending (segment, row), the limit stops the scan
        plain = list(Engine(g).execute(Query("to", WHERE, Project(["id", "state", "age"], 10))))
        assert plain == expected(allc, [], 10)[2]
    finally:
        g.close()


def test_project_op_orders_a_non_fusable_upstream_on_the_host(tmp_path):
    from immutable3_amd.operators import ColumnVectorOperator, GpuSegmentManager, ProjectOp, ScanOp, SelectOp
    allc = make_table(tmp_path, "th", 1024)
    g = GpuSegmentManager(SegmentManager(str(tmp_path)))
    try:
        t = g.getTable("th")
        used = [t.getColumn("age"), t.getColumn("id"), t.getColumn("state")]

        class Replay(ColumnVectorOperator):                               # stands for ResultQueueOp: batches from several segments
            def __init__(self, ops):
                self.ops = ops

            def iterator(self):
                for o in self.ops:
                    yield from o.iterator()

        ops = [SelectOp("age", LT(30), SelectOp("age", GT(18), ScanOp(g, s, "th", used))) for s in range(len(ROWS))]
        for order_by, limit in CASES:
            rows = list(ProjectOp(["id", "state", "age"], Replay(ops), limit, order_by).iterator())
            assert rows == expected(allc, order_by, limit)[2], (order_by, limit)
    finally:
        g.close()
