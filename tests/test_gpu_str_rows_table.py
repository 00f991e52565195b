"""GPU suite: Match on string columns whose width is a multiple of 4 over an imm3_table -- ONE k_filter_str_rows launch over the tile
table of all segments must give exactly the per-segment results in segment order: bitmaps per segment, zero padding up to the next
tile, the global count, rows in (segment, row) order under a global limit, groups merged in first-seen order.  Expectations are the C
oracle's and oracle_np's per segment.  What a table still refuses stays refused."""
import os
import subprocess

import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, GT, LT, MATCH, RawColumn, blocks_of
from immutable3_amd import native
from oracle import oracle_np
from str_rows_util import make_strings, pool_for

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "immutable3_amd", "bin")

# tests/test_gpu_table.py's segment shapes: loader-quirk segments, partial last blocks, a tiny and an empty one
SHAPES = [
    [(8 * 1024 + 1, [1024] * 8 + [1]), (8 * 1024 + 1, [1024] * 8 + [1]), (3 * 1024 + 700, [1024] * 3 + [700])],
    [(100, [100]), (0, []), (1, [1]), (64, [64]), (5000, blocks_of(5000, 1024))],
    [(70000, blocks_of(70000, 1024)), (1024, [1024]), (2048, [1024, 1024]), (1025, [1024, 1])],
    [(4 * 64 + 5, [64, 128, 64, 5])],
]


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


class Pools:
    def __init__(self, seed):
        rng = np.random.default_rng(seed)
        self.name, self.n0, self.n1 = pool_for(rng, 16)
        self.code, self.c0, self.c1 = pool_for(rng, 8)
        self.names = [bytes(self.n0), bytes(self.n1)] + [bytes(p) for p in self.name[:4]]
        self.codes = [bytes(self.c0), bytes(self.c1)] + [bytes(p) for p in self.code[:12]]


def make_segment(rng, pools, n, block_rows):
    """id int32, age int8, name 16 bytes, code 8 bytes"""
    ids = rng.integers(-50, 50, size=n).astype(np.int32)
    age = rng.integers(-128, 128, size=n).astype(np.int8)
    return [RawColumn(DENSE_INT, 4, ids, block_rows), RawColumn(DENSE_TINYINT, 1, age, block_rows),
            RawColumn(DENSE_STRING, 16, make_strings(rng, pools.name, n), block_rows),
            RawColumn(DENSE_STRING, 8, make_strings(rng, pools.code, n), block_rows)]


def make_table(ctx, shape, seed):
    pools = Pools(seed)
    rng = np.random.default_rng(seed + 1)
    segs_cols = [make_segment(rng, pools, n, br) for n, br in shape]
    dsegs = [native.DeviceSegment(ctx, [c.native() for c in cols]) for cols in segs_cols]
    return pools, segs_cols, dsegs, native.DeviceTable(ctx, dsegs)


def expected(oracle, segs_cols, used, sels, proj):
    """per segment: (bitmap words, count), and all rows as (segment, row, [value bytes])"""
    per_seg, rows = [], []
    for si, cols in enumerate(segs_cols):
        ocols = [cols[i].ocol() for i in used]
        ow, oc = oracle.scan_select(ocols, sels, 1024, 1)
        per_seg.append((ow, oc))
        if proj:
            osize, _, _, _ = oracle.layout(ocols[0], 1024)
            n, batch, pos, ovals, _ = oracle.project(ocols, proj, 0, 1024, ow)
            starts = np.concatenate([[0], np.cumsum(osize.astype(np.int64))])
            rows += [(si, int(starts[batch[r]] + pos[r]), [bytes(v[r]) for v in ovals]) for r in range(n)]
    return per_seg, rows


def check_select(q, per_seg):
    words, count = q.bitmap(), q.count()
    fb, fw = q.segment_starts()
    for si, (ow, oc) in enumerate(per_seg):
        assert words[int(fw[si]): int(fw[si]) + ow.size].tolist() == ow.tolist(), si
        assert not words[int(fw[si]) + ow.size: int(fw[si + 1])].any(), si          # padding up to the next tile
    assert count == sum(oc for _, oc in per_seg)


def check_rows(q, proj, exp_rows):
    idx, vals = q.fetch_rows()
    seg_of, row_of = q.locate_rows(idx)
    assert idx.shape[0] == len(exp_rows)
    assert seg_of.tolist() == [e[0] for e in exp_rows] and row_of.tolist() == [e[1] for e in exp_rows]
    for j in range(len(proj)):
        assert [bytes(v) for v in vals[j]] == [e[2][j] for e in exp_rows]


@pytest.mark.parametrize("shape", SHAPES)
def test_table_query_equals_per_segment(ctx, oracle, shape):
    pools, segs_cols, dsegs, table = make_table(ctx, shape, len(shape) * 31 + shape[0][0])
    queries = [
        ([2, 0], [(0, MATCH, pools.names)], [1, 0]),
        ([3, 0], [(0, MATCH, pools.codes)], [1]),
        ([0, 2, 1], [(0, GT, -30.0), (1, MATCH, pools.names), (2, LT, 100.0)], [0, 1, 2]),
        ([2, 3, 0], [(0, MATCH, pools.names + [bytes(p) for p in pools.name[4:14]]), (1, MATCH, pools.codes)], [2, 1]),
    ]
    for used, sels, proj in queries:
        per_seg, rows = expected(oracle, segs_cols, used, sels, proj)
        # limits: none, in the middle of a segment, exactly on a segment boundary (the survivors of the first segments that have any)
        first = next((oc for _, oc in per_seg if oc > 0), 0)
        for limit in sorted({0, max(1, first // 2), first} - ({0} if not rows else set())) if rows else [0]:
            q = native.DeviceQuery(ctx, table, used, sels, proj, limit, 1024)
            q.run()
            check_select(q, per_seg)
            check_rows(q, proj, rows[:limit] if limit > 0 else rows)
            q.close()
        q = native.DeviceQuery(ctx, table, used, sels)
        q.run_count()
        check_select(q, per_seg)
        q.run_select()
        check_select(q, per_seg)
        q.close()
    # group by name (the wide-key entry point) with a Match on the other string column == the per-segment aggregations merged
    used, sels, group, aggs = [2, 3, 1], [(1, MATCH, pools.codes)], [0], [("count", 0), ("max", 2)]
    q = native.DeviceQuery(ctx, table, used, sels, (), 0, 1024, group_cols=group, aggs=[(native.AGG_COUNT, 0), (native.AGG_MAX, 2)], wide_keys=True)
    q.run()
    keys, first, counts, vals = q.fetch_groups()
    kb = q.fetch_group_keys()
    q.close()
    per = []
    for cols in segs_cols:
        ucols = [cols[i].npcol() for i in used]
        _, _, masks = oracle_np.scan_select(ucols, sels, 1024)
        per.append(oracle_np.project_agg(ucols, group, aggs, masks))
    want = oracle_np.combine_agg(per, aggs)
    got = [(bytes(kb[g]).decode(), [int(counts[g]), float(int(vals[g, 1]))]) for g in range(kb.shape[0])]
    assert got == [(k, list(v)) for k, v in want.items()]
    table.close()
    for d in dsegs:
        d.close()


def test_record_and_replay(ctx, oracle):
    pools, segs_cols, dsegs, table = make_table(ctx, SHAPES[0], 5)
    used, sels, proj = [2, 0], [(0, MATCH, pools.names)], [1, 0]
    per_seg, rows = expected(oracle, segs_cols, used, sels, proj)
    assert rows
    q = native.DeviceQuery(ctx, table, used, sels, proj, 0, 1024)
    q.run()
    q.fetch_rows()
    with ctx.capture() as cap:
        q.run()
    for _ in range(2):
        cap.graph.launch()
        check_select(q, per_seg)
        check_rows(q, proj, rows)
    cap.graph.close()
    q.close()
    table.close()
    for d in dsegs:
        d.close()


def test_what_a_table_still_refuses(ctx):
    rng = np.random.default_rng(9)
    n = 300
    cols = [RawColumn(DENSE_STRING, 3, rng.integers(97, 100, size=(n, 3)).astype(np.uint8), [n]),
            RawColumn(DENSE_STRING, 2, rng.integers(97, 100, size=(n, 2)).astype(np.uint8), [n]),
            RawColumn(DENSE_STRING, 16, rng.integers(97, 100, size=(n, 16)).astype(np.uint8), [n]),
            RawColumn(DENSE_TINYINT, 1, rng.integers(0, 100, size=n).astype(np.int8), [n])]
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    table = native.DeviceTable(ctx, [seg])
    nine = [bytes([97 + i // 3, 97 + i % 3]) for i in range(9)]
    for used, sels in (([0], [(0, MATCH, [b"abc"])]), ([1], [(0, MATCH, nine)])):
        with pytest.raises(native.Imm3Error) as e:
            q = native.DeviceQuery(ctx, table, used, sels)
            q.run()
        assert e.value.code == native.ERR_ARG and "still refused" in e.value.msg and "per-segment queries" in e.value.msg
    q = native.DeviceQuery(ctx, table, [1], [(0, MATCH, nine[:8])])     # eight values: the tile kernel, as before
    q.run_select()
    assert q.count() == int(np.isin(cols[1].values.view("<u2").reshape(-1), np.frombuffer(b"".join(nine[:8]), "<u2")).sum())
    q.close()
    # a tree with an OR on the 16-byte column: select trees over a table keep the tile kinds
    with pytest.raises(native.Imm3Error) as e:
        native.DeviceQuery(ctx, table, [2, 3], [(0, MATCH, [bytes(cols[2].values[0])]), (1, GT, 50.0)], expr=[0, 1, native.EXPR_OR])
    assert e.value.code == native.ERR_ARG and e.value.msg.startswith(native.TABLE_TREE_REFUSED)
    table.close()
    seg.close()


# ---- both Engines over a 3-segment table with a 16-byte name column ---------------------------------------------------------------
def run_sql_explained(sql, data_dir):
    r = subprocess.run([os.path.join(BIN, "imm3_sql"), "--explain", "-q", sql, "-d", data_dir], capture_output=True, text=True, check=True, timeout=120)
    paths = [line[len("path: "):] for line in r.stderr.splitlines() if line.startswith("path: ")]
    assert len(paths) == 1, r.stderr
    return r.stdout.splitlines(), paths[0]


def test_engines_run_one_table_query(tmp_path, oracle):
    from immutable3_amd import Count, Max, Project, ProjectAgg, Query, Select
    from immutable3_amd.operators import Engine, GpuSegmentManager, java_double_to_string
    from immutable3_amd.query import Match
    from immutable3_amd.schema import CodecType, Column, Table, TableIO
    from immutable3_amd.storage import SegmentManager, write_segment_arrays
    rng = np.random.default_rng(4242)
    pools = Pools(4242)
    t = Table("people", [Column.make("id", CodecType.DENSE_INT), Column.make("name", CodecType.DENSE_STRING, {"size": "16"}),
                         Column.make("age", CodecType.DENSE_TINYINT)], 1024)
    TableIO.store(str(tmp_path), t)
    shape = [(2 * 1024 + 1, [1024, 1024, 1]), (2 * 1024 + 1, [1024, 1024, 1]), (1500, [1024, 476])]
    segs = []
    for s, (n, br) in enumerate(shape):
        ids = (np.arange(n) + s * 10 ** 5).astype(np.int32)
        names = make_strings(rng, pools.name, n)
        ages = rng.integers(0, 100, size=n).astype(np.int8)
        write_segment_arrays(str(tmp_path), t, s, {"id": ids, "name": names, "age": ages}, block_rows=br)
        segs.append([RawColumn(DENSE_INT, 4, ids, br), RawColumn(DENSE_STRING, 16, names, br), RawColumn(DENSE_TINYINT, 1, ages, br)])
    target = bytes(pools.n0)
    # per-segment expectations from the oracle: rows (id, name) of `name = target`; groups by name under the same Match
    _, rows = expected(oracle, segs, [0, 1], [(1, MATCH, [target])], [0, 1])
    assert len(rows) > 5
    want_rows = [(int.from_bytes(r[2][0], "little", signed=True), r[2][1].decode()) for r in rows]
    aggs = [("count", 0), ("max", 2)]
    per = []
    for cols in segs:
        ucols = [c.npcol() for c in cols]
        _, _, masks = oracle_np.scan_select(ucols, [(1, MATCH, [target])], 1024)
        per.append(oracle_np.project_agg(ucols, [1], aggs, masks))
    want_groups = oracle_np.combine_agg(per, aggs)
    gsm = GpuSegmentManager(SegmentManager(str(tmp_path)))
    try:
        assert gsm.device_table("people") is not None
        eng = Engine(gsm)
        for limit in (5, 0):
            q = Query("people", Select("name", Match([target.decode()])), Project(["id", "name"], limit))
            fused = eng.execute_table_columns(q)
            assert fused is not None                                    # the proof that the table launch was taken
            exp = want_rows[:limit] if limit else want_rows
            assert [(r[0], r[1]) for r in eng.execute(q)] == exp
        qa = Query("people", Select("name", Match([target.decode()])), ProjectAgg([Count("id"), Max("age")], ["name"]))
        assert eng._table_plan(qa) is not None
        got = eng.execute_agg(qa)
        assert list(got) == list(want_groups)
        for k, m in got.items():
            assert [a.get() for a in m.values()] == want_groups[k], k
    finally:
        gsm.close()
    sql = f"select id, name from people where name = '{target.decode()}' limit 5"
    assert run_sql_explained(sql, str(tmp_path)) == ([f"Row({i},{nm})" for i, nm in want_rows[:5]], "one table query")
    gsql = f"select count(id), max(age) from people where name = '{target.decode()}' group by name"
    rows_g, path_g = run_sql_explained(gsql, str(tmp_path))
    assert path_g == "one table query"
    assert rows_g == [f"Row({c},{java_double_to_string(float(m))})" for c, m in want_groups.values()]
