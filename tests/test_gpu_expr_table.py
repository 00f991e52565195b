"""GPU suite: select trees over an imm3_table (imm3_query_create_table_expr / _table_agg_expr; k_filter_expr's TABLE instances):
ONE launch over the tile table of all segments.  Everything is held against numpy -- per segment the leaves' keep masks
(oracle_np.scan_select one leaf at a time) combined with & and | as the tree says -- and against the per-segment tree queries the
table launch replaces (imm3_query_create_expr on each segment): same bitmap words per segment, same counts, rows in ascending
(segment, row) order under the global limit, groups in first-seen order."""
import os
import subprocess

import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, EQ, GT, LT, MATCH, PforColumn, RawColumn, SnappyColumn, blocks_of
from expr_util import AND, OR, expected_masks, has_or, postfix, words_of_masks

pytestmark = pytest.mark.gpu
CODES = [b"CA", b"NY", b"TX", b"WA", b"VA", b"DC", b"CT", b"OR", b"FL", b"MA"]
TILE = 0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# partial last tiles of 1, 63, 64 and 1000 rows, a segment below one tile, a segment of whole tiles
SEG_ROWS = [3 * 1024 + 1, 2 * 1024 + 63, 1024 + 64, 4 * 1024 + 1000, 700, 2 * 1024]


@pytest.fixture(scope="module")
def ctx():
    from immutable3_amd import native
    c = native.Context(0)
    yield c
    c.close()


def str_col(rng, n, width, codes):
    vals = np.array([list(c.ljust(width, b"_")[:width]) for c in codes], np.uint8)
    return vals[rng.integers(0, len(codes), size=n)]


def segment_columns(rng, n):
    """[i0, i1, i2, b0, b1, b2, s2, name16, payload]: values in 0 .. 99, seven state codes, five 16-byte names"""
    br = blocks_of(n, 1024)
    ints = [rng.integers(0, 100, size=n).astype(np.int32) for _ in range(3)]
    byts = [rng.integers(0, 100, size=n).astype(np.int8) for _ in range(3)]
    return ([RawColumn(DENSE_INT, 4, v, br) for v in ints] + [RawColumn(DENSE_TINYINT, 1, v, br) for v in byts] +
            [RawColumn(DENSE_STRING, 2, str_col(rng, n, 2, CODES[:7]), br),
             RawColumn(DENSE_STRING, 16, str_col(rng, n, 16, [b"anna", b"bob", b"carla", b"dmitri", b"eve"]), br),
             RawColumn(DENSE_INT, 4, rng.integers(-10 ** 6, 10 ** 6, size=n).astype(np.int32), br)])


class Fixture:
    def __init__(self, ctx, seed=7, rows=SEG_ROWS):
        from immutable3_amd import native
        rng = np.random.default_rng(seed)
        self.ctx = ctx
        self.cols = [segment_columns(rng, n) for n in rows]
        self.segs = [native.DeviceSegment(ctx, [c.native() for c in cols]) for cols in self.cols]
        self.table = native.DeviceTable(ctx, self.segs)

    def close(self):
        self.table.close()
        for s in self.segs:
            s.close()

    def masks(self, used, leaves, tree):
        """per segment: the per-batch keep masks numpy gives"""
        return [expected_masks([cols[i] for i in used], leaves, tree) for cols in self.cols]

    def keep(self, used, leaves, tree):
        """per segment: one boolean per row"""
        return [np.concatenate(m) if m else np.zeros(0, bool) for m in self.masks(used, leaves, tree)]


@pytest.fixture(scope="module")
def fx(ctx):
    f = Fixture(ctx)
    yield f
    f.close()


def check_bitmap(fx, used, leaves, tree, per_segment=True):
    """the table query's bitmap and count against numpy and against the per-segment tree queries; returns the count"""
    from immutable3_amd import native
    masks = fx.masks(used, leaves, tree)
    q = native.DeviceQuery(fx.ctx, fx.table, used, leaves, expr=postfix(tree))
    q.run()
    words, count = q.bitmap(), q.count()
    fb, fw = q.segment_starts()
    want_total = 0
    for si, m in enumerate(masks):
        want = words_of_masks(m)
        want_total += int(sum(int(x.sum()) for x in m))
        lo = int(fw[si])
        assert words[lo: lo + want.size].tolist() == want.tolist(), (si, leaves, tree)
        assert not words[lo + want.size: int(fw[si + 1])].any(), (si, leaves, tree)       # padding up to the next tile
        if per_segment:
            qs = native.DeviceQuery(fx.ctx, fx.segs[si], used, leaves, expr=postfix(tree))
            qs.run()
            sw = qs.bitmap()
            assert words[lo: lo + sw.size].tolist() == sw.tolist() and qs.count() == int(sum(int(x.sum()) for x in m))
            qs.close()
    assert count == want_total, (leaves, tree)
    pl = q.plan()
    assert not pl["single_pass"] and not pl["records"]
    q.run_count()
    assert q.count() == want_total
    q.run_select()
    assert q.count() == want_total and q.bitmap().tolist() == words.tolist()
    form = q.expr_form()
    q.close()
    return want_total, form


# k_filter_expr's 15 kind combinations (K0 <= K1 <= K2; I32 = 0, I8 = 1, S2 = 2): as used columns of segment_columns()
KINDS = {
    "I32": [0], "I8": [3], "S2": [6], "I32+I32": [0, 1], "I32+I8": [0, 3], "I8+I8": [3, 4], "I32+S2": [0, 6], "I8+S2": [3, 6],
    "I32x3": [0, 1, 2], "I32+I32+I8": [0, 1, 3], "I32+I8+I8": [0, 3, 4], "I8x3": [3, 4, 5], "I32+I32+S2": [0, 1, 6], "I32+I8+S2": [0, 3, 6],
    "I8+I8+S2": [3, 4, 6],
}


def kind_tree(used, n_terms):
    """n_terms DISTINCT terms over the used columns: term t constrains column t % len(used) alone, odd terms AND the next column in
    (so most terms constrain only a subset of the columns); thresholds and IN-lists differ from term to term, so no term is dropped"""
    leaves, terms = [], []
    for t in range(n_terms):
        def leaf_on(ci, t=t):
            if used[ci] == 6:
                leaves.append((ci, MATCH, [CODES[t % 7], b"Z%d" % t]))       # (the second value is one no row holds)
            else:
                leaves.append((ci, GT, 80.0 + 2 * t) if t % 3 else (ci, LT, 8.0 + t))
            return len(leaves) - 1
        term = leaf_on(t % len(used))
        if t % 2 == 1 and len(used) > 1:
            term = (AND, term, leaf_on((t + 1) % len(used)))
        terms.append(term)
    if n_terms == 1:                       # (p or p): one term once the duplicate is dropped, and still a tree query
        leaves, terms = leaves + leaves, [0, 1]
    tree = terms[0]
    for t in terms[1:]:
        tree = (OR, tree, t)
    return leaves, tree


@pytest.mark.parametrize("name", list(KINDS))
def test_every_kind_combination(fx, name):
    used = KINDS[name]
    total = sum(SEG_ROWS)
    for n_terms in (1, 2, 3, 8):
        leaves, tree = kind_tree(used, n_terms)
        cnt, form = check_bitmap(fx, used, leaves, tree)
        assert form == TILE and 0 < cnt <= total, (name, n_terms)
    # a tautology: every row of every segment (partial tiles end where the rows end) ...
    first = (0, MATCH, CODES[:7]) if used[0] == 6 else (0, LT, 50.0)
    second = (0, MATCH, CODES[:7] + [b"ZZ"]) if used[0] == 6 else (0, GT, 30.0)
    cnt, form = check_bitmap(fx, used, [first, second], (OR, 0, 1))
    assert cnt == total and form == TILE
    # ... and a tree that normalises to nothing (every term a contradiction): no launch, an empty bitmap
    if used[0] == 6:
        none = [(0, MATCH, [b"CA"]), (0, MATCH, [b"NY"]), (0, MATCH, [b"TX", b"WA"]), (0, MATCH, [b"VA"])]
    else:
        none = [(0, LT, 10.0), (0, GT, 50.0), (0, LT, 5.0), (0, GT, 60.0)]
    cnt, form = check_bitmap(fx, used, none, (OR, (AND, 0, 1), (AND, 2, 3)))
    assert cnt == 0 and form == -1


def test_single_rows_at_the_segment_ends(ctx):
    """one survivor per segment, in its LAST row (the partial tile's last valid bit), and none past it"""
    from immutable3_amd import native
    rows = [1024 + 1, 63, 2 * 1024 + 64, 1000, 1024]
    cols, segs = [], []
    for n in rows:
        b = np.zeros(n, np.int8)
        i = np.zeros(n, np.int32)
        b[-1], i[-1] = 9, 9
        br = blocks_of(n, 1024)
        cols.append([RawColumn(DENSE_TINYINT, 1, b, br), RawColumn(DENSE_INT, 4, i, br)])
        segs.append(native.DeviceSegment(ctx, [c.native() for c in cols[-1]]))
    table = native.DeviceTable(ctx, segs)
    for used, leaves in (([0], [(0, GT, 5.0), (0, LT, -5.0)]), ([1], [(0, GT, 5.0), (0, LT, -5.0)]), ([0, 1], [(0, GT, 5.0), (1, LT, -5.0)])):
        q = native.DeviceQuery(ctx, table, used, leaves, [0], expr=postfix((OR, 0, 1)))
        q.run()
        idx, _ = q.fetch_rows()
        seg_of, row_of = q.locate_rows(idx)
        assert q.count() == len(rows) and seg_of.tolist() == list(range(len(rows))) and row_of.tolist() == [n - 1 for n in rows]
        q.close()
    table.close()
    for s in segs:
        s.close()


def numpy_rows(fx, keep, limit):
    """(segment, row) of the survivors in ascending order under the global limit"""
    out = [(si, int(r)) for si, k in enumerate(keep) for r in np.flatnonzero(k)]
    return out[:limit] if limit > 0 else out


def test_projection(fx):
    from immutable3_amd import native
    used = [3, 0, 6, 8]                                                     # age-like int8, int32, state; payload is no predicate column
    leaves = [(0, LT, 20.0), (1, GT, 60.0), (2, MATCH, [b"CA", b"NY"]), (0, GT, 90.0)]
    tree = (OR, (AND, 0, 1), (AND, 2, 3))
    keep = fx.keep(used, leaves, tree)
    every = numpy_rows(fx, keep, 0)
    in_first = int(keep[0].sum())
    assert in_first > 5 and len(every) > in_first
    for limit in (0, 1, 5, in_first, in_first + int(keep[1].sum()), len(every) + 100):
        want = numpy_rows(fx, keep, limit)
        q = native.DeviceQuery(fx.ctx, fx.table, used, leaves, [3, 0, 2], limit, expr=postfix(tree))
        q.run()
        pl = q.plan()
        assert not pl["single_pass"] and not pl["records"]
        idx, vals = q.fetch_rows()
        seg_of, row_of = q.locate_rows(idx)
        assert list(zip(seg_of.tolist(), row_of.tolist())) == want, limit
        assert q.count() == len(every)
        for j, ci in enumerate((8, 3, 6)):
            src = [fx.cols[s][ci] for s in range(len(fx.cols))]
            exp = b"".join(src[s].dat.reshape(-1, src[s].width)[r].tobytes() for s, r in want)
            assert vals[j].tobytes() == exp, (limit, ci)
        q.close()
    # survivors on both sides of every segment boundary: the tautology keeps the last row of one segment and the first of the next
    q = native.DeviceQuery(fx.ctx, fx.table, [3, 8], [(0, LT, 50.0), (0, GT, 30.0)], [1], expr=postfix((OR, 0, 1)))
    q.run()
    idx, vals = q.fetch_rows()
    seg_of, row_of = q.locate_rows(idx)
    want = [(si, r) for si, n in enumerate(SEG_ROWS) for r in range(n)]
    assert list(zip(seg_of.tolist(), row_of.tolist())) == want
    assert vals[0].view("<i4").reshape(-1).tolist() == np.concatenate([c[8].values for c in fx.cols]).tolist()
    q.close()


def numpy_groups(fx, keep, key_col):
    """first-seen order over (segment, row): key bytes -> [count, min, max, sum of i0, max of name16]"""
    out = {}
    for si, k in enumerate(keep):
        cols = fx.cols[si]
        for r in np.flatnonzero(k):
            key = bytes(cols[key_col].values[r])
            v, name = int(cols[0].values[r]), bytes(cols[7].values[r])
            st = out.get(key)
            if st is None:
                out[key] = [1, v, v, v, name]
            else:
                st[0] += 1
                st[1], st[2], st[3], st[4] = min(st[1], v), max(st[2], v), st[3] + v, max(st[4], name)
    return out


def gpu_groups(q, key_bytes):
    keys, first, counts, vals = q.fetch_groups()
    kb = q.fetch_group_keys() if key_bytes > 8 else None
    names = q.fetch_group_strings(3)
    out = {}
    for g in range(keys.shape[0]):
        key = bytes(kb[g]) if kb is not None else int(keys[g]).to_bytes(8, "little")[:key_bytes]
        out[key] = [int(counts[g]), int(vals[g, 0]), int(vals[g, 1]), int(vals[g, 2]), bytes(names[g])]
    return out


@pytest.mark.parametrize("key_col,key_bytes", [(6, 2), (7, 16)])
def test_aggregation_under_a_tree(fx, key_col, key_bytes):
    """count / min / max / sum and a 16-byte string MAX, grouped by the 2-byte state and by the 16-byte name (a wide key)"""
    from immutable3_amd import native
    used = [0, 3, 6, 7]
    leaves, tree = [(1, LT, 18.0), (1, GT, 65.0), (0, GT, 90.0)], (OR, (OR, 0, 1), 2)
    keep = fx.keep(used, leaves, tree)
    group = [used.index(key_col)]
    aggs = [(native.AGG_MIN, 0), (native.AGG_MAX, 0), (native.AGG_SUM, 0), (native.AGG_MAX, 3)]      # (the count comes with every group)
    q = native.DeviceQuery(fx.ctx, fx.table, used, leaves, group_cols=group, aggs=aggs, expr=postfix(tree))
    q.run()
    got = gpu_groups(q, key_bytes)
    assert q.count() == int(sum(int(k.sum()) for k in keep)) and q.expr_form() == TILE
    q.close()
    want = numpy_groups(fx, keep, key_col)
    assert list(got.keys()) == list(want.keys())
    assert got == want
    # the host-side combine of the per-segment tree aggregations: first arrival first, segments ascending
    merged = {}
    for seg in fx.segs:
        qs = native.DeviceQuery(fx.ctx, seg, used, leaves, group_cols=group, aggs=aggs, expr=postfix(tree))
        qs.run()
        for key, st in gpu_groups(qs, key_bytes).items():
            cur = merged.get(key)
            if cur is None:
                merged[key] = st
            else:
                merged[key] = [cur[0] + st[0], min(cur[1], st[1]), max(cur[2], st[2]), cur[3] + st[3], max(cur[4], st[4])]
        qs.close()
    assert list(got.keys()) == list(merged.keys()) and got == merged


def test_tree_without_or_takes_the_table_path(fx):
    from immutable3_amd import native
    used = [3, 0, 6]
    leaves = [(0, GT, 18.0), (1, LT, 70.0), (0, LT, 60.0), (2, MATCH, [b"CA", b"TX", b"NY"])]
    tree = (AND, (AND, 0, 1), (AND, 2, 3))
    assert not has_or(tree)
    for limit in (0, 9):
        old = native.DeviceQuery(fx.ctx, fx.table, used, leaves, [1, 0], limit)
        new = native.DeviceQuery(fx.ctx, fx.table, used, leaves, [1, 0], limit, expr=postfix(tree))
        assert old.plan() == new.plan()
        old.run()
        new.run()
        assert old.plan() == new.plan() and new.expr_form() == -1
        assert old.count() == new.count() and old.bitmap().tolist() == new.bitmap().tolist()
        (i0, v0), (i1, v1) = old.fetch_rows(), new.fetch_rows()
        assert i0.tolist() == i1.tolist() and all(a.tobytes() == b.tobytes() for a, b in zip(v0, v1))
        old.close()
        new.close()
    aggs = [(native.AGG_COUNT, 0), (native.AGG_MAX, 1)]
    old = native.DeviceQuery(fx.ctx, fx.table, used, leaves, group_cols=[2], aggs=aggs, wide_keys=True)
    new = native.DeviceQuery(fx.ctx, fx.table, used, leaves, group_cols=[2], aggs=aggs, expr=postfix(tree))
    old.run()
    new.run()
    assert old.plan() == new.plan() and old.agg_form() == new.agg_form()
    assert all(a.tolist() == b.tolist() for a, b in zip(old.fetch_groups(), new.fetch_groups()))
    old.close()
    new.close()


def ors(idx):
    t = idx[0]
    for i in idx[1:]:
        t = (OR, t, i)
    return t


def test_errors_at_creation(ctx):
    from immutable3_amd import native
    rng = np.random.default_rng(3)
    n = 2048 + 5
    br = blocks_of(n, 1024)
    cols = [RawColumn(DENSE_INT, 4, rng.integers(0, 100, size=n).astype(np.int32), br),
            RawColumn(DENSE_TINYINT, 1, rng.integers(0, 100, size=n).astype(np.int8), br),
            RawColumn(DENSE_STRING, 2, str_col(rng, n, 2, CODES), br),
            RawColumn(DENSE_STRING, 3, str_col(rng, n, 3, [b"abc", b"xyz"]), br),
            RawColumn(DENSE_INT, 4, rng.integers(0, 100, size=n).astype(np.int32), br)]
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    seg2 = native.DeviceSegment(ctx, [c.native() for c in cols])
    table = native.DeviceTable(ctx, [seg, seg2])

    def refused(used, leaves, tree, needle, **kw):
        with pytest.raises(native.Imm3Error) as e:
            native.DeviceQuery(ctx, table, used, leaves, expr=postfix(tree), **kw)
        assert e.value.code == native.ERR_ARG and needle in e.value.msg, e.value.msg

    # nine terms: (a0 or a1 or a2) and (b0 or b1 or b2)
    nine = [(0, EQ, float(v)) for v in (1, 2, 3)] + [(1, EQ, float(v)) for v in (10, 20, 30)]
    refused([0, 1], nine, (AND, ors([0, 1, 2]), ors([3, 4, 5])), "at most 8 terms")
    refused([0, 1], nine, (AND, ors([0, 1, 2]), ors([3, 4, 5])), "at most 8 terms", group_cols=[1], aggs=[(native.AGG_COUNT, 0)])
    # four predicate columns
    refused([0, 1, 2, 4], [(0, LT, 5.0), (1, GT, 90.0), (2, MATCH, [b"CA"]), (3, GT, 95.0)], ors([0, 1, 2, 3]), "at most 3 predicate columns")
    # a 3-byte string leaf, an IN-list of 9
    refused([3, 1], [(0, MATCH, [b"abc"]), (1, GT, 90.0)], (OR, 0, 1), "2-byte")
    refused([2, 1], [(0, MATCH, CODES[:9]), (1, GT, 90.0)], (OR, 0, 1), "at most 8 values")
    # malformed programs
    for prog in ([native.EXPR_OR], [0, 1], [0, 5, native.EXPR_OR], [0, 1, -7]):
        with pytest.raises(native.Imm3Error) as e:
            native.DeviceQuery(ctx, table, [1, 0], [(0, LT, 18.0), (0, GT, 65.0)], expr=prog)
        assert e.value.code == native.ERR_ARG
    # leaf errors come before program errors: a bad leaf AND a malformed program
    with pytest.raises(native.Imm3Error) as e:
        native.DeviceQuery(ctx, table, [1, 0], [(0, LT, 18.0), (0, native.NOTMATCH, [b"x"])], expr=[native.EXPR_OR])
    assert e.value.code == native.ERR_UNSUPPORTED_CONDITION and e.value.msg == "Unsupported condition: NotMatch"
    with pytest.raises(native.Imm3Error) as e:
        native.DeviceQuery(ctx, table, [1, 0], [(0, LT, 18.0), (1, MATCH, [b"x"])], expr=[0, 1])
    assert e.value.code == native.ERR_UNSUPPORTED_VECTOR and e.value.msg == "Unsupported column vector"
    with pytest.raises(native.Imm3Error) as e:
        native.DeviceQuery(ctx, table, [1, 9], [(0, LT, 18.0)], expr=[0, 0, native.EXPR_OR])
    assert e.value.code == native.ERR_ARG and "out of range" in e.value.msg
    # eight terms over three columns are taken
    q = native.DeviceQuery(ctx, table, [0, 1], nine[:2] + nine[3:] + [(1, EQ, 40.0)], expr=postfix((AND, ors([0, 1]), ors([2, 3, 4, 5]))))
    q.run()
    keep = np.isin(cols[0].values, [1, 2]) & np.isin(cols[1].values, [10, 20, 30, 40])
    assert q.count() == 2 * int(keep.sum()) and q.expr_form() == TILE
    q.close()
    table.close()
    seg.close()
    seg2.close()


def test_compressed_predicate_columns(ctx, oracle):
    from immutable3_amd import native
    rng = np.random.default_rng(21)
    cols, segs = [], []
    for n in (5 * 1024 + 5, 3 * 1024, 900):
        br = blocks_of(n, 1024)
        v = np.sort(rng.integers(0, 1 << 20, size=n).astype(np.int32))
        age = rng.integers(0, 100, size=n).astype(np.int8)
        cols.append([PforColumn(v, br), SnappyColumn(DENSE_TINYINT, 1, age, br)])
        segs.append(native.DeviceSegment(ctx, [c.native() for c in cols[-1]]))
    table = native.DeviceTable(ctx, segs)
    leaves, tree = [(0, LT, float(1 << 18)), (1, GT, 90.0)], (OR, 0, 1)
    q = native.DeviceQuery(ctx, table, [0, 1], leaves, [1, 0], expr=postfix(tree))
    q.run()
    keep = [(c[0].values < (1 << 18)) | (c[1].values > 90) for c in cols]
    idx, vals = q.fetch_rows()
    seg_of, row_of = q.locate_rows(idx)
    want = [(si, int(r)) for si, k in enumerate(keep) for r in np.flatnonzero(k)]
    assert q.count() == len(want) and list(zip(seg_of.tolist(), row_of.tolist())) == want and q.expr_form() == TILE
    assert vals[1].view("<i4").reshape(-1).tolist() == [int(cols[s][0].values[r]) for s, r in want]
    q.close()
    table.close()
    for s in segs:
        s.close()


def test_graph_replay_and_count_log(fx):
    import torch
    used = [3, 0]
    leaves, tree = [(0, LT, 18.0), (0, GT, 65.0), (1, LT, 10.0)], (OR, (OR, 0, 1), 2)
    from immutable3_amd import native
    keep = fx.keep(used, leaves, tree)
    want = numpy_rows(fx, keep, 0)
    q = native.DeviceQuery(fx.ctx, fx.table, used, leaves, [1, 0], expr=postfix(tree))
    q.run()
    q.fetch_rows()
    words = q.bitmap()
    with fx.ctx.capture() as cap:
        q.run()
    graph = cap.graph
    for _ in range(2):
        graph.launch()
        idx, vals = q.fetch_rows()
        seg_of, row_of = q.locate_rows(idx)
        assert q.count() == len(want) and q.bitmap().tolist() == words.tolist()
        assert list(zip(seg_of.tolist(), row_of.tolist())) == want
        assert vals[0].view("<i4").reshape(-1).tolist() == [int(fx.cols[s][0].values[r]) for s, r in want]
    graph.close()
    q.close()
    # every run's count lands in the device log, for select-only runs and count-only runs alike
    q = native.DeviceQuery(fx.ctx, fx.table, used, leaves, expr=postfix(tree))
    log = torch.zeros(6, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    q.log_counts(log.data_ptr(), 5)
    for _ in range(2):
        q.run_select()
    q.run_count()
    q.run()
    q.sync()
    assert log.tolist() == [len(want)] * 4 + [0, 0]
    q.log_counts(0, 0)
    q.run_select()
    assert q.count() == len(want)
    q.close()


def run_sql(sql, data_dir):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "immutable3_amd", "bin", "imm3_sql")
    return subprocess.run([exe, "--honour-and-or", "-q", sql, "-d", data_dir], capture_output=True, text=True, check=True, timeout=120).stdout.splitlines()


def run_sql_explained(sql, data_dir):
    """(rows, the way the C++ Engine took: imm3_sql --explain's "path: ..." line)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "immutable3_amd", "bin", "imm3_sql")
    r = subprocess.run([exe, "--honour-and-or", "--explain", "-q", sql, "-d", data_dir], capture_output=True, text=True, check=True, timeout=120)
    paths = [line[len("path: "):] for line in r.stderr.splitlines() if line.startswith("path: ")]
    assert len(paths) == 1, r.stderr
    return r.stdout.splitlines(), paths[0]


def numpy_state_groups(keep, age, st):
    """first-seen order: state -> (count, max age)"""
    groups = {}
    for i in np.flatnonzero(keep):
        k = bytes(st[i])
        c, m = groups.get(k, (0, None))
        groups[k] = (c + 1, int(age[i]) if m is None else max(m, int(age[i])))
    return groups


def engine_expectations(gsm, table):
    from immutable3_amd.operators import Engine
    from immutable3_amd.query import NoSelect, Project, Query
    everything = Engine(gsm).execute_columns(Query(table, NoSelect, Project(["id", "age", "state"], 0)))
    return (np.concatenate([c[0] for _, _, c in everything]), np.concatenate([c[1] for _, _, c in everything]).astype(np.int64),
            np.concatenate([c[2] for _, _, c in everything]))


def check_engine(gsm, table, lo, hi, expect_table=True):
    """Engine(honour_and_or=True) over one table directory: (age < lo or age > hi), rows / limit / groups against numpy and against
    the per-segment pipelines; the tree query takes the table launch, a tree the table refuses falls back and is still right"""
    from immutable3_amd.operators import Engine, ScanOp, getColumns, resolveProjectOp
    from immutable3_amd.query import And, Count, EQ as QEQ, GT as QGT, LT as QLT, Max, Or, Project, ProjectAgg, Query, Select
    ids, age, st = engine_expectations(gsm, table)
    eng = Engine(gsm, honour_and_or=True)
    has_table = gsm.device_table(table) is not None                     # (quirk_25's blocks of 4 rows are no table layout: per-segment for every query)
    assert has_table == expect_table
    sel = Or(Select("age", QLT(lo)), Select("age", QGT(hi)))
    keep = (age < lo) | (age > hi)
    assert keep.any() and not keep.all()
    want = list(zip(ids[keep].tolist(), age[keep].tolist()))
    for limit in (0, 5):
        q = Query(table, sel, Project(["id", "age"], limit))
        fused = eng.execute_table_columns(q)
        exp = want[:limit] if limit else want
        if has_table:
            assert fused is not None                                    # the proof that the table launch was taken
            assert list(zip(fused[2][0].tolist(), fused[2][1].tolist())) == exp
        else:
            assert fused is None
        assert [(r[0], r[1]) for r in eng.execute(q)] == exp
        per_segment = [row for _, proj in eng.pipelines(q) for row in proj.iterator()]
        assert [(r[0], r[1]) for r in per_segment][:len(exp)] == exp
    assert list(Engine(gsm).execute(Query(table, sel, Project(["id", "age"], 0)))) == ([] if lo <= hi else want)   # flag off: the conjunction
    qa = Query(table, sel, ProjectAgg([Count("id"), Max("age")], ["state"]))
    res = eng.execute_agg(qa)
    groups = {}
    for i in np.flatnonzero(keep):
        k = bytes(st[i]).decode()
        c, m = groups.get(k, (0, None))
        groups[k] = (c + 1, int(age[i]) if m is None else max(m, int(age[i])))
    assert list(res.keys()) == list(groups.keys())
    for k, aggmap in res.items():
        got = [a.get() for a in aggmap.values()]
        assert (int(got[0]), float(got[1])) == (groups[k][0], float(groups[k][1])), k
    # ... and what the per-segment pipelines give, combined by key in segment order
    merged = {}
    tbl = gsm.getTable(table)
    for seg_idx in range(gsm.getTableSegmentCount(table)):
        op = ScanOp(gsm, seg_idx, table, getColumns(qa, tbl))
        for leaf in eng._select_ops(qa):
            op = leaf(op)
        for key, aggmap in resolveProjectOp(qa.project, tbl)(op).iterator():
            cur = merged.get(key)
            if cur is None:
                merged[key] = aggmap
            else:
                for alias, agg in aggmap.items():
                    cur[alias] = cur[alias].combine(agg)
    assert list(res.keys()) == list(merged.keys())
    assert all([a.get() for a in res[k].values()] == [a.get() for a in merged[k].values()] for k in res)
    # nine terms: the table refuses, the per-segment path answers
    avals = sorted(set(age.tolist()))[:3]
    big = And(Or(Or(Select("age", QEQ(avals[0])), Select("age", QEQ(avals[1]))), Select("age", QEQ(avals[2]))),
              Or(Or(Select("id", QEQ(int(ids[0]))), Select("id", QEQ(int(ids[1])))), Select("id", QEQ(int(ids[2])))))
    q = Query(table, big, Project(["id", "age"], 0))
    assert eng.execute_table_columns(q) is None
    k9 = np.isin(age, avals) & np.isin(ids, ids[:3])
    assert [(r[0], r[1]) for r in eng.execute(q)] == list(zip(ids[k9].tolist(), age[k9].tolist()))
    res9 = eng.execute_agg(Query(table, big, ProjectAgg([Count("id")], ["state"])))
    assert sum(int(m["id_count"].get()) for m in res9.values()) == int(k9.sum())


@pytest.mark.parametrize("table,lo,hi", [("test_100", 20, 60), ("quirk_25", -2, 3)])
def test_python_engine_takes_the_table_launch(table, lo, hi):
    from immutable3_amd.operators import GpuSegmentManager
    from immutable3_amd.storage import SegmentManager
    gsm = GpuSegmentManager(SegmentManager(GOLDEN))
    try:
        check_engine(gsm, table, lo, hi, expect_table=table != "quirk_25")
    finally:
        gsm.close()


def test_python_engine_on_a_loader_made_table(tmp_path):
    """README-style segments as the loader cuts them (S * B + 1 rows: a trailing 1-row block) and a short last one"""
    from immutable3_amd import synth
    from immutable3_amd.operators import GpuSegmentManager
    from immutable3_amd.schema import TableIO
    from immutable3_amd.storage import SegmentManager, write_segment_arrays
    t = synth.table_schema("tq", 1024)
    TableIO.store(str(tmp_path), t)
    for s in range(5):
        n = 4 * 1024 + 1 if s < 4 else 1500
        cols = {"id": (np.arange(n, dtype=np.int64) + s * 10 ** 5).astype(np.int32),
                "age": synth.uniform_below(300 + s, n, 100, np.int8), "state": synth.state_codes(400 + s, n)}
        write_segment_arrays(str(tmp_path), t, s, cols, block_rows=([1024] * 4 + [1]) if s < 4 else [1024, 476])
    gsm = GpuSegmentManager(SegmentManager(str(tmp_path)))
    try:
        assert gsm.device_table("tq") is not None
        check_engine(gsm, "tq", 18, 65)
        ids, age, st = engine_expectations(gsm, "tq")
    finally:
        gsm.close()
    # ... and imm3_sql --honour-and-or over the same directory (its Engine takes the table launch too)
    keep = (age < 18) | (age > 65)
    sql = "select id, age from tq where (age < 18 or age > 65)"
    want = [f"Row({i},{a})" for i, a in zip(ids[keep].tolist(), age[keep].tolist())]
    assert run_sql(sql, str(tmp_path)) == want and run_sql(sql + " limit 7", str(tmp_path)) == want[:7]
    got = run_sql("select count(id), max(age) from tq where (age < 18 or age > 65) group by state", str(tmp_path))
    assert got == [f"Row({c},{float(m)})" for c, m in numpy_state_groups(keep, age, st).values()]
    # the C++ Engine says which way it went: ONE table query whose select launch is the tree's tile kernel ...
    assert run_sql_explained(sql, str(tmp_path)) == (want, "one table query: select tree, tile form")
    assert run_sql_explained(sql + " limit 7", str(tmp_path)) == (want[:7], "one table query: select tree, tile form")
    gsql = "select count(id), max(age) from tq where (age < 18 or age > 65) group by state"
    assert run_sql_explained(gsql, str(tmp_path)) == (got, "one table query: select tree")
    # ... a tree without an Or is the flat table query it always was ...
    flat = "select id, age from tq where (age > 18 and age < 30)"
    k_flat = (age > 18) & (age < 30)
    assert run_sql_explained(flat, str(tmp_path)) == ([f"Row({i},{a})" for i, a in zip(ids[k_flat].tolist(), age[k_flat].tolist())], "one table query")
    # ... and nine terms are refused by the table with the bound by name: per-segment queries, the same rows and groups
    avals = list(dict.fromkeys(age[[0, 5, 4100]].tolist() + [0, 1, 2, 3]))[:3]      # three distinct ages, rows 0 / 5 / 4100's first
    where9 = ("((" + " or ".join(f"age = {a}" for a in avals) + ") and (" + " or ".join(f"id = {int(i)}" for i in ids[[0, 5, 4100]]) + "))")
    k9 = np.isin(age, avals) & np.isin(ids, ids[[0, 5, 4100]])
    rows9, path9 = run_sql_explained("select id, age from tq where " + where9, str(tmp_path))
    assert k9.any() and rows9 == [f"Row({i},{a})" for i, a in zip(ids[k9].tolist(), age[k9].tolist())]
    assert path9.startswith("per-segment queries: a select tree over a table takes at most 8 terms"), path9
    groups9, gpath9 = run_sql_explained("select count(id), max(age) from tq where " + where9 + " group by state", str(tmp_path))
    assert groups9 == [f"Row({c},{float(m)})" for c, m in numpy_state_groups(k9, age, st).values()]
    assert gpath9.startswith("per-segment queries: a select tree over a table takes at most 8 terms"), gpath9


def test_a_real_argument_error_is_no_refusal(fx):
    """only the refusals that begin with TABLE_TREE_REFUSED send the engines to per-segment queries"""
    from immutable3_amd import native
    from immutable3_amd.operators import Engine
    prog = [0, 1, native.EXPR_OR]
    with pytest.raises(native.Imm3Error) as e:        # a used column that does not exist: ERR_ARG, and no refusal
        native.DeviceQuery(fx.ctx, fx.table, [3, 99], [(0, LT, 18.0), (0, GT, 65.0)], expr=prog)
    assert e.value.code == native.ERR_ARG and not Engine._table_tree_refused(e.value, prog)
    nine = [(0, EQ, float(v)) for v in (1, 2, 3)] + [(1, EQ, float(v)) for v in (10, 20, 30)]
    with pytest.raises(native.Imm3Error) as e:
        native.DeviceQuery(fx.ctx, fx.table, [3, 0], nine, expr=postfix((AND, ors([0, 1, 2]), ors([3, 4, 5]))))
    assert e.value.code == native.ERR_ARG and e.value.msg.startswith(native.TABLE_TREE_REFUSED) and Engine._table_tree_refused(e.value, prog)
    assert not Engine._table_tree_refused(e.value, None)


def test_cli_over_the_multi_segment_golden_table():
    """imm3_sql --honour-and-or on quirk_25 (several segments): the rows and every group numpy says"""
    from immutable3_amd.operators import GpuSegmentManager
    from immutable3_amd.storage import SegmentManager
    gsm = GpuSegmentManager(SegmentManager(GOLDEN))
    try:
        ids, age, st = engine_expectations(gsm, "quirk_25")
    finally:
        gsm.close()
    keep = (age < 0) | (age > 3)
    assert keep.any()
    sql = "select id, age from quirk_25 where (age < 0 or age > 3)"
    want = [f"Row({i},{a})" for i, a in zip(ids[keep].tolist(), age[keep].tolist())]
    assert run_sql(sql, GOLDEN) == want and run_sql(sql + " limit 4", GOLDEN) == want[:4]
    got = run_sql("select count(id), max(age) from quirk_25 where (age < 0 or age > 3) group by state", GOLDEN)
    assert got == [f"Row({c},{float(m)})" for c, m in numpy_state_groups(keep, age, st).values()]
    assert run_sql_explained(sql, GOLDEN) == (want, "per-segment queries")      # (blocks of 4 rows: this directory makes no imm3_table)
