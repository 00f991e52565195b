"""GPU suite: IMM3_EXPR_NOT -- complements and NotMatch in a select tree's one launch (csrc/imm3_expr.hip: a negated IN-list in
the in-lane, row-strided, rolled-partial-tile and generic evaluators; csrc/imm3_expr_norm.cpp: everything else is intervals).
Expectations are numpy's: each leaf's per-batch keep mask from oracle_np.scan_select, combined with &, | and ~ (expr_not_util).
The bitmap is compared word for word, so a complement that leaked into the padding bits of a batch's last word would show, and
the count is held against the popcount of those words.

The shapes are the smallest at which each evaluator can go wrong: one segment of 3 x 1024 + 37 rows (two full tiles and the rolled
partial tile, 37 valid bits in the last word), the same rows in blocks of 1000 (ragged: every batch ends in a word of 40 valid
bits), and a table of 1024 + 5, 2 x 1024 and 700 rows (every segment ends in a rolled tile)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, EQ, GT, LT, MATCH, RawColumn, blocks_of
from expr_not_util import AND, NOT, OR, expected_masks, has_not, postfix, random_tree, words_of_masks

pytestmark = pytest.mark.gpu
CODES = [b"CA", b"NY", b"TX", b"WA", b"VA", b"DC", b"CT", b"OR", b"FL", b"MA", b"NV", b"AZ"]
CODES4 = [b"ab12", b"zz00", b"q\\N\x00", b"none"]
TILE, GENERIC = 0, 1
N_SEG = 3 * 1024 + 37
TABLE_ROWS = [1024 + 5, 2 * 1024, 700]
ID, AGE, STATE, CODE = 0, 1, 2, 3          # the columns of every segment here


@pytest.fixture(scope="module")
def ctx():
    from immutable3_amd import native
    c = native.Context(0)
    yield c
    c.close()


def columns(rng, n, block_rows):
    ident = rng.permutation(n).astype(np.int32)
    ident[rng.integers(0, n, size=max(n // 50, 1))] = np.int32(-2 ** 31)           # Int.MinValue is an ordinary value
    age = rng.integers(0, 100, size=n).astype(np.int8)
    state = np.array([list(c) for c in CODES], np.uint8)[rng.integers(0, len(CODES), size=n)]
    code = np.array([list(c) for c in CODES4], np.uint8)[rng.integers(0, len(CODES4), size=n)]
    return [RawColumn(DENSE_INT, 4, ident, block_rows), RawColumn(DENSE_TINYINT, 1, age, block_rows),
            RawColumn(DENSE_STRING, 2, state, block_rows), RawColumn(DENSE_STRING, 4, code, block_rows)]


class Segment:
    def __init__(self, ctx, block):
        from immutable3_amd import native
        self.ctx = ctx
        self.cols = columns(np.random.default_rng(99), N_SEG, blocks_of(N_SEG, block))
        self.seg = native.DeviceSegment(ctx, [c.native() for c in self.cols])

    def close(self):
        self.seg.close()


@pytest.fixture(scope="module")
def uniform(ctx):
    s = Segment(ctx, 1024)
    yield s
    s.close()


@pytest.fixture(scope="module")
def ragged(ctx):
    s = Segment(ctx, 1000)
    yield s
    s.close()


class Table:
    def __init__(self, ctx):
        from immutable3_amd import native
        rng = np.random.default_rng(5)
        self.ctx = ctx
        self.cols = [columns(rng, n, blocks_of(n, 1024)) for n in TABLE_ROWS]
        self.segs = [native.DeviceSegment(ctx, [c.native() for c in cols]) for cols in self.cols]
        self.table = native.DeviceTable(ctx, self.segs)

    def close(self):
        self.table.close()
        for s in self.segs:
            s.close()

    def masks(self, used, leaves, tree):
        return [expected_masks([cols[i] for i in used], leaves, tree) for cols in self.cols]

    def keep(self, used, leaves, tree):
        return [np.concatenate(m) for m in self.masks(used, leaves, tree)]


@pytest.fixture(scope="module")
def tb(ctx):
    t = Table(ctx)
    yield t
    t.close()


# (used columns, leaves, tree): the trees of the issue that fit the tile form
TILE_TREES = {
    "not state in (CA)": ([STATE], [(0, MATCH, [b"CA"])], (NOT, 0)),
    "not state in (8 values)": ([STATE], [(0, MATCH, CODES[:8])], (NOT, 0)),
    "age > 30 and not state in (CA, NY)": ([AGE, STATE], [(0, GT, 30.0), (1, MATCH, [b"CA", b"NY"])], (AND, 0, (NOT, 1))),      # in-lane kinds, a negated mask
    "id < 1000 or not state in (CA)": ([ID, STATE], [(0, LT, 1000.0), (1, MATCH, [b"CA"])], (OR, 0, (NOT, 1))),                 # row-strided kinds
    "not (age > 18 and age < 30)": ([AGE], [(0, GT, 18.0), (0, LT, 30.0)], (NOT, (AND, 0, 1))),
    "not id = 7": ([ID], [(0, EQ, 7.0)], (NOT, 0)),
    "not (not state in (CA) or age < 5)": ([STATE, AGE], [(0, MATCH, [b"CA"]), (1, LT, 5.0)], (NOT, (OR, (NOT, 0), 1))),
    "not state in (wrong lengths only)": ([STATE], [(0, MATCH, [b"CAL", b"N"])], (NOT, 0)),                                         # universal: the NoSelect form
}
GENERIC_TREES = {
    "not code in (ab12)": ([CODE], [(0, MATCH, [b"ab12"])], (NOT, 0)),
    "a union of 9 exclusions": ([STATE], [(0, MATCH, CODES[:5]), (0, MATCH, CODES[5:9])], (AND, (NOT, 0), (NOT, 1))),
    "nine terms": ([ID, AGE], [(0, EQ, 10.0), (0, EQ, 20.0), (1, EQ, 10.0), (1, EQ, 20.0)], (AND, (NOT, (OR, 0, 1)), (NOT, (OR, 2, 3)))),
}


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


def check_segment(s, used, leaves, tree, form, block):
    """run_select and run_count of one tree query: the bitmap word for word, the count its popcount, the form"""
    from immutable3_amd import native
    masks = expected_masks([s.cols[i] for i in used], leaves, tree, block)
    want = words_of_masks(masks)
    want_count = int(sum(int(m.sum()) for m in masks))
    assert popcount(want) == want_count
    q = native.DeviceQuery(s.ctx, s.seg, used, leaves, expr=postfix(tree))
    q.run_select()
    got = q.bitmap()
    assert got.tolist() == want.tolist()
    assert q.count() == want_count == popcount(got)
    assert q.expr_form() == form
    q.run_count()
    assert q.count() == want_count
    q.close()
    return want_count


@pytest.mark.parametrize("name", list(TILE_TREES))
def test_tile_form_over_one_segment(uniform, name):
    used, leaves, tree = TILE_TREES[name]
    cnt = check_segment(uniform, used, leaves, tree, TILE, 1024)
    assert 0 < cnt <= N_SEG and (cnt == N_SEG) == ("wrong lengths" in name)


def test_normal_forms_of_the_generic_trees():
    """what sends each of them to the generic kernel"""
    from immutable3_amd import native
    codecs, widths = [DENSE_INT, DENSE_TINYINT, DENSE_STRING, DENSE_STRING], [4, 1, 2, 4]
    def norm(name):
        used, leaves, tree = GENERIC_TREES[name]
        return native.expr_normalize(codecs, widths, [(used[c], k, v) for c, k, v in leaves], postfix(tree))
    assert norm("not code in (ab12)") == [[{"col": CODE, "not_match": [b"ab12"]}]]
    assert norm("a union of 9 exclusions") == [[{"col": STATE, "not_match": CODES[:9]}]]
    assert len(norm("nine terms")) == 9


@pytest.mark.parametrize("name", list(GENERIC_TREES))
def test_generic_form_over_one_segment(uniform, name):
    used, leaves, tree = GENERIC_TREES[name]
    cnt = check_segment(uniform, used, leaves, tree, GENERIC, 1024)
    assert 0 < cnt < N_SEG


@pytest.mark.parametrize("name", list(TILE_TREES) + list(GENERIC_TREES))
def test_ragged_layout(ragged, name):
    """blocks of 1000 rows: every batch starts a fresh word and ends in one of 40 valid bits -- where a complement would leak"""
    used, leaves, tree = {**TILE_TREES, **GENERIC_TREES}[name]
    check_segment(ragged, used, leaves, tree, GENERIC, 1000)


def check_table(tb, used, leaves, tree):
    from immutable3_amd import native
    masks = tb.masks(used, leaves, tree)
    q = native.DeviceQuery(tb.ctx, tb.table, used, leaves, expr=postfix(tree))
    q.run_select()
    words, count = q.bitmap(), q.count()
    _, fw = q.segment_starts()
    total = 0
    for si, m in enumerate(masks):
        want = words_of_masks(m)
        total += int(sum(int(x.sum()) for x in m))
        lo = int(fw[si])
        assert words[lo: lo + want.size].tolist() == want.tolist(), si
        assert not words[lo + want.size: int(fw[si + 1])].any(), si                  # padding up to the next segment's first tile
    assert count == total == popcount(words)
    assert q.expr_form() == TILE
    q.run_count()
    assert q.count() == total
    q.close()
    return total


@pytest.mark.parametrize("name", list(TILE_TREES))
def test_tile_form_over_a_table(tb, name):
    used, leaves, tree = TILE_TREES[name]
    cnt = check_table(tb, used, leaves, tree)
    assert (cnt == sum(TABLE_ROWS)) == ("wrong lengths" in name)


def test_table_projection_with_a_limit_and_group_by(tb):
    from immutable3_amd import native
    used, leaves, tree = [AGE, STATE, ID], [(0, GT, 30.0), (1, MATCH, [b"CA", b"NY"])], (AND, 0, (NOT, 1))
    keep = tb.keep(used, leaves, tree)
    want = [(si, int(r)) for si, k in enumerate(keep) for r in np.flatnonzero(k)]
    q = native.DeviceQuery(tb.ctx, tb.table, used, leaves, [2, 1], 10, expr=postfix(tree))
    q.run()
    pl = q.plan()
    assert not pl["single_pass"] and not pl["records"]
    idx, vals = q.fetch_rows()
    seg_of, row_of = q.locate_rows(idx)
    assert list(zip(seg_of.tolist(), row_of.tolist())) == want[:10] and q.count() == len(want)
    assert vals[0].view("<i4").reshape(-1).tolist() == [int(tb.cols[s][ID].values[r]) for s, r in want[:10]]
    assert vals[1].tobytes() == b"".join(bytes(tb.cols[s][STATE].values[r]) for s, r in want[:10])
    q.close()
    # group by state: count + max(age), first-seen order over (segment, row)
    groups = {}
    for s, r in want:
        k, a = bytes(tb.cols[s][STATE].values[r]), int(tb.cols[s][AGE].values[r])
        c, m = groups.get(k, (0, a))
        groups[k] = (c + 1, max(m, a))
    q = native.DeviceQuery(tb.ctx, tb.table, used, leaves, group_cols=[1], aggs=[(native.AGG_COUNT, 0), (native.AGG_MAX, 0)], expr=postfix(tree))
    q.run()
    keys, _, counts, gvals = q.fetch_groups()
    got = {int(keys[g]).to_bytes(8, "little")[:2]: (int(counts[g]), int(gvals[g, 1])) for g in range(keys.shape[0])}
    assert list(got.keys()) == list(groups.keys()) and got == groups
    assert b"CA" not in got and b"NY" not in got and q.count() == len(want)
    q.close()


def test_table_refusals(tb):
    from immutable3_amd import native
    for name, needle in (("not code in (ab12)", "2-byte"), ("a union of 9 exclusions", "at most 8 values")):
        used, leaves, tree = GENERIC_TREES[name]
        for kw in ({}, {"group_cols": [0], "aggs": [(native.AGG_COUNT, 0)]}):
            with pytest.raises(native.Imm3Error) as e:
                native.DeviceQuery(tb.ctx, tb.table, used, leaves, expr=postfix(tree), **kw)
            assert e.value.code == native.ERR_ARG and e.value.msg.startswith(native.TABLE_TREE_REFUSED) and needle in e.value.msg, e.value.msg
    for target in (tb.table, tb.segs[0]):                                  # a lone NOT: a malformed program, no refusal
        with pytest.raises(native.Imm3Error) as e:
            native.DeviceQuery(tb.ctx, target, [STATE], [(0, MATCH, [b"CA"])], expr=[native.EXPR_NOT])
        assert e.value.code == native.ERR_ARG and "stack underflow" in e.value.msg and not e.value.msg.startswith(native.TABLE_TREE_REFUSED)
    with pytest.raises(native.Imm3Error) as e:                             # the leaf itself stays what the reference makes of it
        native.DeviceQuery(tb.ctx, tb.table, [STATE], [(0, native.NOTMATCH, [b"CA"])], expr=[0])
    assert e.value.code == native.ERR_UNSUPPORTED_CONDITION


def test_match_then_not_is_the_inverted_match_bitmap(uniform, ragged, tb):
    from immutable3_amd import native
    leaf = [(0, MATCH, [b"CA", b"TX"])]

    def inverted(words, batch_rows):
        """~words confined to each batch's valid rows (every batch starts a fresh word)"""
        out, w = [], 0
        for n in batch_rows:
            nw = -(-n // 64)
            inv = ~words[w: w + nw]
            if n % 64:
                inv[-1] &= np.uint64((1 << (n % 64)) - 1)
            out.append(inv)
            w += nw
        return np.concatenate(out), w

    for s, block in ((uniform, 1024), (ragged, 1000)):
        flat = native.DeviceQuery(s.ctx, s.seg, [STATE], leaf)
        flat.run_select()
        neg = native.DeviceQuery(s.ctx, s.seg, [STATE], leaf, expr=[0, native.EXPR_NOT])
        neg.run_select()
        want, used_words = inverted(flat.bitmap(), blocks_of(N_SEG, block))
        assert used_words == flat.bitmap().size and neg.bitmap().tolist() == want.tolist()
        assert neg.count() == N_SEG - flat.count()
        flat.close()
        neg.close()
    flat = native.DeviceQuery(tb.ctx, tb.table, [STATE], leaf)
    flat.run_select()
    neg = native.DeviceQuery(tb.ctx, tb.table, [STATE], leaf, expr=[0, native.EXPR_NOT])
    neg.run_select()
    fw_words, nw_words = flat.bitmap(), neg.bitmap()
    _, fw = flat.segment_starts()
    for si, n in enumerate(TABLE_ROWS):
        lo, hi = int(fw[si]), int(fw[si + 1])
        want, used_words = inverted(fw_words[lo:hi], blocks_of(n, 1024))
        assert nw_words[lo: lo + used_words].tolist() == want.tolist() and not nw_words[lo + used_words: hi].any()
    assert neg.count() == sum(TABLE_ROWS) - flat.count()
    flat.close()
    neg.close()


# ---- fuzz: 40 seeded random trees with NOT nodes, on whichever form each takes ----
# FUZZ_SEED was chosen on the CPU (imm3_expr_normalize tells the form without a device) so that the normaliser alone keeps the trees
# the table refuses within a quarter: with this seed 6 of the 40 normal forms do not fit the table's tile form (FUZZ_REFUSED).
FUZZ_SEED, FUZZ_TREES, FUZZ_REFUSED = 20261018, 40, 6


def fuzz_leaf(rng):
    col = int(rng.choice([ID, AGE, STATE, CODE], p=[0.3, 0.32, 0.32, 0.06]))
    if col == STATE:
        k = int(rng.integers(1, 5))
        return (col, MATCH, [CODES[i] for i in rng.choice(len(CODES), size=k, replace=False)] + ([b"XYZ"] if rng.random() < 0.2 else []))
    if col == CODE:
        return (col, MATCH, [CODES4[int(rng.integers(0, len(CODES4)))]])
    if col == ID:
        return (col, int(rng.choice([GT, LT, EQ])), float(rng.choice([-2.0 ** 31, 7.0, 500.0, 1500.0, 1e12])))
    return (col, int(rng.choice([GT, LT, EQ])), float(rng.choice([5.0, 18.0, 30.0, 65.0, 99.0, 200.0])))


def fuzz_cases():
    rng = np.random.default_rng(FUZZ_SEED)
    out = []
    for _ in range(FUZZ_TREES):
        n = int(rng.integers(2, 6))
        out.append(([fuzz_leaf(rng) for _ in range(n)], random_tree(rng, n)))
    return out


def fits_table(terms):
    """the tile form's rules on a normal form (the universal and the empty one run without a tree launch)"""
    preds = [p for t in terms for p in t]
    lists = [p.get("match", p.get("not_match")) for p in preds if "lo" not in p]
    return len(terms) <= 8 and all(p["col"] != CODE for p in preds) and all(len(v) <= 8 for v in lists) and len({p["col"] for p in preds}) <= 3


def test_fuzz_seed_keeps_the_table_refusals_within_a_quarter():
    from immutable3_amd import native
    codecs, widths = [DENSE_INT, DENSE_TINYINT, DENSE_STRING, DENSE_STRING], [4, 1, 2, 4]
    forms = [native.expr_normalize(codecs, widths, leaves, postfix(tree)) for leaves, tree in fuzz_cases()]
    refused = sum(not fits_table(f) for f in forms)
    assert refused == FUZZ_REFUSED and 4 * refused <= FUZZ_TREES
    # ... and the trees are about NOT: nearly all hold one, and in many a negated list reaches the kernels (so a later change to
    # random_tree's defaults cannot hollow the fuzz out).  With this seed: 39 trees with a NOT, 18 normal forms with a negated list.
    with_not = sum(has_not(tree) for _, tree in fuzz_cases())
    negated_lists = sum(any("not_match" in p for t in f for p in t) for f in forms)
    assert with_not >= 30 and negated_lists >= 12, (with_not, negated_lists)


def test_fuzz(uniform, tb):
    from immutable3_amd import native
    used = [ID, AGE, STATE, CODE]
    codecs, widths = [DENSE_INT, DENSE_TINYINT, DENSE_STRING, DENSE_STRING], [4, 1, 2, 4]
    refused = 0
    for case, (leaves, tree) in enumerate(fuzz_cases()):
        prog = postfix(tree)
        masks = expected_masks(uniform.cols, leaves, tree)
        want = words_of_masks(masks)
        q = native.DeviceQuery(uniform.ctx, uniform.seg, used, leaves, expr=prog)
        q.run_select()
        assert q.bitmap().tolist() == want.tolist() and q.count() == popcount(want), (case, leaves, tree)
        q.close()
        fits = fits_table(native.expr_normalize(codecs, widths, leaves, prog))
        try:
            qt = native.DeviceQuery(tb.ctx, tb.table, used, leaves, expr=prog)
        except native.Imm3Error as e:
            assert e.code == native.ERR_ARG and e.msg.startswith(native.TABLE_TREE_REFUSED) and not fits, (case, e.msg)
            refused += 1
            for si, cols in enumerate(tb.cols):                              # a refusal passes only when the per-segment queries are right
                qs = native.DeviceQuery(tb.ctx, tb.segs[si], used, leaves, expr=prog)
                qs.run_select()
                ws = words_of_masks(expected_masks(cols, leaves, tree))
                assert qs.bitmap().tolist() == ws.tolist() and qs.count() == popcount(ws), (case, si)
                qs.close()
            continue
        assert fits, (case, leaves, tree)
        qt.run_select()
        words = qt.bitmap()
        _, fw = qt.segment_starts()
        total = 0
        for si, cols in enumerate(tb.cols):
            ws = words_of_masks(expected_masks(cols, leaves, tree))
            total += popcount(ws)
            lo = int(fw[si])
            assert words[lo: lo + ws.size].tolist() == ws.tolist() and not words[lo + ws.size: int(fw[si + 1])].any(), (case, si, leaves, tree)
        assert qt.count() == total
        qt.close()
    assert refused == FUZZ_REFUSED and 4 * refused <= FUZZ_TREES


def test_graph_replay(uniform):
    from immutable3_amd import native
    used, leaves, tree = TILE_TREES["age > 30 and not state in (CA, NY)"]
    q = native.DeviceQuery(uniform.ctx, uniform.seg, used, leaves, expr=postfix(tree))
    q.run_select()
    words, count = q.bitmap(), q.count()
    assert words.tolist() == words_of_masks(expected_masks([uniform.cols[i] for i in used], leaves, tree)).tolist()
    with uniform.ctx.capture() as cap:
        q.run_select()
    graph = cap.graph
    graph.launch()
    assert q.count() == count and q.bitmap().tolist() == words.tolist()
    graph.close()
    q.close()


# ---- the engines ----
def loader_made_table(path):
    """three README-style segments as the loader cuts them (a trailing 1-row block) and a short last one"""
    from immutable3_amd import synth
    from immutable3_amd.schema import TableIO
    from immutable3_amd.storage import write_segment_arrays
    t = synth.table_schema("tn", 1024)
    TableIO.store(str(path), t)
    ids, age, st = [], [], []
    for s in range(3):
        n = 2 * 1024 + 1 if s < 2 else 700
        cols = {"id": (np.arange(n, dtype=np.int64) + s * 10 ** 5).astype(np.int32),
                "age": synth.uniform_below(30 + s, n, 100, np.int8), "state": synth.state_codes(40 + s, n, ["CA", "NY", "TX", "WA", "FL"])}
        write_segment_arrays(str(path), t, s, cols, block_rows=([1024] * 2 + [1]) if s < 2 else [700])
        ids.append(cols["id"]), age.append(cols["age"]), st.append(cols["state"])
    return np.concatenate(ids), np.concatenate(age).astype(np.int64), np.concatenate(st)


def engine_queries(ids, age, st):
    """(SelectADT, numpy keep) for: the NotMatch leaf alone, under an And, under an Or"""
    from immutable3_amd.query import GT as QGT, And, NotMatch, Or, Select
    not_ca = ~((st[:, 0] == ord("C")) & (st[:, 1] == ord("A")))
    leaf = Select("state", NotMatch(["CA"]))
    return [(leaf, not_ca), (And(Select("age", QGT(30)), leaf), (age > 30) & not_ca), (Or(Select("age", QGT(90)), leaf), (age > 90) | not_ca)]


def test_python_engine(tmp_path):
    from immutable3_amd.operators import Engine, GpuSegmentManager
    from immutable3_amd.query import Count, Max, Project, ProjectAgg, Query
    from immutable3_amd.storage import SegmentManager
    ids, age, st = loader_made_table(tmp_path)
    gsm = GpuSegmentManager(SegmentManager(str(tmp_path)))
    try:
        assert gsm.device_table("tn") is not None
        on, off = Engine(gsm, honour_not_match=True), Engine(gsm)
        for sel, keep in engine_queries(ids, age, st):
            assert keep.any() and not keep.all()
            want = list(zip(ids[keep].tolist(), age[keep].tolist()))
            for limit in (0, 10):
                q = Query("tn", sel, Project(["id", "age"], limit))
                exp = want[:limit] if limit else want
                assert on.execute_table_columns(q) is not None                    # the one table launch was taken
                assert [(r[0], r[1]) for r in on.execute(q)] == exp
                per_segment = [row for _, proj in on.pipelines(q) for row in proj.iterator()]       # SelectTreeOp per segment
                assert [(r[0], r[1]) for r in per_segment][:len(exp)] == exp
                assert [(i, a) for _, _, c in on.execute_columns(q) for i, a in zip(c[0].tolist(), c[1].tolist())][:len(exp)] == exp
            groups = {}
            for i in np.flatnonzero(keep):
                k = bytes(st[i]).decode()
                c, m = groups.get(k, (0, None))
                groups[k] = (c + 1, int(age[i]) if m is None else max(m, int(age[i])))
            res = on.execute_agg(Query("tn", sel, ProjectAgg([Count("id"), Max("age")], ["state"])))
            assert list(res.keys()) == list(groups.keys())
            for k, aggmap in res.items():
                got = [a.get() for a in aggmap.values()]
                assert (int(got[0]), float(got[1])) == (groups[k][0], float(groups[k][1])), k
            # flag off: the reference's refusal, wherever the query goes
            for run in (lambda: list(off.execute(Query("tn", sel, Project(["id"], 0)))),
                        lambda: off.execute_columns(Query("tn", sel, Project(["id"], 0))),
                        lambda: off.execute_table_columns(Query("tn", sel, Project(["id"], 0))),
                        lambda: off.execute_agg(Query("tn", sel, ProjectAgg([Count("id")], ["state"])))):
                with pytest.raises(Exception, match="Unsupported condition"):
                    run()
    finally:
        gsm.close()


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cpp_engine(tmp_path):
    """host/operators.hpp's Engine(sm, honourAndOr, honourNotMatch) through a small stand-alone program (tests/native/engine_not.cpp):
    the same three queries over the same directory, rows and groups against numpy; flag off: "Unsupported condition" """
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    data = tmp_path / "data"
    data.mkdir()
    ids, age, st = loader_made_table(data)
    exe = str(tmp_path / "engine_not")
    lib = os.path.join(root, "immutable3_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O0", os.path.join(here, "native", "engine_not.cpp"), "-o", exe,
                           "-L", lib, "-limm3", f"-Wl,-rpath,{lib}"])
    for which, (_, keep) in enumerate(engine_queries(ids, age, st)):
        r = subprocess.run([exe, str(data), str(which), "1"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        rows = [l for l in r.stdout.splitlines() if l.startswith("Row(")]
        groups = [l[len("group "):] for l in r.stdout.splitlines() if l.startswith("group ")]
        assert rows == [f"Row({i},{a})" for i, a in zip(ids[keep].tolist(), age[keep].tolist())]
        want = {}
        for i in np.flatnonzero(keep):
            k = bytes(st[i])
            c, m = want.get(k, (0, None))
            want[k] = (c + 1, int(age[i]) if m is None else max(m, int(age[i])))
        assert groups == [f"Row({c},{float(m)})" for c, m in want.values()]
        r = subprocess.run([exe, str(data), str(which), "0"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 3 and "Unsupported condition" in r.stderr, (r.returncode, r.stderr[-2000:])
