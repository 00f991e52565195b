"""Seeded differential fuzzing of TABLE queries (imm3_table: one launch over the tile table of all segments) against the oracles run
per segment and concatenated in segment order (table_fuzz_util.py: the generator and the reference side).  What test_gpu_fuzz.py is
to one segment: random segment counts and lengths (empty and one-row segments in the middle included), block layouts, codecs per
column, predicates at random selectivities, SELECT lists, limits, reservations, group-bys and select trees.

Bit-exact, no tolerance anywhere: bitmap words per segment at segment_starts, zero padding up to the next segment's first word, the
global count, the batches() layout per segment, row identity through locate_rows, the bytes of every projected column, the global
limit cut in (segment, row) order; group keys, first-seen order, counts and values.  test_table_fuzz_host.py walks the same seeds on
the CPU and asserts that none of this is hollow."""
import os

import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT
from immutable3_amd import native
from table_fuzz_util import (GROUP_SEEDS, LIMIT_SEEDS, NAME, SELECT_SEEDS, STATE, TREE_COUNT, TREE_REFUSED, Expected, expected_groups,
                             group_cases, limit_case_stops, limit_cases, limit_of, limit_rng, postfix, random_limit_table, select_cases,
                             tree_cases, tree_is_refused, tree_keep)
from test_gpu_str_rows_table import check_select
from test_gpu_table_limit import read_words, shrunk

pytestmark = pytest.mark.gpu
MORE = int(os.environ.get("IMM3_FUZZ_MORE", "0"))      # extra seeds per fuzzer for a long hunt (default: the bounded set)
KIND = {"count": native.AGG_COUNT, "min": native.AGG_MIN, "max": native.AGG_MAX, "sum": native.AGG_SUM}
VALUE_CODECS = [DENSE_INT, DENSE_INT, DENSE_TINYINT, DENSE_STRING, DENSE_STRING]


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.set_tuning(0, 0)
    c.close()


class OnDevice:
    """a FuzzTable's segments and its imm3_table"""

    def __init__(self, ctx, t):
        self.segs = [native.DeviceSegment(ctx, [c.native() for c in cols]) for cols in t.segs]
        self.table = native.DeviceTable(ctx, self.segs)

    def close(self):
        self.table.close()
        for s in self.segs:
            s.close()


def check_layout(q, e):
    size, oid, woff = q.batches()
    fb, fw = q.segment_starts()
    assert fb.size == len(e.layouts) + 1
    for si, (osize, ooid, owoff) in enumerate(e.layouts):
        b0, b1 = int(fb[si]), int(fb[si + 1])
        assert size[b0:b1].tolist() == osize.tolist() and oid[b0:b1].tolist() == ooid.tolist(), si
        assert (woff[b0:b1] - fw[si]).tolist() == owoff.tolist(), si


def check_rows(q, e, k, what):
    """the query's rows are the first k survivors in (segment, row) order, with the oracle's bytes in every projected column"""
    idx, vals = q.fetch_rows()
    assert idx.size == k and q.row_count() == k, (what, idx.size, k)
    seg_of, row_of = q.locate_rows(idx)
    assert np.array_equal(seg_of, e.seg[:k]) and np.array_equal(row_of, e.row[:k]), what
    for j in range(len(e.vals)):
        assert vals[j].tobytes() == np.ascontiguousarray(e.vals[j][:k]).tobytes(), (what, "column", j)


def run_flat(ctx, dev, t, fq, e, limit, what):
    """run(), every getter; run_count() gives the same count; run_select() brings the bitmap back; a second run() the same rows"""
    q = native.DeviceQuery(ctx, dev.table, fq.used, fq.sels, fq.proj, limit, 1024)
    if fq.reserve is not None:
        q.reserve_rows(fq.reserve)
    k = min(limit, e.total) if limit > 0 else e.total
    q.run()
    check_select(q, e.per_seg)
    check_layout(q, e)
    if fq.proj:
        check_rows(q, e, k, what)
    q.run_count()
    assert q.count() == e.total, what
    q.run_select()
    check_select(q, e.per_seg)
    q.run()
    if fq.proj:
        check_rows(q, e, k, (what, "second run"))
    check_select(q, e.per_seg)
    q.close()


@pytest.mark.parametrize("seed", range(SELECT_SEEDS + MORE))
def test_fuzz_table_select_project(ctx, oracle, seed):
    for ti, (t, queries) in enumerate(select_cases(seed)):
        dev = OnDevice(ctx, t)
        for qi, fq in enumerate(queries):
            e = Expected(oracle, t, fq.used, fq.sels, fq.proj)
            for kind in fq.limit_kinds:
                run_flat(ctx, dev, t, fq, e, limit_of(kind, e.counts), (seed, ti, qi, kind, t.describe(), fq.used, fq.sels, fq.proj))
        dev.close()


@pytest.mark.parametrize("seed", range(LIMIT_SEEDS + MORE))
def test_fuzz_table_limit_stops_right(ctx, oracle, seed):
    """Tables of more tiles than the shrunken launch claims at once, so the stopping launch (k_filter_table_limit) engages wherever the
    plan allows it -- every case but the ones with a wide-string Match beside the range, which keep the whole select
    (limit_case_stops; those cases check the same rows through the other path).  The rows and values of a run, then count and
    bitmap (the whole table's), then the rows again, then a further run.  That the stopping launch ran is read from the finish
    block (its scanned-tile word is written by that launch alone); how far it went is not asserted (test_gpu_table_limit.py:
    check_stopped says why that is no invariant)."""
    rng = limit_rng(seed)
    t, G = random_limit_table(rng, seed)
    assert sum(t.tiles) > G * native.TABLE_LIMIT_CLAIM_TILES
    dev = OnDevice(ctx, t)
    for what, used, sels, proj in limit_cases(rng, t, seed):
        e = Expected(oracle, t, used, sels, proj)
        for limit in sorted({1, 10, max(1, e.total // 2), 1000, e.total + 7}):
            tag = (seed, G, what, limit, t.seg_rows, t.codecs)
            k = min(limit, e.total)
            with shrunk(ctx, G):
                q = native.DeviceQuery(ctx, dev.table, used, sels, proj, limit, 1024)
                assert q.total_words == sum(t.tiles) * 16
                for rnd in range(2):
                    q.run()
                    if rnd == 0 and limit_case_stops(used, sels):
                        ctx.sync()
                        head, _ = read_words(q, 1)
                        assert 0 < int(head[native.FINISH_LIMIT_TILES]) <= sum(t.tiles), tag
                    check_rows(q, e, k, (tag, rnd))
                assert q.count() == e.total, tag                            # the whole select runs now: the table's count
                check_select(q, e.per_seg)
                check_rows(q, e, k, (tag, "after the getters"))
                q.run()                                                       # and a stopping run again behind the whole one
                check_rows(q, e, k, (tag, "a further run"))
                q.close()
    dev.close()


def check_groups(ctx, dev, t, aq, keep, what):
    want_keys, want_first, want_counts, want_vals = expected_groups(t, aq, keep)
    q = native.DeviceQuery(ctx, dev.table, aq.used, aq.sels, (), 0, 1024, group_cols=aq.group, aggs=[(KIND[k], c) for k, c in aq.aggs],
                           wide_keys=aq.wide_keys)
    q.run()
    keys, first, counts, vals = q.fetch_groups()
    g = len(want_counts)
    assert keys.size == g, (what, keys.size, g)
    assert counts.tolist() == want_counts, what                              # (first-seen order: the counts line up group by group)
    prefix = [int.from_bytes(bytes(kb[:8]), "little") for kb in want_keys]   # keys[g]: the first 8 key bytes little-endian
    assert keys.tolist() == prefix, what
    if aq.wide_keys:
        got_kb = q.fetch_group_keys()
        assert got_kb.shape == want_keys.shape and got_kb.tobytes() == want_keys.tobytes(), what
    seg_of, row_of = q.locate_rows(first)                                     # every group's first selected row, as (segment, row)
    want_seg = np.repeat(np.arange(len(t.seg_rows)), t.seg_rows)[want_first]
    assert seg_of.tolist() == want_seg.tolist() and row_of.tolist() == (want_first - t.starts[want_seg]).tolist(), what
    for j, (kind, c) in enumerate(aq.aggs):
        col = aq.used[c]
        want = [v[j] for v in want_vals]
        if kind != "count" and col in (STATE, NAME):                          # a string MAX: its first 8 bytes big-endian, and the exact bytes
            assert vals[:, j].tolist() == [int.from_bytes(w[:8], "big") for w in want], (what, j)
            assert [bytes(r) for r in q.fetch_group_strings(j)] == want, (what, j)
        else:
            assert [int(x) for x in vals[:, j]] == want, (what, j)
    q.close()


@pytest.mark.parametrize("seed", range(GROUP_SEEDS + MORE))
def test_fuzz_table_group_by(ctx, oracle, seed):
    """Random aggregations over random tables: groups in first-seen order over (segment, row); SUM, count / min / max, string maxima,
    and name as a group key through the wide-key entry point.  (The numpy expectation is held against oracle_np.project_agg +
    combine_agg on the CPU, for the aggregates that knows: test_table_fuzz_host.py.)"""
    for ti, (t, queries) in enumerate(group_cases(seed)):
        dev = OnDevice(ctx, t)
        for qi, aq in enumerate(queries):
            keep = Expected(oracle, t, aq.used, aq.sels, [0]).keep(t)
            check_groups(ctx, dev, t, aq, keep, (seed, ti, qi, t.describe(), aq.used, aq.sels, aq.group, aq.aggs, aq.wide_keys))
        dev.close()


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


def test_fuzz_table_trees(ctx):
    """Random AND / OR / NOT trees over random tables through imm3_query_create_table_expr, with a projection and a limit: the bitmap
    and the count are the whole table's (a tree scans it all), the limit cuts the rows.  A tree the table refuses passes only when
    the normal form predicts the refusal and the per-segment queries are right."""
    tables, cases = tree_cases()
    devs = [OnDevice(ctx, t) for t in tables]
    used = [0, 1, 2, 3, 4]
    refused = 0
    for case, (ti, leaves, tree, proj, limit_kind) in enumerate(cases):
        t, dev = tables[ti], devs[ti]
        prog = postfix(tree)
        tag = (case, t.describe(), leaves, tree, proj, limit_kind)
        words, keep = tree_keep(t, leaves, tree)
        predicted = tree_is_refused(t, tree, native.expr_normalize(VALUE_CODECS, t.widths, leaves, prog))
        rows = np.flatnonzero(keep)
        limit = {"none": 0, "one": 1, "half": max(1, rows.size // 2), "total": rows.size, "total + 7": rows.size + 7}[limit_kind]
        try:
            q = native.DeviceQuery(ctx, dev.table, used, leaves, proj, limit, 1024, expr=prog)
        except native.Imm3Error as err:
            assert err.code == native.ERR_ARG and err.msg.startswith(native.TABLE_TREE_REFUSED) and predicted, (tag, err.msg)
            refused += 1
            for si, seg in enumerate(dev.segs):                               # a refusal passes only when the per-segment queries are right
                qs = native.DeviceQuery(ctx, seg, used, leaves, expr=prog)
                qs.run_select()
                assert qs.bitmap().tolist() == words[si].tolist() and qs.count() == popcount(words[si]), (tag, si)
                qs.close()
            continue
        assert not predicted, tag
        for rnd in range(2):
            q.run()
            got = q.bitmap()
            _, fw = q.segment_starts()
            for si, ws in enumerate(words):
                lo = int(fw[si])
                assert got[lo: lo + ws.size].tolist() == ws.tolist() and not got[lo + ws.size: int(fw[si + 1])].any(), (tag, si, rnd)
            assert q.count() == rows.size, (tag, rnd)
            want = rows[:limit] if limit > 0 else rows
            idx, vals = q.fetch_rows()
            assert idx.size == want.size, (tag, rnd, idx.size, want.size)
            seg_of, row_of = q.locate_rows(idx)
            want_seg = np.repeat(np.arange(len(t.seg_rows)), t.seg_rows)[want]
            assert seg_of.tolist() == want_seg.tolist() and row_of.tolist() == (want - t.starts[want_seg]).tolist(), (tag, rnd)
            for j, c in enumerate(proj):
                assert vals[j].tobytes() == t.value_bytes(c, want).tobytes(), (tag, rnd, "column", j)
        q.close()
    for d in devs:
        d.close()
    assert refused == TREE_REFUSED and 4 * refused <= TREE_COUNT
