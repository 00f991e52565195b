"""GPU suite: `limit` stops the scan of a TABLE query, in one launch.  ProjectIterator.hasNext ends after `limit` rows
(engine/src/main/scala/immutabledb/engine/operator/Project.scala:73-80) and the per-segment workers stall on the bounded result queue
(engine/Engine.scala:166,253-258): segments behind the limit are never scanned.  Over an imm3_table the select launch's work-groups
claim runs of TABLE_LIMIT_CLAIM_TILES consecutive virtual tiles from one ticket counter, in ascending order, and stop claiming once
the finished runs hold `limit` rows (csrc/imm3_kernels.hip: k_filter_table_limit); the offsets scan and the gather stop at the claimed
prefix.  Checked on the loader's quirk shape (every segment ends in a one-row partial tile), with the launch shrunk to a few
work-groups so that a table of a few hundred tiles is more than they claim at once: the rows are the first `limit` survivors in
(segment, row) order (numpy, and the C oracle per segment) for limits met in the first tile, across a segment boundary, in the last
third and never; count and bitmap stay the whole table's; the scan really stops (the bitmap lines behind the scanned prefix keep
their poison); a recorded graph replays the stopped scan; the vetoes keep the whole select."""
import ctypes as C

import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, GT, LT, MATCH, RawColumn, blocks_of
from immutable3_amd import native

pytestmark = pytest.mark.gpu

CLAIM = native.TABLE_LIMIT_CLAIM_TILES
SEG_ROWS, SEG_TILES = 8 * 1024 + 1, 9          # the loader's quirk: full blocks and a trailing one-row block -> a one-row partial tile
N_SEGS = 48
N_TILES = N_SEGS * SEG_TILES                    # 432 = 13 claims and half a claim
POISON = 0xA5A5A5A5A5A5A5A5
CODES = [b"CA", b"NY", b"TX", b"WA", b"VA", b"DC", b"CT"]


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.set_tuning(0, 0)
    c.close()


class Table:
    """id:int32 ascending over the whole table, age:int8, state:string(2); numpy's view of it in rows and in virtual tiles."""

    def __init__(self, ctx, n_segs, seed=5):
        rng = np.random.default_rng(seed)
        self.n_segs, self.n_tiles = n_segs, n_segs * SEG_TILES
        self.cols, self.dsegs = [], []
        for s in range(n_segs):
            ids = np.arange(s * SEG_ROWS, (s + 1) * SEG_ROWS, dtype=np.int32)
            age = rng.integers(0, 100, size=SEG_ROWS).astype(np.int8)
            st = np.array([list(c) for c in CODES], dtype=np.uint8)[rng.integers(0, len(CODES), size=SEG_ROWS)].reshape(SEG_ROWS, 2)
            br = blocks_of(SEG_ROWS, 1024)
            cols = [RawColumn(DENSE_INT, 4, ids, br), RawColumn(DENSE_TINYINT, 1, age, br), RawColumn(DENSE_STRING, 2, st, br)]
            self.cols.append(cols)
            self.dsegs.append(native.DeviceSegment(ctx, [c.native() for c in cols]))
        self.table = native.DeviceTable(ctx, self.dsegs)
        self.data = [np.concatenate([cols[u].values for cols in self.cols]) for u in range(3)]   # rows of all segments, in order

    def virtual_bitmap(self, keep):
        """the table's bitmap words: every segment's rows start on a fresh tile, bits behind its last row are zero"""
        v = np.zeros((self.n_segs, SEG_TILES * 1024), bool)
        v[:, :SEG_ROWS] = keep.reshape(self.n_segs, SEG_ROWS)
        return np.packbits(v.reshape(-1), bitorder="little").view("<u8")

    def tile_of(self, row):
        """virtual tile of a row of the concatenated table"""
        return (row // SEG_ROWS) * SEG_TILES + (row % SEG_ROWS) // 1024

    def close(self):
        self.table.close()
        for d in self.dsegs:
            d.close()


@pytest.fixture(scope="module")
def tab(ctx):
    t = Table(ctx, N_SEGS)
    yield t
    t.close()


class shrunk:
    """the launch shrunk to `grid_blocks` work-groups (tuning is read by every run), restored afterwards"""

    def __init__(self, ctx, grid_blocks, variant=0):
        self.ctx, self.g, self.v = ctx, grid_blocks, variant

    def __enter__(self):
        self.ctx.set_tuning(self.v, self.g)

    def __exit__(self, *exc):
        self.ctx.set_tuning(0, 0)


hip = None


def _hip():
    global hip
    if hip is None:
        hip = C.CDLL("libamdhip64.so")
    return hip


def poison_bitmap(q, n_tiles):
    p = np.full(n_tiles * 16, POISON, np.uint64)
    assert _hip().hipMemcpy(C.c_void_p(q.device_ptr(0)), C.c_void_p(p.ctypes.data), C.c_size_t(p.nbytes), C.c_int(1)) == 0


def read_words(q, n_tiles):
    """(the finish block's first 16 words, the raw bitmap) as they sit on the device"""
    head = np.zeros(16, np.uint64)
    assert _hip().hipMemcpy(C.c_void_p(head.ctypes.data), C.c_void_p(q.device_ptr(1)), C.c_size_t(head.nbytes), C.c_int(2)) == 0
    raw = np.zeros(n_tiles * 16, np.uint64)
    assert _hip().hipMemcpy(C.c_void_p(raw.ctypes.data), C.c_void_p(q.device_ptr(0)), C.c_size_t(raw.nbytes), C.c_int(2)) == 0
    return head, raw


# used columns index [id, age, state]; keep(ids, age, state) over the concatenated rows
LAST_THIRD = 36 * SEG_ROWS + 100
BOUNDARY = 20 * SEG_ROWS + 8190                 # survivors start at row 8191 of segment 20: one row of its last full tile, its one-row partial tile, segment 21
CASES = {
    "age above 89": ([1, 0], [(0, GT, 89.0)], [1, 0], lambda i, a, s: a > 89),
    "id inside the first segment": ([0, 1], [(0, GT, 4000.0)], [0, 1], lambda i, a, s: i > 4000),
    "id in the last third": ([0, 2, 1], [(0, GT, float(LAST_THIRD))], [2, 0, 1], lambda i, a, s: i > LAST_THIRD),
    "id one row before a segment's end": ([0], [(0, GT, float(BOUNDARY))], [0], lambda i, a, s: i > BOUNDARY),
    "state match": ([2, 0, 1], [(0, MATCH, [b"CA"])], [1, 0, 2], lambda i, a, s: (s[:, 0] == ord("C")) & (s[:, 1] == ord("A"))),
    "nothing survives": ([1, 0], [(0, GT, 100.0)], [1], lambda i, a, s: np.zeros(i.shape[0], bool)),
}
G_ROWS = 3                                      # work-groups of the shrunken launch: 96 tiles claimed at once


def rows_and_values(t, q, proj, used, want, tag):
    idx, vals = q.fetch_rows()
    assert idx.size == want.size, (tag, idx.size, want.size)
    seg_of, row_of = q.locate_rows(idx)
    assert (seg_of == want // SEG_ROWS).all() and (row_of == want % SEG_ROWS).all(), tag
    for j, pj in enumerate(proj):
        assert vals[j].tobytes() == np.ascontiguousarray(t.data[used[pj]][want]).tobytes(), (tag, "column", j)


@pytest.mark.parametrize("name", list(CASES))
def test_rows_are_the_first_survivors_and_count_and_bitmap_stay_the_tables(ctx, tab, name):
    used, sels, proj, keepf = CASES[name]
    keep = keepf(*tab.data)
    rows = np.flatnonzero(keep)
    bitmap = tab.virtual_bitmap(keep)
    for limit in (1, 10, 1000, 5000, rows.size + 7):
        want = rows[:limit]
        with shrunk(ctx, G_ROWS):
            q = native.DeviceQuery(ctx, tab.table, used, sels, proj, limit, 1024)
            assert q.total_words == N_TILES * 16
            for rnd in range(2):
                q.run()
                rows_and_values(tab, q, proj, used, want, (name, limit, rnd))
            assert q.row_count() == want.size
            assert q.count() == rows.size, (name, limit)                    # the whole select runs now: the table's count, not the prefix's
            assert q.bitmap().tobytes() == bitmap.tobytes(), (name, limit)
            rows_and_values(tab, q, proj, used, want, (name, limit, "after the getters"))
            q.run()                                                          # and a stopping run again behind the whole one
            rows_and_values(tab, q, proj, used, want, (name, limit, "a further run"))
            q.close()


def test_against_the_oracle_per_segment(ctx, tab, oracle):
    """select id, age where (age > 18 and age < 30) -- the reference's README query -- against the C oracle's scan_select + project of
    every segment, rows concatenated in segment order and cut at the limit."""
    used, sels, proj = [1, 0], [(0, GT, 18.0), (0, LT, 30.0)], [1, 0]
    exp_seg, exp_row, exp_vals = [], [], [[] for _ in proj]
    for si, cols in enumerate(tab.cols):
        ocols = [cols[u].ocol() for u in used]
        words, _ = oracle.scan_select(ocols, sels, 1024, 1)
        size, _, _, _ = oracle.layout(ocols[0], 1024)
        n, batch, pos, ovals, _ = oracle.project(ocols, proj, 0, 1024, words)
        starts = np.concatenate([[0], np.cumsum(size.astype(np.int64))])
        exp_seg.append(np.full(n, si, np.int64))
        exp_row.append(starts[batch[:n]] + pos[:n])
        for j in range(len(proj)):
            exp_vals[j].append(np.asarray(ovals[j])[:n])
    exp_seg, exp_row = np.concatenate(exp_seg), np.concatenate(exp_row)
    exp_vals = [np.concatenate(v) for v in exp_vals]
    for limit in (1, 10, 1000, 5000, exp_seg.size + 1):
        with shrunk(ctx, G_ROWS):
            q = native.DeviceQuery(ctx, tab.table, used, sels, proj, limit, 1024)
            q.run()
            idx, vals = q.fetch_rows()
            seg_of, row_of = q.locate_rows(idx)
            q.close()
        k = min(limit, exp_seg.size)
        assert idx.size == k, limit
        assert (seg_of == exp_seg[:k]).all() and (row_of == exp_row[:k]).all(), limit
        for j in range(len(proj)):
            assert vals[j].tobytes() == np.ascontiguousarray(exp_vals[j][:k]).tobytes(), (limit, j)


def check_stopped(t, q, head, raw, keep, limit, G, tag):
    """the scanned-tile word and the bitmap behind a stopping run whose survivors start in the first tile.
    The upper bound, one claim per work-group behind the tile that completes the limit, is NOT an invariant of the protocol (a
    work-group that is held back lets the others claim on until its run reports); it holds for the callers' predicates because
    every single run of theirs either meets the limit on its own (id > 5 limit 10: 32 768 survivors per run) or the runs report in
    step (age > 89 limit 1000 with two work-groups: ~3 300 survivors per run).  Keep that true for any predicate added here."""
    scanned = int(head[native.FINISH_LIMIT_TILES])
    rows = np.flatnonzero(keep)
    last = int(t.tile_of(rows[limit - 1]))                                   # tile of the limit-th survivor
    assert scanned % CLAIM == 0 or scanned == t.n_tiles, (tag, scanned)
    assert last + 1 <= scanned <= last + 1 + G * CLAIM, (tag, scanned, last)
    assert scanned < t.n_tiles, (tag, scanned)                               # the scan STOPPED (the whole select writes every line)
    assert (raw[scanned * 16:] == POISON).all(), tag                         # untouched behind the scanned prefix
    assert raw[: scanned * 16].tobytes() == t.virtual_bitmap(keep)[: scanned * 16].tobytes(), tag
    return scanned


@pytest.mark.parametrize("G", [1, 2, 5])
def test_the_scan_stops_and_lines_behind_it_are_never_written(ctx, tab, G):
    ids = tab.data[0]
    with shrunk(ctx, G):
        keep = ids > 5
        q = native.DeviceQuery(ctx, tab.table, [0], [(0, GT, 5.0)], [0], 10, 1024)
        q.run()                                                              # (allocates everything)
        ctx.sync()
        poison_bitmap(q, N_TILES)
        q.run()
        ctx.sync()
        head, raw = read_words(q, N_TILES)
        scanned = check_stopped(tab, q, head, raw, keep, 10, G, ("id > 5", G))
        assert scanned == G * CLAIM, (G, scanned)                            # every work-group's first run alone meets the limit: one claim each
        idx, _ = q.fetch_rows()
        assert (idx == np.flatnonzero(keep)[:10]).all()                      # (segment 0: virtual row = row)
        q.close()
        # the survivors in the last segment: every tile is scanned
        thr = float((N_SEGS - 1) * SEG_ROWS + 50)
        keep = ids > thr
        q = native.DeviceQuery(ctx, tab.table, [0], [(0, GT, thr)], [0], 10, 1024)
        q.run()
        ctx.sync()
        poison_bitmap(q, N_TILES)
        q.run()
        ctx.sync()
        head, raw = read_words(q, N_TILES)
        assert int(head[native.FINISH_LIMIT_TILES]) == N_TILES, G
        assert raw.tobytes() == tab.virtual_bitmap(keep).tobytes(), G
        idx, _ = q.fetch_rows()
        seg_of, row_of = q.locate_rows(idx)
        assert (seg_of == N_SEGS - 1).all() and (row_of == np.arange(51, 61)).all(), G
        q.close()


def test_a_limit_met_in_the_middle_stops_behind_it(ctx, tab):
    """age > 89 limit 1000: the limit-th survivor sits about a quarter into the table; the scan goes on until the runs that are done
    hold 1000 rows, and no further than one claim per work-group behind the tile that completes them."""
    G = 2
    keep = tab.data[1] > 89
    with shrunk(ctx, G):
        q = native.DeviceQuery(ctx, tab.table, [1, 0], [(0, GT, 89.0)], [1, 0], 1000, 1024)
        q.run()
        ctx.sync()
        poison_bitmap(q, N_TILES)
        q.run()
        ctx.sync()
        head, raw = read_words(q, N_TILES)
        check_stopped(tab, q, head, raw, keep, 1000, G, "age > 89 limit 1000")
        rows_and_values(tab, q, [1, 0], [1, 0], np.flatnonzero(keep)[:1000], "age > 89 limit 1000")
        q.close()


def test_a_recorded_graph_replays_the_stopped_scan(ctx, tab):
    """The ticket counter and the rows word start from zero in every run without a memset: three replays, each behind a poisoned
    bitmap, stop where the recorded run stopped and give the same rows."""
    G = 2
    keep = tab.data[0] > 5
    want = np.flatnonzero(keep)[:10]
    with shrunk(ctx, G):
        q = native.DeviceQuery(ctx, tab.table, [0, 1], [(0, GT, 5.0)], [1, 0], 10, 1024)
        q.run()
        ctx.sync()
        with ctx.capture() as cap:
            q.run()
        for i in range(3):
            poison_bitmap(q, N_TILES)
            cap.graph.launch()
            ctx.sync()
            head, raw = read_words(q, N_TILES)
            check_stopped(tab, q, head, raw, keep, 10, G, ("replay", i))
            rows_and_values(tab, q, [1, 0], [0, 1], want, ("replay", i))
        assert q.count() == int(keep.sum())
        cap.graph.close()
        q.run()                                                              # a direct run behind the replays
        rows_and_values(tab, q, [1, 0], [0, 1], want, "direct run behind the replays")
        q.close()


def test_vetoes_keep_the_whole_select(ctx, tab):
    G = 2
    ids = tab.data[0]
    keep = ids > 5
    want = np.flatnonzero(keep)[:10]
    # tuning variant 14 ("no limit chunks"): the whole table in one launch, the scanned-tile word is nobody's
    with shrunk(ctx, G, native.TV_NO_LIMIT_CHUNKS):
        q = native.DeviceQuery(ctx, tab.table, [0], [(0, GT, 5.0)], [0], 10, 1024)
        q.run()
        ctx.sync()
        poison_bitmap(q, N_TILES)
        q.run()
        ctx.sync()
        head, raw = read_words(q, N_TILES)
        assert int(head[native.FINISH_LIMIT_TILES]) == 0
        assert raw.tobytes() == tab.virtual_bitmap(keep).tobytes()
        rows_and_values(tab, q, [0], [0], want, "variant 14")
        q.close()
    # a select tree (an OR in it) over the same table with the same limit: k_filter_expr, whole, the same rows as before
    with shrunk(ctx, G):
        q = native.DeviceQuery(ctx, tab.table, [0], [(0, GT, 5.0), (0, GT, 100_000.0)], [0], 10, 1024, expr=[0, 1, native.EXPR_OR])
        q.run()
        ctx.sync()
        poison_bitmap(q, N_TILES)
        q.run()
        ctx.sync()
        head, raw = read_words(q, N_TILES)
        assert int(head[native.FINISH_LIMIT_TILES]) == 0
        assert raw.tobytes() == tab.virtual_bitmap(keep).tobytes()
        rows_and_values(tab, q, [0], [0], want, "select tree")
        assert q.count() == int(keep.sum())
        q.close()


def test_a_table_smaller_than_one_claim_per_work_group_scans_whole(ctx):
    t = Table(ctx, 3, seed=9)                                                # 27 tiles: fewer than the 64 that two work-groups claim at once
    try:
        keep = t.data[1] > 89
        rows = np.flatnonzero(keep)
        for G in (2, 0):                                                     # (0: the library's own grid -- 7 work-groups, 224 tiles at once)
            for limit in (1, 10, rows.size + 1):
                with shrunk(ctx, G):
                    q = native.DeviceQuery(ctx, t.table, [1, 0], [(0, GT, 89.0)], [1, 0], limit, 1024)
                    q.run()
                    ctx.sync()
                    poison_bitmap(q, t.n_tiles)
                    q.run()
                    ctx.sync()
                    head, raw = read_words(q, t.n_tiles)
                    assert int(head[native.FINISH_LIMIT_TILES]) == 0, (G, limit)
                    assert raw.tobytes() == t.virtual_bitmap(keep).tobytes(), (G, limit)
                    want = rows[:limit]
                    idx, vals = q.fetch_rows()
                    seg_of, row_of = q.locate_rows(idx)
                    assert idx.size == want.size and (seg_of == want // SEG_ROWS).all() and (row_of == want % SEG_ROWS).all(), (G, limit)
                    assert vals[1].tobytes() == np.ascontiguousarray(t.data[1][want]).tobytes(), (G, limit)
                    assert q.count() == rows.size
                    q.close()
    finally:
        t.close()
