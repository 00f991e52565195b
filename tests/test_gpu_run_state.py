"""GPU suite: random call sequences on one query handle, held to the run-state model of tests/run_state_model.py.

One test per subject -- a query at the smallest shape that still takes the plan it names.  The test builds the segment (or table) and
the numpy expectation once, then walks the subject's seeded sequences with the walker test_run_state_host.py has shown to fail every
mutant: run entries, recordings, launches, reservations, group orders and every getter in orders nobody wrote by hand, IMM3_ERR_STATE
exactly where include/imm3.h says so and every value equal to numpy's.  A failure message is the subject, the seed and the operations
so far: a script.

What the first walk found in the library as it was before this file (subject, seed, step; each fixed since, and each a mutant of
the stand-in in test_run_state_host.py):
  - "aggregation, lanes, fused select", seed 0, step 2: bitmap() behind run(), run_count() answered, where the header promises
    IMM3_ERR_STATE -- run_select did not clear agg_select_skipped, so the getter ran the select chain (csrc/imm3_run.cpp).
  - "select, one int32 range", seed 1, step 2: bitmap() behind run_count(), a recording of run_select() answered from a buffer no
    kernel had written; "survivor records", seed 0, step 19: fetch_rows() behind run() and a recording ending in run_select()
    answered IMM3_ERR_STATE over rows that were there -- a recording left its run record in the live handle
    (imm3_ctx_capture_end now puts back the record each query came with).
  - "table aggregation, four segments", seed 1, step 19: group_count() behind a launch of a run_select() recorded before the
    first run() answered IMM3_ERR_STATE -- the launch took ran_agg from the recording (imm3_graph_launch).
  - "ordered projection, limit", seed 6, step 30: fetch_rows() behind run(), reserve_rows(every row) gave other values than numpy
    -- the reservation moved the row arrays and the getter copied the new, unwritten ones (imm3_query_reserve_rows, settle_rows).
  - "aggregation, 64 keys", seed 0, step 4 (once the first finding was fixed): fetch_groups() behind run(), run_count() gave wrong
    keys -- the form behind the overflowed lanes form read a bitmap the count-only run had not stored (settle_groups)."""
import ctypes as C

import numpy as np
import pytest

import order_util
from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, GT, LT, MATCH, PforColumn, RawColumn, blocks_of
from immutable3_amd import native
from run_state_model import AGG, GROUP_COL, SUBJECTS, sequences, walk

pytestmark = pytest.mark.gpu

N = 40 * 1024 + 333
CODES = [b"CA", b"NY", b"TX", b"WA", b"VA", b"DC", b"CT"]
OR, AND, NOT = native.EXPR_OR, native.EXPR_AND, native.EXPR_NOT
TREE = [0, 1, OR, 2, NOT, AND]              # (age < -100 or age > 100) and not state = 'CA', over leaves {LT, GT, Match}
_hip = None


def hip():
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
    return _hip


def device_words(ptr, n):
    out = np.zeros(n, np.uint64)
    assert hip().hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes), C.c_int(2)) == 0
    return out


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.set_tuning(0, 0)
    c.close()


# ---- what numpy says of a query ---------------------------------------------------------------------------------------------------
def raw_bytes(values, codec):
    """uint8[n, width]: a column's values as the segment stores them"""
    if codec == DENSE_INT:
        return np.ascontiguousarray(values, "<i4").view(np.uint8).reshape(-1, 4)
    if codec == DENSE_TINYINT:
        return np.ascontiguousarray(values, np.int8).view(np.uint8).reshape(-1, 1)
    return np.ascontiguousarray(values, np.uint8)


class Truth:
    """The answers of one query over segments of seg_rows rows each (all rows concatenated): keep = the select; proj = [(values, codec)]
    of the SELECT list; limit; order = (order_by, limit) of an ordered query; group = ([(values, codec)] of the group columns,
    [(kind, values, codec)] of the aggregates).  A table's row ids and bitmap are virtual: every segment starts on a fresh tile."""

    def __init__(self, seg_rows, keep, proj=(), limit=0, order=None, group=None, table=False):
        seg_rows = np.asarray(seg_rows, np.int64)
        self.n_rows = int(seg_rows.sum())
        tiles = (seg_rows + 1023) // 1024
        self.seg_of = np.repeat(np.arange(seg_rows.size), seg_rows)
        self.row_of = np.arange(self.n_rows) - np.repeat(np.cumsum(seg_rows) - seg_rows, seg_rows)
        self.vrow = np.repeat(np.cumsum(tiles) - tiles, seg_rows) * 1024 + self.row_of
        self.n_tiles = int(tiles.sum())
        self.keep, self.surv, self.count = keep, np.flatnonzero(keep), int(keep.sum())
        bits = np.zeros(self.n_tiles * 1024, np.uint8)
        bits[self.vrow[self.surv]] = 1
        self.words = np.packbits(bits, bitorder="little").view(np.uint64)
        self.bitmap = None                                    # (cut to the query's words: set_words)
        self.proj, self.limit, self.order, self.group, self.table = [(raw_bytes(v, c), c) for v, c in proj], limit, order, group, table
        self._rows = self._groups = None

    def set_words(self, n_words):
        assert n_words <= self.words.size and not self.words[n_words:].any()
        self.bitmap = self.words[:n_words].copy()

    def picked(self):
        if self._rows is None:
            sel = self.surv
            if self.order is not None:
                order_by, limit = self.order
                keys = order_util.normalised_keys([v[sel] for v, _ in self.proj], [c for _, c in self.proj], order_by)
                sel = sel[order_util.order_permutation(keys, limit)]
            elif self.limit > 0:
                sel = sel[: self.limit]
            self._rows = sel
        return self._rows

    def rows(self):
        sel = self.picked()
        return self.vrow[sel].astype(np.uint32), [v[sel] for v, _ in self.proj]

    def locate(self):
        sel = self.picked()
        return self.seg_of[sel].astype(np.uint32), self.row_of[sel].astype(np.uint32)

    def reserve(self, kind):
        return {"small": self.count // 3 + 1, "exact": self.count, "whole": self.n_rows}[kind]

    # groups, in first-seen order
    def first_seen(self):
        if self._groups is None:
            gcols, aggs = self.group
            s = self.surv
            keyb = np.concatenate([raw_bytes(v, c)[s] for v, c in gcols], axis=1) if gcols else np.zeros((s.size, 0), np.uint8)
            uniq, first, inv = np.unique(keyb, axis=0, return_index=True, return_inverse=True) if s.size else (keyb, np.zeros(0, np.int64), np.zeros(0, np.int64))
            inv = np.asarray(inv).reshape(-1)
            by_first = np.argsort(first, kind="stable")
            rank = np.empty_like(by_first)
            rank[by_first] = np.arange(by_first.size)
            inv, g = rank[inv], by_first.size                                   # group number = place in first-seen order
            key_bytes = uniq[by_first]
            counts = np.bincount(inv, minlength=g).astype(np.uint64)
            vals, strings, sort_vals = np.zeros((g, len(aggs)), np.int64), None, []
            for j, (kind, v, codec) in enumerate(aggs):
                if kind == native.AGG_COUNT:
                    vals[:, j] = counts
                elif codec == DENSE_STRING:
                    rb = raw_bytes(v, codec)[s]
                    best = [max(r.tobytes() for r in rb[inv == k]) for k in range(g)]
                    strings = np.frombuffer(b"".join(best), np.uint8).reshape(g, rb.shape[1]).copy()
                    vals[:, j] = [int.from_bytes(b[:8], "big") for b in best]
                    sort_vals.append(best)
                    continue
                else:
                    x = np.asarray(v)[s].astype(np.int64)
                    out = np.full(g, {native.AGG_MIN: np.iinfo(np.int64).max, native.AGG_MAX: np.iinfo(np.int64).min, native.AGG_SUM: 0}[kind], np.int64)
                    {native.AGG_MIN: np.minimum, native.AGG_MAX: np.maximum, native.AGG_SUM: np.add}[kind].at(out, inv, x)
                    vals[:, j] = out
                sort_vals.append(vals[:, j].tolist())
            keys = np.zeros(g, np.uint64)
            for b in range(min(8, key_bytes.shape[1])):
                keys |= key_bytes[:, b].astype(np.uint64) << np.uint64(8 * b)
            gvals = []                                                           # per group column: what the order compares
            off = 0
            for v, codec in gcols:
                w = raw_bytes(v, codec).shape[1]
                part = key_bytes[:, off: off + w]
                gvals.append([bytes(r) for r in part] if codec == DENSE_STRING else
                             part.copy().view("<i4" if codec == DENSE_INT else np.int8).reshape(-1).tolist())
                off += w
            self._groups = {"keys": keys, "first": self.vrow[s[first[by_first]]].astype(np.uint32), "counts": counts, "vals": vals,
                            "key_bytes": key_bytes, "strings": strings, "sort": {GROUP_COL: gvals, AGG: sort_vals}}
        return self._groups

    def group_order_args(self, op):
        g = len(self.first_seen()["first"])
        return list(op[1]), {"all": 0, "one": 1, "half": max(1, g // 2), "more": g + 3}[op[2]]

    def groups(self, order):
        """the groups in the order imm3_query_set_group_order was last given (include/imm3.h): lexicographic over the keys, integers
        signed, strings byte-wise, a descending key reversed alone, ties in first-seen order; cut to the limit"""
        f = self.first_seen()
        places = list(range(len(f["first"])))
        if order is not None:
            keys, limit = self.group_order_args(order)

            def part(i, kind, index, desc):
                x = f["sort"][kind][index][i]
                if isinstance(x, bytes):
                    return bytes(255 - b for b in x) if desc else x
                return -x if desc else x
            places.sort(key=lambda i: tuple(part(i, *k) for k in keys))
            places = places[:limit] if limit > 0 else places
        p = np.array(places, np.int64)
        return {k: (v[p] if v is not None else None) for k, v in f.items() if k != "sort"}


# ---- the handle the walker drives -------------------------------------------------------------------------------------------------
class Handle:
    """native.DeviceQuery with the few calls the walker needs on top; `after_run(handle)` is the subject's look at its plan"""

    def __init__(self, ctx, q, after_run=None):
        self.ctx, self.q, self.after_run = ctx, q, after_run
        self.full_runs = 0
        self.group_getters = 0
        for name in ("run_select", "run_count", "sync", "count", "bitmap", "row_count", "fetch_rows", "locate_rows", "reserve_rows",
                     "set_order", "set_group_order"):
            setattr(self, name, getattr(q, name))

    def run(self):
        self.q.run()
        self.full_runs += 1
        if self.after_run:
            self.after_run(self)

    def ran(self, last, ran_full):
        pass

    def record(self, entries):
        with self.ctx.capture() as cap:                       # (a refused run ends the capture and drops what was recorded)
            for e in entries:
                getattr(self.q, e)()
        return cap.graph

    def device_count(self):
        self.q.join_count()
        self.ctx.sync()
        return int(device_words(self.q.device_ptr(1), 1)[0])

    def _answered(self, got):
        self.group_getters += 1                               # (group getters that answered: the first one settles the form)
        return got

    def group_count(self):
        n = C.c_uint32(0)
        native._check(native.load().imm3_query_group_count(self.q._h, C.byref(n)))
        return self._answered(n.value)

    def fetch_groups(self):
        return self._answered(self.q.fetch_groups())

    def fetch_group_keys(self):
        return self._answered(self.q.fetch_group_keys())

    def fetch_group_strings(self, j):
        return self._answered(self.q.fetch_group_strings(j))


def census(ctx, q, call):
    """launches per kernel id 0 .. 4 (select, offsets scan, gather, count reduce, aggregation) of one call on a query"""
    ctx.timing_enable(64)
    try:
        call(q)
        ctx.sync()
        return [int(ctx.timing_collect(k).size) for k in range(5)]
    finally:
        ctx.timing_enable(0)


# ---- the subjects -----------------------------------------------------------------------------------------------------------------
class Case:
    """segments on the device, the query's arguments, numpy's answers, and the subject's plan checks"""

    def __init__(self, ctx, seg_cols, kw, truth, created=None, after_run=None, first=None):
        self.ctx, self.kw, self.truth, self.created, self.after_run, self.first = ctx, kw, truth, created, after_run, first
        self.segs = [native.DeviceSegment(ctx, [c.native() for c in cols]) for cols in seg_cols]
        self.table = native.DeviceTable(ctx, self.segs) if truth.table else None

    def query(self, s):
        kw = dict(self.kw)
        order = kw.pop("order", None)
        q = native.DeviceQuery(self.ctx, self.table or self.segs[0], kw.pop("used"), kw.pop("sels"), **kw)
        if order:
            q.set_order(*order)
        if s.reserve0:
            q.reserve_rows(self.truth.reserve(s.reserve0))
        if self.created:
            self.created(q)
        return q

    def close(self):
        if self.table:
            self.table.close()
        for d in self.segs:
            d.close()


def columns(seed, n, pool16=0):
    rng = np.random.default_rng(seed)
    d = {"id": rng.integers(-1000, 1000, size=n).astype(np.int32), "age": rng.integers(-128, 128, size=n).astype(np.int8),
         "st": np.array([list(c) for c in CODES], np.uint8)[rng.integers(0, len(CODES), size=n)]}
    return rng, d


def seg_of(d, names, n):
    br = blocks_of(n, 1024)
    kinds = {"id": (DENSE_INT, 4), "age": (DENSE_TINYINT, 1)}
    return [RawColumn(*kinds.get(k, (DENSE_STRING, np.asarray(d[k]).shape[-1])), d[k], br) for k in names]


def is_in(col, values):
    keep = np.zeros(col.shape[0], bool)
    for v in values:
        keep |= (col == np.frombuffer(v, np.uint8)).all(axis=1)
    return keep


def tree_keep(d):
    return ((d["age"] < -100) | (d["age"] > 100)) & ~is_in(d["st"], [b"CA"])


TREE_LEAVES = [(0, LT, -100.0), (0, GT, 100.0), (1, MATCH, [b"CA"])]
FOUR = [3 * 1024 + 5, 1, 2 * 1024, 1024 + 700]          # a table of four segments of unequal length, one of them a single row


def four_segments(seed, names):
    parts = [columns(seed + k, n)[1] for k, n in enumerate(FOUR)]
    return [seg_of(p, names, n) for p, n in zip(parts, FOUR)], {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def plan_is(**want):
    def check(q):
        p = q.plan()
        assert {k: p[k] for k in want} == want, p
    return check


def build(ctx, s, oracle):
    name = s.name
    if name == "select, one int32 range":
        _, d = columns(1, N)
        keep = (d["id"] > -300) & (d["id"] < 400)
        return Case(ctx, [seg_of(d, ["id"], N)], dict(used=[0], sels=[(0, GT, -300.0), (0, LT, 400.0)]), Truth([N], keep),
                    first=lambda q: check_census(census(ctx, q, lambda x: x.run_select()), {0: 1, 3: 0}))
    if name == "select, PFOR_INT and two 2-byte strings":
        rng, d = columns(2, N)
        pid = (np.arange(N, dtype=np.int32) * 3) % 5000
        st2 = np.array([list(c) for c in CODES], np.uint8)[rng.integers(0, len(CODES), size=N)]
        br = blocks_of(N, 1024)
        cols = [PforColumn(pid, br), RawColumn(DENSE_STRING, 2, d["st"], br), RawColumn(DENSE_STRING, 2, st2, br)]
        keep = (pid > 1000) & (pid < 4000) & is_in(d["st"], CODES[:4]) & is_in(st2, CODES[2:])
        sels = [(0, GT, 1000.0), (0, LT, 4000.0), (1, MATCH, CODES[:4]), (2, MATCH, CODES[2:])]
        # (several passes: the fused PFOR_INT launch and a tile launch per string column; the count by k_total)
        return Case(ctx, [cols], dict(used=[0, 1, 2], sels=sels), Truth([N], keep),
                    first=lambda q: several_passes(census(ctx, q, lambda x: x.run_select())))
    if name.startswith("one launch"):
        n = 300 * 1024 + 77
        _, d = columns(3, n)
        keep = (d["age"] > 18) & (d["age"] < 60) & (d["id"] > 100)
        kw = dict(used=[1, 0], sels=[(0, GT, 18.0), (0, LT, 60.0), (1, GT, 100.0)], proj=[1, 0])
        return Case(ctx, [seg_of(d, ["id", "age"], n)], kw, Truth([n], keep, [(d["id"], DENSE_INT), (d["age"], DENSE_TINYINT)]),
                    created=plan_is(single_pass=True), after_run=lambda h: plan_is(single_pass=True, ran_single_pass=True)(h.q))
    if name == "survivor records":
        _, d = columns(4, N)
        keep = is_in(d["st"], [b"CA", b"TX"])
        kw = dict(used=[0, 1], sels=[(0, MATCH, [b"CA", b"TX"])], proj=[1, 0])
        return Case(ctx, [seg_of(d, ["st", "id"], N)], kw, Truth([N], keep, [(d["id"], DENSE_INT), (d["st"], DENSE_STRING)]),
                    created=plan_is(single_pass=False, records=True), after_run=lambda h: plan_is(single_pass=False, records=True)(h.q))
    if name == "bitmap path":
        _, d = columns(5, N)
        keep = d["age"] > 100
        kw = dict(used=[0, 1], sels=[(0, GT, 100.0)], proj=[1, 0])
        return Case(ctx, [seg_of(d, ["age", "id"], N)], kw, Truth([N], keep, [(d["id"], DENSE_INT), (d["age"], DENSE_TINYINT)]),
                    created=plan_is(single_pass=False, records=False))
    if name.startswith("segment limit"):
        n = 1024 * 1024 + 1                                   # 1025 tiles: the first shape with two chunks
        assert native.plan_limit_chunks(1025) == [1024, 1025] and len(native.plan_limit_chunks(1024)) == 1
        rng = np.random.default_rng(6)
        d = {"age": rng.integers(0, 100, size=n).astype(np.int8), "id": np.arange(n, dtype=np.int32)}
        d["age"][-1] = 99                                     # (the second chunk holds a survivor: the prefix's count is not the segment's)
        keep = d["age"] > 98
        limit = 10 if s.limit == "small" else int(keep.sum()) + 7
        kw = dict(used=[0, 1], sels=[(0, GT, 98.0)], proj=[1, 0], limit=limit)
        two = s.tuning[0] == 15

        def first(q):                                         # a small limit: one launch gathers (k_limit_gather), or scan + gather
            got = census(ctx, q, lambda x: x.run())
            if s.limit == "small":
                check_census(got, {0: 2, 1: 1 if two else 0, 2: 1})
                assert int(device_words(q.device_ptr(1), 16)[native.FINISH_LIMIT_TILES]) == 1024      # stopped in the first chunk
        return Case(ctx, [seg_of(d, ["age", "id"], n)], kw, Truth([n], keep, [(d["id"], DENSE_INT), (d["age"], DENSE_TINYINT)], limit=limit),
                    created=plan_is(single_pass=False, records=False), first=first)
    if name == "table limit":
        rows, n_segs = 8 * 1024 + 1, 48                       # 432 tiles > 32 x 4 work-groups
        rng = np.random.default_rng(7)
        parts = [{"id": np.arange(k * rows, (k + 1) * rows, dtype=np.int32), "age": rng.integers(0, 100, size=rows).astype(np.int8)} for k in range(n_segs)]
        d = {k: np.concatenate([p[k] for p in parts]) for k in ("id", "age")}
        keep = d["age"] > 89
        assert native.plan_table_limit(limit=10, n_tiles=n_segs * 9, grid=4) == 1
        kw = dict(used=[1, 0], sels=[(0, GT, 89.0)], proj=[1, 0], limit=10)

        def first(q):
            q.run()
            ctx.sync()
            assert 0 < int(device_words(q.device_ptr(1), 16)[native.FINISH_LIMIT_TILES]) < n_segs * 9                  # the scan stopped
        return Case(ctx, [seg_of(p, ["id", "age"], rows) for p in parts], kw,
                    Truth([rows] * n_segs, keep, [(d["id"], DENSE_INT), (d["age"], DENSE_TINYINT)], limit=10, table=True), first=first)
    if name.startswith("aggregation, lanes"):
        _, d = columns(8, N)
        keep = (d["age"] > 18) & (d["age"] < 30)
        kw = dict(used=[1, 2, 0], sels=[(0, GT, 18.0), (0, LT, 30.0)], group_cols=[1], aggs=[(native.AGG_COUNT, 2), (native.AGG_MAX, 0)])
        group = ([(d["st"], DENSE_STRING)], [(native.AGG_COUNT, d["id"], DENSE_INT), (native.AGG_MAX, d["age"], DENSE_TINYINT)])
        fused = "fused" in name
        return Case(ctx, [seg_of(d, ["id", "age", "st"], N)], kw, Truth([N], keep, group=group),
                    first=lambda q: check_census(census(ctx, q, lambda x: x.run()), {0: 0 if fused else 1, 4: 1}),
                    after_run=lambda h: agg_form_is(h, native.AGG_FORM_LANES))
    if name == "aggregation, 64 keys":
        rng, d = columns(9, N)
        codes = np.array([[65 + k // 8, 97 + k % 8] for k in range(64)], np.uint8)
        d["key"] = codes[rng.integers(0, 64, size=N)]
        keep = d["id"] > 0
        kw = dict(used=[0, 1], sels=[(0, GT, 0.0)], group_cols=[1], aggs=[(native.AGG_COUNT, 0), (native.AGG_MAX, 0)])
        group = ([(d["key"], DENSE_STRING)], [(native.AGG_COUNT, d["id"], DENSE_INT), (native.AGG_MAX, d["id"], DENSE_INT)])

        def form(h):                                          # the first getter finds the 63-key form overflowed: later runs start behind it
            want = (native.AGG_FORM_LANES,) if not h.group_getters else (native.AGG_FORM_LANES_WIDE, native.AGG_FORM_DIRECT)
            assert h.q.agg_form() in want, (h.q.agg_form(), h.group_getters)
        return Case(ctx, [seg_of(d, ["id", "key"], N)], kw, Truth([N], keep, group=group), after_run=form)
    if name == "aggregation, 16-byte key and string MAX":
        rng, d = columns(10, N)
        pool = rng.integers(97, 123, size=(20, 16)).astype(np.uint8)
        pool[:, :8] = pool[0, :8]                             # (the keys differ behind the eight bytes fetch_groups gives)
        d["k16"] = pool[rng.integers(0, 20, size=N)]
        d["s16"] = rng.integers(97, 123, size=(50, 16)).astype(np.uint8)[rng.integers(0, 50, size=N)]
        keep = d["id"] > -500
        kw = dict(used=[0, 1, 2], sels=[(2, GT, -500.0)], group_cols=[0], wide_keys=True,
                  aggs=[(native.AGG_COUNT, 2), (native.AGG_MAX, 1), (native.AGG_MIN, 2)])
        group = ([(d["k16"], DENSE_STRING)],
                 [(native.AGG_COUNT, d["id"], DENSE_INT), (native.AGG_MAX, d["s16"], DENSE_STRING), (native.AGG_MIN, d["id"], DENSE_INT)])
        return Case(ctx, [seg_of(d, ["k16", "s16", "id"], N)], kw, Truth([N], keep, group=group),
                    after_run=lambda h: agg_form_is(h, native.AGG_FORM_GENERAL))
    if name == "tile tree with OR and NOT":
        _, d = columns(11, N)
        return Case(ctx, [seg_of(d, ["age", "st"], N)], dict(used=[0, 1], sels=TREE_LEAVES, expr=TREE), Truth([N], tree_keep(d)),
                    first=lambda q: (q.run_select(), expr_form_is(q, native.EXPR_FORM_TILE)))
    if name == "generic tree":
        _, d = columns(12, N)
        kw = dict(used=[0, 1, 2], sels=TREE_LEAVES, expr=TREE, proj=[2, 0])
        return Case(ctx, [seg_of(d, ["age", "st", "id"], N)], kw, Truth([N], tree_keep(d), [(d["id"], DENSE_INT), (d["age"], DENSE_TINYINT)]),
                    created=plan_is(single_pass=False, records=False), after_run=lambda h: expr_form_is(h.q, native.EXPR_FORM_GENERIC))
    if name == "table tile tree, limit":
        segs, d = four_segments(13, ["age", "st", "id"])
        kw = dict(used=[0, 1, 2], sels=TREE_LEAVES, expr=TREE, proj=[2, 0], limit=10)
        return Case(ctx, segs, kw, Truth(FOUR, tree_keep(d), [(d["id"], DENSE_INT), (d["age"], DENSE_TINYINT)], limit=10, table=True),
                    after_run=lambda h: expr_form_is(h.q, native.EXPR_FORM_TILE))
    if name.startswith("ordered projection"):
        _, d = columns(14, N)
        keep = d["age"] > 100
        order = ([(1, True), (0, False)], 25 if s.order_limit else 0)          # age descending, then id; 25 rows are fewer than survive
        assert 25 < int(keep.sum())
        kw = dict(used=[0, 1], sels=[(0, GT, 100.0)], proj=[1, 0], order=order)
        return Case(ctx, [seg_of(d, ["age", "id"], N)], kw,
                    Truth([N], keep, [(d["id"], DENSE_INT), (d["age"], DENSE_TINYINT)], order=order))
    if name == "table projection, four segments":
        segs, d = four_segments(15, ["age", "id"])
        kw = dict(used=[0, 1], sels=[(0, GT, 50.0)], proj=[1, 0])
        return Case(ctx, segs, kw, Truth(FOUR, d["age"] > 50, [(d["id"], DENSE_INT), (d["age"], DENSE_TINYINT)], table=True))
    if name == "table aggregation, four segments":
        segs, d = four_segments(16, ["id", "age", "st"])
        kw = dict(used=[1, 2, 0], sels=[(0, GT, 0.0)], group_cols=[1], aggs=[(native.AGG_COUNT, 2), (native.AGG_MAX, 0)])
        group = ([(d["st"], DENSE_STRING)], [(native.AGG_COUNT, d["id"], DENSE_INT), (native.AGG_MAX, d["age"], DENSE_TINYINT)])
        return Case(ctx, segs, kw, Truth(FOUR, d["age"] > 0, group=group, table=True))
    raise AssertionError("no builder for " + name)


def check_census(got, want):
    assert {k: got[k] for k in want} == want, (got, want)


def several_passes(got):
    assert got[0] >= 2 and got[3] == 1, got


def agg_form_is(h, form):
    assert h.q.agg_form() == form, (h.q.agg_form(), form)


def expr_form_is(q, form):
    assert q.expr_form() == form, (q.expr_form(), form)


@pytest.mark.parametrize("s", SUBJECTS, ids=repr)
def test_walk(ctx, oracle, s):
    ctx.set_tuning(*s.tuning)
    case = None
    try:
        case = build(ctx, s, oracle)
        if case.first:                                        # the subject takes the launches it names (a query of its own)
            q = case.query(s)
            case.truth.set_words(q.total_words)
            case.first(q)
            q.close()
        for seed, ops in sequences(s):
            q = case.query(s)
            case.truth.set_words(q.total_words)
            try:
                walk(s, seed, ops, Handle(ctx, q, case.after_run), case.truth)
            finally:
                q.close()
    finally:
        ctx.set_tuning(0, 0)
        if case:
            case.close()
