"""Seeded differential fuzzing of the merges of group tables -- imm3_comm_merge_groups, imm3_comm_merge_groups_wide and their _all
flavours (csrc/imm3_merge_groups.cpp, csrc/imm3_merge_wide.cpp, the k_merge_* kernels of csrc/imm3_agg.hip) -- against plain numpy
(merge_fuzz_util.py: the generator and the reference side): one aggregation query per segment of a random table, dealt out under
random global indices, hand-over orders and owners, sometimes with an extra query that selects nothing or a segment brought twice.

Bit-exact, no tolerance anywhere, and the library is asked nothing about the expected answer: the group count, the key bytes (the u64
keys of the narrow merge), first as (global segment, row), counts, values and the bytes of every string MAX.
test_merge_fuzz_host.py walks the same seeds on the CPU and asserts that none of this is hollow.

The directed tests pin the one key with a code path of its own: 8 bytes of 0xFF, the free-slot marker of every u64 hash table."""
import os

import numpy as np
import pytest

import merge_fuzz_util as F
import order_fuzz_util as O
import table_fuzz_util as U
from immutable3_amd import native
from merge_wide_util import assert_merged
from test_gpu_fuzz_order import fetch_all
from test_gpu_group_order import assert_same

pytestmark = pytest.mark.gpu
MORE = int(os.environ.get("IMM3_FUZZ_MORE", "0"))      # extra seeds for a long hunt (default: the bounded set)
KIND = {"count": native.AGG_COUNT, "min": native.AGG_MIN, "max": native.AGG_MAX, "sum": native.AGG_SUM}
FORMS = [native.AGG_FORM_LANES, native.AGG_FORM_LANES_WIDE, native.AGG_FORM_DIRECT, native.AGG_FORM_TILE, native.AGG_FORM_GENERAL]


@pytest.fixture(scope="module")
def two():
    """(contexts, communicators): two contexts on device 0, each with a communicator of a world of one (the one-rank tests use the
    first pair)"""
    ctxs = [native.Context(0) for _ in range(2)]
    comms = [native.Comm(c, 1, 0, native.comm_unique_id()) for c in ctxs]
    yield ctxs, comms
    for c in comms:
        c.close()
    for c in ctxs:
        c.set_tuning(0, 0)
        c.close()


def agg_query(ctx, target, aq, sels=None):
    q = native.DeviceQuery(ctx, target, aq.used, aq.sels if sels is None else sels, (), 0, 1024, group_cols=aq.group,
                           aggs=[(KIND[k], c) for k, c in aq.aggs], wide_keys=aq.wide_keys)
    q.run()
    return q


class Segments:
    """a table's segments on a context, made when first asked for"""

    def __init__(self, ctx, t):
        self.ctx, self.t, self.made = ctx, t, {}

    def __getitem__(self, si):
        if si not in self.made:
            self.made[si] = native.DeviceSegment(self.ctx, [c.native() for c in self.t.segs[si]])
        return self.made[si]

    def close(self):
        for s in self.made.values():
            s.close()


def narrow_merge(comm, qs, idx, max_groups=None):
    """imm3_comm_merge_groups; max_groups: write only that many -> (..., the total)"""
    if max_groups is None:
        return comm.merge_groups(qs, idx)
    arr = (native.C.c_void_p * len(qs))(*[q._h for q in qs])
    seg = np.ascontiguousarray(idx, dtype=np.int32)
    m, na = max(max_groups, 1), len(qs[0].aggs)
    keys, first, counts, vals = np.zeros(m, np.uint64), np.zeros(m, np.uint64), np.zeros(m, np.uint64), np.zeros((m, na), np.int64)
    n = native.C.c_uint32(0)
    native._check(native.load().imm3_comm_merge_groups(comm._h, arr, seg.ctypes.data, len(qs), keys.ctypes.data, first.ctypes.data, counts.ctypes.data,
                                                       vals.ctypes.data, max_groups, native.C.byref(n)))
    return keys[:max_groups], first[:max_groups], counts[:max_groups], vals[:max_groups], n.value


def check_refused(fn, what):
    with pytest.raises(native.Imm3Error) as e:
        fn()
    assert e.value.code == native.ERR_ARG and "wider than 8 bytes" in e.value.msg, (what, e.value.msg)


# ---- 1. one rank ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(F.SEEDS + MORE))
def test_fuzz_merge_one_rank(two, oracle, seed):
    """Every case's queries on one context, merged by a world-of-one communicator: the wide merge always, the narrow one where it takes
    the query (ERR_ARG where it must not); a second hand-over order gives the same bytes; max_groups below the total writes the first
    rows and reports the total; and the _all flavour with a second communicator that brings no query gives the same table."""
    (ctx, _), (comm, idle) = two
    for ti, (t, cases) in enumerate(F.merge_cases(seed)):
        segs = Segments(ctx, t)
        for ci, case in enumerate(cases):
            ref = F.reference(oracle, t, case)
            want, g = ref.arrays, len(ref.merged)
            what = (seed, ti, ci, t.describe(), case.describe(), g)
            queries = [agg_query(ctx, segs[e.seg], case.aq, case.sels(e)) for e in case.entries]
            orders = [case.passed, case.passed[::-1]]
            wide = [comm.merge_groups_wide([queries[i] for i in o], [case.entries[i].index for i in o]) for o in orders]
            assert wide[0][0].shape[0] == g, (what, wide[0][0].shape[0])
            for k, got in enumerate(wide):
                assert_merged(got, want, (what, "wide, order", k))
            qs, idx = [queries[i] for i in orders[0]], [case.entries[i].index for i in orders[0]]
            if F.narrow_accepts(t, case.aq):
                for k, o in enumerate(orders):
                    got = narrow_merge(comm, [queries[i] for i in o], [case.entries[i].index for i in o])
                    F.assert_narrow(got, want, (what, "narrow, order", k))
                F.assert_narrow(native.Comm.merge_groups_all([comm, idle], [qs, []], [idx, []]), want, (what, "narrow, _all, the second brings nothing"))
            else:
                check_refused(lambda: narrow_merge(comm, qs, idx), what)
                check_refused(lambda: native.Comm.merge_groups_all([idle, comm], [[], qs], [[], idx]), (what, "_all"))
            assert_merged(native.Comm.merge_groups_wide_all([idle, comm], [[], qs], [[], idx]), want, (what, "wide, _all, the first brings nothing"))
            if g >= 1:
                m = g // 2
                short = comm.merge_groups_wide(qs, idx, max_groups=m)
                assert short[5] == g and short[0].shape[0] == m, (what, short[5], m)
                assert_merged(short, ref.prefix(m), (what, "wide, max_groups", m))
                if F.narrow_accepts(t, case.aq):
                    short = narrow_merge(comm, qs, idx, max_groups=m)
                    assert short[4] == g, (what, short[4])
                    F.assert_narrow(short, ref.prefix(m), (what, "narrow, max_groups", m))
            for q in queries:
                q.close()
        segs.close()


# ---- 2. the _all flavours over two communicators ----------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(F.SEEDS + MORE))
def test_fuzz_merge_all_two_communicators(two, oracle, seed):
    """The same cases dealt by their drawn owners to two contexts with a communicator each: the host combine of the two local merges."""
    ctxs, comms = two
    for ti, (t, cases) in enumerate(F.merge_cases(seed)):
        segs = [Segments(c, t) for c in ctxs]
        for ci, case in enumerate(cases):
            ref = F.reference(oracle, t, case)
            want = ref.arrays
            what = (seed, ti, ci, t.describe(), case.describe(), len(ref.merged), [len(x) for x in ref.local])
            queries = [agg_query(ctxs[e.owner], segs[e.owner][e.seg], case.aq, case.sels(e)) for e in case.entries]
            qs = [[queries[i] for i in case.of_owner(r)] for r in range(2)]
            idx = [[case.entries[i].index for i in case.of_owner(r)] for r in range(2)]
            assert qs[0] and qs[1]
            assert_merged(native.Comm.merge_groups_wide_all(comms, qs, idx), want, (what, "wide"))
            if F.narrow_accepts(t, case.aq):
                F.assert_narrow(native.Comm.merge_groups_all(comms, qs, idx), want, (what, "narrow"))
            else:
                check_refused(lambda: native.Comm.merge_groups_all(comms, qs, idx), what)
            for q in queries:
                q.close()
        for s in segs:
            s.close()


# ---- 3. the all-ones key ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ones(two):
    (ctx, _), _ = two
    t = F.OnesTable(np.random.default_rng(7))
    segs = Segments(ctx, t)
    table = native.DeviceTable(ctx, [segs[si] for si in range(len(t.seg_rows))])
    yield t, segs, table
    table.close()
    segs.close()


def check_segment_query(q, t, aq, groups, what):
    """a query over one segment against segment_groups' list: every getter"""
    wk, wf, wc, wv, ws = F.as_arrays(t, aq, F.combine(aq, [(0, groups)]))
    keys, first, counts, vals = q.fetch_groups()
    assert keys.size == len(groups), (what, keys.size, len(groups))
    assert keys.tolist() == F.u64_keys(wk) and first.tolist() == wf.tolist(), what
    assert counts.tolist() == wc.tolist() and vals.tolist() == wv.tolist(), what
    kb = q.fetch_group_keys()
    assert kb.shape == wk.shape and kb.tobytes() == wk.tobytes(), what
    for j in ws:
        assert q.fetch_group_strings(j).tobytes() == ws[j].tobytes(), (what, j)


ONES_CASES = F.ones_queries()


@pytest.mark.parametrize("case", range(len(ONES_CASES)), ids=["%s-%s-%d" % (w[0].replace(" ", "_"), "name" if w[1] == [U.NAME] else "id_v", F.ONES_AGGS.index(w[2])) for w, _ in ONES_CASES])
def test_all_ones_key(two, ones, case):
    """`group by id, v` with id = v = -1, and `group by name` with a name of eight 0xFF bytes: the key that equals the free-slot marker
    lives in an extra slot of the LDS table, of the global table and of the merge table, and comes back from the slot index.  Against
    numpy: a query per segment, under every pinned aggregation form (an 8-byte key: all of them land on the general kernel); the query
    over the imm3_table; both merges under two sets of global indices; an order over the table's groups."""
    (ctx, _), (comm, _) = two
    t, segs, table = ones
    what, aq = ONES_CASES[case]
    keep = F.ones_keep(t, aq.sels)
    n = len(t.seg_rows)
    per = [F.segment_groups(t, aq, keep, si) for si in range(n)]
    ones_key = b"\xff" * 8
    holds = [any(g[0] == ones_key for g in groups) for groups in per]
    assert holds == ([True, True, False, True] if what[0] != "the all-ones key removed" else [False] * 4)
    # a query per segment, then under every form
    queries = [agg_query(ctx, segs[si], aq) for si in range(n)]
    for si, q in enumerate(queries):
        check_segment_query(q, t, aq, per[si], (what, "segment", si))
        assert q.agg_form() == native.AGG_FORM_GENERAL, (what, si, q.agg_form())
    for form in FORMS:
        ctx.set_tuning(100 + form, 0)
        try:
            for si in (0, 1):
                q = agg_query(ctx, segs[si], aq)
                assert q.agg_form() == native.AGG_FORM_GENERAL, (what, form, q.agg_form())
                check_segment_query(q, t, aq, per[si], (what, "segment", si, "form", form))
                q.close()
        finally:
            ctx.set_tuning(0, 0)
    # the table query, first-seen and ordered
    groups = U.expected_groups(t, aq, keep)
    g = len(groups[2])
    tq = agg_query(ctx, table, aq)
    assert_same(fetch_all(tq, t, aq), O.groups_result(t, aq, groups, np.arange(g)), (what, "table"))
    seg_of = np.repeat(np.arange(n), t.seg_rows)[groups[1]]
    assert tq.fetch_groups()[1].tolist() == F.virtual_rows(t, seg_of, groups[1] - t.starts[seg_of]).tolist(), (what, "table: virtual rows")
    col_desc = [(O.G_COL, i, True) for i in range(len(aq.group))][::-1]
    for order in (col_desc, [(O.G_COL, 0, False)], [(O.G_AGG, 1, False)], [(O.G_AGG, 2, True)] if aq.aggs[2][0] == "sum" else [(O.G_AGG, 0, True)]):
        for limit in (0, 3):
            perm = O.lex_perm(O.group_key_bytes(t, aq, groups, order), limit)
            tq.set_group_order(order, limit)
            assert_same(fetch_all(tq, t, aq), O.groups_result(t, aq, groups, perm), (what, "table, order", order, limit))
    tq.close()
    # the merges
    for index in ([0, 1, 2, 3], [2, 3, 1, 0]):
        want = F.as_arrays(t, aq, F.combine(aq, list(zip(index, per))))
        assert want[0].shape[0] == g
        for passed in ([0, 1, 2, 3], [3, 1, 0, 2]):
            qs, idx = [queries[i] for i in passed], [index[i] for i in passed]
            F.assert_narrow(narrow_merge(comm, qs, idx), want, (what, "narrow", index, passed))
            assert_merged(comm.merge_groups_wide(qs, idx), want, (what, "wide", index, passed))
    if holds[0]:                          # (under identity the key arrives deep inside segment 0, under the other indices with segment 3's one row)
        assert [dict((m[0], m[1]) for m in F.combine(aq, list(zip(index, per))))[ones_key] for index in ([0, 1, 2, 3], [2, 3, 1, 0])] == [F.ONES_DEEP, 0]
    for q in queries:
        q.close()


# ---- 4. a table query and segment queries in one wide merge -------------------------------------------------------------------------
@pytest.mark.parametrize("case", [0, 3, 6, 9])
def test_table_and_segment_queries_mixed(two, ones, case):
    """imm3_comm_merge_groups_wide over a query on the imm3_table of segments 0 and 1 next to queries on segments 2 and 3: the table
    brings ONE global index, and `first` of a group it brings is that index << 32 | the group's first virtual row of the table
    (tile * 1024 + position: include/imm3.h)."""
    (ctx, _), (comm, _) = two
    t, segs, _ = ones
    what, aq = ONES_CASES[case]
    keep = F.ones_keep(t, aq.sels)
    front = np.zeros(t.n_rows, bool)
    front[: t.starts[2]] = keep[: t.starts[2]]
    keys, first, counts, vals = U.expected_groups(t, aq, front)
    seg_of = (first >= t.starts[1]).astype(np.int64)
    virt = F.virtual_rows(t, seg_of, first - t.starts[seg_of])
    from_table = [(bytes(keys[g]), int(virt[g]), int(counts[g]), list(vals[g])) for g in range(len(counts))]
    table = native.DeviceTable(ctx, [segs[0], segs[1]])
    queries = [agg_query(ctx, table, aq), agg_query(ctx, segs[2], aq), agg_query(ctx, segs[3], aq)]
    for index in ([0, 1, 2], [1, 0, 2], [2, 1, 0]):
        parts = [(index[0], from_table), (index[1], F.segment_groups(t, aq, keep, 2)), (index[2], F.segment_groups(t, aq, keep, 3))]
        want = F.as_arrays(t, aq, F.combine(aq, parts))
        assert_merged(comm.merge_groups_wide(queries, index), want, (what, index))
        assert_merged(comm.merge_groups_wide(queries[::-1], index[::-1]), want, (what, index, "reversed"))
    for q in queries:
        q.close()
    table.close()
