"""GPU suite: the group merge by byte key, imm3_comm_merge_groups_wide[_all] -- group keys of 0 .. 256 bytes and string maxima of any
width merged across queries on the device (one immutable record per (query, group), a hash table whose slots hold the
index of the claiming record, a compare-and-swap walk for the string maxima).  Every comparison is exact.  The expected result is
combined on the host from the queries' own getters (merge_wide_util.host_combine); where the segments form a table, one
imm3_table query over the same segments must agree too."""
import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, GT, RawColumn, blocks_of
from immutable3_amd import native
from merge_wide_util import (AGGS, C, GROUP, MN, MX, PAIR_8A, PAIR_8B, PAIR_FROM2, PAIR_LAST1, PAIR_LAST2, PAIR_ONES, PAIR_ONLY1, PAIR_ZERO, S,
                             SIZES, assert_merged, breaker_columns, host_combine, pair_key)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def comm(ctx):
    c = native.Comm(ctx, 1, 0, native.comm_unique_id())
    yield c
    c.close()


def agg_query(ctx, seg, n_cols, sels, group, aggs):
    q = native.DeviceQuery(ctx, seg, list(range(n_cols)), sels, (), 0, 1024, group_cols=group, aggs=aggs, wide_keys=True)
    q.run()
    return q


def table_result(ctx, segs, n_cols, group, aggs):
    """one table query over the segments: (key bytes, counts, vals, {j: strings}) in first-seen order"""
    table = native.DeviceTable(ctx, segs)
    q = agg_query(ctx, table, n_cols, [], group, aggs)
    _, _, counts, vals = q.fetch_groups()
    out = q.fetch_group_keys(), counts, vals, {j: q.fetch_group_strings(j) for j, (k, c) in enumerate(aggs)
                                                if k == MX and table.codecs[c] == DENSE_STRING}
    q.close()
    table.close()
    return out


def assert_table_agrees(got, tab, what=None):
    keys, _, counts, vals, strs = got
    tk, tc, tv, ts = tab
    assert np.array_equal(keys, tk) and counts.tolist() == tc.tolist() and vals.tolist() == tv.tolist(), what
    assert sorted(strs) == sorted(ts) and all(np.array_equal(strs[j], ts[j]) for j in ts), what


@pytest.fixture(scope="module")
def breaker(ctx):
    """the four segments of the wide-key case, a query over each and a fifth whose select keeps no row; the host combine, once"""
    rng = np.random.default_rng(20)
    cols = [breaker_columns(rng, s) for s in range(len(SIZES))]
    segs = [native.DeviceSegment(ctx, [c.native() for c in cs]) for cs in cols]
    queries = [agg_query(ctx, seg, 4, [], GROUP, AGGS) for seg in segs]
    queries.append(agg_query(ctx, segs[1], 4, [(2, GT, 2.0e6)], GROUP, AGGS))        # val < 10^6: nothing selected, 0 groups
    seg_idx = [0, 1, 2, 3, 1]
    want = host_combine(queries, seg_idx)
    yield segs, queries, seg_idx, want
    for q in queries:
        q.close()
    for s in segs:
        s.close()


# ---- 1. wide key, one rank, several queries ---------------------------------------------------------------------------------------
def test_wide_key_one_rank_several_queries(ctx, comm, breaker):
    segs, queries, seg_idx, want = breaker
    assert queries[4].fetch_groups()[0].size == 0
    keys = [bytes(k) for k in want[0]]
    assert len(set(keys)) == len(keys) == 10
    for pair in (PAIR_8A, PAIR_8B, PAIR_LAST1, PAIR_LAST2, PAIR_ZERO, PAIR_ONES, PAIR_ONLY1, PAIR_FROM2):
        assert pair_key(pair) in keys, pair
    assert int(want[1][keys.index(pair_key(PAIR_ONLY1))]) >> 32 == 1 and int(want[1][keys.index(pair_key(PAIR_FROM2))]) >> 32 == 2
    assert int(want[2].sum()) == sum(SIZES)
    got = comm.merge_groups_wide(queries, seg_idx)
    assert_merged(got, want)
    assert_table_agrees(got, table_result(ctx, segs, 4, GROUP, AGGS))
    # the order the queries are handed over in does not matter
    back = comm.merge_groups_wide(queries[::-1], seg_idx[::-1])
    assert_merged(back, want, "reversed")


# ---- 2. key widths -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [0, 4, 9, 16, 256])
def test_key_widths(ctx, comm, w):
    rng = np.random.default_rng(300 + w)
    sizes = [2000, 1025, 70]
    sw = {0: 3, 4: 3, 9: 9, 16: 16, 256: 255}[w]                   # width of the string column 0
    pool = rng.integers(97, 123, size=(40, sw)).astype(np.uint8)
    pool[:, : min(8, sw - 1)] = ord("k")                            # the keys share their first bytes
    if w == 256:
        pool = pool[:1].repeat(40, axis=0)                           # one name: the two groups differ only in the key's last byte (the int8)
    group = {0: [], 4: [2], 9: [0], 16: [0], 256: [0, 1]}[w]
    aggs = [(C, 2), (MN, 2), (S, 2), (MX, 3)]
    segs, queries = [], []
    for s, n in enumerate(sizes):
        br = blocks_of(n, 1024)
        sname = rng.integers(97, 123, size=(n, 16)).astype(np.uint8)
        sname[:, :8] = ord("p")
        cols = [RawColumn(DENSE_STRING, sw, pool[rng.integers(s * 5, 30 + s * 5, size=n)], br),
                RawColumn(DENSE_TINYINT, 1, rng.integers(0, 2, size=n).astype(np.int8), br),
                RawColumn(DENSE_INT, 4, rng.integers(-50, 50, size=n).astype(np.int32), br), RawColumn(DENSE_STRING, 16, sname, br)]
        segs.append(native.DeviceSegment(ctx, [c.native() for c in cols]))
        queries.append(agg_query(ctx, segs[-1], 4, [], group, aggs))
    want = host_combine(queries, [0, 1, 2])
    assert want[0].shape[1] == w and want[0].shape[0] == {0: 1, 256: 2}.get(w, want[0].shape[0]) and want[0].shape[0] >= 1
    got = comm.merge_groups_wide(queries, [0, 1, 2])
    assert_merged(got, want, w)
    assert_table_agrees(got, table_result(ctx, segs, 4, group, aggs), w)
    for q in queries:
        q.close()
    for s in segs:
        s.close()


# ---- 3. many groups ------------------------------------------------------------------------------------------------------------------
def test_many_groups_and_a_short_output(ctx, comm):
    rng = np.random.default_rng(33)
    pool = np.unique(rng.integers(97, 123, size=(6000, 12)).astype(np.uint8), axis=0)[:5000]
    assert pool.shape[0] == 5000
    pool = pool[rng.permutation(5000)]
    slices = [(0, 2500), (1500, 4000), (3000, 5000)]                # partial overlap
    aggs = [(C, 1), (MX, 1), (MN, 1), (S, 1)]
    segs, queries = [], []
    for lo, hi in slices:
        n = 6000
        pick = rng.permutation(np.concatenate([np.arange(lo, hi), rng.integers(lo, hi, size=n - (hi - lo))]))   # every key of the slice occurs
        br = blocks_of(n, 1024)
        cols = [RawColumn(DENSE_STRING, 12, pool[pick], br), RawColumn(DENSE_INT, 4, rng.integers(-10 ** 6, 10 ** 6, size=n).astype(np.int32), br)]
        segs.append(native.DeviceSegment(ctx, [c.native() for c in cols]))
        queries.append(agg_query(ctx, segs[-1], 2, [], [0], aggs))
    want = host_combine(queries, [0, 1, 2])
    assert want[0].shape == (5000, 12)
    got = comm.merge_groups_wide(queries, [0, 1, 2])
    assert_merged(got, want)
    assert_table_agrees(got, table_result(ctx, segs, 2, [0], aggs))
    short = comm.merge_groups_wide(queries, [0, 1, 2], max_groups=10)
    assert short[5] == 5000 and short[0].shape == (10, 12)
    assert_merged(short, tuple(a[:10] for a in want[:4]) + ({},), "max_groups = 10")
    for q in queries:
        q.close()
    for s in segs:
        s.close()


# ---- 4. wide string MAX under a narrow key ---------------------------------------------------------------------------------------------
def test_wide_string_max_under_a_narrow_key(ctx, comm):
    rng = np.random.default_rng(44)
    states = np.array([list(b"AA"), list(b"BB"), list(b"CC"), list(b"DD"), list(b"EE")], np.uint8)
    sizes = [1500, 1025, 300]

    def strings(n, w):
        """random w-byte strings that share their first 8 bytes and stay below 'z' behind them"""
        v = rng.integers(97, 122, size=(n, w)).astype(np.uint8)
        v[:, :8] = ord("p")
        return v

    def top(w, tag):
        v = np.full(w, ord("p"), np.uint8)
        v[8] = ord("z")                                                # above every random string, from byte 9 on
        v[-1] = tag
        return v
    per = []
    for n in sizes:
        st = rng.integers(0, 5, size=n)
        st[:5] = np.arange(5)                                          # every state in every segment; rows 0 .. 4 are set below
        per.append([st, strings(n, 16), strings(n, 256)])
    for col, w in ((1, 16), (2, 256)):
        per[2][col][0] = top(w, ord("1"))                              # state AA: the maximum sits in the last segment
        per[0][col][1] = top(w, ord("2"))                              # state BB: in the first
        per[0][col][2] = top(w, ord("3"))                              # state CC: two segments hold the identical maximum
        per[1][col][2] = top(w, ord("3"))
    aggs = [(MX, 1), (C, 0), (MX, 2)]
    segs, queries = [], []
    for (st, s16, s256), n in zip(per, sizes):
        br = blocks_of(n, 1024)
        cols = [RawColumn(DENSE_STRING, 2, states[st], br), RawColumn(DENSE_STRING, 16, s16, br), RawColumn(DENSE_STRING, 256, s256, br)]
        segs.append(native.DeviceSegment(ctx, [c.native() for c in cols]))
        queries.append(agg_query(ctx, segs[-1], 3, [], [0], aggs))
    want = host_combine(queries, [0, 1, 2])
    got = comm.merge_groups_wide(queries, [0, 1, 2])
    assert_merged(got, want)
    keys = [bytes(k) for k in got[0]]
    for state, tag in ((b"AA", "1"), (b"BB", "2"), (b"CC", "3")):
        g = keys.index(state)
        for j, w in ((0, 16), (2, 256)):
            assert bytes(got[4][j][g]) == bytes(top(w, ord(tag))), (state, w)
            assert int(got[3][g, j]) == int.from_bytes(b"pppppppp", "big")     # the shared first 8 bytes, big-endian
    assert_table_agrees(got, table_result(ctx, segs, 3, [0], aggs))
    for q in queries:
        q.close()
    for s in segs:
        s.close()


# ---- 5. narrow equals old --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [[], [1], [0], [1, 0], [3]])
def test_narrow_keys_equal_the_existing_merge(ctx, comm, group):
    rng = np.random.default_rng(55)
    n8 = rng.integers(97, 123, size=(30, 8)).astype(np.uint8)
    aggs = [(C, 2), (MX, 2), (MN, 2), (S, 2)] if group != [3] else [(MX, 3), (C, 2), (MX, 4)]
    segs, queries = [], []
    for n in (3000, 1025, 64):
        br = blocks_of(n, 1024)
        cols = [RawColumn(DENSE_INT, 4, rng.integers(0, 700, size=n).astype(np.int32) * 3 - 1000, br),
                RawColumn(DENSE_TINYINT, 1, rng.integers(-20, 20, size=n).astype(np.int8), br),
                RawColumn(DENSE_INT, 4, rng.integers(-10 ** 6, 10 ** 6, size=n).astype(np.int32), br),
                RawColumn(DENSE_STRING, 8, n8[rng.integers(0, 30, size=n)], br),
                RawColumn(DENSE_STRING, 2, n8[rng.integers(0, 30, size=n), :2], br)]
        segs.append(native.DeviceSegment(ctx, [c.native() for c in cols]))
        queries.append(agg_query(ctx, segs[-1], 5, [], group, aggs))
    keys, first, counts, vals = comm.merge_groups(queries, [0, 1, 2])
    got = comm.merge_groups_wide(queries, [0, 1, 2])
    kb = sum([4, 1, 4, 8, 2][g] for g in group)
    assert got[0].shape == (keys.size, kb)
    assert np.array_equal(got[0], np.ascontiguousarray(keys, dtype="<u8").view(np.uint8).reshape(-1, 8)[:, :kb])
    assert got[1].tolist() == first.tolist() and got[2].tolist() == counts.tolist() and got[3].tolist() == vals.tolist()
    assert_merged(got, host_combine(queries, [0, 1, 2]), group)
    for q in queries:
        q.close()
    for s in segs:
        s.close()


# ---- 6. the single-process flavour -----------------------------------------------------------------------------------------------------
def test_all_flavour_gives_the_same_table(ctx, breaker):
    _, queries, seg_idx, want = breaker
    (c0,) = native.Comm.create_all([ctx])
    try:
        assert_merged(native.Comm.merge_groups_wide_all([c0], [queries], [seg_idx]), want)
    finally:
        c0.close()


# ---- 7. errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors(ctx, comm, breaker):
    segs, queries, seg_idx, want = breaker
    L = native.load()

    def merge(qs, str_ptrs=None):
        arr = (native.C.c_void_p * len(qs))(*[q._h for q in qs])
        seg = np.arange(len(qs), dtype=np.int32)
        n = native.C.c_uint32(0)
        native._check(L.imm3_comm_merge_groups_wide(comm._h, arr, seg.ctypes.data, len(qs), None, None, None, None, str_ptrs, 0, native.C.byref(n)))
        return n.value
    assert merge(queries[:4]) == want[0].shape[0]
    rng = np.random.default_rng(77)
    n = 500
    br = blocks_of(n, 1024)
    cols = [RawColumn(DENSE_STRING, 12, rng.integers(97, 100, size=(n, 12)).astype(np.uint8), br), RawColumn(DENSE_TINYINT, 1, np.zeros(n, np.int8), br),
            RawColumn(DENSE_INT, 4, np.arange(n, dtype=np.int32), br), RawColumn(DENSE_STRING, 24, rng.integers(97, 100, size=(n, 24)).astype(np.uint8), br),
            RawColumn(DENSE_STRING, 16, rng.integers(97, 100, size=(n, 16)).astype(np.uint8), br)]
    other = native.DeviceSegment(ctx, [c.native() for c in cols])
    narrower = agg_query(ctx, other, 5, [], GROUP, AGGS)                            # a 13-byte key beside the 17-byte ones
    with pytest.raises(native.Imm3Error) as e:
        merge([queries[0], narrower])
    assert e.value.code == native.ERR_ARG and "width" in e.value.msg
    same_key = agg_query(ctx, segs[0], 4, [], GROUP, [(C, 2), (MX, 2), (S, 2), (MX, 0)])   # MAX over the 16-byte name ...
    wider_max = agg_query(ctx, other, 5, [], [3], [(C, 2), (MX, 2), (S, 2), (MX, 3)])      # ... and over a 24-byte string, keys of 17 / 24 bytes
    same_w = agg_query(ctx, other, 5, [], [4, 1], [(C, 2), (MX, 2), (S, 2), (MX, 3)])      # a 17-byte key, MAX over 24 bytes: only the string width differs
    with pytest.raises(native.Imm3Error) as e:
        merge([same_key, same_w])
    assert e.value.code == native.ERR_ARG and "string MAX" in e.value.msg
    with pytest.raises(native.Imm3Error) as e:
        merge([queries[0], wider_max])
    assert e.value.code == native.ERR_ARG
    unrun = native.DeviceQuery(ctx, segs[0], [0, 1, 2, 3], [], (), 0, 1024, group_cols=GROUP, aggs=AGGS, wide_keys=True)
    with pytest.raises(native.Imm3Error) as e:
        merge([queries[0], unrun])
    assert e.value.code == native.ERR_STATE
    proj = native.DeviceQuery(ctx, segs[0], [0, 1, 2, 3], [], [2], 0, 1024)
    proj.run()
    with pytest.raises(native.Imm3Error) as e:
        merge([queries[0], proj])
    assert e.value.code == native.ERR_ARG and "not an aggregation" in e.value.msg
    buf = np.zeros((want[0].shape[0], 16), np.uint8)
    with pytest.raises(native.Imm3Error) as e:                                      # aggregate 0 is a COUNT
        merge(queries[:4], (native.C.c_void_p * 4)(buf.ctypes.data, None, None, None))
    assert e.value.code == native.ERR_ARG and "str_out[0]" in e.value.msg
    assert merge(queries[:4], (native.C.c_void_p * 4)(None, None, None, None)) == want[0].shape[0]
    assert_merged(comm.merge_groups_wide(queries, seg_idx), want, "after the refusals")
    for q in (narrower, same_key, wider_max, same_w, unrun, proj):
        q.close()
    other.close()


# ---- 9. Engine(device_merge=True) ------------------------------------------------------------------------------------------------------
def test_engine_device_merge_equals_the_host_combine(tmp_path):
    from immutable3_amd import Count, Max, Min, NoSelect, ProjectAgg, Query
    from immutable3_amd.operators import Engine, GpuSegmentManager
    from immutable3_amd.schema import CodecType, Column, Table, TableIO
    from immutable3_amd.storage import SegmentManager, write_segment_arrays
    rng = np.random.default_rng(99)
    t = Table("people", [Column.make("id", CodecType.DENSE_INT), Column.make("state", CodecType.DENSE_STRING, {"size": "2"}),
                         Column.make("name", CodecType.DENSE_STRING, {"size": "16"}), Column.make("age", CodecType.DENSE_TINYINT),
                         Column.make("email", CodecType.DENSE_STRING, {"size": "24"})], 1000)
    TableIO.store(str(tmp_path), t)
    names = rng.integers(97, 123, size=(60, 16)).astype(np.uint8)
    names[:, :8] = ord("n")
    states = np.array([list(b"%c%c" % (65 + i, 66 + i)) for i in range(7)], np.uint8)
    for s, br in enumerate(([1000, 777], [1000, 1000, 5], [300])):               # ragged: no imm3_table, per-segment queries
        n = sum(br)
        email = rng.integers(97, 123, size=(n, 24)).astype(np.uint8)
        email[:, :8] = ord("e")
        write_segment_arrays(str(tmp_path), t, s, {"id": np.arange(n, dtype=np.int32) + s * 10 ** 4, "state": states[rng.integers(0, 7, size=n)],
                                                    "name": names[rng.integers(s * 10, 40 + s * 10, size=n)],
                                                    "age": rng.integers(0, 100, size=n).astype(np.int8), "email": email}, block_rows=br)
    gsm = GpuSegmentManager(SegmentManager(str(tmp_path)))
    try:
        assert gsm.device_table("people") is None
        for aggs, group in (([Count("id"), Max("age"), Min("age"), Max("email")], ["name"]),
                            ([Count("id"), Max("email")], ["state", "name"]), ([Max("name"), Count("id")], ["state"])):
            q = Query("people", NoSelect, ProjectAgg(aggs, group))
            want = Engine(gsm).execute_agg(q)
            got = Engine(gsm, device_merge=True).execute_agg(q)
            assert len(want) > 6 and list(got) == list(want), group
            for k in want:
                assert list(got[k]) == list(want[k]) and [type(a) for a in got[k].values()] == [type(a) for a in want[k].values()], (group, k)
                assert [a.repr() for a in got[k].values()] == [a.repr() for a in want[k].values()], (group, k)
    finally:
        gsm.close()
