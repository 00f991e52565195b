"""GPU suite: group-by aggregation on group keys wider than 8 bytes (the reference joins any group values into a string key,
ProjectAggregate.scala:135-156).  imm3_query_create_agg_wide / imm3_query_create_table_agg_wide take keys of up to
IMM3_GROUP_KEY_MAX_WIDTH bytes; the tables hold a tag (hash32 << 32 | representative row) and compare the key bytes in the columns
(DESIGN.md §10).  Expectations come from numpy (np.unique over the packed key bytes, first-seen order) and oracle_np.project_agg."""
import os
import subprocess

import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, GT, LT, MATCH, PforColumn, RawColumn, SnappyColumn, blocks_of
from immutable3_amd import native

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "immutable3_amd", "bin")
C, MN, MX, S = native.AGG_COUNT, native.AGG_MIN, native.AGG_MAX, native.AGG_SUM
FORMS = [native.AGG_FORM_LANES, native.AGG_FORM_LANES_WIDE, native.AGG_FORM_DIRECT, native.AGG_FORM_TILE, native.AGG_FORM_GENERAL]
STATES = np.array([list(b"%c%c" % (65 + i // 26, 65 + i % 26)) for i in range(51)], np.uint8)


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def key_bytes_of(col):
    """uint8[n, width]: the column's raw bytes per row, as the group key packs them"""
    if col.codec == DENSE_STRING:
        return np.ascontiguousarray(col.values, dtype=np.uint8).reshape(-1, col.width)
    return np.ascontiguousarray(col.values).view(np.uint8).reshape(-1, col.width)


def packed_keys(cols, group):
    n = cols[0].values.shape[0]
    parts = [key_bytes_of(cols[g]) for g in group]
    return np.concatenate(parts, axis=1) if parts else np.zeros((n, 0), np.uint8)


def prefix_u64(kb):
    """the first 8 key bytes little-endian: what fetch_groups returns as keys[g]"""
    v = np.zeros(kb.shape[0], np.uint64)
    for b in range(min(8, kb.shape[1])):
        v |= kb[:, b].astype(np.uint64) << np.uint64(8 * b)
    return v


def expect(cols, group, aggs, mask):
    """(prefix keys, first, counts, vals[g, j], {j: uint8[g, width]}, key bytes uint8[g, key_bytes]) in first-seen order"""
    packed = packed_keys(cols, group)
    sel = np.flatnonzero(mask)
    kb = packed.shape[1]
    kv = np.ascontiguousarray(packed[sel]).view(np.dtype((np.void, kb))).reshape(-1) if kb else np.zeros(sel.size, np.uint8)
    _, idx, inv = np.unique(kv, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    ng = idx.size
    order = np.argsort(idx, kind="stable")
    counts = np.bincount(inv, minlength=ng).astype(np.int64)
    vals = np.zeros((ng, len(aggs)), np.int64)
    strs = {}
    for j, (kind, c) in enumerate(aggs):
        col = cols[c]
        if kind == C:
            vals[:, j] = counts
        elif col.codec == DENSE_STRING:      # byte-lexicographic max: the last row of each group after a sort by (group, bytes)
            s = col.values[sel]
            last = np.lexsort(tuple(s[:, b] for b in range(col.width - 1, -1, -1)) + (inv,))
            best = s[last[np.cumsum(counts) - 1]] if ng else np.zeros((0, col.width), np.uint8)
            strs[j] = best[order]
            pre = np.zeros(ng, np.uint64)
            for b in range(min(8, col.width)):
                pre = (pre << np.uint64(8)) | best[:, b].astype(np.uint64)
            vals[:, j] = pre.view(np.int64)
        else:
            v = np.asarray(col.values, dtype=np.int64)[sel]
            out = np.zeros(ng, np.int64)
            if kind == S:
                np.add.at(out, inv, v)
            elif kind == MX:
                out[:] = np.iinfo(np.int64).min
                np.maximum.at(out, inv, v)
            else:
                out[:] = np.iinfo(np.int64).max
                np.minimum.at(out, inv, v)
            vals[:, j] = out
    keys = packed[sel[idx[order]]]
    return prefix_u64(keys), sel[idx[order]], counts[order], vals[order], strs, keys


def run_query(ctx, seg, used, sels, group, aggs, tuning=0, wide=True):
    """-> (form, prefix keys, first, counts, vals, {j: exact strings}, key bytes) of one run"""
    ctx.set_tuning(tuning, 0)
    try:
        q = native.DeviceQuery(ctx, seg, used, sels, (), 0, 1024, group_cols=group, aggs=aggs, wide_keys=wide)
        q.run()
        keys, first, counts, vals = q.fetch_groups()
        strs = {j: q.fetch_group_strings(j) for j, (k, c) in enumerate(aggs) if k == MX and seg.codecs[used[c]] == DENSE_STRING}
        kb = q.fetch_group_keys()
        form = q.agg_form()
        q.close()
    finally:
        ctx.set_tuning(0, 0)
    return form, keys, first, counts, vals, strs, kb


def assert_same(got, want, what=None):
    _, keys, first, counts, vals, strs, kb = got
    wk, wf, wc, wv, ws, wkb = want
    assert kb.shape == wkb.shape and np.array_equal(kb, wkb), what
    assert keys.tolist() == wk.tolist(), what
    assert first.tolist() == wf.tolist(), what
    assert counts.tolist() == wc.tolist(), what
    assert vals.tolist() == wv.tolist(), what
    assert sorted(strs) == sorted(ws), what
    for j in ws:
        assert strs[j].shape == ws[j].shape and np.array_equal(strs[j], ws[j]), (what, j)


def name_pool(rng, n_distinct, w, shared=0):
    """n_distinct distinct w-byte names; the first `shared` bytes are the same in all of them (prefix ties)"""
    pool = rng.integers(97, 123, size=(n_distinct * 2, w)).astype(np.uint8)
    pool[:, :shared] = ord("p")
    pool = np.unique(pool, axis=0)
    return pool[rng.permutation(pool.shape[0])[:n_distinct]]


def make_cols(rng, n, w, br=None, distinct=300, shared=0):
    """0 id int32, 1 age int8, 2 state 2-byte, 3 name (w bytes, `distinct` values), 4 / 5 / 6 small int32 (8 x 7 x 5 values),
    7 k8 int8 (4 values), 8 name8 8-byte string (40 values), 9 email 40-byte string"""
    br = br or blocks_of(n, 1024)
    names = name_pool(rng, distinct, w, shared)
    n8 = name_pool(rng, 40, 8)
    return [RawColumn(DENSE_INT, 4, rng.integers(-2 ** 31, 2 ** 31, size=n).astype(np.int32), br),
            RawColumn(DENSE_TINYINT, 1, rng.integers(-128, 128, size=n).astype(np.int8), br),
            RawColumn(DENSE_STRING, 2, STATES[rng.integers(0, 51, size=n)], br),
            RawColumn(DENSE_STRING, w, names[rng.integers(0, names.shape[0], size=n)], br),
            RawColumn(DENSE_INT, 4, rng.integers(0, 8, size=n).astype(np.int32), br),
            RawColumn(DENSE_INT, 4, rng.integers(-3, 4, size=n).astype(np.int32), br),
            RawColumn(DENSE_INT, 4, rng.integers(100, 105, size=n).astype(np.int32), br),
            RawColumn(DENSE_TINYINT, 1, rng.integers(0, 4, size=n).astype(np.int8), br),
            RawColumn(DENSE_STRING, 8, n8[rng.integers(0, 40, size=n)], br),
            RawColumn(DENSE_STRING, 40, rng.integers(97, 123, size=(n, 40)).astype(np.uint8), br)]


AGG_SETS = [[(C, 0), (MX, 1), (S, 0), (MN, 0)], [(MN, 1), (S, 1), (MX, 0), (C, 0)]]


def selections(cols, n):
    age = cols[1].values
    names = cols[3].values
    pick = [bytes(names[i]) for i in (0, 5, 17)]
    m = np.zeros(n, bool)
    for p in pick:
        m |= (names == np.frombuffer(p, np.uint8)).all(axis=1)
    return [([], np.ones(n, bool)), ([(1, GT, 18.0), (1, LT, 30.0)], (age > 18) & (age < 30)), ([(3, MATCH, pick)], m)]


# ---- 1. key widths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,group", [(9, [3]), (12, [4, 5, 6]), (16, [3]), (17, [3]), (32, [3]), (64, [3]), (256, [3]),
                                     (16, [7, 2, 3]), (16, [3, 2]), (30, [4, 3, 7, 5])])
def test_key_widths_against_numpy(ctx, w, group):
    rng = np.random.default_rng(w * 7 + len(group))
    n = 30_000 + w
    cols = make_cols(rng, n, w, shared=min(8, w - 1))
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    used = list(range(len(cols)))
    for aggs in AGG_SETS:
        for sels, mask in selections(cols, n):
            got = run_query(ctx, seg, used, sels, group, aggs)
            assert got[0] == native.AGG_FORM_GENERAL
            assert_same(got, expect(cols, group, aggs, mask), (w, group, aggs, sels))
    seg.close()


@pytest.mark.parametrize("codec", ["pfor", "snappy"])
def test_compressed_int_column_in_the_key(ctx, codec):
    rng = np.random.default_rng(3 if codec == "pfor" else 4)
    n = 50_000
    br = blocks_of(n, 1024)
    cols = make_cols(rng, n, 16, br=br)
    k = np.sort(rng.integers(0, 30, size=n)).astype(np.int32)     # sorted: PFOR blocks with few bits
    cols[4] = PforColumn(k, br) if codec == "pfor" else SnappyColumn(DENSE_INT, 4, k, br)
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    used = list(range(len(cols)))
    for aggs in AGG_SETS:
        for sels, mask in selections(cols, n)[:2]:
            assert_same(run_query(ctx, seg, used, sels, [4, 8], aggs), expect(cols, [4, 8], aggs, mask), (codec, aggs, sels))
    seg.close()


# ---- 2. forms and layouts --------------------------------------------------------------------------------------------------------
def test_every_forced_form_gives_the_general_form(ctx):
    rng = np.random.default_rng(31)
    n = 70_000
    cols = make_cols(rng, n, 16)
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    used = list(range(len(cols)))
    aggs = [(C, 0), (MX, 1)]
    sels = [(1, GT, 18.0), (1, LT, 30.0)]
    want = expect(cols, [3], aggs, (cols[1].values > 18) & (cols[1].values < 30))
    for form in FORMS:
        got = run_query(ctx, seg, used, sels, [3], aggs, tuning=100 + form)
        assert got[0] == native.AGG_FORM_GENERAL, form
        assert_same(got, want, form)
    seg.close()


def test_ragged_layout(ctx):
    rng = np.random.default_rng(51)
    br = [1000, 777, 3001] * 10 + [5]
    n = sum(br)
    cols = make_cols(rng, n, 17, br=br)
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    used = list(range(len(cols)))
    for group in ([3], [4, 5, 6], [2, 3]):
        for aggs in AGG_SETS:
            for sels, mask in selections(cols, n)[:2]:
                assert_same(run_query(ctx, seg, used, sels, group, aggs), expect(cols, group, aggs, mask), (group, aggs, sels))
    seg.close()


def test_table_query_over_segments(ctx):
    rng = np.random.default_rng(61)
    sizes = [70_000, 1024, 33_333, 90_000, 5_000]
    pool = name_pool(rng, 500, 20)
    per = []
    for n in sizes:
        cols = make_cols(rng, n, 20)
        cols[3] = RawColumn(DENSE_STRING, 20, pool[rng.integers(0, pool.shape[0], size=n)], blocks_of(n, 1024))
        per.append(cols)
    segs = [native.DeviceSegment(ctx, [c.native() for c in cols]) for cols in per]
    cat = [RawColumn(c.codec, c.width, np.concatenate([p[i].values for p in per]), [1]) for i, c in enumerate(per[0])]
    table = native.DeviceTable(ctx, segs)
    used = list(range(len(cat)))
    age = cat[1].values
    for group in ([3], [2, 3], [4, 5, 6]):
        for aggs in AGG_SETS:
            for sels, mask in (([], np.ones(age.size, bool)), ([(1, GT, 18.0), (1, LT, 30.0)], (age > 18) & (age < 30))):
                wk, _, wc, wv, _, wkb = expect(cat, group, aggs, mask)
                _, keys, first, counts, vals, _, kb = run_query(ctx, table, used, sels, group, aggs)
                assert np.array_equal(kb, wkb), (group, aggs, sels)
                assert keys.tolist() == wk.tolist() and counts.tolist() == wc.tolist() and vals.tolist() == wv.tolist(), (group, sels)
    table.close()
    for s in segs:
        s.close()


# ---- 3. cardinality ------------------------------------------------------------------------------------------------------------
def test_high_cardinality_spills_past_the_lds_table(ctx):
    rng = np.random.default_rng(71)
    n = 200_000
    cols = make_cols(rng, n, 16, distinct=100_000)
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    used = list(range(len(cols)))
    aggs = AGG_SETS[0]
    for sels, mask in selections(cols, n)[:2]:
        want = expect(cols, [3], aggs, mask)
        assert want[2].size > (50_000 if not sels else 5_000)
        assert_same(run_query(ctx, seg, used, sels, [3], aggs), want, sels)
    seg.close()


def test_few_groups_over_millions_of_rows(ctx):
    rng = np.random.default_rng(81)
    n = (1 << 22) + 12_345
    br = blocks_of(n, 1024)
    names = name_pool(rng, 5, 24, shared=20)            # five keys that differ only in their last 4 bytes
    cols = [RawColumn(DENSE_INT, 4, np.arange(n, dtype=np.int32), br),
            RawColumn(DENSE_TINYINT, 1, rng.integers(0, 100, size=n).astype(np.int8), br),
            RawColumn(DENSE_STRING, 24, names[rng.integers(0, 5, size=n)], br)]
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    aggs = [(C, 0), (MX, 1), (S, 0), (MN, 1)]
    age = cols[1].values
    for sels, mask in (([], np.ones(n, bool)), ([(1, GT, 18.0), (1, LT, 30.0)], (age > 18) & (age < 30))):
        assert_same(run_query(ctx, seg, [0, 1, 2], sels, [2], aggs), expect(cols, [2], aggs, mask), sels)
    seg.close()


# ---- 4. collisions: hash32 cut to 3 bits --------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["uniform", "ragged"])
def test_exact_under_forced_hash_collisions(ctx, layout):
    rng = np.random.default_rng(91)
    br = [1000, 777, 3001] * 8 if layout == "ragged" else None
    n = sum(br) if br else 40_000
    cols = make_cols(rng, n, 16, br=br, distinct=3_000, shared=12)
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    used = list(range(len(cols)))
    for group in ([3], [4, 3]):
        for sels, mask in selections(cols, n)[:2]:
            want = expect(cols, group, AGG_SETS[0], mask)
            assert want[2].size > (1_000 if not sels else 500)
            got = run_query(ctx, seg, used, sels, group, AGG_SETS[0], tuning=native.TV_AGG_WEAK_HASH)
            assert_same(got, want, (group, sels))
    # a wide string MAX under the weak hash too (its refine passes find rows' slots by the same compare)
    aggs = [(MX, 9), (C, 0)]
    assert_same(run_query(ctx, seg, used, [], [3], aggs, tuning=native.TV_AGG_WEAK_HASH), expect(cols, [3], aggs, np.ones(n, bool)))
    seg.close()


# ---- 5. wide string MAX under a wide key -------------------------------------------------------------------------------------
def test_wide_string_max_by_wide_key(ctx):
    rng = np.random.default_rng(101)
    n = 60_000
    cols = make_cols(rng, n, 16)
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    used = list(range(len(cols)))
    for group in ([3], [2, 3]):
        for aggs in ([(MX, 9), (C, 0)], [(C, 0), (MX, 9), (MX, 8), (MX, 2)]):
            for sels, mask in selections(cols, n):
                assert_same(run_query(ctx, seg, used, sels, group, aggs), expect(cols, group, aggs, mask), (group, aggs, sels))
    seg.close()


# ---- 6. narrow keys: the new getter, and the _wide entry at <= 8 bytes ----------------------------------------------------------
def test_narrow_keys_through_the_new_getter_and_entry(ctx):
    rng = np.random.default_rng(111)
    n = 50_000
    cols = make_cols(rng, n, 16)
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    used = list(range(len(cols)))
    for group, aggs in (([2], [(C, 0), (MX, 1)]), ([7, 2], [(C, 0), (S, 1)]), ([4, 5], [(C, 0), (MX, 1)]),
                        ([8], [(MX, 1), (MN, 0)]), ([], [(C, 0), (MX, 0)]), ([2], [(MX, 9), (C, 0)])):
        old = run_query(ctx, seg, used, [], group, aggs, wide=False)
        new = run_query(ctx, seg, used, [], group, aggs, wide=True)
        assert new[0] == old[0], (group, aggs)
        for a, b in zip(old[1:5], new[1:5]):
            assert a.tolist() == b.tolist(), (group, aggs)
        assert np.array_equal(old[6], new[6])
        kb = sum(cols[g].width for g in group)
        assert old[6].shape == (old[1].size, kb)
        u64 = np.ascontiguousarray(old[1], dtype="<u8").view(np.uint8).reshape(-1, 8)[:, :kb]
        assert np.array_equal(old[6], u64), (group, aggs)
        assert_same(new, expect(cols, group, aggs, np.ones(n, bool)), (group, aggs))
    # the forms the narrow key reaches are the old entry's: the lanes form for a 2-byte key
    assert run_query(ctx, seg, used, [], [2], [(C, 0), (MX, 1)])[0] == native.AGG_FORM_LANES
    seg.close()


# ---- 7. ABI errors and merges --------------------------------------------------------------------------------------------------
def test_abi_errors_and_merges(ctx):
    rng = np.random.default_rng(121)
    n = 5_000
    cols = make_cols(rng, n, 255)
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    used = list(range(len(cols)))
    with pytest.raises(native.Imm3Error) as e:                 # 255 + 2 = 257 bytes
        native.DeviceQuery(ctx, seg, used, [], (), 0, 1024, group_cols=[3, 2], aggs=[(C, 0)], wide_keys=True)
    assert e.value.code == native.ERR_ARG and "256" in e.value.msg
    with pytest.raises(native.Imm3Error) as e:                 # the old entry keeps its 8-byte bound
        native.DeviceQuery(ctx, seg, used, [], (), 0, 1024, group_cols=[4, 5, 6], aggs=[(C, 0)])
    assert e.value.code == native.ERR_ARG
    q = native.DeviceQuery(ctx, seg, used, [], (), 0, 1024, group_cols=[3, 7], aggs=[(C, 0), (MX, 1)], wide_keys=True)
    with pytest.raises(native.Imm3Error) as e:                 # before the first run
        q.fetch_group_keys()
    assert e.value.code == native.ERR_STATE
    q.run()
    assert q.fetch_group_keys().shape[1] == 256
    (c0,) = native.Comm.create_all([ctx])
    with pytest.raises(native.Imm3Error) as e:
        native.Comm.merge_groups_all([c0], [[q]], [[0]])
    assert e.value.code == native.ERR_ARG and "8 bytes" in e.value.msg
    c0.close()
    comm = native.Comm(ctx, 1, 0, native.comm_unique_id())
    with pytest.raises(native.Imm3Error) as e:
        comm.merge_groups([q], [0])
    assert e.value.code == native.ERR_ARG
    comm.close()
    q.close()
    p = native.DeviceQuery(ctx, seg, used, [], [0], 0, 1024)   # not an aggregation
    p.run()
    with pytest.raises(native.Imm3Error) as e:
        native._check(native.load().imm3_query_fetch_group_keys(p._h, None, 0))
    assert e.value.code == native.ERR_ARG
    p.close()
    seg.close()


# ---- 8. graph capture ----------------------------------------------------------------------------------------------------------
def test_graph_replay(ctx):
    rng = np.random.default_rng(131)
    n = 70_000
    cols = make_cols(rng, n, 16)
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    used = list(range(len(cols)))
    sels = [(1, GT, 18.0), (1, LT, 30.0)]
    aggs = [(C, 0), (MX, 9), (S, 1)]
    want = expect(cols, [3, 2], aggs, (cols[1].values > 18) & (cols[1].values < 30))
    q = native.DeviceQuery(ctx, seg, used, sels, (), 0, 1024, group_cols=[3, 2], aggs=aggs, wide_keys=True)
    for _ in range(2):
        q.run()
        assert np.array_equal(q.fetch_group_keys(), want[5])
    with ctx.capture() as cap:
        q.run()
    for _ in range(2):
        cap.graph.launch()
        keys, first, counts, vals = q.fetch_groups()
        assert keys.tolist() == want[0].tolist() and first.tolist() == want[1].tolist() and counts.tolist() == want[2].tolist()
        assert vals.tolist() == want[3].tolist()
        assert np.array_equal(q.fetch_group_keys(), want[5])
        assert np.array_equal(q.fetch_group_strings(1), want[4][1])
    cap.graph.close()
    q.close()
    seg.close()


# ---- 9. end to end: loader-made table, Engine (table and per-segment paths), imm3_sql ------------------------------------------
def test_engine_and_cli_end_to_end(tmp_path):
    from oracle import oracle_np
    from immutable3_amd import Count, Max, NoSelect, ProjectAgg, Query
    from immutable3_amd.operators import Engine, GpuSegmentManager, java_double_to_string
    from immutable3_amd.storage import SegmentManager
    rng = np.random.default_rng(141)
    n = 7_000
    st = STATES[rng.integers(0, 20, size=n)]
    names = name_pool(rng, 60, 16, shared=6)[rng.integers(0, 60, size=n)]
    ages = rng.integers(0, 100, size=n).astype(np.int8)
    csv = tmp_path / "people.csv"
    with open(csv, "w") as f:
        f.write("id,state,name,age\n")
        for i in range(n):
            f.write(f"{i},{bytes(st[i]).decode()},{bytes(names[i]).decode()},{ages[i]}\n")
    ocols = [RawColumn(DENSE_INT, 4, np.arange(n, dtype=np.int32), [n]).npcol(), RawColumn(DENSE_STRING, 2, st, [n]).npcol(),
             RawColumn(DENSE_STRING, 16, names, [n]).npcol(), RawColumn(DENSE_TINYINT, 1, ages, [n]).npcol()]
    for block in (1024, 1000):
        d = tmp_path / f"data{block}"
        d.mkdir()
        p = subprocess.run([os.path.join(BIN, "imm3_loader"), "-t", "people", "-c",
                            "id:DENSE_INT,state:DENSE_STRING:size=2,name:DENSE_STRING:size=16,age:DENSE_TINYINT",
                            "-d", str(d), "-i", str(csv), "--block-size", str(block), "--segment-size", "2"],
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        for group in (["name"], ["state", "name"]):
            gi = [{"id": 0, "state": 1, "name": 2, "age": 3}[g] for g in group]
            want = oracle_np.project_agg(ocols, gi, [("count", 0), ("max", 3)], [np.ones(n, bool)])
            gsm = GpuSegmentManager(SegmentManager(str(d)))
            try:
                assert gsm.getTableSegmentCount("people") >= 3
                q = Query("people", NoSelect, ProjectAgg([Count("id"), Max("age")], group))
                got = Engine(gsm).execute_agg(q)
                assert list(got) == list(want), (block, group)
                for k, m in got.items():
                    assert [a.get() for a in m.values()] == want[k], (block, group, k)
            finally:
                gsm.close()
            sql = f"select count(id), max(age) from people group by {', '.join(group)}"
            p = subprocess.run([os.path.join(BIN, "imm3_sql"), "-q", sql, "-d", str(d)], capture_output=True, text=True, timeout=120)
            assert p.returncode == 0, p.stderr
            rows = [f"Row({c},{java_double_to_string(float(m))})" for c, m in want.values()]
            assert p.stdout.splitlines() == rows, (block, group)
