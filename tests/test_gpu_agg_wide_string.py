"""GPU suite: MAX over STRING columns wider than 8 bytes in the group-by aggregation (MaxStringAggr at any width,
ProjectAggregate.scala:77-89; max(col) and min(col) on a STRING column both become it, Engine.scala:130-156).  The aggregation
launch folds the first 8 bytes; refine passes settle the rest.  Expectations come from numpy (a lexicographic
sort per group) and from oracle_np.project_agg."""
import os
import subprocess

import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, GT, LT, MATCH, RawColumn, blocks_of
from immutable3_amd import native

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "immutable3_amd", "bin")
C, MN, MX, S = native.AGG_COUNT, native.AGG_MIN, native.AGG_MAX, native.AGG_SUM
FORMS = [native.AGG_FORM_LANES, native.AGG_FORM_LANES_WIDE, native.AGG_FORM_DIRECT, native.AGG_FORM_TILE, native.AGG_FORM_GENERAL]
WIDTHS = [9, 12, 16, 17, 24, 31, 32, 64, 256]
STATES = np.array([list(b"%c%c" % (65 + i // 26, 65 + i % 26)) for i in range(51)], np.uint8)


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def raw_of(col):
    """the column's values as the unsigned little-endian integers the group key packs"""
    if col.codec == DENSE_STRING:
        v = np.zeros(col.values.shape[0], np.uint64)
        for b in range(col.width):
            v |= col.values[:, b].astype(np.uint64) << np.uint64(8 * b)
        return v
    return np.ascontiguousarray(col.values).view({1: np.uint8, 4: np.uint32}[col.width]).astype(np.uint64)


def be_prefix(strs):
    """first 8 bytes of each value packed big-endian, as fetch_groups returns them for a wide string MAX"""
    v = np.zeros(strs.shape[0], np.uint64)
    for b in range(min(8, strs.shape[1])):
        v = (v << np.uint64(8)) | strs[:, b].astype(np.uint64)
    return v.view(np.int64)


def expect(cols, group, aggs, mask):
    """(keys, first, counts, vals[g, j], {j: uint8[g, width]}) in first-seen order"""
    key = np.zeros(mask.size, np.uint64)
    shift = 0
    for g in group:
        key |= raw_of(cols[g]) << np.uint64(8 * shift)
        shift += cols[g].width
    sel = np.flatnonzero(mask)
    uniq, idx, inv = np.unique(key[sel], return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(idx, kind="stable")
    counts = np.bincount(inv, minlength=uniq.size).astype(np.int64)
    vals = np.zeros((uniq.size, len(aggs)), np.int64)
    strs = {}
    for j, (kind, c) in enumerate(aggs):
        col = cols[c]
        if kind == C:
            vals[:, j] = counts
        elif col.codec == DENSE_STRING:      # byte-lexicographic max: sort by group, then by every byte; the last row of a group wins
            s = col.values[sel]
            chunks = []                      # the bytes as big-endian u64 chunks: the same order, fewer sort keys
            for k in range(0, col.width, 8):
                v = np.zeros(s.shape[0], np.uint64)
                for b in range(k, min(k + 8, col.width)):
                    v = (v << np.uint64(8)) | s[:, b].astype(np.uint64)
                chunks.append(v)
            last = np.lexsort(tuple(chunks[::-1]) + (inv,))
            ends = np.cumsum(counts) - 1
            best = s[last[ends]] if uniq.size else np.zeros((0, col.width), np.uint8)
            strs[j] = best[order]
            vals[:, j] = be_prefix(best)
        else:
            v = np.asarray(col.values, dtype=np.int64)[sel]
            out = np.zeros(uniq.size, np.int64)
            if kind == S:
                np.add.at(out, inv, v)
            elif kind == MX:
                out[:] = np.iinfo(np.int64).min
                np.maximum.at(out, inv, v)
            else:
                out[:] = np.iinfo(np.int64).max
                np.minimum.at(out, inv, v)
            vals[:, j] = out
    return uniq[order], sel[idx[order]], counts[order], vals[order], strs


def run_query(ctx, seg, used, sels, group, aggs, tuning=0):
    """-> (form, keys, first, counts, vals, {j: exact strings}) of one run"""
    ctx.set_tuning(tuning, 0)
    try:
        q = native.DeviceQuery(ctx, seg, used, sels, (), 0, 1024, group_cols=group, aggs=aggs)
        q.run()
        keys, first, counts, vals = q.fetch_groups()
        strs = {j: q.fetch_group_strings(j) for j, (k, c) in enumerate(aggs) if k == MX and seg.codecs[used[c]] == DENSE_STRING}
        form = q.agg_form()
        q.close()
    finally:
        ctx.set_tuning(0, 0)
    return form, keys, first, counts, vals, strs


def assert_same(got, want, what=None):
    _, keys, first, counts, vals, strs = got
    wk, wf, wc, wv, ws = want
    assert keys.tolist() == wk.tolist(), what
    assert first.tolist() == wf.tolist(), what
    assert counts.tolist() == wc.tolist(), what
    assert vals.tolist() == wv.tolist(), what
    assert sorted(strs) == sorted(ws), what
    for j in ws:
        assert strs[j].shape == ws[j].shape and np.array_equal(strs[j], ws[j]), (what, j)


def rand_strings(rng, n, w, alphabet=b"abcdefghijklmnopqrstuvwxyz"):
    a = np.frombuffer(alphabet, np.uint8)
    return a[rng.integers(0, a.size, size=(n, w))]


def make_cols(rng, n, w, br=None, w2=None):
    """id int32, age int8, state 2-byte (51 codes), k600 int32 (~600 keys), ka / kb int32 (an 8-byte key), name (w bytes)[, name2]"""
    br = br or blocks_of(n, 1024)
    cols = [RawColumn(DENSE_INT, 4, rng.integers(-2 ** 31, 2 ** 31, size=n).astype(np.int32), br),
            RawColumn(DENSE_TINYINT, 1, rng.integers(-128, 128, size=n).astype(np.int8), br),
            RawColumn(DENSE_STRING, 2, STATES[rng.integers(0, 51, size=n)], br),
            RawColumn(DENSE_INT, 4, rng.integers(0, 600, size=n).astype(np.int32), br),
            RawColumn(DENSE_INT, 4, rng.integers(0, 7, size=n).astype(np.int32), br),
            RawColumn(DENSE_INT, 4, rng.integers(-3, 3, size=n).astype(np.int32), br),
            RawColumn(DENSE_STRING, w, rand_strings(rng, n, w), br)]
    if w2:
        cols.append(RawColumn(DENSE_STRING, w2, rand_strings(rng, n, w2, b"AB"), br))
    return cols


GROUPS = [[], [2], [3], [4, 5]]   # no group; 51 two-byte states; ~600 keys (the global table takes the overflow); an 8-byte key


# ---- random data, every width and group layout, with and without a select --------------------------------------------------------
@pytest.mark.parametrize("w", WIDTHS)
def test_wide_max_against_numpy(ctx, w):
    rng = np.random.default_rng(w)
    n = 40_000 + w
    cols = make_cols(rng, n, w)
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    used = list(range(len(cols)))
    age = cols[1].values
    aggs = [(C, 0), (MX, 6), (MN, 1), (S, 1)]
    for group in GROUPS:
        for sels, mask in (([], np.ones(n, bool)), ([(1, GT, 18.0), (1, LT, 30.0)], (age > 18) & (age < 30))):
            got = run_query(ctx, seg, used, sels, group, aggs)
            assert got[0] == native.AGG_FORM_GENERAL
            assert_same(got, expect(cols, group, aggs, mask), (w, group, sels))
    seg.close()


def test_two_wide_maxima_and_a_match_on_the_wide_column(ctx):
    rng = np.random.default_rng(5)
    n = 60_000
    cols = make_cols(rng, n, 16, w2=33)
    names = cols[6].values
    pick = [bytes(names[i]) for i in (3, 77, 1234, 50_000)]
    mask = np.zeros(n, bool)
    for p in pick:
        mask |= (names == np.frombuffer(p, np.uint8)).all(axis=1)
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    used = list(range(len(cols)))
    aggs = [(MX, 7), (C, 0), (MX, 6), (MN, 0)]
    for group in GROUPS:
        assert_same(run_query(ctx, seg, used, [], group, aggs), expect(cols, group, aggs, np.ones(n, bool)), group)
        assert_same(run_query(ctx, seg, used, [(6, MATCH, pick)], group, aggs), expect(cols, group, aggs, mask), group)
    seg.close()


def test_against_the_oracle(ctx):
    from oracle import oracle_np
    rng = np.random.default_rng(11)
    n = 6_000
    cols = make_cols(rng, n, 12)
    br = blocks_of(n, 1024)
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    used = list(range(len(cols)))
    age = cols[1].values
    for sels, keep in (([], np.ones(n, bool)), ([(1, GT, 18.0), (1, LT, 30.0)], (age > 18) & (age < 30))):
        masks, off = [], 0
        for b in br:
            masks.append(keep[off: off + b])
            off += b
        want = oracle_np.project_agg([c.npcol() for c in cols], [2], [("max", 6), ("count", 0)], masks)
        _, keys, first, counts, vals, strs = run_query(ctx, seg, used, sels, [2], [(MX, 6), (C, 0)])
        got = {int(k).to_bytes(2, "little").decode(): [bytes(strs[0][g]).decode("utf-8", "replace"), int(counts[g])]
               for g, k in enumerate(keys)}
        assert list(got) == list(want) and got == want
    seg.close()


# ---- adversarial data ----------------------------------------------------------------------------------------------------------
def test_shared_prefixes_ties_and_nul_maxima(ctx):
    rng = np.random.default_rng(21)
    w, n = 32, 50_000 + 333
    cols = make_cols(rng, n, w)
    names = cols[6].values
    st = rng.integers(0, 51, size=n)
    cols[2] = RawColumn(DENSE_STRING, 2, STATES[st], blocks_of(n, 1024))
    # groups 0..9: every row shares its first 8 / 16 / w - 1 bytes with the others of its group
    for g, share in zip(range(10), [8, 16, w - 1, 8, 16, w - 1, 8, 16, w - 1, w - 1]):
        rows = st == g
        names[rows, :share] = np.frombuffer(b"%02d" % g + b"x" * (w - 2), np.uint8)[:share]
    # group 10: the maximum sits in several rows, the last of them in the last tile
    rows = np.flatnonzero(st == 10)
    top = np.frombuffer(b"~" * w, np.uint8)
    for r in (rows[0], rows[rows.size // 2], rows[-1]):
        names[r] = top
    # group 11: every value all NUL bytes (the maximum is that value, not "unset")
    names[st == 11] = 0
    cols[6] = RawColumn(DENSE_STRING, w, names, blocks_of(n, 1024))     # (a RawColumn copies its bytes when it is made)
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    used = list(range(len(cols)))
    aggs = [(C, 0), (MX, 6)]
    want = expect(cols, [2], aggs, np.ones(n, bool))
    got = run_query(ctx, seg, used, [], [2], aggs)
    assert_same(got, want)
    strs, keys = got[5][1], got[1]
    k11 = int(STATES[11][0]) | (int(STATES[11][1]) << 8)
    assert strs[keys.tolist().index(k11)].tolist() == [0] * w
    k10 = int(STATES[10][0]) | (int(STATES[10][1]) << 8)
    assert bytes(strs[keys.tolist().index(k10)]) == b"~" * w
    # an empty selection
    got = run_query(ctx, seg, used, [(1, GT, 127.0)], [2], aggs)
    assert got[1].size == 0 and got[5][1].shape == (0, w)
    got = run_query(ctx, seg, used, [(1, GT, 127.0)], [], aggs)
    assert got[1].size == 0 and got[5][1].shape == (0, w)
    seg.close()


# ---- execution paths -------------------------------------------------------------------------------------------------------------
def test_every_forced_form_repeated_runs_and_a_graph(ctx):
    rng = np.random.default_rng(31)
    n = 70_000
    cols = make_cols(rng, n, 24)
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    used = list(range(len(cols)))
    aggs = [(C, 0), (MX, 6)]
    sels = [(1, GT, 18.0), (1, LT, 30.0)]
    want = expect(cols, [2], aggs, (cols[1].values > 18) & (cols[1].values < 30))
    for form in FORMS:    # every form that accepts the query gives the same bytes: the general form is the one that does
        got = run_query(ctx, seg, used, sels, [2], aggs, tuning=100 + form)
        assert got[0] == native.AGG_FORM_GENERAL
        assert_same(got, want, form)
    q = native.DeviceQuery(ctx, seg, used, sels, (), 0, 1024, group_cols=[2], aggs=aggs)
    for _ in range(3):
        q.run()
        assert np.array_equal(q.fetch_group_strings(1), want[4][1])
    with ctx.capture() as cap:
        q.run()
    for _ in range(2):
        cap.graph.launch()
        keys, first, counts, vals = q.fetch_groups()
        assert keys.tolist() == want[0].tolist() and counts.tolist() == want[2].tolist()
        assert np.array_equal(q.fetch_group_strings(1), want[4][1])
    cap.graph.close()
    q.close()
    seg.close()


def test_large_segment_against_numpy(ctx):
    rng = np.random.default_rng(41)
    n = (1 << 24) + (1 << 20)
    w = 16
    br = blocks_of(n, 1024)
    st = rng.integers(0, 51, size=n)
    names = rand_strings(rng, n, w, b"abcd")        # four letters: long shared prefixes, many ties on the first 8 bytes
    cols = [RawColumn(DENSE_INT, 4, np.arange(n, dtype=np.int32), br),
            RawColumn(DENSE_TINYINT, 1, rng.integers(0, 100, size=n).astype(np.int8), br),
            RawColumn(DENSE_STRING, 2, STATES[st], br),
            RawColumn(DENSE_STRING, w, names, br)]
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    aggs = [(C, 0), (MX, 3)]
    age = cols[1].values
    for sels, mask in (([], np.ones(n, bool)), ([(1, GT, 18.0), (1, LT, 30.0)], (age > 18) & (age < 30))):
        assert_same(run_query(ctx, seg, [0, 1, 2, 3], sels, [2], aggs), expect(cols, [2], aggs, mask), sels)
    seg.close()


# ---- layouts: ragged blocks, table queries over several segments --------------------------------------------------------------
def test_ragged_layout(ctx):
    rng = np.random.default_rng(51)
    br = [1000, 777, 3001] * 10 + [5]
    n = sum(br)
    cols = make_cols(rng, n, 17, br=br)
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    used = list(range(len(cols)))
    aggs = [(MX, 6), (C, 0), (MX, 1)]
    for group in GROUPS:
        for sels, mask in (([], np.ones(n, bool)), ([(1, GT, 0.0)], cols[1].values > 0)):
            assert_same(run_query(ctx, seg, used, sels, group, aggs), expect(cols, group, aggs, mask), (group, sels))
    seg.close()


def test_table_query_over_segments(ctx):
    rng = np.random.default_rng(61)
    sizes = [70_000, 1024, 33_333, 90_000, 5_000]
    per = [make_cols(rng, n, 20) for n in sizes]
    # the maximum of every state in the last segment's last rows
    last = per[-1]
    last[6].values[-51:] = np.frombuffer(b"z" * 20, np.uint8)
    last[2].values[-51:] = STATES
    for i in (2, 6):                 # (a RawColumn copies its bytes when it is made)
        last[i] = RawColumn(DENSE_STRING, last[i].width, last[i].values, blocks_of(sizes[-1], 1024))
    segs = [native.DeviceSegment(ctx, [c.native() for c in cols]) for cols in per]
    cat = [RawColumn(c.codec, c.width, np.concatenate([p[i].values for p in per]), [1]) for i, c in enumerate(per[0])]
    table = native.DeviceTable(ctx, segs)
    used = list(range(len(cat)))
    age = cat[1].values
    aggs = [(C, 0), (MX, 6), (S, 1)]
    for group in GROUPS:
        for sels, mask in (([], np.ones(age.size, bool)), ([(1, GT, 18.0), (1, LT, 30.0)], (age > 18) & (age < 30))):
            wk, _, wc, wv, ws = expect(cat, group, aggs, mask)
            _, keys, first, counts, vals, strs = run_query(ctx, table, used, sels, group, aggs)
            assert keys.tolist() == wk.tolist() and counts.tolist() == wc.tolist() and vals.tolist() == wv.tolist(), (group, sels)
            assert np.array_equal(strs[1], ws[1]), (group, sels)
    table.close()
    for s in segs:
        s.close()


# ---- ABI -----------------------------------------------------------------------------------------------------------------------
def test_abi_errors_and_merges(ctx):
    rng = np.random.default_rng(71)
    n = 5_000
    cols = make_cols(rng, n, 16, w2=257)
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    used = list(range(len(cols)))
    with pytest.raises(native.Imm3Error) as e:
        native.DeviceQuery(ctx, seg, used, [], (), 0, 1024, group_cols=[2], aggs=[(MX, 7)])
    assert e.value.code == native.ERR_ARG and "256" in e.value.msg
    for kind in (MN, S):     # the other checks keep their text
        with pytest.raises(native.Imm3Error) as e:
            native.DeviceQuery(ctx, seg, used, [], (), 0, 1024, group_cols=[2], aggs=[(kind, 6)])
        assert e.value.code == native.ERR_UNSUPPORTED_VECTOR and "bad aggregator for this data type" in e.value.msg
    q = native.DeviceQuery(ctx, seg, used, [], (), 0, 1024, group_cols=[2], aggs=[(C, 0), (MX, 6), (MX, 0)])
    q.run()
    for j in (0, 2, 3, -1):  # a count, a numeric max, out of range
        with pytest.raises(native.Imm3Error) as e:
            q.fetch_group_strings(j)
        assert e.value.code == native.ERR_ARG
    (c0,) = native.Comm.create_all([ctx])
    with pytest.raises(native.Imm3Error) as e:
        native.Comm.merge_groups_all([c0], [[q]], [[0]])
    assert e.value.code == native.ERR_ARG
    c0.close()
    comm = native.Comm(ctx, 1, 0, native.comm_unique_id())
    with pytest.raises(native.Imm3Error) as e:
        comm.merge_groups([q], [0])
    assert e.value.code == native.ERR_ARG
    comm.close()
    q.close()
    seg.close()


def test_narrow_string_max_unchanged(ctx):
    rng = np.random.default_rng(81)
    n = 50_000
    cols = make_cols(rng, n, 16)
    cols.append(RawColumn(DENSE_STRING, 8, rand_strings(rng, n, 8), blocks_of(n, 1024)))
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    used = list(range(len(cols)))
    for group, aggs, form in (([2], [(C, 0), (MX, 2)], native.AGG_FORM_LANES), ([3], [(MX, 2), (C, 0)], None),
                              ([2], [(MX, 7)], native.AGG_FORM_GENERAL), ([], [(MX, 7), (MX, 2)], native.AGG_FORM_GENERAL)):
        got = run_query(ctx, seg, used, [], group, aggs)
        assert form is None or got[0] == form, (group, aggs)
        want = expect(cols, group, aggs, np.ones(n, bool))
        assert_same(got, want, (group, aggs))
        for j, (k, c) in enumerate(aggs):     # vals: the value's bytes packed big-endian, as fetch_group_strings has them
            if k == MX:
                w = cols[c].width
                packed = [int(v).to_bytes(8, "big", signed=True)[8 - w:] for v in got[4][:, j]]
                assert packed == [bytes(r) for r in got[5][j]]
    seg.close()


# ---- end to end: loader-made table, Engine (table and per-segment paths) and imm3_sql ---------------------------------------------
def test_engine_and_cli_end_to_end(tmp_path):
    from immutable3_amd import Count, Max, Min, NoSelect, ProjectAgg, Query
    from immutable3_amd.operators import Engine, GpuSegmentManager
    from immutable3_amd.storage import SegmentManager
    rng = np.random.default_rng(91)
    n = 7_000
    st = STATES[rng.integers(0, 51, size=n)]
    names = rand_strings(rng, n, 16, b"abcXYZ")
    ages = rng.integers(0, 100, size=n)
    csv = tmp_path / "people.csv"
    with open(csv, "w") as f:
        f.write("id,state,name,age\n")
        for i in range(n):
            f.write(f"{i},{bytes(st[i]).decode()},{bytes(names[i]).decode()},{ages[i]}\n")
    # first-seen order of the states, their maxima and counts
    want, order = {}, []
    for i in range(n):
        k = bytes(st[i]).decode()
        if k not in want:
            want[k] = [b"", 0]
            order.append(k)
        want[k][0] = max(want[k][0], bytes(names[i]))
        want[k][1] += 1
    rows = [f"Row({want[k][0].decode()},{want[k][0].decode()},{want[k][1]})" for k in order]
    sql = "select max(name), min(name), count(id) from people group by state"
    for block in (1024, 1000):
        d = tmp_path / f"data{block}"
        d.mkdir()
        p = subprocess.run([os.path.join(BIN, "imm3_loader"), "-t", "people", "-c",
                            "id:DENSE_INT,state:DENSE_STRING:size=2,name:DENSE_STRING:size=16,age:DENSE_TINYINT",
                            "-d", str(d), "-i", str(csv), "--block-size", str(block), "--segment-size", "2"],
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        gsm = GpuSegmentManager(SegmentManager(str(d)))
        try:
            assert gsm.getTableSegmentCount("people") >= 3
            q = Query("people", NoSelect, ProjectAgg([Max("name"), Min("name"), Count("id")], ["state"]))
            got = [f"Row({','.join(a.repr() for a in m.values())})" for m in Engine(gsm).execute_agg(q).values()]
            assert got == rows, block
        finally:
            gsm.close()
        p = subprocess.run([os.path.join(BIN, "imm3_sql"), "-q", sql, "-d", str(d)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        assert p.stdout.splitlines() == rows, block
