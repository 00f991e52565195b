"""Shared by the imm3_comm_merge_ordered tests: small segments with heavy ties, the ordered per-segment queries over them, and the
expectation (tests/order_util.expected_table: the unchanged oracle's projection plus numpy.lexsort with (segment, row) last)."""
import numpy as np

from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, GT, LT, RawColumn, blocks_of
import order_util

ID, AGE, NAME, TAG = range(4)
CODECS = [DENSE_INT, DENSE_TINYINT, DENSE_STRING, DENSE_STRING]
WIDTHS = [4, 1, 12, 5]
AGES = np.array([-5, 0, 7], np.int8)
NAMES = [b"alpha\x00\x00\x00\x00\x00\x00\x00", b"alphabet\x00\x00\x00\x00", b"\x80mega\xff\x00\x00\x00\x00\x00\x00", b"beta\x00\x00\x00\x00\x00\x00\x00\x01", b"zz\xfe\x7f\x80\x00\x00\x00\x00\x00\x00\x00"]


def id_of(v):
    """ids grow with v and use every byte of an int32: v = 0 .. 6700 spans the whole signed range"""
    v = np.asarray(v, dtype=np.int64)
    return (v * 640_000 + (v % 256) - 2 ** 31).astype(np.int64)


def between(lo, hi):
    """the select `id_of(lo) < id < id_of(hi)` over used column 0 (the id); lo None: no lower bound"""
    return ([] if lo is None else [(0, GT, float(id_of(lo)))]) + [(0, LT, float(id_of(hi)))]


def segment_columns(rng, n, first_v, few_ids=0):
    """One segment of n rows whose ids are id_of(first_v .. first_v + n) in random row order -- or, with few_ids, random values below
    few_ids: whole (age, id) keys then tie inside and across segments."""
    ids = rng.integers(0, few_ids, size=n).astype(np.int32) if few_ids else id_of(first_v + rng.permutation(n)).astype(np.int32)
    age = AGES[rng.integers(0, len(AGES), size=n)]
    name = np.array([list(NAMES[i]) for i in rng.integers(0, len(NAMES), size=n)], dtype=np.uint8).reshape(n, 12)
    tag = rng.integers(0, 256, size=(n, 5)).astype(np.uint8)
    br = blocks_of(n, 1024)
    return [RawColumn(DENSE_INT, 4, ids, br), RawColumn(DENSE_TINYINT, 1, age, br), RawColumn(DENSE_STRING, 12, name, br), RawColumn(DENSE_STRING, 5, tag, br)]


def ordered_query(native, ctx, target, used, sels, proj, order_by, limit=0, run=True):
    q = native.DeviceQuery(ctx, target, used, sels, proj, 0, 1024)
    q.set_order(order_by, limit)
    if run:
        q.run()
    return q


def expected(cols_by_global, used, sels, proj, order_by, limit=0):
    """cols_by_global: {global segment index: its RawColumns}.  (segment, row, [uint8[n, width]]) with the GLOBAL segment indices."""
    order = sorted(cols_by_global)
    seg, row, vals = order_util.expected_table([[cols_by_global[g][u].npcol() for u in used] for g in order], [CODECS[u] for u in used], sels, proj, order_by, limit)
    return np.asarray(order, np.int64)[seg] if seg.size else seg, row, vals


def assert_rows(got, want, what=""):
    seg, row, cols = got[:3]
    wseg, wrow, wvals = want
    assert seg.astype(np.int64).tolist() == wseg.tolist(), ("segment", what)
    assert row.astype(np.int64).tolist() == wrow.tolist(), ("row", what)
    assert len(cols) == len(wvals)
    for j, (g, w) in enumerate(zip(cols, wvals)):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), ("column", j, what)
