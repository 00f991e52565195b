"""GPU suite: IMM3_STR_RANGE over an imm3_table -- ONE k_filter_str_range launch over the tile table of three segments (1025, 1024
and 1 rows) gives the per-segment results in segment order and tests/str_range_util.py's reference; what a table refuses carries
the new messages; one graph capture and replay."""
import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_STRING, GT, RawColumn
from immutable3_amd import native
import str_range_util as U

pytestmark = pytest.mark.gpu
STR_RANGE = native.STR_RANGE
SHAPE = [(1025, [1024, 1]), (1024, [1024]), (1, [1])]
LO16, HI16 = b"Jo", b"M\x80"
LO32 = b"prefix-of-16-byt" + b"es\x7f"
HI32 = b"prefix-of-16-byt" + b"es\x80\x01"


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def table(ctx):
    """id int32, name 16 bytes, note 32 bytes (rows that tie with the bounds' first 16 bytes), tag 3 bytes; the rows at both ends of
    every segment are inside the ranges, so the survivors straddle the segment boundaries"""
    rng = np.random.default_rng(77)
    segs_cols = []
    for (n, br) in SHAPE:
        ids = rng.integers(-50, 50, size=n).astype(np.int32)
        name = rng.integers(0x40, 0x60, size=(n, 16)).astype(np.uint8)
        note = rng.integers(0, 256, size=(n, 32)).astype(np.uint8)
        note[::3, :16] = np.frombuffer(LO32[:16], dtype=np.uint8)
        note[::3, 16:19] = rng.integers(0x60, 0x90, size=(len(range(0, n, 3)), 3)).astype(np.uint8)
        for r in {0, n - 1}:
            name[r] = np.frombuffer(U.pad(b"K", b"K", 16)[0 if r == 0 else 1], dtype=np.uint8)
            note[r] = np.frombuffer(U.pad(LO32, LO32, 32)[0], dtype=np.uint8)
        tag = rng.integers(97, 100, size=(n, 3)).astype(np.uint8)
        segs_cols.append([RawColumn(DENSE_INT, 4, ids, br), RawColumn(DENSE_STRING, 16, name, br), RawColumn(DENSE_STRING, 32, note, br),
                          RawColumn(DENSE_STRING, 3, tag, br)])
    dsegs = [native.DeviceSegment(ctx, [c.native() for c in cols]) for cols in segs_cols]
    t = native.DeviceTable(ctx, dsegs)
    yield segs_cols, dsegs, t
    t.close()
    for d in dsegs:
        d.close()


def reference(segs_cols, used, sels):
    """per segment: the row mask of a conjunction of STR_RANGE / GT leaves over `used`"""
    masks = []
    for cols in segs_cols:
        m = np.ones(cols[0].values.shape[0], dtype=bool)
        for (c, cond, operand) in sels:
            v = cols[used[c]].values
            m &= U.in_range(v, *operand) if cond == STR_RANGE else (v > operand)
        masks.append(m)
    return masks


def check_select(q, masks):
    words, count = q.bitmap(), q.count()
    fb, fw = q.segment_starts()
    for si, (m, (n, br)) in enumerate(zip(masks, SHAPE)):
        ow = U.bitmap_words(m, br)
        assert words[int(fw[si]): int(fw[si]) + ow.size].tolist() == ow.tolist(), si
        assert not words[int(fw[si]) + ow.size: int(fw[si + 1])].any(), si          # padding up to the next tile
    assert count == sum(int(m.sum()) for m in masks)


QUERIES = [
    ([1], [(0, STR_RANGE, (LO16, HI16))]),
    ([2], [(0, STR_RANGE, (LO32, HI32))]),
    ([2], [(0, STR_RANGE, (LO32[:16], LO32[:16]))]),
    ([1, 0, 2], [(0, STR_RANGE, (LO16, HI16)), (1, GT, -20), (2, STR_RANGE, (LO32[:5], b""))]),
    ([0, 1], [(0, GT, 0), (1, STR_RANGE, (b"K", b"K")), (1, STR_RANGE, (b"", b"KZ"))]),
]


@pytest.mark.parametrize("used,sels", QUERIES)
def test_table_equals_per_segment_and_reference(ctx, table, used, sels):
    segs_cols, dsegs, t = table
    masks = reference(segs_cols, used, sels)
    if len(sels) == 1:
        assert all(m[0] and m[-1] for m in masks)             # survivors on both sides of every segment boundary
    q = native.DeviceQuery(ctx, t, used, sels)
    q.run_select()
    check_select(q, masks)
    words, (fb, fw) = q.bitmap(), q.segment_starts()
    q.close()
    total = 0
    for si, d in enumerate(dsegs):                             # the per-segment queries, concatenated
        qs = native.DeviceQuery(ctx, d, used, sels)
        qs.run_select()
        w, c = qs.bitmap(), qs.count()
        qs.close()
        assert words[int(fw[si]): int(fw[si]) + w.size].tolist() == w.tolist() and c == int(masks[si].sum())
        total += c
    assert total == sum(int(m.sum()) for m in masks)
    # the projection behind it: rows in (segment, row) order, a limit across the first boundary
    keep = [(si, int(r)) for si, m in enumerate(masks) for r in np.flatnonzero(m)]
    first = int(masks[0].sum())
    for limit in (0, first + 1):
        q = native.DeviceQuery(ctx, t, used, sels, [0], limit, 1024)
        q.run()
        idx, vals = q.fetch_rows()
        seg_of, row_of = q.locate_rows(idx)
        q.close()
        want = keep[:limit] if limit else keep
        assert list(zip(seg_of.tolist(), row_of.tolist())) == want
        col = used[0]
        assert vals[0].tobytes() == b"".join(np.ascontiguousarray(segs_cols[si][col].values[r]).tobytes() for si, r in want)


def test_refusals_carry_their_own_messages(ctx, table):
    segs_cols, dsegs, t = table
    with pytest.raises(native.Imm3Error) as e:                 # a 3-byte column: a table has no word-at-a-time kernel
        native.DeviceQuery(ctx, t, [3], [(0, STR_RANGE, (b"a", b"b"))])
    assert e.value.code == native.ERR_ARG and "IMM3_STR_RANGE" in e.value.msg and "multiple of 4" in e.value.msg and "per-segment queries" in e.value.msg
    assert "still refused" not in e.value.msg                  # (not kTableGenericRefusal, which stays Match's)
    q = native.DeviceQuery(ctx, dsegs[0], [3], [(0, STR_RANGE, (b"a", b"b"))])   # ... and a segment takes it
    q.run_select()
    assert q.count() == int(U.in_range(segs_cols[0][3].values, b"a", b"b").sum())
    q.close()
    q = native.DeviceQuery(ctx, t, [3], [(0, STR_RANGE, (b"", b""))])            # every row: no predicate is left to refuse
    q.run_select()
    assert q.count() == sum(n for n, _ in SHAPE)
    q.close()
    for prog in ([0, 1, native.EXPR_OR], [0, native.EXPR_NOT, 1, native.EXPR_AND]):
        with pytest.raises(native.Imm3Error) as e:
            native.DeviceQuery(ctx, t, [1, 0], [(0, STR_RANGE, (LO16, HI16)), (1, GT, 3.0)], expr=prog)
        assert e.value.code == native.ERR_ARG and "IMM3_STR_RANGE" in e.value.msg and not e.value.msg.startswith(native.TABLE_TREE_REFUSED)
    masks = reference(segs_cols, [1, 0], [(0, STR_RANGE, (LO16, HI16)), (1, GT, 3)])
    q = native.DeviceQuery(ctx, t, [1, 0], [(0, STR_RANGE, (LO16, HI16)), (1, GT, 3.0)], expr=[0, 1, native.EXPR_AND])   # AND alone: the flat list
    q.run_select()
    check_select(q, masks)
    q.close()


def test_record_and_replay(ctx, table):
    segs_cols, dsegs, t = table
    used, sels = [2, 0], [(0, STR_RANGE, (LO32, HI32))]
    masks = reference(segs_cols, used, sels)
    keep = [(si, int(r)) for si, m in enumerate(masks) for r in np.flatnonzero(m)]
    assert keep
    q = native.DeviceQuery(ctx, t, used, sels, [1, 0], 0, 1024)
    q.run()
    q.fetch_rows()
    with ctx.capture() as cap:
        q.run()
    for _ in range(2):
        cap.graph.launch()
        check_select(q, masks)
        idx, vals = q.fetch_rows()
        seg_of, row_of = q.locate_rows(idx)
        assert list(zip(seg_of.tolist(), row_of.tolist())) == keep
        assert vals[0].view("<i4").reshape(-1).tolist() == [int(segs_cols[si][0].values[r]) for si, r in keep]
    cap.graph.close()
    q.close()
