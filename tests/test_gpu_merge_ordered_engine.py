"""GPU suite: Engine(gsm, device_merge=True) on an ORDER BY statement that runs as per-segment ordered queries -- the merge is then
one imm3_comm_merge_ordered on the device instead of operators.merge_ordered's lexsort on the host.  Both must give exactly the rows
of tests/order_util.expected_table (the unchanged oracle's projection, lexsort with (segment, row) last).

The statement holds a Match on a 3-byte string column, which a table query refuses: the Engine falls to per-segment queries."""
import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, LT, MATCH, RawColumn, blocks_of
import order_util

pytestmark = pytest.mark.gpu
ROWS = (1025, 64, 700)
CODES = ["aab", "abc", "cab", "bbb"]


@pytest.fixture(scope="module")
def stored(tmp_path_factory):
    """id int32, code 3 bytes over 'a' .. 'c', age int8 with four values (ties across the segments), name 8 bytes from a small pool"""
    from immutable3_amd.schema import CodecType, Column, Table, TableIO
    from immutable3_amd.storage import write_segment_arrays
    d = str(tmp_path_factory.mktemp("merge_ordered"))
    t = Table("mo", [Column.make("id", CodecType.DENSE_INT), Column.make("code", CodecType.DENSE_STRING, {"size": "3"}),
                     Column.make("age", CodecType.DENSE_TINYINT), Column.make("name", CodecType.DENSE_STRING, {"size": "8"})], 1024)
    TableIO.store(d, t)
    rng = np.random.default_rng(4242)
    pool = np.frombuffer(b"".join(n.ljust(8, b"0") for n in (b"Jo", b"Joanna", b"Mary", b"Zed")), dtype=np.uint8).reshape(-1, 8)
    segs = []
    for s, n in enumerate(ROWS):
        cols = {"id": rng.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64).astype(np.int32),
                "code": rng.integers(97, 100, size=(n, 3)).astype(np.uint8),
                "age": rng.integers(-2, 2, size=n).astype(np.int8),
                "name": pool[rng.integers(0, 4, size=n)].copy()}
        write_segment_arrays(d, t, s, cols)
        br = blocks_of(n, 1024)
        segs.append([RawColumn(DENSE_STRING, 3, cols["code"], br), RawColumn(DENSE_INT, 4, cols["id"], br), RawColumn(DENSE_TINYINT, 1, cols["age"], br),
                     RawColumn(DENSE_STRING, 8, cols["name"], br)])
    return d, segs


SELECT = ["id", "age", "name"]                                  # used columns of the expectation: code, id, age, name -> proj 1, 2, 3


@pytest.mark.parametrize("order_by", [[("age", False)], [("age", True)], [("name", True), ("age", False)], [("id", True)]])
@pytest.mark.parametrize("limit", [0, 9])
def test_device_merge_gives_the_host_merge_rows(stored, order_by, limit):
    from immutable3_amd import And, Match, Project, Query, Row, Select
    from immutable3_amd import LT as QLT
    from immutable3_amd.operators import Engine, GpuSegmentManager
    from immutable3_amd.storage import SegmentManager
    d, segs = stored
    sels = [(0, MATCH, [c.encode() for c in CODES]), (2, LT, 1.0)]
    keys = [(SELECT.index(c), desc) for c, desc in order_by]
    _, _, vals = order_util.expected_table([[c.npcol() for c in cols] for cols in segs], [DENSE_STRING, DENSE_INT, DENSE_TINYINT, DENSE_STRING], sels, [1, 2, 3], keys, limit)
    want = [Row(int(i), int(a), bytes(n).decode()) for i, a, n in zip(vals[0].view("<i4").reshape(-1), vals[1].view(np.int8).reshape(-1), vals[2])]
    assert len(want) == limit or (limit == 0 and 9 < len(want) < sum(ROWS))
    q = Query("mo", And(Select("code", Match(CODES)), Select("age", QLT(1))), Project(SELECT, limit, order_by))
    gsm = GpuSegmentManager(SegmentManager(d))
    try:
        assert Engine(gsm)._table_plan(q) is None               # a 3-byte Match: no one-table query
        host = list(Engine(gsm).execute(q))
        device = list(Engine(gsm, device_merge=True).execute(q))
        assert device == host == want
    finally:
        gsm.close()
