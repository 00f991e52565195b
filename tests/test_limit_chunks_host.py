"""Host test (no GPU): the chunks of a limit scan as the library schedules them -- a pure function (csrc/imm3_planner.cpp::
limit_chunk_ends, exported as imm3_plan_limit_chunks next to imm3_plan_limit_scan).  A schedule that skipped or repeated a tile would
show only in runs whose limit is met late; here it is walked directly: the ends are 1024, 8192, 32 768, ... (x 4) while they are below
the segment's tiles, then the segment's end."""
import pytest

from immutable3_amd import native

K_CHUNK_TILES = 256                                                     # csrc/imm3_internal.h: kChunkTiles, the offsets scan's unit
SIZES = [1, 1024, 1025, 8191, 8192, 8193, 32_768, 32_769, 97_657, 2 ** 40]


def inner_ends(limit):
    out, e = [], 1024
    while e < limit:
        out.append(e)
        e = 8192 if e == 1024 else e * 4
    return out


@pytest.mark.parametrize("n_tiles", SIZES)
def test_ends_ascend_to_the_segments_end_on_the_schedule(n_tiles):
    ends = native.plan_limit_chunks(n_tiles)
    assert 1 <= len(ends) <= 32
    assert all(a < b for a, b in zip(ends, ends[1:])), ends             # strictly ascending: no tile twice, none skipped
    assert ends[-1] == n_tiles
    assert set(ends[:-1]) <= set(inner_ends(2 ** 62)), ends             # every end but the last: 1024, 8192, 32 768, 131 072, ...
    assert ends[:-1] == inner_ends(n_tiles), ends                      # ... all of them below n_tiles
    assert all(e % K_CHUNK_TILES == 0 for e in ends[:-1]) and (ends[-1] % K_CHUNK_TILES == 0 or ends[-1] == n_tiles)


def test_known_schedules():
    assert native.plan_limit_chunks(97_657) == [1024, 8192, 32_768, 97_657]   # 100 M rows: four launches
    assert native.plan_limit_chunks(1025) == [1024, 1025]
    assert native.plan_limit_chunks(1024) == [1024] and native.plan_limit_chunks(1) == [1]
    assert native.plan_limit_chunks(8193) == [1024, 8192, 8193]
    assert native.plan_limit_chunks(0) == []
    assert len(native.plan_limit_chunks(2 ** 63 - 1)) <= 32              # any int64_t fits the fixed array
