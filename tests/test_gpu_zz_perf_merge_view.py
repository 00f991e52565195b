"""GPU suite, with the other assertions on a TIME (`zz`): a view of merged groups.

Two segment queries of 2^19 distinct int32 groups each (1 M merged groups), `order by age_max desc limit 10`, with and without `having
id_count > 0`.  The wall time of ONE merge_groups_view call must not exceed the wall time of what a caller did before on the same
queries: one merge_groups_wide(..., max_groups=total) call plus the numpy filter and np.lexsort.  No margin: both sides run the same
merge and differ by what crosses PCIe and who sorts -- if the view is not faster it has not paid.  Each side twice, the better run
kept; the results must be equal."""
import time

import numpy as np
import pytest

from immutable3_amd import native, synth

pytestmark = pytest.mark.gpu
C, MX = native.AGG_COUNT, native.AGG_MAX
A = native.GROUP_ORDER_AGG
HALF = 1 << 19


@pytest.fixture(scope="module")
def million():
    rng = np.random.default_rng(10)
    ctx = native.Context(0)
    comm = native.Comm(ctx, 1, 0, native.comm_unique_id())
    ids = rng.permutation(2 * HALF).astype(np.int32)
    age = rng.integers(-128, 128, size=2 * HALF).astype(np.int8)
    segs, queries = [], []
    for s in range(2):
        i, a = np.ascontiguousarray(ids[s * HALF:(s + 1) * HALF]), np.ascontiguousarray(age[s * HALF:(s + 1) * HALF])
        segs.append(native.DeviceSegment(ctx, [(native.DENSE_INT, 4, i.view(np.uint8), HALF * 4, synth.block_offsets(HALF, 4)),
                                               (native.DENSE_TINYINT, 1, a.view(np.uint8), HALF, synth.block_offsets(HALF, 1))]))
        q = native.DeviceQuery(ctx, segs[-1], [0, 1], [], (), 0, 1024, group_cols=[0], aggs=[(MX, 1), (C, 0)])
        q.run()
        assert q.fetch_groups()[1].size == HALF
        queries.append(q)
    yield ctx, comm, queries, ids, age
    for q in queries:
        q.close()
    for s in segs:
        s.close()
    comm.close()
    ctx.close()


@pytest.mark.parametrize("having", [False, True], ids=["unfiltered", "having id_count > 0"])
def test_top_10_of_a_million_merged_groups_beats_merge_everything_and_lexsort(million, having):
    ctx, comm, queries, ids, age = million
    seg_index, total = [0, 1], 2 * HALF
    leaves, prog = ([(native.GROUP_FILTER_COUNT, 0, native.GT, 0)], [0]) if having else ([], [])
    t = {"view": [], "merge all + lexsort": []}
    comm.merge_groups_view(queries, seg_index, order=[(A, 0, True)], leaves=leaves, prog=prog, limit=10)      # (both sides warm: allocator, kernels)
    comm.merge_groups_wide(queries, seg_index, max_groups=total)
    for _ in range(2):
        ctx.sync()
        t0 = time.perf_counter()
        keys, first, counts, vals, _, n = comm.merge_groups_wide(queries, seg_index, max_groups=total)
        kept = np.flatnonzero(counts > 0) if having else np.arange(n)
        top = kept[np.lexsort((first[kept], -vals[kept, 0]))[:10]]
        old = (keys[top].tolist(), first[top].tolist(), counts[top].tolist(), vals[top].tolist(), int(kept.size))
        t["merge all + lexsort"].append(time.perf_counter() - t0)
        ctx.sync()
        t0 = time.perf_counter()
        got = comm.merge_groups_view(queries, seg_index, order=[(A, 0, True)], leaves=leaves, prog=prog, limit=10)
        new = (got[0].tolist(), got[1].tolist(), got[2].tolist(), got[3].tolist(), got[5])
        t["view"].append(time.perf_counter() - t0)
        assert comm.merge_view_path() == native.GROUP_ORDER_RADIX_SELECT
        assert new == old
    pos = np.lexsort((np.arange(total), -age.astype(np.int64)))[:10]                                               # first = segment << 32 | row: the position in `ids`
    assert [((f >> 32) * HALF + (f & 0xFFFFFFFF)) for f in new[1]] == pos.tolist() and new[4] == total
    assert [int.from_bytes(bytes(k), "little", signed=True) for k in new[0]] == ids[pos].tolist()
    new_ms, old_ms = min(t["view"]) * 1e3, min(t["merge all + lexsort"]) * 1e3
    print(f"top-10 of {total} merged groups by age_max{' having id_count > 0' if having else ''}: view on the device {new_ms:.2f} ms, "
          f"merge_groups_wide of every group + numpy {old_ms:.2f} ms (ratio {new_ms / old_ms:.3f})")
    assert new_ms <= old_ms, t
