"""GPU suite: imm3_comm_merge_ordered with TWO ranks -- the shape vote, the list-length all-reduce, ncclAllGather of the ranks' slots
and the rank kernel over them -- over the loopback transport of test_gpu_comm_loopback.py (tests/native/loopback_rccl.cpp: two
threads of one process as the ranks, IMM3_RCCL_LIB).  Six segments, segment s on rank s mod 2: interleaved global indices, so the
concatenation of the ranks' lists is not the order.  Every rank must receive order_util.expected_table's rows bit for bit, and every
rank must come back when one of them fails before the first collective."""
import pytest

from loopback_util import run_worker

pytestmark = pytest.mark.gpu

WORKER = r'''
import sys
import numpy as np
import torch  # noqa: F401  (its HIP runtime first: conftest.py says why)
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from conftest import GT
from immutable3_amd import native
import merge_order_util as U
from merge_order_util import AGE, ID, TAG

from loopback_ranks import WORLD, both, start

ctxs, comms = start()

# ---- six segments, segment s on rank s mod 2; ids below 3 and three ages: whole (age, id) keys tie inside and across segments
rng = np.random.default_rng(31)
SIZES = [130, 65, 64, 1, 200, 97]
N_SEG = len(SIZES)
owner = [s % WORLD for s in range(N_SEG)]
cols = [U.segment_columns(rng, n, 0, few_ids=3) for n in SIZES]
segs = [native.DeviceSegment(ctxs[owner[s]], [c.native() for c in cols[s]]) for s in range(N_SEG)]
table0 = native.DeviceTable(ctxs[0], [segs[s] for s in (0, 2, 4)])
USED, PROJ = [ID, AGE, TAG], [0, 1, 2]
ORDER = [(1, True), (0, False)]                                              # age desc, id
nothing = [(0, GT, 100.0)]                                                   # id < 3: no row selected

def make(sels_of_rank, order_by, limit, rank0_table=False):
    queries, seg_idx = [[], []], [[], []]
    for s in range(N_SEG):
        if rank0_table and owner[s] == 0:
            continue
        queries[owner[s]].append(U.ordered_query(native, ctxs[owner[s]], segs[s], USED, sels_of_rank[owner[s]], PROJ, order_by, limit))
        seg_idx[owner[s]].append(s)
    if rank0_table:
        queries[0].append(U.ordered_query(native, ctxs[0], table0, USED, sels_of_rank[0], PROJ, order_by, limit))
        seg_idx[0].append([0, 2, 4])
    return queries, seg_idx

def want_of(sels_of_rank, order_by, limit):
    if sels_of_rank[0] == sels_of_rank[1]:
        return U.expected(dict(enumerate(cols)), USED, sels_of_rank[0], PROJ, order_by, limit)
    assert sels_of_rank[1] == nothing                                        # rank 1 contributes nothing: the even segments alone
    return U.expected({s: cols[s] for s in range(N_SEG) if owner[s] == 0}, USED, sels_of_rank[0], PROJ, order_by, limit)

top = [int(((c[AGE].values == U.AGES.max()) & (c[ID].values == 0)).sum()) for c in cols]   # the first tie group, per segment
assert all(t > 2 for t in (top[0], top[1], top[2]))
K = top[0] + top[1] + 2                                                      # cuts that group inside segment 2: it spans both ranks
CASES = [("limit inside a tie group", [[], []], K, False), ("unlimited", [[], []], 0, False), ("rank 1 selects nothing", [[], nothing], K, False),
         ("nobody selects anything", [nothing, nothing], 0, False), ("rank 0 brings a table query", [[], []], K, True),
         ("rank 0 brings a table query, unlimited", [[], []], 0, True)]
for what, sels_of_rank, limit, rank0_table in CASES:
    queries, seg_idx = make(sels_of_rank, ORDER, limit, rank0_table)
    want = want_of(sels_of_rank, ORDER, limit)
    lens = [sum(q.row_count() for q in queries[r]) for r in range(WORLD)]
    out, err = both(lambda r: comms[r].merge_ordered(queries[r], seg_idx[r], limit))
    assert err == [None, None], (what, err)
    for r in range(WORLD):
        U.assert_rows(out[r], want, (what, "rank", r))
    if what == "limit inside a tie group":
        last = want[0].size - 1
        assert want[0].size == K and want[0][last] == 2 and set(want[0].tolist()) == {0, 1, 2}, want[0]
    if what == "unlimited":
        assert lens[0] != lens[1] and want[0].size == sum(SIZES), lens      # the ranks' lists differ in length
        assert (np.diff(want[0]) < 0).any()                                  # interleaved segments: not a concatenation of the ranks' lists
    print("merge ok:", what, "list lengths", lens, "rows", want[0].size, flush=True)
    if what == "unlimited":
        # ---- rank 1 brings a query that has not been run: both ranks come back with an error, none is left in a collective
        unrun = U.ordered_query(native, ctxs[1], segs[1], USED, [], PROJ, ORDER, 0, run=False)
        bad = [queries[0], [queries[1][0], unrun]]
        out, err = both(lambda r: comms[r].merge_ordered(bad[r], [seg_idx[0], [1, 3]][r], 0))
        assert isinstance(err[0], native.Imm3Error) and isinstance(err[1], native.Imm3Error), (out, err)
        assert "another rank failed" in str(err[0]) and err[1].code == native.ERR_STATE, err
        unrun.close()
        # ---- the ranks' keys differ (rank 1 orders by age alone): every rank sees it in the vote and leaves
        other = U.ordered_query(native, ctxs[1], segs[1], USED, [], PROJ, [(1, True)], 0)
        out, err = both(lambda r: comms[r].merge_ordered([queries[0], [other]][r], [seg_idx[0], [1]][r], 0))
        assert all(isinstance(e, native.Imm3Error) and e.code == native.ERR_ARG and "differ" in str(e) for e in err), err
        other.close()
        # ... and the communicators still work afterwards
        out, err = both(lambda r: comms[r].merge_ordered(queries[r], seg_idx[r], 0))
        assert err == [None, None], err
        U.assert_rows(out[0], want, "after the failures")
        U.assert_rows(out[1], want, "after the failures, rank 1")
        print("failure exits ok", flush=True)
    for qs in queries:
        for q in qs:
            q.close()
table0.close()
for c in comms: c.close()
for s in segs: s.close()
for c in ctxs: c.close()
print("LOOPBACK-ORDERED-OK", flush=True)
'''


def test_two_ranks_merge_ordered_over_the_loopback_transport(tmp_path):
    run_worker(tmp_path, "loopback_ordered_worker.py", WORKER, "LOOPBACK-ORDERED-OK")
