"""GPU suite: imm3_comm_merge_groups_wide with TWO ranks -- the shape vote that now carries the key width and the string widths, the
list-length all-reduce, ncclAllGather of the ranks' records and the second table -- over the loopback transport of
test_gpu_comm_loopback.py (tests/native/loopback_rccl.cpp: two threads of one process as the ranks, IMM3_RCCL_LIB).  Every rank must
receive the table the host combine gives, and every rank must come back when one of them fails before the first collective."""
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
from merge_wide_util import AGGS, GROUP, SIZES, assert_merged, breaker_columns, host_combine

from loopback_ranks import WORLD, both, start

ctxs, comms = start()

# ---- four segments, segment s on rank s mod 2; key = 16-byte name + int8, MAX over a 16-byte string among the aggregates
rng = np.random.default_rng(20)
N_SEG = len(SIZES)
owner = [s % WORLD for s in range(N_SEG)]
segs = [native.DeviceSegment(ctxs[owner[s]], [c.native() for c in breaker_columns(rng, s)]) for s in range(N_SEG)]

def make(sels_of_rank):
    queries, seg_idx = [[], []], [[], []]
    for s in range(N_SEG):
        q = native.DeviceQuery(ctxs[owner[s]], segs[s], [0, 1, 2, 3], sels_of_rank[owner[s]], (), 0, 1024, group_cols=GROUP, aggs=AGGS, wide_keys=True)
        q.run()
        queries[owner[s]].append(q)
        seg_idx[owner[s]].append(s)
    return queries, seg_idx

nothing = [(2, GT, 2.0e6)]                                                   # val < 10^6: no row selected
for what, sels_of_rank in (("all rows", [[], []]), ("rank 1 selects nothing", [[], nothing]), ("nobody selects anything", [nothing, nothing])):
    queries, seg_idx = make(sels_of_rank)
    want = host_combine(queries[0] + queries[1], seg_idx[0] + seg_idx[1])
    lens = [host_combine(queries[r], seg_idx[r])[0].shape[0] for r in range(WORLD)]
    out, err = both(lambda r: comms[r].merge_groups_wide(queries[r], seg_idx[r]))
    assert err == [None, None], err
    for r in range(WORLD):
        assert_merged(out[r], want, (what, "rank", r))
    if what == "all rows":
        assert lens[0] != lens[1] and want[0].shape == (10, 17), (lens, want[0].shape)     # the ranks' lists differ in length
    print("merge ok:", what, "list lengths", lens, "groups", want[0].shape[0], flush=True)
    if what == "all rows":
        # ---- rank 1 brings a query that has not been run: both ranks come back with an error, none is left in a collective
        unrun = native.DeviceQuery(ctxs[1], segs[1], [0, 1, 2, 3], [], (), 0, 1024, group_cols=GROUP, aggs=AGGS, wide_keys=True)
        bad = [queries[0], [queries[1][0], unrun]]
        out, err = both(lambda r: comms[r].merge_groups_wide(bad[r], seg_idx[r]))
        assert isinstance(err[0], native.Imm3Error) and isinstance(err[1], native.Imm3Error), (out, err)
        assert "another rank failed" in str(err[0]) and err[1].code == native.ERR_STATE, err
        unrun.close()
        # ---- the ranks disagree on the key width (rank 1 groups by the name only: 16 bytes against 17): every rank sees it in the
        # vote and leaves
        narrow = native.DeviceQuery(ctxs[1], segs[1], [0, 1, 2, 3], [], (), 0, 1024, group_cols=[0], aggs=AGGS, wide_keys=True)
        narrow.run()
        out, err = both(lambda r: comms[r].merge_groups_wide([queries[0], [narrow]][r], [seg_idx[0], [1]][r]))
        assert all(isinstance(e, native.Imm3Error) and e.code == native.ERR_ARG and "differ" in str(e) for e in err), err
        narrow.close()
        # ... and the communicator still works afterwards
        out, err = both(lambda r: comms[r].merge_groups_wide(queries[r], seg_idx[r]))
        assert err == [None, None], err
        assert_merged(out[0], want, "after the failures")
        print("failure exits ok", flush=True)
    for qs in queries:
        for q in qs:
            q.close()
for c in comms: c.close()
for s in segs: s.close()
for c in ctxs: c.close()
print("LOOPBACK-WIDE-OK", flush=True)
'''


def test_two_ranks_merge_wide_over_the_loopback_transport(tmp_path):
    run_worker(tmp_path, "loopback_wide_worker.py", WORKER, "LOOPBACK-WIDE-OK")
