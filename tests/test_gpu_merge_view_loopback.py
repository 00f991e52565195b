"""GPU suite: imm3_comm_merge_groups_view with TWO ranks over the loopback transport of test_gpu_comm_loopback.py -- the view's vote
(a hash of its canonical bytes), the all-reduce of the largest segment index that sizes the tie, the refusal on every rank in the same
call, and the view computed on every rank behind the exchange.  The segments of test_gpu_merge_view.py, segment s on rank s mod 2:
rank 1 alone brings the index above 255.  The reference is the two-rank merge_groups_wide through merge_view_util.reference_view."""
import pytest

from loopback_util import run_worker

pytestmark = pytest.mark.gpu

WORKER = r'''
import sys
import numpy as np
import torch  # noqa: F401  (its HIP runtime first: conftest.py says why)
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from immutable3_amd import native
from merge_view_util import AGG, AGGS_A, AND, CNT, EQ, G_K8KID, GCOL, GT, LT, NOT, OR, SEG_INDEX, SIZES, agg_query, assert_view, columns, reference_view

from loopback_ranks import WORLD, both, start

ctxs, comms = start()
rng = np.random.default_rng(2110)
owner = [s % WORLD for s in range(len(SIZES))]
segs = [native.DeviceSegment(ctxs[owner[s]], [c.native() for c in columns(rng, n)]) for s, n in enumerate(SIZES)]
queries, seg_idx = [[], []], [[], []]
for s in range(len(SIZES)):
    queries[owner[s]].append(agg_query(ctxs[owner[s]], segs[s], [], G_K8KID, AGGS_A))
    seg_idx[owner[s]].append(SEG_INDEX[s])
assert max(seg_idx[0]) <= 255 < max(seg_idx[1])                      # rank 1 alone makes the tie two segment bytes wide

out, err = both(lambda r: comms[r].merge_groups_wide(queries[r], seg_idx[r]))
assert err == [None, None], err
merged = out[0]
assert merged[1].size > 600

def view(order=(), leaves=(), prog=(), limit=0):
    return dict(order=list(order), leaves=list(leaves), prog=list(prog), limit=limit)

TEN = [(AGG, 0, 1), (AGG, 1, 0), (AGG, 2, 1)]                        # COUNT 5 + MIN 4 + MAX(int8) 1: with 2 + 4 bytes of tie, 16
VIEWS = [view(TEN), view([(GCOL, 0, 1), (AGG, 3, 0)], [(CNT, 0, GT, 2), (3, 1, LT, 0), (2, 0, EQ, 100)], [0, 1, OR, 2, NOT, AND], 25),
         view([(AGG, 2, 0)], [(3, 0, GT, 0)], [0]), view(limit=40), view()]
for v in VIEWS:
    want = reference_view(merged, G_K8KID, AGGS_A, **v)
    out, err = both(lambda r: comms[r].merge_groups_view(queries[r], seg_idx[r], **v))
    assert err == [None, None], (v, err)
    for r in range(WORLD):
        assert_view(out[r], want, (v, "rank", r))
        assert comms[r].merge_view_path() == (native.GROUP_ORDER_SMALL if merged[1].size <= native.GROUP_ORDER_SMALL_MAX else
                                              native.GROUP_ORDER_RADIX_SELECT if 0 < v["limit"] * 4 <= want[5] else native.GROUP_ORDER_RADIX_FULL)
print("views ok", len(VIEWS), flush=True)

# ---- 11 user bytes: rank 0's own largest index (7) would leave room, rank 1's (300) does not -- BOTH refuse, with the prefix, in the same call
ELEVEN = TEN + [(GCOL, 0, 0)]
out, err = both(lambda r: comms[r].merge_groups_view(queries[r], seg_idx[r], order=ELEVEN))
for e in err:
    assert isinstance(e, native.Imm3Error) and e.code == native.ERR_ARG and e.msg.startswith(native.MERGE_VIEW_REFUSED), err
# ---- the ranks bring views that differ in one flag: both are told so
flipped = [TEN, [TEN[0], (AGG, 1, 1), TEN[2]]]
out, err = both(lambda r: comms[r].merge_groups_view(queries[r], seg_idx[r], order=flipped[r]))
for e in err:
    assert isinstance(e, native.Imm3Error) and e.code == native.ERR_ARG and "views of the merged groups differ" in e.msg, err
# ---- a bad key on rank 1 alone travels with the vote
out, err = both(lambda r: comms[r].merge_groups_view(queries[r], seg_idx[r], order=[TEN, [(GCOL, 9, 0)]][r]))
assert isinstance(err[0], native.Imm3Error) and "another rank failed" in err[0].msg, err
assert isinstance(err[1], native.Imm3Error) and err[1].code == native.ERR_ARG and not err[1].msg.startswith(native.MERGE_VIEW_REFUSED), err
# ... and the next merge on the same communicators succeeds
out, err = both(lambda r: comms[r].merge_groups_view(queries[r], seg_idx[r], **VIEWS[0]))
assert err == [None, None], err
assert_view(out[1], reference_view(merged, G_K8KID, AGGS_A, **VIEWS[0]), "after the failures")
print("failure exits ok", flush=True)

for qs in queries:
    for q in qs:
        q.close()
for c in comms: c.close()
for s in segs: s.close()
for c in ctxs: c.close()
print("LOOPBACK-VIEW-OK", flush=True)
'''


def test_two_ranks_merge_views_over_the_loopback_transport(tmp_path):
    run_worker(tmp_path, "loopback_view_worker.py", WORKER, "LOOPBACK-VIEW-OK")
