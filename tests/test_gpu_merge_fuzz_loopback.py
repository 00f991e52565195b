"""GPU suite: the group merges with TWO ranks over fuzzed deals -- imm3_comm_merge_groups (the direct table's all-reduces, the hash
list's all-gather and second table) and imm3_comm_merge_groups_wide (the records' all-gather and second table) -- over the loopback
transport of test_gpu_comm_loopback.py (tests/native/loopback_rccl.cpp: two threads of one process as the ranks, IMM3_RCCL_LIB).  One
worker walks merge_fuzz_util.LOOPBACK_CASES, dealt by their drawn owners (a rank may bring only queries without groups), and the
all-ones key with its rows on one rank only and on both; every rank must receive the table plain numpy gives (merge_fuzz_util.py), in
the same order.  test_merge_fuzz_host.py asserts on the CPU that the cases walked are not hollow."""
import pytest

from loopback_util import run_worker

pytestmark = pytest.mark.gpu

WORKER = r'''
import sys
import numpy as np
import torch  # noqa: F401  (its HIP runtime first: conftest.py says why)
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from immutable3_amd import native
from oracle import oracle_c
import merge_fuzz_util as F
from merge_wide_util import assert_merged

from loopback_ranks import WORLD, both, start

oracle_c.build()
ctxs, comms = start()
KIND = {"count": native.AGG_COUNT, "min": native.AGG_MIN, "max": native.AGG_MAX, "sum": native.AGG_SUM}


def merge_on_both(t, aq, brought, want, what):
    """brought: [(segment, global index, owner, predicates)], in hand-over order"""
    segs, qs, idx = {}, [[], []], [[], []]
    for si, index, owner, sels in brought:
        if (owner, si) not in segs:
            segs[(owner, si)] = native.DeviceSegment(ctxs[owner], [c.native() for c in t.segs[si]])
        q = native.DeviceQuery(ctxs[owner], segs[(owner, si)], aq.used, sels, (), 0, 1024, group_cols=aq.group, aggs=[(KIND[k], c) for k, c in aq.aggs],
                               wide_keys=aq.wide_keys)
        q.run()
        qs[owner].append(q)
        idx[owner].append(index)
    assert qs[0] and qs[1], what
    out, err = both(lambda r: comms[r].merge_groups_wide(qs[r], idx[r]))
    assert err == [None, None], (what, err)
    for r in range(WORLD):
        assert_merged(out[r], want, (what, "wide, rank", r))
    narrow = F.narrow_accepts(t, aq)
    if narrow:
        out, err = both(lambda r: comms[r].merge_groups(qs[r], idx[r]))
        assert err == [None, None], (what, err)
        for r in range(WORLD):
            F.assert_narrow(out[r], want, (what, "narrow, rank", r))
    for r in range(WORLD):
        for q in qs[r]:
            q.close()
    for s in segs.values():
        s.close()
    return narrow


# ---- the fuzzed cases
for seed in sorted({s for s, _, _ in F.LOOPBACK_CASES}):
    for ti, (t, cases) in enumerate(F.merge_cases(seed)):
        for ci, case in enumerate(cases):
            if (seed, ti, ci) not in F.LOOPBACK_CASES:
                continue
            ref = F.reference(oracle_c, t, case)
            brought = [(case.entries[i].seg, case.entries[i].index, case.entries[i].owner, case.sels(case.entries[i])) for i in case.passed]
            what = (seed, ti, ci, t.describe(), case.describe())
            narrow = merge_on_both(t, case.aq, brought, ref.arrays, what)
            print("merge ok:", (seed, ti, ci), "key bytes", F.key_width(t, case.aq), "narrow too" if narrow else "wide only", "list lengths",
                  [len(x) for x in ref.local], "groups", len(ref.merged), flush=True)

# ---- the all-ones key: segments 0, 1 and 3 hold it
t = F.OnesTable(np.random.default_rng(7))
cases = F.ones_queries()
for owners in ([0, 0, 1, 0], [0, 1, 0, 1], [1, 0, 1, 1]):
    for index in ([0, 1, 2, 3], [3, 0, 2, 1]):
        for what, aq in (cases[0], cases[3], cases[5], cases[10]):
            keep = F.ones_keep(t, aq.sels)
            per = [F.segment_groups(t, aq, keep, si) for si in range(4)]
            want = F.as_arrays(t, aq, F.combine(aq, list(zip(index, per))))
            on = sorted({owners[si] for si in range(4) if any(g[0] == b"\xff" * 8 for g in per[si])})
            assert on == ([] if what[0] == "the all-ones key removed" else [0] if owners == [0, 0, 1, 0] else [0, 1]), (what, owners, on)
            assert merge_on_both(t, aq, [(si, index[si], owners[si], aq.sels) for si in (2, 0, 3, 1)], want, (what, owners, index))
    print("all-ones ok: owners", owners, flush=True)

for c in comms: c.close()
for c in ctxs: c.close()
print("LOOPBACK-MERGE-FUZZ-OK", flush=True)
'''


def test_two_ranks_merge_fuzzed_deals_over_the_loopback_transport(tmp_path):
    run_worker(tmp_path, "loopback_merge_fuzz_worker.py", WORKER, "LOOPBACK-MERGE-FUZZ-OK")
