"""GPU timing: a one-launch disjunction must beat what it replaces -- one conjunctive launch per term (and the host's OR of the
bitmaps, not even counted here).  I8 + I32, two terms, 16 M rows; kernel time by HIP events around the select launch (kernel id 0),
the three queries alternated in one process, median of 11 rounds, no margin: the two conjunctive launches read the same bytes
twice.  Measured on MI355X when this test was written: (a) 21.4 us, (c) 30.0 us, one conjunctive launch (b) 15.0 us
(profiles/expr_filter.txt; at 100 M rows: 110.9 / 160.1 / 79.8)."""
import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_TINYINT, GT, LT, RawColumn, blocks_of
from expr_util import AND, OR, postfix

pytestmark = pytest.mark.gpu


def test_two_term_tree_beats_two_conjunctive_launches():
    from immutable3_amd import native
    n = 16 * 1024 * 1024
    rng = np.random.default_rng(16)
    ident = rng.integers(0, 1 << 30, size=n, dtype=np.int32)
    age = rng.integers(0, 100, size=n).astype(np.int8)
    br = blocks_of(n, 1024)
    ctx = native.Context(0)
    seg = native.DeviceSegment(ctx, [RawColumn(DENSE_TINYINT, 1, age, br).native(), RawColumn(DENSE_INT, 4, ident, br).native()])
    # (age < 18 and id < 2^29) or (age > 65 and id > 2^29)
    t1 = [(0, LT, 18.0), (1, LT, float(1 << 29))]
    t2 = [(0, GT, 65.0), (1, GT, float(1 << 29))]
    tree = (OR, (AND, 0, 1), (AND, 2, 3))
    q_tree = native.DeviceQuery(ctx, seg, [0, 1], t1 + t2, expr=postfix(tree))
    q_1 = native.DeviceQuery(ctx, seg, [0, 1], t1)
    q_2 = native.DeviceQuery(ctx, seg, [0, 1], t2)
    want = ((age < 18) & (ident < (1 << 29))) | ((age > 65) & (ident > (1 << 29)))
    for q in (q_tree, q_1, q_2):            # warm-up (and the answer)
        q.run_select()
        q.sync()
    assert q_tree.count() == int(want.sum()) and q_tree.count() == q_1.count() + q_2.count()   # (the terms are disjoint)
    assert q_tree.expr_form() == native.EXPR_FORM_TILE
    rounds = 11
    ctx.timing_enable(8 * rounds)
    ctx.timing_mask(1)
    ctx.timing_reset()
    for _ in range(rounds):
        for q in (q_tree, q_1, q_2):
            q.run_select()
    ms = ctx.timing_collect(0)
    assert ms.size == 3 * rounds
    a = ms[0::3] * 1e3
    c = (ms[1::3] + ms[2::3]) * 1e3
    print(f"tree launch (a): median {np.median(a):.1f} us; two conjunctive launches (c): median {np.median(c):.1f} us; "
          f"single conjunctive launch (b): median {np.median(ms[1::3]) * 1e3:.1f} us; a/b = {np.median(a) / (np.median(ms[1::3]) * 1e3):.3f}")
    assert np.median(a) < np.median(c)
    for q in (q_tree, q_1, q_2):
        q.close()
    seg.close()
    ctx.close()
