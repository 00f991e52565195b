"""GPU timing (`zz`: with the other assertions on a time): the list pass must beat what a list cost before it existed.  16 M rows of an
int32 column; `id in (8 values)` through k_filter_int_list against the 8-term OR tree of IMM3_EQ leaves on the same column
(k_filter_expr's tile form) in the same process: kernel time by HIP events around the select launch (kernel id 0), the queries
alternated round by round, median of 11 rounds, no margin -- the list must be STRICTLY faster.  A one-compare range over the same
column (k_filter_tile: the floor, it reads the same bytes) and a 9-value list (the LDS form) are timed alongside and printed, not
asserted.  Measured on MI355X when this test was written: list 18.8 us, tree 27.3 us, floor 11.5 us, 9-value list 22.7 us
(profiles/int_in.txt)."""
import numpy as np
import pytest

from conftest import DENSE_INT, EQ, GT, RawColumn, blocks_of

pytestmark = pytest.mark.gpu


def test_eight_value_list_beats_the_eight_term_or_tree():
    from immutable3_amd import native
    n = 16 * 1024 * 1024
    rng = np.random.default_rng(16)
    ident = rng.integers(0, 1 << 20, size=n, dtype=np.int32)
    br = blocks_of(n, 1024)
    ctx = native.Context(0)
    seg = native.DeviceSegment(ctx, [RawColumn(DENSE_INT, 4, ident, br).native()])
    values = [int(v) for v in rng.choice(1 << 20, size=9, replace=False)]
    eight = values[:8]
    assert native.plan_int_list_form(4, 8) == native.INT_LIST_ARGS and native.plan_int_list_form(4, 9) == native.INT_LIST_LDS
    prog = [0]
    for k in range(1, 8):
        prog += [k, native.EXPR_OR]
    q_list = native.DeviceQuery(ctx, seg, [0], [(0, native.INT_IN, eight)])
    q_tree = native.DeviceQuery(ctx, seg, [0], [(0, EQ, float(v)) for v in eight], expr=prog)
    q_floor = native.DeviceQuery(ctx, seg, [0], [(0, GT, float(1 << 19))])
    q_nine = native.DeviceQuery(ctx, seg, [0], [(0, native.INT_IN, values)])
    queries = (q_list, q_tree, q_floor, q_nine)
    for q in queries:                       # warm-up (and the answer)
        q.run_select()
        q.sync()
    want = int(np.isin(ident, eight).sum())
    assert want > 0 and q_list.count() == want and q_tree.count() == want
    assert q_nine.count() == int(np.isin(ident, values).sum()) and q_floor.count() == int((ident > (1 << 19)).sum())
    assert q_tree.expr_form() == native.EXPR_FORM_TILE
    assert q_list.bitmap().tolist() == q_tree.bitmap().tolist()
    rounds = 11
    ctx.timing_enable(8 * rounds)
    ctx.timing_mask(1)
    ctx.timing_reset()
    for _ in range(rounds):
        for q in queries:
            q.run_select()
    ms = ctx.timing_collect(0)
    assert ms.size == len(queries) * rounds
    lst, tree, floor, nine = (np.median(ms[k::len(queries)]) * 1e3 for k in range(len(queries)))
    print(f"8-value list: median {lst:.1f} us; 8-term OR tree of EQ: {tree:.1f} us; one-compare range (floor): {floor:.1f} us; "
          f"9-value list (LDS form): {nine:.1f} us; list / floor = {lst / floor:.3f}, list / tree = {lst / tree:.3f}")
    assert lst < tree
    for q in queries:
        q.close()
    seg.close()
    ctx.close()
