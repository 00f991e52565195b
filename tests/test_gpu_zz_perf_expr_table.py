"""GPU timing: ONE table-tree launch over all segments must take less time than the per-segment tree launches it replaces.
64 segments x 262 144 rows of I8 + I32, the two-term tree of test_gpu_zz_perf_expr.py; kernel time by HIP events around the select
launch (kernel id 0), the candidates alternated in one process, median of 11 rounds, no margin: the baseline is the sum of the 64
per-segment k_filter_expr launches (their kernel times alone -- the gaps between 64 dependent launches are not even counted).
Reported, not asserted: the table-tree launch against one conjunctive table launch (imm3_query_create_table, the first term) and
against the single-segment tree launch over the same rows concatenated.
Measured on MI355X (tools/expr_table_bench.py, profiles/expr_table.txt; DESIGN.md section 20's addendum reads them): (a) 25.5 us
against (c) 321.9 us, c/a = 12.6; a/b = 1.46, a/w = 1.17.  100 M rows as 98 segments: 133.5 against 533.8 us, c/a = 4.0."""
import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_TINYINT, GT, LT, RawColumn, blocks_of
from expr_util import AND, OR, postfix

pytestmark = pytest.mark.gpu


def test_one_table_tree_launch_beats_the_per_segment_launches():
    from immutable3_amd import native
    n_segs, n = 64, 262144
    rng = np.random.default_rng(64)
    ident = rng.integers(0, 1 << 30, size=n_segs * n, dtype=np.int32)
    age = rng.integers(0, 100, size=n_segs * n).astype(np.int8)
    ctx = native.Context(0)
    br = blocks_of(n, 1024)
    segs = [native.DeviceSegment(ctx, [RawColumn(DENSE_TINYINT, 1, age[s * n:(s + 1) * n], br).native(),
                                       RawColumn(DENSE_INT, 4, ident[s * n:(s + 1) * n], br).native()]) for s in range(n_segs)]
    whole = native.DeviceSegment(ctx, [RawColumn(DENSE_TINYINT, 1, age, blocks_of(n_segs * n, 1024)).native(),
                                       RawColumn(DENSE_INT, 4, ident, blocks_of(n_segs * n, 1024)).native()])
    table = native.DeviceTable(ctx, segs)
    # (age < 18 and id < 2^29) or (age > 65 and id > 2^29)
    t1 = [(0, LT, 18.0), (1, LT, float(1 << 29))]
    t2 = [(0, GT, 65.0), (1, GT, float(1 << 29))]
    tree = (OR, (AND, 0, 1), (AND, 2, 3))
    q_table = native.DeviceQuery(ctx, table, [0, 1], t1 + t2, expr=postfix(tree))
    q_segs = [native.DeviceQuery(ctx, s, [0, 1], t1 + t2, expr=postfix(tree)) for s in segs]
    q_conj = native.DeviceQuery(ctx, table, [0, 1], t1)
    q_whole = native.DeviceQuery(ctx, whole, [0, 1], t1 + t2, expr=postfix(tree))
    everything = [q_table] + q_segs + [q_conj, q_whole]
    want = ((age < 18) & (ident < (1 << 29))) | ((age > 65) & (ident > (1 << 29)))
    for q in everything:                     # warm-up (and the answer)
        q.run_select()
        q.sync()
    assert q_table.count() == int(want.sum()) == sum(q.count() for q in q_segs) == q_whole.count()
    assert q_table.expr_form() == native.EXPR_FORM_TILE
    assert q_table.bitmap().tolist() == q_whole.bitmap().tolist()     # (whole tiles per segment: the virtual row space is the concatenation)
    rounds = 11
    per_round = len(everything)
    ctx.timing_enable(per_round * rounds + 8)
    ctx.timing_mask(1)
    ctx.timing_reset()
    for _ in range(rounds):
        for q in everything:
            q.run_select()
    ms = ctx.timing_collect(0)
    assert ms.size == per_round * rounds
    us = ms.reshape(rounds, per_round) * 1e3
    a = us[:, 0]
    c = us[:, 1:1 + n_segs].sum(axis=1)
    b, w = us[:, 1 + n_segs], us[:, 2 + n_segs]
    print(f"table-tree launch (a): median {np.median(a):.1f} us; sum of the {n_segs} per-segment tree launches (c): median {np.median(c):.1f} us "
          f"(c/a = {np.median(c) / np.median(a):.2f}); one conjunctive table launch (b): median {np.median(b):.1f} us, a/b = {np.median(a) / np.median(b):.3f}; "
          f"single-segment tree over the same rows (w): median {np.median(w):.1f} us, a/w = {np.median(a) / np.median(w):.3f}")
    assert np.median(a) < np.median(c)
    for q in everything:
        q.close()
    table.close()
    whole.close()
    for s in segs:
        s.close()
    ctx.close()
