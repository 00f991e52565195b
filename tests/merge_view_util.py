"""Shared by the tests of imm3_comm_merge_groups_view (test_gpu_merge_view*.py, their two-rank worker, the timing test): the segments
they merge and the REFERENCE of a view -- never the library's own host ordering: merge_groups_wide's output (fuzzed against numpy by
test_gpu_merge_fuzz.py) passed through a filter in exact Python integers and np.lexsort, then cut to the limit."""
import numpy as np

from immutable3_amd import native

C, MN, MX, S = native.AGG_COUNT, native.AGG_MIN, native.AGG_MAX, native.AGG_SUM
GCOL, AGG = native.GROUP_ORDER_GROUP_COL, native.GROUP_ORDER_AGG
GT, LT, EQ = native.GT, native.LT, native.EQ
AND, OR, NOT = native.EXPR_AND, native.EXPR_OR, native.EXPR_NOT
CNT = native.GROUP_FILTER_COUNT

# ---- the columns: 0 state (2-byte string, 51 values), 1 k8 (int8, 4 values), 2 kid (int32, ~600 values, negative ones too), 3 name
# (12-byte string, 80 values sharing their first 8 bytes), 4 val (int32, small: sums and extremes tie), 5 s4 (4-byte string), 6 s12
# (12-byte string, a shared 8-byte prefix)
COL_KIND = ["str", "i8", "i32", "str", "i32", "str", "str"]
COL_WIDTH = [2, 1, 4, 12, 4, 4, 12]
K8_VALUES = np.array([-3, 0, 5, 100], np.int8)
SIZES = [3000, 1024, 1, 0]
SEG_INDEX = [7, 300, 2, 0]            # out of order, one above 255: two bytes of segment in the tie
AGGS_A = [(C, 4), (MN, 4), (MX, 1), (S, 4)]      # COUNT, MIN(int32), MAX(int8), SUM
AGGS_B = [(C, 4), (S, 4), (MX, 5), (MX, 6)]      # COUNT, SUM, MAX(4-byte string), MAX(12-byte string)
G_STATE, G_KID, G_NAME, G_K8KID = [0], [2], [3], [1, 2]


def columns(rng, n, kid_values=None):
    """the seven columns of a segment of n rows (RawColumn each); kid_values: the int32 group column, given"""
    from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, RawColumn, blocks_of
    states = np.array([[65 + i // 26, 65 + i % 26] for i in range(51)], np.uint8)
    names = rng.integers(97, 123, size=(80, 12)).astype(np.uint8)
    names[:, :8] = ord("n")
    kid = np.asarray(kid_values, np.int32) if kid_values is not None else (rng.integers(0, 600, size=n) * 7919 - 2_000_000).astype(np.int32)
    s12 = rng.integers(97, 123, size=(n, 12)).astype(np.uint8)
    s12[:, :8] = ord("p")
    br = blocks_of(n, 1024)
    return [RawColumn(DENSE_STRING, 2, states[rng.integers(0, 51, size=n)].reshape(n, 2), br),
            RawColumn(DENSE_TINYINT, 1, K8_VALUES[rng.integers(0, 4, size=n)], br),
            RawColumn(DENSE_INT, 4, kid, br),
            RawColumn(DENSE_STRING, 12, names[rng.integers(0, 80, size=n)].reshape(n, 12), br),
            RawColumn(DENSE_INT, 4, rng.integers(-50, 51, size=n).astype(np.int32), br),
            RawColumn(DENSE_STRING, 4, rng.integers(97, 100, size=(n, 4)).astype(np.uint8), br),
            RawColumn(DENSE_STRING, 12, s12, br)]


def agg_query(ctx, seg, sels, group, aggs, run=True):
    q = native.DeviceQuery(ctx, seg, list(range(7)), sels, (), 0, 1024, group_cols=group, aggs=aggs, wide_keys=True)
    if run:
        q.run()
    return q


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def _leaf(leaf, aggs, count, vals):
    agg, average, cond, value = leaf
    if agg == CNT or aggs[agg][0] == C:
        lhs, rhs = int(count), int(value)
    elif average:
        lhs, rhs = int(vals[agg]), int(value) * int(count)
    else:
        lhs, rhs = int(vals[agg]), int(value)
    return lhs > rhs if cond == GT else (lhs < rhs if cond == LT else lhs == rhs)


def keep_mask(merged, aggs, leaves, prog):
    """the groups the program keeps, in exact Python integers"""
    _, _, counts, vals, _ = merged[:5]
    out = np.ones(counts.shape[0], bool)
    if not prog:
        return out
    for g in range(counts.shape[0]):
        stack = []
        for op in prog:
            if op >= 0:
                stack.append(_leaf(leaves[op], aggs, counts[g], vals[g]))
            elif op == NOT:
                stack.append(not stack.pop())
            else:
                y, x = stack.pop(), stack.pop()
                stack.append((x and y) if op == AND else (x or y))
        out[g] = stack[-1]
    return out


def _key_columns(merged, group, aggs, key):
    """the lexsort columns of one order key, most significant first (int64 each; a descending key order-reversed)"""
    keys, _, counts, vals, strs = merged[:5]
    kind, index, desc = key
    if kind == GCOL:
        at = sum(COL_WIDTH[c] for c in group[:index])
        col = group[index]
        raw = keys[:, at: at + COL_WIDTH[col]]
        if COL_KIND[col] == "i32":
            cols = [np.ascontiguousarray(raw).view("<i4").reshape(-1).astype(np.int64)]
        elif COL_KIND[col] == "i8":
            cols = [raw.reshape(-1).view(np.int8).astype(np.int64)]
        else:
            cols = [raw[:, b].astype(np.int64) for b in range(raw.shape[1])]
    else:
        akind, _ = aggs[index]
        if akind == C:
            cols = [counts.astype(np.int64)]
        elif index in strs:
            cols = [strs[index][:, b].astype(np.int64) for b in range(strs[index].shape[1])]
        else:
            cols = [vals[:, index].astype(np.int64)]
    return [~c for c in cols] if desc else cols


def reference_view(merged, group, aggs, order=(), leaves=(), prog=(), limit=0):
    """(key_bytes, first, counts, vals, strs, n_kept) of the view over merge_groups_wide's `merged`: filter, then order -- ties in
    ascending `first` --, then limit"""
    keys, first, counts, vals, strs = merged[:5]
    kept = np.flatnonzero(keep_mask(merged, aggs, leaves, prog))
    cols = []
    for key in order:
        cols += _key_columns(merged, group, aggs, key)
    cols.append(first.astype(np.int64))
    perm = kept[np.lexsort([c[kept] for c in cols[::-1]])]
    if limit > 0:
        perm = perm[:limit]
    return keys[perm], first[perm], counts[perm], vals[perm], {j: b[perm] for j, b in strs.items()}, int(kept.size)


def assert_view(got, want, what=None):
    for i, name in enumerate(("keys", "first", "counts", "vals")):
        assert got[i].shape == want[i].shape and np.array_equal(got[i], want[i]), (what, name)
    assert sorted(got[4]) == sorted(want[4]), what
    for j in want[4]:
        assert got[4][j].shape == want[4][j].shape and np.array_equal(got[4][j], want[4][j]), (what, "string", j)
    assert got[5] == want[5], (what, "n_kept", got[5], want[5])
