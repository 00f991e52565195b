"""The expected result of an ordered projection, from the unchanged oracle: oracle_np's projected rows of the UNORDERED query, then
numpy.lexsort over the normalised key bytes with the row's place in the unordered result as the last key.

Normalised key (include/imm3.h, imm3_query_set_order): per key column, most significant first -- int32 as 4 big-endian bytes of
x ^ 0x80000000, int8 as x ^ 0x80, a string's bytes as they are; a descending key's bytes complemented.  Unsigned byte order of that
key is the order asked for, and rows whose keys are all equal keep their ascending (segment, row) order."""
import numpy as np

from oracle import oracle_np

DENSE_INT, DENSE_TINYINT, DENSE_STRING = 1, 2, 3
EXPR_AND, EXPR_OR, EXPR_NOT = -1, -2, -4
PROJECT_CHECK_ROWS = 5000        # up to here the vectorised projection below is held against oracle_np.project's row loop


def select_masks(npcols, sels, block_size, expr=None):
    """Per-batch keep masks of the select: oracle_np.scan_select's for a flat list; for a tree (`expr`: the postfix program over the
    leaves `sels`) every leaf's masks from oracle_np.scan_select, combined by the program."""
    if expr is None:
        return oracle_np.scan_select(npcols, sels, block_size)[2]
    stack = []
    for op in expr:
        if op >= 0:
            stack.append(oracle_np.scan_select(npcols, [sels[op]], block_size)[2])
        elif op == EXPR_NOT:
            stack.append([~m for m in stack.pop()])
        else:
            b, a = stack.pop(), stack.pop()
            stack.append([(x & y) if op == EXPR_AND else (x | y) for x, y in zip(a, b)])
    assert len(stack) == 1
    return stack[0]


def projected(npcols, proj, masks):
    """The unordered, unlimited projection: (row number in the segment int64[n], [uint8[n, width] per SELECT-list column]) in emission
    order -- oracle_np.decode_block of every batch under its mask; small results are checked against oracle_np.project itself."""
    bounds = [oracle_np._block_bounds(c[1]) for c in npcols]
    rows, vals, start = [], [[] for _ in proj], 0
    for k, keep in enumerate(masks):
        idx = np.flatnonzero(keep)
        rows.append(start + idx)
        for slot, j in enumerate(proj):
            dat, _, codec, width = npcols[j]
            s, ln = bounds[j][k]
            raw = np.asarray(dat[s: s + ln], dtype=np.uint8).reshape(-1, width)
            vals[slot].append(raw[idx])
        start += keep.shape[0]
    row_index = np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64)
    out = [np.concatenate(v) if v else np.zeros((0, npcols[j][3]), np.uint8) for v, j in zip(vals, proj)]
    if row_index.size <= PROJECT_CHECK_ROWS:
        ref_rows, _, _ = oracle_np.project(npcols, list(proj), 0, masks)
        assert len(ref_rows) == row_index.size
        for slot, j in enumerate(proj):
            codec, width = npcols[j][2], npcols[j][3]
            for r in range(row_index.size):
                mine = out[slot][r].tobytes()
                want = ref_rows[r][slot]
                if codec == DENSE_STRING:
                    assert mine == want
                else:
                    assert int.from_bytes(mine, "little", signed=True) == want
    return row_index, out


def normalised_keys(vals, codecs, order_by):
    """uint8[n, key_bytes]: the normalised key of every projected row.  vals: uint8[n, width] per SELECT-list column; codecs: the
    DENSE_* value codec of each; order_by: [(index into the SELECT list, descending)]."""
    parts = []
    for (j, desc) in order_by:
        v = np.ascontiguousarray(vals[j], dtype=np.uint8)
        if codecs[j] == DENSE_INT:
            k = v[:, ::-1].copy()
            k[:, 0] ^= 0x80
        elif codecs[j] == DENSE_TINYINT:
            k = v ^ np.uint8(0x80)
        else:
            k = v.copy()
        parts.append(~k if desc else k)
    n = vals[0].shape[0] if vals else 0
    return np.concatenate(parts, axis=1) if parts else np.zeros((n, 0), np.uint8)


def order_permutation(keys, limit=0):
    """Places (into the unordered result) of the ordered rows: lexsort over the key bytes, byte 0 most significant, the place itself
    the last key; the first `limit` of them when limit > 0."""
    n, kb = keys.shape
    place = np.arange(n, dtype=np.int64)
    perm = np.lexsort(tuple([place] + [keys[:, b] for b in range(kb - 1, -1, -1)])) if n else place
    return perm[:limit] if limit > 0 else perm


def expected(npcols, used_codecs, sels, proj, order_by, limit=0, block_size=1024, expr=None):
    """(row_index int64[m], [uint8[m, width]]) of `select proj where sels order by order_by limit limit` over one segment."""
    masks = select_masks(npcols, sels, block_size, expr)
    row_index, vals = projected(npcols, proj, masks)
    keys = normalised_keys(vals, [used_codecs[j] for j in proj], order_by)
    perm = order_permutation(keys, limit)
    return row_index[perm], [v[perm] for v in vals]


def expected_table(per_segment_npcols, used_codecs, sels, proj, order_by, limit=0, block_size=1024, expr=None):
    """The same over the segments of a table: (segment int64[m], row int64[m], [uint8[m, width]]); ties in (segment, row) order."""
    segs, rows, vals = [], [], None
    for s, npcols in enumerate(per_segment_npcols):
        ri, v = projected(npcols, proj, select_masks(npcols, sels, block_size, expr))
        segs.append(np.full(ri.size, s, np.int64))
        rows.append(ri)
        vals = [[x] for x in v] if vals is None else [a + [x] for a, x in zip(vals, v)]
    seg, row = np.concatenate(segs), np.concatenate(rows)
    vals = [np.concatenate(v) for v in vals]
    perm = order_permutation(normalised_keys(vals, [used_codecs[j] for j in proj], order_by), limit)
    return seg[perm], row[perm], [v[perm] for v in vals]


def merge_ordered(parts, codecs, order_by, limit=0):
    """What a host merge of per-segment ordered results must give: parts = [(segment, row_index, vals)] -> (segment, row, vals),
    stable by (keys, segment, row)."""
    seg = np.concatenate([np.full(np.asarray(ri).size, s, np.int64) for (s, ri, _) in parts])
    row = np.concatenate([np.asarray(ri, dtype=np.int64) for (_, ri, _) in parts])
    vals = [np.concatenate([p[2][j] for p in parts]) for j in range(len(codecs))]
    keys = normalised_keys(vals, codecs, order_by)
    n, kb = keys.shape
    perm = np.lexsort(tuple([row, seg] + [keys[:, b] for b in range(kb - 1, -1, -1)])) if n else np.arange(0)
    if limit > 0:
        perm = perm[:limit]
    return seg[perm], row[perm], [v[perm] for v in vals]
