"""The generator and the reference side of the table fuzzers (test_gpu_fuzz_table.py, test_table_fuzz_host.py): random imm3_table
shapes, codecs and queries, and what the oracles say about them.  Pure numpy and the CPU oracles: nothing here touches a device.

A table is 1 to 6 segments of [id int32, v int32, age int8, state string(2), name string(8 | 16)], every segment in a block layout
that imm3_table_create accepts (every non-final block a multiple of 64 rows and at most 1024), every column in one codec for the
whole table.  Expectations are the C oracle's scan_select / layout / project per segment, concatenated in segment order; group-by
expectations are plain numpy with Python-int sums (and oracle_np.project_agg + combine_agg where that knows the aggregates); a select
tree's are expr_not_util.expected_masks per segment.  The library is never asked what the answer is."""
import numpy as np

from conftest import (DENSE_INT, DENSE_STRING, DENSE_TINYINT, EQ, GT, LT, MATCH, PforColumn, RawColumn, SnappyColumn, blocks_of)
from immutable3_amd import native
from expr_not_util import expected_masks, has_not, postfix, random_tree, words_of_masks  # noqa: F401  (re-exported)
from oracle import oracle_np
from str_rows_util import make_strings, pool_for
from test_gpu_fuzz import random_numeric_pred

ID, V, AGE, STATE, NAME = range(5)
COLUMN_NAMES = ["id", "v", "age", "state", "name"]
DENSE_OF = [(DENSE_INT, 4), (DENSE_INT, 4), (DENSE_TINYINT, 1), (DENSE_STRING, 2), (DENSE_STRING, None)]
DENSE, PFOR, SNAPPY = "dense", "pfor", "snappy"
CODECS_OF = [(DENSE, PFOR, SNAPPY), (DENSE, PFOR, SNAPPY), (DENSE, SNAPPY), (DENSE, SNAPPY), (DENSE, SNAPPY)]
SNAPPY_MAX_BLOCK_BYTES = 24_000                     # the bound test_gpu_fuzz.py uses (the GPU decoder's LDS window)
SEG_ROWS = [0, 1, 63, 64, 100, 1024, 1025, 3 * 1024 + 700, 8 * 1024 + 1, 20_000]
LIMIT_SEG_ROWS = [0, 1, 1025, 4 * 1024 + 1, 8 * 1024 + 1, 12 * 1024 + 300]
CODES = [bytes([65 + i, 66 + j]) for i in range(4) for j in range(3)]          # 12 two-byte codes
TINY_V = 1000                                       # v of the rows of one-row segments in a marked table (every other v is small)

# seeds of the GPU fuzzers (test_gpu_fuzz_table.py) -- the census (test_table_fuzz_host.py) walks the same
SELECT_SEEDS, SELECT_TABLES, SELECT_QUERIES = 32, 4, 3
LIMIT_SEEDS = 16
GROUP_SEEDS, GROUP_TABLES, GROUP_QUERIES = 16, 2, 3
# TREE_SEED was chosen on the CPU (imm3_expr_normalize tells the form without a device) so that the normaliser alone keeps the trees a
# table refuses within a quarter: with this seed TREE_REFUSED of the TREE_COUNT normal forms do not fit the table's tile form.
TREE_SEED, TREE_TABLES, TREE_COUNT, TREE_REFUSED = 20261114, 4, 40, 8
LIMIT_KINDS = ["none", "one", "half of the first segment", "the first segment", "total - 1", "total", "total + 7"]


# ---- tables ---------------------------------------------------------------------------------------------------------------------
def table_layout(rng, n):
    """block rows of a segment of n rows: uniform 1024 (n = k * 1024 + 1: the loader's quirk, full blocks and a one-row block),
    uniform 64 / 128 / 512, or mixed multiples of 64; the final block is whatever is left"""
    if n == 0:
        return []
    kind = int(rng.integers(0, 4))
    if kind <= 1:
        return blocks_of(n, 1024)
    if kind == 2:
        return blocks_of(n, int(rng.choice([64, 128, 512])))
    out, left = [], n
    while left > 0:
        b = int(rng.choice([64, 128, 256, 512, 1024]))
        if b >= left:
            out.append(left)
            break
        out.append(b)
        left -= b
    return out


def layout_ok(block_rows):
    """the rule of imm3_table_create, and the bound this fuzz keeps to"""
    return all(b % 64 == 0 and 0 < b <= 1024 for b in block_rows[:-1]) and (not block_rows or block_rows[-1] >= 1)


def is_quirk(block_rows):
    return len(block_rows) >= 2 and all(b == 1024 for b in block_rows[:-1]) and block_rows[-1] == 1


def make_column(c, codec, values, block_rows, width):
    dense, _ = DENSE_OF[c]
    if codec == PFOR:
        return PforColumn(values, block_rows)
    if codec == SNAPPY:
        return SnappyColumn(dense, width, values, block_rows)
    return RawColumn(dense, width, values, block_rows)


class FuzzTable:
    """per-segment column objects (segs[si][c]: RawColumn / PforColumn / SnappyColumn) and numpy's view of all rows (data[c])"""

    def __init__(self, rng, seg_rows, layouts, codecs=None, mark_tiny=False, ascending_id=None):
        """ascending_id: None -- drawn; "row" -- id is the row of the whole table.  mark_tiny: v = TINY_V in one-row segments."""
        self.seg_rows, self.layouts = [int(n) for n in seg_rows], layouts
        self.n_rows = sum(self.seg_rows)
        self.starts = np.concatenate([[0], np.cumsum(self.seg_rows)]).astype(np.int64)
        self.tiles = [-(-n // 1024) for n in self.seg_rows]
        self.name_width = int(rng.choice([8, 16]))
        self.widths = [4, 4, 1, 2, self.name_width]
        self.pool, self.t0, self.t1 = pool_for(rng, self.name_width)
        self.n_codes = int(rng.choice([1, 3, 12]))
        n = self.n_rows
        self.ascending_id = bool(rng.random() < 0.5) if ascending_id is None else True
        if ascending_id == "row":
            ids = np.arange(n, dtype=np.int32)
        elif self.ascending_id:
            ids = (np.arange(n, dtype=np.int64) * int(rng.choice([1, 3])) - int(rng.choice([0, 1000]))).astype(np.int32)
        else:
            ids = rng.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64).astype(np.int32)
        v = rng.integers(-40, 40, size=n).astype(np.int32)
        if mark_tiny:
            for si, rows in enumerate(self.seg_rows):
                if rows == 1:
                    v[self.starts[si]] = TINY_V
        age = (rng.integers(0, 100, size=n) if (mark_tiny or rng.random() < 0.5) else rng.integers(-128, 128, size=n)).astype(np.int8)
        state = np.array([list(c) for c in CODES], np.uint8)[rng.integers(0, self.n_codes, size=n)].reshape(n, 2)
        name = make_strings(rng, self.pool, n)
        self.data = [ids, v, age, state, name]
        biggest = max([max(br) for br in layouts if br], default=0)
        if codecs is None:
            codecs = [str(rng.choice(CODECS_OF[c])) for c in range(5)]
        self.codecs = [DENSE if (k == SNAPPY and biggest * self.widths[c] > SNAPPY_MAX_BLOCK_BYTES) else k for c, k in enumerate(codecs)]
        self.segs = []
        for si, rows in enumerate(self.seg_rows):
            lo, hi = int(self.starts[si]), int(self.starts[si + 1])
            self.segs.append([make_column(c, self.codecs[c], self.data[c][lo:hi], layouts[si], self.widths[c]) for c in range(5)])

    def value_bytes(self, c, rows):
        """uint8[len(rows), width]: the raw bytes of column c at these rows of the whole table"""
        return np.ascontiguousarray(self.data[c][rows]).view(np.uint8).reshape(len(rows), self.widths[c])

    def describe(self):
        return {"rows": self.seg_rows, "codecs": self.codecs, "name": self.name_width, "blocks": [br[:3] + ["..."] if len(br) > 4 else br for br in self.layouts]}


def random_table(rng):
    """-> FuzzTable: .segs the per-segment column objects, .data the numpy view of all rows"""
    n_segs = int(rng.integers(1, 7))
    rows = [int(x) for x in rng.choice(SEG_ROWS, size=n_segs)]
    if n_segs >= 2 and rng.random() < 0.45:                                   # an empty or one-row segment that is not the last
        rows[int(rng.integers(0, n_segs - 1))] = int(rng.choice([0, 1]))
    return FuzzTable(rng, rows, [table_layout(rng, n) for n in rows])


def has_tiny_before_last(rows):
    return any(n <= 1 for n in rows[:-1])


def limit_table_shape(rng, G):
    """10 to 16 segments of unequal length with more tiles than G work-groups claim at once, an empty and a one-row segment
    somewhere in the middle.  (G = 5 needs more than 160 tiles, and 16 segments get there only with most of them at 12 x 1024 + 300
    rows: those tables hold up to about 170 000 rows, every other one stays below 150 000.)"""
    need = G * native.TABLE_LIMIT_CLAIM_TILES
    for attempt in range(200):
        n_segs = int(rng.integers(10, 17)) if attempt < 3 else 16
        big = min(0.92, 0.4 + 0.1 * attempt)
        p = [(1 - big) / 4] * 4 + [big * 0.4, big * 0.6]
        rows = [int(x) for x in rng.choice(LIMIT_SEG_ROWS, size=n_segs, p=p)]
        a, b = (int(x) for x in rng.choice(np.arange(1, n_segs - 1), size=2, replace=False))
        rows[a], rows[b] = 0, 1
        if sum(-(-n // 1024) for n in rows) > need and len(set(rows)) >= 4:
            return rows
    raise AssertionError("no table shape with more than %d tiles" % need)


def random_limit_table(rng, seed):
    """-> (FuzzTable, G): the table of one seed of test_fuzz_table_limit_stops_right; its id ascends (id = row of the whole table),
    v marks the rows of one-row segments, one seed in three has compressed predicate columns"""
    G = [1, 2, 3, 5][seed % 4]
    rows = limit_table_shape(rng, G)
    codecs = [DENSE] * 5
    if seed % 3 == 0:
        codecs[ID], codecs[V], codecs[AGE] = str(rng.choice([PFOR, SNAPPY])), str(rng.choice([PFOR, SNAPPY])), SNAPPY
    return FuzzTable(rng, rows, [blocks_of(n, 1024) for n in rows], codecs=codecs, mark_tiny=True, ascending_id="row"), G


def limit_cases(rng, t, seed):
    """[(what, used, sels, proj)]: where the survivors lie.  One seed in three carries a wide-string Match beside the range."""
    n, rows = t.n_rows, t.seg_rows
    mid = [si for si in range(1, len(rows) - 1) if rows[si] >= 1025]
    k = mid[int(rng.integers(0, len(mid)))]
    before_end = int(t.starts[k + 1]) - 2                                      # id > this: the last row of segment k and all behind
    cases = [
        ("from the first tile", [ID, AGE], [(0, GT, 5.0)], [1, 0]),
        ("only in the last third", [ID, STATE, AGE], [(0, GT, float(2 * n // 3))], [2, 0, 1]),
        ("from one row before a segment's end", [ID], [(0, GT, float(before_end))], [0]),
        ("only in one-row segments", [V, ID], [(0, EQ, float(TINY_V))], [1, 0, 1]),
        ("sparse", [AGE, ID, V], [(0, EQ, float(rng.integers(0, 100)))], [1, 0]),
        ("nowhere", [AGE, ID], [(0, GT, 100.0)], [1]),
    ]
    if seed % 3 == 1:
        half = [bytes(p) for p in t.pool[: t.pool.shape[0] // 2]] + [bytes(t.t0)]
        cases = [(what + ", and a wide Match", used + [NAME], sels + [(len(used), MATCH, half)], proj + [len(used)]) for what, used, sels, proj in cases]
    return cases


def limit_case_stops(used, sels):
    """can this case run the stopping launch (k_filter_table_limit)?  The plan takes it only for a select chain of ONE tile pass
    (imm3_planner.cpp: plan_select_chain, table_limit_applies): a wide-string Match is a pass of its own and keeps the whole
    select.  Compressed columns do not matter: a table decodes them when it is created."""
    return not any(cond == MATCH and used[j] == NAME for j, cond, _ in sels)


# ---- flat queries ---------------------------------------------------------------------------------------------------------------
def state_match(rng, t):
    """an IN-list of at most 8 two-byte values at a random selectivity: no row, every row (when at most 8 codes occur), or some"""
    present, absent = CODES[: t.n_codes], CODES[t.n_codes:] + [b"zz", b"Z~"]
    how = int(rng.integers(0, 4))
    if how == 0:
        return [absent[int(i)] for i in rng.permutation(len(absent))[: int(rng.integers(1, 3))]]
    if how == 1 and len(present) <= 8:
        return list(present)
    m = int(rng.choice([1, 2, 4, 8]))
    return [CODES[int(i)] for i in rng.permutation(len(CODES))[:m]]


def name_match(rng, t):
    """an IN-list on the wide column: values that occur, values that do not, and values that share a prefix with ones that do"""
    w = t.name_width
    absent = [bytes(rng.integers(65, 91, size=w).astype(np.uint8)) for _ in range(3)]          # upper case: in no row
    near = t.t0.copy()
    near[-1] ^= 0x40                                                                          # all but the last byte of t0
    near2 = t.t1.copy()
    near2[w // 2] ^= 0x20
    pool = [bytes(p) for p in t.pool]
    how = int(rng.integers(0, 4))
    if how == 0:
        return absent + [bytes(near), bytes(near2)]                                           # no row
    if how == 1:
        return pool + absent[:1]                                                              # every row
    k = int(rng.choice([1, 3, 9]))
    return [bytes(t.t0), bytes(near)] + absent[:2] + [pool[int(i)] for i in rng.permutation(len(pool))[:k]]


def column_preds(rng, t, j, c):
    """0 to 2 predicates on used column j (table column c)"""
    k = int(rng.choice([0, 1, 1, 2]))
    out = []
    while len(out) < k:
        if c == STATE:
            out.append((j, MATCH, state_match(rng, t)))
        elif c == NAME:
            out.append((j, MATCH, name_match(rng, t)))
        else:
            out += random_numeric_pred(rng, j, t.data[c])
    return out[:2]


class FlatQuery:
    def __init__(self, used, sels, proj, limit_kinds, reserve):
        self.used, self.sels, self.proj, self.limit_kinds, self.reserve = used, sels, proj, limit_kinds, reserve


def random_flat_query(rng, t):
    n_used = int(rng.integers(1, 6))
    used = [int(x) for x in rng.permutation(5)[:n_used]]
    sels = []
    for j, c in enumerate(used):
        sels += column_preds(rng, t, j, c)
    proj = [int(x) for x in rng.integers(0, n_used, size=int(rng.integers(0, n_used + 2)))]    # repeats allowed
    kinds = [LIMIT_KINDS[int(i)] for i in sorted(rng.permutation(len(LIMIT_KINDS))[:3])] if proj else ["none"]
    reserve = [None, None, 10, t.n_rows + 8][int(rng.integers(0, 4))] if proj else None
    return FlatQuery(used, sels, proj, kinds, reserve)


def limit_of(kind, seg_counts):
    """the limit a kind names, from the oracle's per-segment survivor counts (0: no limit)"""
    total = sum(seg_counts)
    first = next((c for c in seg_counts if c > 0), 0)
    return {"none": 0, "one": 1, "half of the first segment": max(1, first // 2), "the first segment": first, "total - 1": max(total - 1, 0),
            "total": total, "total + 7": total + 7}[kind]


class Expected:
    """what the C oracle says of a flat query over a table: per segment (bitmap words, count) and the batch layout; all survivors in
    (segment, row) order with the bytes of every projected column"""

    def __init__(self, oracle, t, used, sels, proj):
        self.per_seg, self.layouts = [], []
        seg, row, vals = [], [], [[] for _ in proj]
        for si, cols in enumerate(t.segs):
            ocols = [cols[c].ocol() for c in used]
            ow, oc = oracle.scan_select(ocols, sels, 1024, 1)
            size, oid, woff, _ = oracle.layout(ocols[0], 1024)
            self.per_seg.append((ow, oc))
            self.layouts.append((size, oid, woff))
            if proj:
                n, batch, pos, ovals, _ = oracle.project(ocols, proj, 0, 1024, ow)
                assert n == oc
                starts = np.concatenate([[0], np.cumsum(size.astype(np.int64))])
                seg.append(np.full(n, si, np.int64))
                row.append(starts[batch[:n]] + pos[:n])
                for j in range(len(proj)):
                    vals[j].append(np.asarray(ovals[j])[:n])
        self.counts = [oc for _, oc in self.per_seg]
        self.total = sum(self.counts)
        self.seg = np.concatenate(seg) if seg else np.zeros(0, np.int64)
        self.row = np.concatenate(row) if row else np.zeros(0, np.int64)
        self.vals = [np.concatenate(v) for v in vals] if seg else [np.zeros((0, t.widths[used[j]]), np.uint8) for j in proj]
        if proj:                                                              # the oracle's values are numpy's view at the oracle's rows
            where = t.starts[self.seg] + self.row
            for j, pj in enumerate(proj):
                assert self.vals[j].tobytes() == t.value_bytes(used[pj], where).tobytes()

    def keep(self, t):
        """bool over all rows of the table"""
        k = np.zeros(t.n_rows, bool)
        k[t.starts[self.seg] + self.row] = True
        return k


# ---- group-by -------------------------------------------------------------------------------------------------------------------
class AggQuery:
    def __init__(self, used, sels, group, aggs, wide_keys):
        self.used, self.sels, self.group, self.aggs, self.wide_keys = used, sels, group, aggs, wide_keys


def random_agg_query(rng, t):
    """group columns from {age, state, v, name (the wide-key entry point)}, 1 to 4 aggregates of count / min / max / sum (no min and
    no sum over strings), a predicate chain"""
    used = [int(x) for x in rng.permutation(5)]
    at = {c: j for j, c in enumerate(used)}
    cand = [AGE, STATE, V] + ([NAME] if rng.random() < 0.4 else [])
    group_cols = [cand[int(i)] for i in rng.permutation(len(cand))[: int(rng.integers(0, 3))]]
    wide = NAME in group_cols or bool(group_cols and rng.random() < 0.15)
    aggs = []
    for _ in range(int(rng.integers(1, 5))):
        c = int(rng.integers(0, 5))
        kind = str(rng.choice(["count", "min", "max", "sum"]))
        if c in (STATE, NAME) and kind in ("min", "sum"):
            kind = "max"
        aggs.append((kind, at[c]))
    sels = []
    for c in rng.permutation(5)[: int(rng.integers(0, 3))]:
        sels += column_preds(rng, t, at[int(c)], int(c))
    return AggQuery(used, sels, [at[c] for c in group_cols], aggs, wide)


def expected_groups(t, q, keep):
    """plain numpy over the whole table's rows: groups in first-seen order over (segment, row).
    -> (key bytes uint8[g, kb], first rows (of the whole table) int64[g], counts [int], vals [[int | bytes] per aggregate] per group)"""
    sel = np.flatnonzero(keep)
    parts = [t.value_bytes(q.used[g], sel) for g in q.group]
    packed = np.concatenate(parts, axis=1) if parts else np.zeros((sel.size, 0), np.uint8)
    kb = packed.shape[1]
    if sel.size == 0:
        return packed, np.zeros(0, np.int64), [], []
    kv = np.ascontiguousarray(packed).view(np.dtype((np.void, kb))).reshape(-1) if kb else np.zeros(sel.size, np.uint8)
    _, idx, inv = np.unique(kv, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(idx, kind="stable")                                   # groups by their first selected row
    rank = np.empty(order.size, np.int64)
    rank[order] = np.arange(order.size)
    gid = rank[inv]                                                            # every selected row's group, numbered first-seen
    by_group = np.argsort(gid, kind="stable")
    counts = np.bincount(gid, minlength=order.size)
    ends = np.cumsum(counts)
    vals = [[] for _ in range(order.size)]
    for kind, j in q.aggs:
        c = q.used[j]
        col = t.data[c][sel][by_group]
        if c in (STATE, NAME):
            rows = [bytes(r) for r in col]
        else:
            rows = [int(x) for x in col]
        for g in range(order.size):
            mine = rows[ends[g] - counts[g]: ends[g]]
            vals[g].append(len(mine) if kind == "count" else (sum(mine) if kind == "sum" else (max(mine) if kind == "max" else min(mine))))
    return packed[idx[order]], sel[idx[order]], [int(x) for x in counts], vals


def oracle_np_groups(t, q):
    """oracle_np.project_agg per segment merged by combine_agg, for the aggregates it knows: [(key string, [states])]"""
    per = []
    for cols in t.segs:
        ucols = [cols[c].npcol() for c in q.used]
        _, _, masks = oracle_np.scan_select(ucols, q.sels, 1024)
        per.append(oracle_np.project_agg(ucols, q.group, q.aggs, masks))
    return list(oracle_np.combine_agg(per, q.aggs).items())


def as_oracle_np(t, q, groups):
    """expected_groups' result the way oracle_np spells it (the two references are held against each other)"""
    keys, _, counts, vals = groups
    out = []
    for g in range(len(counts)):
        parts, off = [], 0
        for j in q.group:
            w = t.widths[q.used[j]]
            chunk = bytes(keys[g, off: off + w])
            parts.append(chunk.decode() if q.used[j] in (STATE, NAME) else str(int.from_bytes(chunk, "little", signed=True)))
            off += w
        st = [v if kind == "count" else (v.decode() if isinstance(v, bytes) else float(v)) for (kind, _), v in zip(q.aggs, vals[g])]
        out.append(("_".join(parts), st))
    return out


# ---- select trees ---------------------------------------------------------------------------------------------------------------
def tree_leaf(rng, t):
    c = int(rng.choice([ID, V, AGE, STATE, NAME], p=[0.3, 0.18, 0.26, 0.2, 0.06]))
    if c == STATE:
        k = int(rng.integers(1, 5))
        return (c, MATCH, [CODES[int(i)] for i in rng.choice(len(CODES), size=k, replace=False)] + ([b"XYZ"] if rng.random() < 0.2 else []))
    if c == NAME:
        return (c, MATCH, [bytes(t.t0)])
    return random_numeric_pred(rng, c, t.data[c])[0]


def tree_cases():
    """[(table index, leaves, tree, proj, limit kind)]: TREE_COUNT trees over TREE_TABLES tables, all five columns used in order"""
    rng = np.random.default_rng(TREE_SEED)
    tables = [random_table(rng) for _ in range(TREE_TABLES)]
    out = []
    for i in range(TREE_COUNT):
        t = tables[i % TREE_TABLES]
        n = int(rng.integers(2, 6))
        leaves = [tree_leaf(rng, t) for _ in range(n)]
        tree = random_tree(rng, n)
        proj = [int(x) for x in rng.integers(0, 5, size=int(rng.integers(1, 4)))]
        out.append((i % TREE_TABLES, leaves, tree, proj, str(rng.choice(["none", "one", "half", "total", "total + 7"]))))
    return tables, out


def tree_fits_table(terms):
    """the tile form's rules on a normal form (native.expr_normalize): what imm3_query_create_table_expr takes"""
    preds = [p for term in terms for p in term]
    lists = [p.get("match", p.get("not_match")) for p in preds if "lo" not in p]
    return len(terms) <= 8 and all(p["col"] != NAME for p in preds) and all(len(v) <= 8 for v in lists) and len({p["col"] for p in preds}) <= 3


def has_or_or_not(tree):
    return not isinstance(tree, int) and (tree[0] != "and" or any(has_or_or_not(x) for x in tree[1:]))


def tree_is_refused(t, tree, terms):
    """does imm3_query_create_table_expr refuse this tree over this table?  A program without OR and NOT is a flat select list (every
    route of a flat table query is open to it), and a table without a single batch folds nothing."""
    return has_or_or_not(tree) and any(t.layouts) and not tree_fits_table(terms)


def tree_keep(t, leaves, tree):
    """per segment the words of the tree's bitmap, and bool over all rows of the table"""
    words, keep = [], []
    for cols in t.segs:
        masks = expected_masks(cols, leaves, tree)
        words.append(words_of_masks(masks))
        keep.append(np.concatenate(masks) if masks else np.zeros(0, bool))
    return words, (np.concatenate(keep) if keep else np.zeros(0, bool))


# ---- the cases of every seed ----------------------------------------------------------------------------------------------------
def select_cases(seed):
    """the tables of one seed of test_fuzz_table_select_project, each with its flat queries"""
    rng = np.random.default_rng(31_000 + seed)
    for _ in range(SELECT_TABLES):
        t = random_table(rng)
        yield t, [random_flat_query(rng, t) for _ in range(SELECT_QUERIES)]


def group_cases(seed):
    rng = np.random.default_rng(47_000 + seed)
    for _ in range(GROUP_TABLES):
        t = random_table(rng)
        yield t, [random_agg_query(rng, t) for _ in range(GROUP_QUERIES)]


def limit_rng(seed):
    return np.random.default_rng(59_000 + seed)
