"""The generator and the reference side of the order fuzzers (test_gpu_fuzz_order.py, test_order_fuzz_host.py): table_fuzz_util's random
tables with a sixth column `note` (a string of 3, 5, 20 or 32 bytes that can ride in a SELECT list, and be a key when it is narrow),
ordered flat queries, ordered select trees and ordered aggregations over them, and what the oracles say.  Pure numpy and the CPU
oracles: nothing here touches a device, and the library is never asked what the answer is.

Rows: table_fuzz_util.Expected's survivors in (segment, row) order, cut by str_range_util.in_range where the query carries an
IMM3_STR_RANGE leaf, then order_util.normalised_keys and order_util.order_permutation.  Groups: table_fuzz_util.expected_groups, then a
normalised key written here from Python ints and bytes by the table of include/imm3.h (group_key_bytes), then numpy.lexsort.

Every generator of table_fuzz_util is called as it is, with generators of this file's own seed bases; whatever is new (the note
column, the ties, the range leaf, keys, limits, reservations) draws from a second generator per seed."""
import numpy as np

from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, GT, RawColumn, SnappyColumn
from immutable3_amd import native
import order_util
import str_range_util
import table_fuzz_util as U
from table_fuzz_util import AGE, ID, NAME, STATE, V

NOTE = 5
NOTE_WIDTHS = [3, 5, 20, 32]
VALUE_CODECS = [DENSE_INT, DENSE_INT, DENSE_TINYINT, DENSE_STRING, DENSE_STRING, DENSE_STRING]
COLUMN_NAMES = U.COLUMN_NAMES + ["note"]
ROW_LIMIT_KINDS = ["none", "one", "T // 4", "T // 4 + 1", "T - 1", "T", "T + 7"]
GROUP_LIMIT_KINDS = ["none", "one", "g // 4", "g // 4 + 1", "g", "g + 7"]
RESERVES = ["none", "none", "ten", "rows + 8"]
G_COL, G_AGG = native.GROUP_ORDER_GROUP_COL, native.GROUP_ORDER_AGG
KEY_MAX = native.GROUP_ORDER_KEY_MAX_WIDTH

# seeds of the GPU fuzzers (test_gpu_fuzz_order.py) -- the census (test_order_fuzz_host.py) walks the same.  The bases were chosen on the
# CPU so that the reference side alone meets the census: the counts it pins are stated there.
ROW_SEEDS, ROW_TABLES, ROW_QUERIES = 48, 1, 3
ROW_BASE, ROW_EXTRA_BASE = 107_000, 109_000
BIG_EVERY, BIG_AT = 16, 5                           # seeds with seed % BIG_EVERY == BIG_AT open with a table of 20,000-row segments
GROUP_SEEDS, GROUP_TABLES, GROUP_QUERIES = 32, 1, 3
GROUP_MAX_ROWS = 12 * 1024                          # the reference side walks every group in Python: tables above this are drawn again
GROUP_BASE, GROUP_EXTRA_BASE = 151_000, 157_000
ORDER_TREE_SEED, ORDER_TREE_TABLES, ORDER_TREE_COUNT = 20261207, 3, 24


# ---- tables ---------------------------------------------------------------------------------------------------------------------
def note_pool(x, w):
    """a few dozen distinct values of w bytes on both sides of 0x80; half of them share all but their last two bytes (a wide note:
    its first 16 bytes and more), so the bytes behind the first chunk are what tells them apart"""
    k = int(x.integers(24, 48))
    pool = x.integers(0, 256, size=(k, w)).astype(np.uint8)
    pool[: k // 2, : max(1, w - 2)] = pool[0, : max(1, w - 2)]
    pool[k // 2, 0], pool[k // 2 + 1, 0] = 0x7F, 0x80
    return np.unique(pool, axis=0)


def extend_table(t, x, few):
    """the sixth column, and (few) v and age drawn from three values each so that ties decide; the columns touched are built again"""
    w = int(x.choice(NOTE_WIDTHS))
    pool = note_pool(x, w)
    note = pool[x.integers(0, pool.shape[0], size=t.n_rows)].reshape(t.n_rows, w).copy()
    biggest = max([max(br) for br in t.layouts if br], default=0)
    codec = U.SNAPPY if (x.random() < 0.4 and biggest * w <= U.SNAPPY_MAX_BLOCK_BYTES) else U.DENSE
    t.few = bool(few)
    if few:
        vs = x.choice(np.arange(-40, 40), size=3, replace=False).astype(np.int32)
        ages = np.array([-int(x.integers(1, 129)), int(x.integers(0, 50)), int(x.integers(50, 128))], np.int8)
        t.data[V] = vs[x.integers(0, 3, size=t.n_rows)]
        t.data[AGE] = ages[x.integers(0, 3, size=t.n_rows)]
    t.note_width, t.note_pool = w, pool
    t.widths = t.widths + [w]
    t.codecs = t.codecs + [codec]
    t.data = t.data + [note]
    for si, cols in enumerate(t.segs):
        lo, hi = int(t.starts[si]), int(t.starts[si + 1])
        if few:
            for c in (V, AGE):
                cols[c] = U.make_column(c, t.codecs[c], t.data[c][lo:hi], t.layouts[si], t.widths[c])
        make = SnappyColumn if codec == U.SNAPPY else RawColumn
        cols.append(make(DENSE_STRING, w, note[lo:hi], t.layouts[si]))
    return t


def big_table(rng, x):
    """four 20,000-row segments around an empty or a one-row one, sometimes a short one behind: with a predicate of selectivity 1 the
    order walks several steps per wave (more than 65,536 survivors)"""
    rows = [20_000, 20_000, int(x.choice([0, 1])), 20_000, 20_000] + ([int(x.choice([100, 1025]))] if x.random() < 0.5 else [])
    return U.FuzzTable(rng, rows, [U.table_layout(rng, n) for n in rows])


def describe(t):
    d = t.describe()
    d["note"], d["few"] = t.note_width, t.few
    return d


def is_mixed(t):
    return any(len(set(br[:-1])) > 1 for br in t.layouts if br)


# ---- order keys -----------------------------------------------------------------------------------------------------------------
def key_sets(t, n_keys):
    """column sets that make four keys, or exactly sixteen key bytes, on this table"""
    nw, mw = t.note_width, t.name_width
    if n_keys == 4:
        sets = [[ID, V, AGE, STATE]]
        if nw <= 5:
            sets += [[NOTE, ID, AGE, STATE], [V, AGE, STATE, NOTE]]
        if mw == 8:
            sets += [[NAME, AGE, STATE, ID]]
        return sets
    if mw == 16:
        return [[NAME]]
    return [[NAME, ID, V]] + ([[NOTE, NAME, STATE, AGE]] if nw == 5 else []) + ([[NOTE, NAME, ID, AGE]] if nw == 3 else [])


def draw_order(x, t, used, proj, at):
    """1 to 4 distinct SELECT-list entries of at most 16 bytes together, a direction each; a column a chosen shape needs is appended to
    the SELECT list (at(c): the place of table column c in `used`, added there when missing)"""
    def width(i):
        return t.widths[used[proj[i]]]

    def entry_of(c):
        have = [i for i in range(len(proj)) if used[proj[i]] == c]
        if have:
            return have[int(x.integers(0, len(have)))]
        proj.append(at(c))
        return len(proj) - 1

    shape = str(x.choice(["one", "four", "sixteen", "any", "any"]))
    picked = []
    if shape in ("four", "sixteen"):
        sets = key_sets(t, 4 if shape == "four" else 0)
        cols = sets[int(x.integers(0, len(sets)))]
        picked = [entry_of(c) for c in [cols[int(i)] for i in x.permutation(len(cols))]]
    elif shape == "any":
        total = 0
        for i in x.permutation(len(proj)):
            i = int(i)
            if len(picked) < 4 and total + width(i) <= 16 and (not picked or x.random() < 0.6):
                picked.append(i)
                total += width(i)
    if not picked:
        fits = [i for i in range(len(proj)) if width(i) <= 16]
        picked = [fits[int(x.integers(0, len(fits)))] if fits else entry_of(int(x.choice([ID, V, AGE, STATE])))]
    assert len(set(picked)) == len(picked) and sum(width(i) for i in picked) <= 16
    return [(i, bool(x.random() < 0.5)) for i in picked]


def range_bounds(x, t, c):
    """the bounds of an IMM3_STR_RANGE leaf on column c: full width, short, a prefix, or empty on one side (str_range_util.pad says
    what a short bound means)"""
    w = t.widths[c]
    pool = t.note_pool if c == NOTE else t.pool
    a, b = (bytes(pool[int(i)]) for i in x.integers(0, pool.shape[0], size=2))
    k1, k2 = (int(k) for k in x.integers(1, w, size=2))
    how = int(x.integers(0, 5))
    if how == 0:
        return min(a, b), max(a, b)
    if how == 1:
        lo, hi = a[:k1], b[:k2]
        if str_range_util.pad(lo, hi, w)[0] > str_range_util.pad(lo, hi, w)[1]:
            lo, hi = b[:k1], a[:k2]
        return lo, hi
    if how == 2:
        return a[:k1], a[:k1]
    return (a[:k1], b"") if how == 3 else (b"", b[:k2])


def range_mask(values, lo, hi):
    """str_range_util.in_range over the distinct values, spread back over the rows"""
    if values.shape[0] == 0:
        return np.zeros(0, bool)
    uniq, inv = np.unique(values, axis=0, return_inverse=True)
    return str_range_util.in_range(uniq, lo, hi)[np.asarray(inv).reshape(-1)]


# ---- ordered flat queries -------------------------------------------------------------------------------------------------------
class OrderedQuery:
    """sels: the whole conjunction; base_sels: what the C oracle answers; ranges: [(used index, (lo, hi))], answered by in_range"""

    def __init__(self, used, base_sels, ranges, proj, order_by, limit_kind, reserve):
        self.used, self.base_sels, self.ranges, self.proj, self.order_by = used, base_sels, ranges, proj, order_by
        self.limit_kind, self.reserve = limit_kind, reserve
        self.sels = base_sels + [(j, native.STR_RANGE, bounds) for j, bounds in ranges]

    def describe(self):
        return {"used": self.used, "sels": self.sels, "proj": self.proj, "order": self.order_by, "limit": self.limit_kind, "reserve": self.reserve}


def ordered_flat_query(rng, x, t, all_rows=False):
    """random_flat_query's used columns, predicates (thinned) and SELECT list (made non-empty, usually with the note in it); one query in four
    carries a range leaf on name or note -- a table takes a range only on a width that is a multiple of 4 (include/imm3.h), so a
    3- or 5-byte note never gets one; then keys, a limit kind and a reservation.  all_rows: one predicate of selectivity 1."""
    fq = U.random_flat_query(rng, t)
    used, sels, proj = list(fq.used), list(fq.sels), list(fq.proj)

    def at(c):
        if c not in used:
            used.append(c)
        return used.index(c)

    # a conjunction of up to ten random predicates selects no row more often than not, and an order over nothing tests nothing: most
    # queries keep only some of the predicates drawn (the census caps the share of empty results)
    n_kept = min(len(sels), int(x.choice([0, 0, 0, 1, 1, 2, 10])))
    sels = [sels[int(i)] for i in sorted(x.permutation(len(sels))[:n_kept])]
    if all_rows:
        sels = [(at(V), GT, -1000.0)]
    if not proj:
        proj = [int(x.integers(0, len(used)))]
    if x.random() < 0.75:
        proj.insert(int(x.integers(0, len(proj) + 1)), at(NOTE))
    ranges = []
    if x.random() < 0.25 and not all_rows:
        c = NOTE if (t.note_width % 4 == 0 and x.random() < 0.5) else NAME
        ranges.append((at(c), range_bounds(x, t, c)))
    order_by = draw_order(x, t, used, proj, at)
    kind = ROW_LIMIT_KINDS[int(x.integers(0, len(ROW_LIMIT_KINDS)))]
    reserve = {"none": None, "ten": 10, "rows + 8": t.n_rows + 8}[RESERVES[int(x.integers(0, len(RESERVES)))]]
    return OrderedQuery(used, sels, ranges, proj, order_by, kind, reserve)


def row_limit(kind, T):
    """the limit a kind names over T survivors (0: no limit): T // 4 still takes the select (T >= 4 x limit), T // 4 + 1 sorts all"""
    return {"none": 0, "one": 1, "T // 4": max(1, T // 4), "T // 4 + 1": T // 4 + 1, "T - 1": max(1, T - 1), "T": max(1, T), "T + 7": T + 7}[kind]


def group_limit(kind, g):
    return {"none": 0, "one": 1, "g // 4": max(1, g // 4), "g // 4 + 1": g // 4 + 1, "g": max(1, g), "g + 7": g + 7}[kind]


class Survivors:
    """the unordered result -- (segment, row) ascending, the bytes of every SELECT-list column -- and its orders"""

    def __init__(self, t, proj_cols, seg, row, vals):
        self.seg, self.row, self.vals, self.total = seg, row, vals, int(seg.size)
        self.codecs = [VALUE_CODECS[c] for c in proj_cols]
        self.n_segs = len(t.seg_rows)

    def keys(self, order_by):
        return order_util.normalised_keys(self.vals, self.codecs, order_by)

    def ordered(self, order_by, limit=0):
        perm = order_util.order_permutation(self.keys(order_by), limit)
        return self.seg[perm], self.row[perm], [v[perm] for v in self.vals]

    def parts(self, global_of):
        """per segment (its global index, rows, values): what order_util.merge_ordered takes"""
        out = []
        for si in range(self.n_segs):
            m = self.seg == si
            out.append((int(global_of[si]), self.row[m], [v[m] for v in self.vals]))
        return out


class RowExpected(Survivors):
    """an ordered flat query over a table: table_fuzz_util.Expected for the conjunction the C oracle knows, its survivors cut by
    in_range for a range leaf; per_seg and layouts as Expected has them (what check_select and the batch getters are held to)"""

    def __init__(self, oracle, t, q):
        e = U.Expected(oracle, t, q.used, q.base_sels, q.proj)
        self.layouts = e.layouts
        keep = e.keep(t)
        for j, (lo, hi) in q.ranges:
            keep &= range_mask(t.data[q.used[j]], lo, hi)
        self.per_seg = []
        for si, (size, _, _) in enumerate(e.layouts):
            words = str_range_util.bitmap_words(keep[t.starts[si]: t.starts[si + 1]], [int(n) for n in size])
            if not q.ranges:
                assert words.tolist() == np.asarray(e.per_seg[si][0]).tolist(), si       # (the oracle's own words, spelled again)
            self.per_seg.append((words, int(keep[t.starts[si]: t.starts[si + 1]].sum())))
        on = keep[t.starts[e.seg] + e.row]
        Survivors.__init__(self, t, [q.used[j] for j in q.proj], e.seg[on], e.row[on], [np.ascontiguousarray(v[on]) for v in e.vals])
        where = t.starts[self.seg] + self.row
        for j, pj in enumerate(q.proj):                                                  # the note's bytes: numpy's own data at the oracle's rows
            assert self.vals[j].tobytes() == t.value_bytes(q.used[pj], where).tobytes()


def row_cases(seed):
    """the tables of one seed of the row fuzzers, each with its ordered flat queries"""
    rng, x = np.random.default_rng(ROW_BASE + seed), np.random.default_rng(ROW_EXTRA_BASE + seed)
    for ti in range(ROW_TABLES):
        big = seed % BIG_EVERY == BIG_AT and ti == 0
        t = extend_table(big_table(rng, x) if big else U.random_table(rng), x, few=(seed + ti) % 2 == 1)
        yield t, [ordered_flat_query(rng, x, t, all_rows=big and qi == 0) for qi in range(ROW_QUERIES)]


# ---- ordered trees --------------------------------------------------------------------------------------------------------------
def ordered_tree_cases():
    """[(table index, leaves, tree, proj, order_by, limit kind)]: trees as table_fuzz_util.tree_cases draws them, over the five
    original columns; all six columns used in order, so a SELECT-list entry is a table column"""
    rng, x = np.random.default_rng(ORDER_TREE_SEED), np.random.default_rng(ORDER_TREE_SEED + 1)
    tables = [extend_table(U.random_table(rng), x, few=i % 2 == 1) for i in range(ORDER_TREE_TABLES)]
    used = list(range(6))
    out = []
    for i in range(ORDER_TREE_COUNT):
        t = tables[i % ORDER_TREE_TABLES]
        n = int(rng.integers(2, 6))
        leaves = [U.tree_leaf(rng, t) for _ in range(n)]
        tree = U.random_tree(rng, n)
        proj = [int(c) for c in x.integers(0, 6, size=int(x.integers(1, 4)))]
        order_by = draw_order(x, t, used, proj, lambda c: c)
        out.append((i % ORDER_TREE_TABLES, leaves, tree, proj, order_by, ROW_LIMIT_KINDS[int(x.integers(0, len(ROW_LIMIT_KINDS)))]))
    return tables, out


def tree_survivors(t, leaves, tree, proj):
    """-> (per-segment bitmap words, Survivors): expr_not_util.expected_masks per segment, the bytes from numpy's view of the table"""
    words, keep = U.tree_keep(t, leaves, tree)
    rows = np.flatnonzero(keep)
    seg = np.repeat(np.arange(len(t.seg_rows)), t.seg_rows)[rows].astype(np.int64)
    return words, Survivors(t, proj, seg, rows - t.starts[seg], [t.value_bytes(c, rows) for c in proj])


def tree_prediction(t, leaves, tree):
    """does the table refuse the tree?  (imm3_expr_normalize tells the form without a device)"""
    return U.tree_is_refused(t, tree, native.expr_normalize(VALUE_CODECS, t.widths, leaves, U.postfix(tree)))


# ---- ordered aggregations -------------------------------------------------------------------------------------------------------
class OrderedAgg:
    def __init__(self, aq, order, kinds, limit_kind):
        self.aq, self.order, self.kinds, self.limit_kind = aq, order, kinds, limit_kind

    def describe(self):
        return {"used": self.aq.used, "sels": self.aq.sels, "group": self.aq.group, "aggs": self.aq.aggs, "wide": self.aq.wide_keys,
                "order": self.order, "limit": self.limit_kind}


def group_key_candidates(t, aq):
    """[(kind, index, normalised width, what)] by the rules of imm3_query_set_group_order: a key of at most 12 bytes"""
    out = []
    for gi, j in enumerate(aq.group):
        c = aq.used[j]
        out.append((G_COL, gi, t.widths[c], "group " + ("int32" if c in (ID, V) else "int8" if c == AGE else "string")))
    for ai, (kind, j) in enumerate(aq.aggs):
        c = aq.used[j]
        if kind == "count":
            out.append((G_AGG, ai, 5, "count"))
        elif kind == "sum":
            out.append((G_AGG, ai, 8, "sum"))
        elif c in (STATE, NAME):
            out.append((G_AGG, ai, t.widths[c], "string max"))
        else:
            out.append((G_AGG, ai, t.widths[c], "int " + kind))
    return [k for k in out if k[2] <= KEY_MAX]


def ordered_agg_query(rng, x, t):
    """random_agg_query; one in three groups by id alone (every row its own group: past the small launch's 2048); 1 to 4 order keys
    whose widths and the 4 bytes of first_row sum to at most 16"""
    aq = U.random_agg_query(rng, t)
    if x.random() < 1 / 3:
        aq.group, aq.wide_keys = [aq.used.index(ID)], bool(x.random() < 0.3)
    elif not aq.group and x.random() < 0.9:                                  # one group, or none, orders nothing: most of those get a column
        aq.group = [aq.used.index(int(x.choice([AGE, STATE, V])))]
    thin = x.random()                                                        # (a long conjunction mostly selects no row: most are cut)
    aq.sels = [] if thin < 0.4 else aq.sels[:1] if thin < 0.8 else aq.sels
    cands = group_key_candidates(t, aq)
    if not cands:                                                            # (a 16-byte name as the only group column and the only maximum)
        aq.aggs[-1] = ("count", aq.aggs[-1][1])
        cands = group_key_candidates(t, aq)
    want, order, kinds, total = int(x.integers(1, 5)), [], [], 0
    if x.random() < 0.3:                                                     # `order by count desc limit k`, the query the feature is for, leads
        if not any(c[3] == "count" for c in cands):
            aq.aggs = (aq.aggs + [("count", aq.aggs[0][1])]) if len(aq.aggs) < 4 else (aq.aggs[:-1] + [("count", aq.aggs[-1][1])])
            cands = group_key_candidates(t, aq)
        kind, index, total, what = next(c for c in cands if c[3] == "count")
        order.append((kind, index, bool(x.random() < 0.7)))
        kinds.append(what)
    for i in x.permutation(len(cands)):
        kind, index, w, what = cands[int(i)]
        if (kind, index) not in [(k, j) for k, j, _ in order] and len(order) < want and total + w <= KEY_MAX:
            order.append((kind, index, bool(x.random() < 0.5)))
            kinds.append(what)
            total += w
    assert order and total + 4 <= 16
    return OrderedAgg(aq, order, kinds, GROUP_LIMIT_KINDS[int(x.integers(0, len(GROUP_LIMIT_KINDS)))])


def flip(b, descending):
    return bytes(255 - v for v in b) if descending else b


def group_key_bytes(t, aq, groups, order):
    """uint8[g, user key bytes + 4]: the normalised key of every group of expected_groups' result, from Python ints and bytes by the
    table in include/imm3.h: a count 5 big-endian bytes, a sum 8 with the sign bit flipped, int32 and int8 sign-flipped, strings as
    they are, a descending key complemented; the first-seen rank last, never complemented"""
    keys, _, counts, vals = groups
    offs = np.concatenate([[0], np.cumsum([t.widths[aq.used[j]] for j in aq.group])]).astype(int)
    rows = []
    for g in range(len(counts)):
        out = b""
        for kind, index, desc in order:
            if kind == G_COL:
                c = aq.used[aq.group[index]]
                raw = bytes(keys[g, offs[index]: offs[index + 1]])
                value = raw if c in (STATE, NAME) else int.from_bytes(raw, "little", signed=True)
            else:
                akind, j = aq.aggs[index]
                c, value = aq.used[j], vals[g][index]
            if kind == G_AGG and akind == "count":
                part = int(value).to_bytes(5, "big")
            elif kind == G_AGG and akind == "sum":
                part = (int(value) + (1 << 63)).to_bytes(8, "big")
            elif isinstance(value, bytes):
                part = value
            elif c == AGE:
                part = (int(value) + 128).to_bytes(1, "big")
            else:
                part = (int(value) + (1 << 31)).to_bytes(4, "big")
            out += flip(part, desc)
        rows.append(out + g.to_bytes(4, "big"))
    widths = {(k, i): w for k, i, w, _ in group_key_candidates(t, aq)}
    width = sum(widths[(k, i)] for k, i, _ in order) + 4
    assert all(len(r) == width for r in rows)
    return np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), width).copy()


def lex_perm(nk, limit=0):
    perm = np.lexsort(tuple(nk[:, b] for b in range(nk.shape[1] - 1, -1, -1))) if nk.shape[0] else np.arange(0)
    return perm[:limit] if limit > 0 else perm


def groups_result(t, aq, groups, perm):
    """the groups at `perm` as the four getters give them: (prefix keys uint64, first rows of the whole table, counts, vals int64[g, aggs]
    -- a string maximum as its first 8 bytes big-endian --, {aggregate: uint8[g, width]}, key bytes uint8[g, kb])"""
    keys, first, counts, vals = groups
    g, na = len(counts), len(aq.aggs)
    prefix = np.array([int.from_bytes(bytes(kb[:8]), "little") for kb in keys], np.uint64).reshape(g)
    v = np.zeros((g, na), np.uint64)
    strs = {}
    for j, (kind, cj) in enumerate(aq.aggs):
        col = [vals[i][j] for i in range(g)]
        if kind != "count" and aq.used[cj] in (STATE, NAME):
            v[:, j] = [int.from_bytes(s[:8], "big") for s in col] if g else []
            strs[j] = np.frombuffer(b"".join(col), np.uint8).reshape(g, t.widths[aq.used[cj]])
        else:
            v[:, j] = np.array([int(a) for a in col], np.int64).view(np.uint64) if g else []
    return prefix[perm], np.asarray(first, np.int64)[perm], np.array(counts, np.uint64).reshape(g)[perm], v.view(np.int64)[perm], {j: s[perm] for j, s in strs.items()}, np.asarray(keys)[perm]


def group_cases(seed):
    rng, x = np.random.default_rng(GROUP_BASE + seed), np.random.default_rng(GROUP_EXTRA_BASE + seed)
    for ti in range(GROUP_TABLES):
        t = U.random_table(rng)
        while t.n_rows > GROUP_MAX_ROWS:
            t = U.random_table(rng)
        t = extend_table(t, x, few=(seed + ti) % 2 == 1)
        yield t, [ordered_agg_query(rng, x, t) for _ in range(GROUP_QUERIES)]
