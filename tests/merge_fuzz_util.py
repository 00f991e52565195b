"""The generator and the reference side of the group-merge fuzzers (test_gpu_merge_fuzz.py, test_gpu_merge_fuzz_loopback.py,
test_merge_fuzz_host.py): table_fuzz_util's random tables and aggregations, dealt out as one aggregation query per segment to the merges
of group tables (imm3_comm_merge_groups, _merge_groups_wide and their _all flavours), and what plain numpy says the merged table is.
Pure numpy and the CPU oracles: nothing here touches a device, and the library is never asked what the answer is.

A case is a table, an aggregation and a DEAL: per segment a global segment index (identity or a permutation), the order the queries
are handed over in, an owner in {0, 1} per query, sometimes one more query over a segment whose predicate selects nothing, sometimes
one segment brought a second time under a further global index (its counts and sums double).  The reference runs
table_fuzz_util.expected_groups once per segment with `keep` cut to that segment and combines the lists with a plain dict in ascending
global index: counts and SUM add as Python ints, numeric MIN / MAX as signed ints, a string MAX as bytes, first = global << 32 | row,
output in ascending first.

The directed table of the all-ones key (OnesTable) has the same five columns, so the same reference serves it."""
import numpy as np

import table_fuzz_util as U
from conftest import GT, blocks_of
from table_fuzz_util import AGE, ID, NAME, STATE, V

# seeds of the GPU fuzzers -- the census (test_merge_fuzz_host.py) walks the same.  The bases were chosen on the CPU so that the
# reference side alone meets the census: the counts it pins are stated there.
SEEDS, TABLES, QUERIES = 24, 2, 3
BASE, EXTRA_BASE = 211_000, 223_000
MAX_ROWS = 12 * 1024                                # the reference walks every group in Python (order_fuzz_util.GROUP_MAX_ROWS)
# (seed, table, query) of the cases the two-rank worker walks: the direct table, the hash list and the byte-key records, a rank
# whose queries have no group on each of the three, more than 2048 groups, a doubled segment, an extra empty query
LOOPBACK_CASES = [(0, 1, 2), (1, 1, 1), (2, 0, 2), (7, 0, 0), (7, 1, 1), (10, 1, 2), (12, 1, 0), (14, 0, 2), (15, 0, 1)]
NOTHING_AGE = 127.0                                 # age is an int8: `age > 127` selects no row (a constant beyond int8 would wrap: the reference casts it)


class Entry:
    """one query of a deal: over segment `seg`, brought under global index `index` by `owner`; nothing: its predicate selects no row"""

    def __init__(self, seg, index, owner, nothing=False, doubled=False):
        self.seg, self.index, self.owner, self.nothing, self.doubled = int(seg), int(index), int(owner), bool(nothing), bool(doubled)


class MergeCase:
    def __init__(self, aq, entries, passed, permuted):
        self.aq, self.entries, self.passed, self.permuted = aq, entries, passed, permuted

    def sels(self, e):
        """the predicates of entry e's query (the extra query's: one more that no row passes)"""
        return self.aq.sels + ([(self.aq.used.index(AGE), GT, NOTHING_AGE)] if e.nothing else [])

    def of_owner(self, r):
        """the entries rank / communicator r brings, in the order they are handed over"""
        return [i for i in self.passed if self.entries[i].owner == r]

    def describe(self):
        return {"used": self.aq.used, "sels": self.aq.sels, "group": self.aq.group, "aggs": self.aq.aggs, "wide": self.aq.wide_keys,
                "entries": [(e.seg, e.index, e.owner, e.nothing) for e in self.entries], "passed": self.passed}


# ---- queries and deals ----------------------------------------------------------------------------------------------------------
def merge_agg_query(rng, x, t):
    """random_agg_query with its predicates thinned as order_fuzz_util.ordered_agg_query thins them (a long conjunction mostly selects
    no row, and then at most one segment contributes); name a group column, and the maximum of name an aggregate, more often"""
    aq = U.random_agg_query(rng, t)
    thin = x.random()
    aq.sels = [] if thin < 0.4 else aq.sels[:1] if thin < 0.8 else aq.sels
    at = {c: j for j, c in enumerate(aq.used)}
    more = x.random()
    if more < 0.3 and at[NAME] not in aq.group:
        aq.group = ([at[NAME]] + aq.group[:1]) if more < 0.15 else [at[NAME]]
        aq.wide_keys = True
    if x.random() < 0.15:
        aq.aggs[-1] = ("max", at[NAME])
    return aq


def deal(x, t):
    """-> (entries, passed, permuted)"""
    n = len(t.seg_rows)
    extra = int(x.integers(0, n)) if x.random() < 0.3 else None
    with_rows = [si for si in range(n) if t.seg_rows[si] > 0]
    twice = with_rows[int(x.integers(0, len(with_rows)))] if x.random() < 0.3 else None
    total = n + (extra is not None) + (twice is not None)
    permuted = bool(x.random() < 0.5)
    index = [int(i) for i in x.permutation(total)] if permuted else list(range(total))
    if permuted and index == sorted(index):
        index.reverse()
    owners = [int(o) for o in x.integers(0, 2, size=total)]
    if len(set(owners)) == 1:
        owners[int(x.integers(0, total))] ^= 1
    entries = [Entry(si, index[si], owners[si]) for si in range(n)]
    if extra is not None:
        entries.append(Entry(extra, index[len(entries)], owners[len(entries)], nothing=True))
    if twice is not None:
        entries.append(Entry(twice, index[len(entries)], owners[len(entries)], doubled=True))
    return entries, [int(i) for i in x.permutation(total)], permuted


def random_merge_table(rng):
    """random_table, drawn again until at least two segments have rows and the reference can walk its groups"""
    while True:
        t = U.random_table(rng)
        if t.n_rows <= MAX_ROWS and sum(1 for r in t.seg_rows if r > 0) >= 2:
            return t


def merge_cases(seed):
    """the tables of one seed, each with its cases"""
    rng, x = np.random.default_rng(BASE + seed), np.random.default_rng(EXTRA_BASE + seed)
    for _ in range(TABLES):
        t = random_merge_table(rng)
        cases = []
        for _ in range(QUERIES):
            aq = merge_agg_query(rng, x, t)
            cases.append(MergeCase(aq, *deal(x, t)))
        yield t, cases


# ---- the reference --------------------------------------------------------------------------------------------------------------
def key_width(t, aq):
    return sum(t.widths[aq.used[j]] for j in aq.group)


def string_aggs(t, aq):
    """{aggregate: width} of the maxima over string columns"""
    return {j: t.widths[aq.used[c]] for j, (kind, c) in enumerate(aq.aggs) if kind != "count" and aq.used[c] in (STATE, NAME)}


def narrow_accepts(t, aq):
    """does imm3_comm_merge_groups take the query?  (include/imm3.h: no key and no string MAX wider than 8 bytes)"""
    return key_width(t, aq) <= 8 and all(w <= 8 for w in string_aggs(t, aq).values())


def segment_groups(t, aq, keep, si):
    """the groups of the query over segment si alone: [(key bytes, first row in the segment, count, [value per aggregate])]"""
    lo, hi = int(t.starts[si]), int(t.starts[si + 1])
    cut = np.zeros(t.n_rows, bool)
    cut[lo:hi] = keep[lo:hi]
    keys, first, counts, vals = U.expected_groups(t, aq, cut)
    return [(bytes(keys[g]), int(first[g]) - lo, int(counts[g]), list(vals[g])) for g in range(len(counts))]


def combine(aq, parts):
    """parts: [(global index, segment_groups' list)] -> [(key bytes, first = global << 32 | row, count, values)] in ascending first"""
    table = {}
    for index, groups in sorted(parts, key=lambda p: p[0]):
        for key, row, count, vals in groups:
            first = (index << 32) | row
            cur = table.get(key)
            if cur is None:
                table[key] = [first, count, list(vals)]
                continue
            cur[0] = min(cur[0], first)
            cur[1] += count
            for j, (kind, _) in enumerate(aq.aggs):
                if kind in ("count", "sum"):
                    cur[2][j] += vals[j]
                elif kind == "max":
                    cur[2][j] = max(cur[2][j], vals[j])                       # (ints as signed ints, bytes as bytes)
                else:
                    cur[2][j] = min(cur[2][j], vals[j])
    return sorted(((k, e[0], e[1], e[2]) for k, e in table.items()), key=lambda g: g[1])


def as_arrays(t, aq, merged):
    """combine's list the way the merges return it: (key bytes uint8[g, kb], first uint64[g], counts uint64[g], vals int64[g, n_aggs] --
    a string MAX as its first 8 bytes big-endian --, {aggregate: uint8[g, width]} for every string MAX)"""
    g, kb, na = len(merged), key_width(t, aq), len(aq.aggs)
    keys = np.frombuffer(b"".join(m[0] for m in merged), np.uint8).reshape(g, kb).copy() if kb else np.zeros((g, 0), np.uint8)
    first = np.array([m[1] for m in merged], np.uint64).reshape(g)
    counts = np.array([m[2] for m in merged], np.uint64).reshape(g)
    vals = np.zeros((g, na), np.uint64)
    strs = {}
    sw = string_aggs(t, aq)
    for j in range(na):
        col = [m[3][j] for m in merged]
        if j in sw:
            vals[:, j] = [int.from_bytes(s[:8], "big") for s in col] if g else []
            strs[j] = np.frombuffer(b"".join(col), np.uint8).reshape(g, sw[j]).copy()
        else:
            vals[:, j] = np.array([int(a) for a in col], np.int64).view(np.uint64) if g else []
    return keys, first, counts, vals.view(np.int64), strs


def u64_keys(keys):
    """the u64 keys of the narrow merge: the first 8 key bytes little-endian"""
    return [int.from_bytes(bytes(k[:8]), "little") for k in keys]


def assert_narrow(got, want, what=None):
    """imm3_comm_merge_groups' (keys, first, counts, vals) against as_arrays' result"""
    keys, first, counts, vals = got[:4]
    wk, wf, wc, wv, _ = want
    assert keys.size == wk.shape[0], (what, keys.size, wk.shape[0])
    assert keys.tolist() == u64_keys(wk), what
    assert first.tolist() == wf.tolist() and counts.tolist() == wc.tolist() and vals.tolist() == wv.tolist(), what


class Reference:
    """per entry its groups (parts), the merged list and its arrays; per owner the merged list of what it brings alone"""

    def __init__(self, t, case, keep):
        self.keep, self.per_seg = keep, {}
        for e in case.entries:
            if not e.nothing and e.seg not in self.per_seg:
                self.per_seg[e.seg] = segment_groups(t, case.aq, keep, e.seg)
        self.parts = [(e.index, [] if e.nothing else self.per_seg[e.seg]) for e in case.entries]
        self.merged = combine(case.aq, self.parts)
        self.arrays = as_arrays(t, case.aq, self.merged)
        self.local = [combine(case.aq, [p for p, e in zip(self.parts, case.entries) if e.owner == r]) for r in range(2)]

    def prefix(self, n):
        k, f, c, v, s = self.arrays
        return k[:n], f[:n], c[:n], v[:n], {j: a[:n] for j, a in s.items()}


def reference(oracle, t, case):
    keep = U.Expected(oracle, t, case.aq.used, case.aq.sels, [0]).keep(t)
    for e in case.entries:                                                     # the extra query's predicates select nothing: the oracle's word
        assert not e.nothing or not U.Expected(oracle, t, case.aq.used, case.sels(e), [0]).keep(t).any()
    return Reference(t, case, keep)


def whole_table(t, aq, keep):
    """expected_groups over the whole table as combine spells a merge under identity indices: first = segment << 32 | row"""
    keys, first, counts, vals = U.expected_groups(t, aq, keep)
    seg = np.repeat(np.arange(len(t.seg_rows)), t.seg_rows)[first] if len(counts) else np.zeros(0, np.int64)
    return [(bytes(keys[g]), (int(seg[g]) << 32) | (int(first[g]) - int(t.starts[seg[g]])), int(counts[g]), list(vals[g])) for g in range(len(counts))]


def virtual_rows(t, seg, row):
    """the virtual row of (segment, row) in the imm3_table over all of t's segments: tile * 1024 + position (include/imm3.h)"""
    tile0 = np.concatenate([[0], np.cumsum(t.tiles)]).astype(np.int64)
    return tile0[np.asarray(seg, np.int64)] * 1024 + np.asarray(row, np.int64)


# ---- the all-ones key -----------------------------------------------------------------------------------------------------------
ONES_SIZES = [3000, 1025, 64, 1]
ONES = (-1, -1)                                     # group by id, v: eight 0xFF bytes, the free-slot marker of every u64 hash table
NEIGHBOURS = [(-1, -2), (-2, -1), (-1, 0)]
ONES_PAIRS = [ONES] + NEIGHBOURS + [(0, 0), (0, -1), (5, 7), (2 ** 31 - 1, -1), (-1, 2 ** 31 - 1), (-2 ** 31, -2 ** 31)]
ONES_NAME = b"\xff" * 8
ONES_NAMES = [ONES_NAME, b"\xff" * 7 + b"\xfe", b"\xfe" + b"\xff" * 7, b"\xff" * 7 + b"\x00", b"\x00" * 8, b"\x00" + b"\xff" * 7, b"plainnam",
              b"\xff\xff\xff\xff\x00\x00\x00\x00", b"\x00\x00\x00\x00\xff\xff\xff\xff", b"\xff\xff\xff\xff\xff\xff\xff\x7f"]
ONES_DEEP = 2500                                    # segment 0 holds the all-ones key from this row on only


class OnesTable(U.FuzzTable):
    """segments of 3000, 1025, 64 and 1 rows of [id, v, age, state, name(8)]: (id, v) walks ONES_PAIRS and name the matching entry of
    ONES_NAMES, so `group by id, v` and `group by name` are the same partition.  The all-ones key: deep inside segment 0 (from row
    ONES_DEEP on), from row 0 of segment 1, nowhere in segment 2, the one row of segment 3.  Dense columns, blocks of 1024."""

    def __init__(self, rng):
        self.seg_rows = list(ONES_SIZES)
        self.layouts = [blocks_of(n, 1024) for n in self.seg_rows]
        self.n_rows = sum(self.seg_rows)
        self.starts = np.concatenate([[0], np.cumsum(self.seg_rows)]).astype(np.int64)
        self.tiles = [-(-n // 1024) for n in self.seg_rows]
        self.name_width, self.widths, self.codecs, self.n_codes = 8, [4, 4, 1, 2, 8], [U.DENSE] * 5, 12
        picks = []
        for si, n in enumerate(self.seg_rows):
            p = rng.integers(1, len(ONES_PAIRS), size=n)                      # everything but the all-ones key ...
            if si == 0:
                p[ONES_DEEP:] = rng.integers(0, len(ONES_PAIRS), size=n - ONES_DEEP)
                p[ONES_DEEP] = 0
                p[:len(ONES_PAIRS) - 1] = np.arange(1, len(ONES_PAIRS))       # every other pair from the first rows on
            elif si == 1:
                p = rng.integers(0, len(ONES_PAIRS), size=n)
                p[0] = 0
                p[-1] = 0                                                     # (and in the one-row tile behind the full one)
            elif si == 3:
                p[:] = 0
            picks.append(p)
        pick = np.concatenate(picks)
        pairs = np.array(ONES_PAIRS, np.int64)
        names = np.array([list(b) for b in ONES_NAMES], np.uint8)
        n = self.n_rows
        self.pick = pick
        self.data = [pairs[pick, 0].astype(np.int32), pairs[pick, 1].astype(np.int32), rng.integers(-128, 128, size=n).astype(np.int8),
                     np.array([list(c) for c in U.CODES], np.uint8)[rng.integers(0, 12, size=n)].reshape(n, 2), names[pick].reshape(n, 8)]
        self.segs = []
        for si in range(len(self.seg_rows)):
            lo, hi = int(self.starts[si]), int(self.starts[si + 1])
            self.segs.append([U.make_column(c, U.DENSE, self.data[c][lo:hi], self.layouts[si], self.widths[c]) for c in range(5)])


ONES_USED = [ID, V, AGE, STATE, NAME]
ONES_AGGS = [[("count", AGE), ("min", AGE), ("sum", AGE), ("max", STATE)], [("max", AGE), ("sum", V), ("max", NAME), ("min", ID)]]
ONES_SELS = {"every row": [], "the all-ones key alone": [(ID, U.EQ, -1.0), (V, U.EQ, -1.0)], "the all-ones key removed": [(V, GT, -1.0)]}


def ones_queries():
    """[(what, AggQuery)]: group by (id, v) and by the 8-byte name, both through the narrow entry point, over every predicate"""
    out = []
    for what, sels in ONES_SELS.items():
        for group in ([ID, V], [NAME]):
            for aggs in ONES_AGGS:
                out.append(((what, group, aggs), U.AggQuery(list(ONES_USED), list(sels), list(group), list(aggs), False)))
    return out


def ones_keep(t, sels):
    """numpy's answer to the three predicates of ONES_SELS"""
    keep = np.ones(t.n_rows, bool)
    for c, cond, value in sels:
        keep &= (t.data[c] == int(value)) if cond == U.EQ else (t.data[c] > value)
    return keep
