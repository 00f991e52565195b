"""Shared by test_gpu_merge_wide.py and the two-rank worker of test_gpu_merge_wide_loopback.py: the expected result of a merge by byte
key, combined on the host from the queries' own getters (fetch_groups / fetch_group_keys / fetch_group_strings) with a plain dict, in
(segment, first row) order."""
import numpy as np

from immutable3_amd import native

C, MN, MX, S = native.AGG_COUNT, native.AGG_MIN, native.AGG_MAX, native.AGG_SUM
STRING_CODECS = (native.DENSE_STRING, native.SNAPPY_STRING)


def string_aggs(q):
    """indices of q's MAX over STRING aggregates"""
    return [j for j, (k, c) in enumerate(q.aggs) if k == MX and q.seg.codecs[q.used_cols[c]] in STRING_CODECS]


def host_combine(queries, segment_index):
    """(key bytes uint8[g, kb], first uint64[g], counts uint64[g], vals int64[g, n_aggs], {j: uint8[g, w]}) of the queries' groups
    merged by key: counts and SUM add, numeric MIN / MAX as signed integers, a string MAX by its bytes; first arrival first."""
    aggs = queries[0].aggs
    sj = string_aggs(queries[0])
    table = {}
    for s, q in sorted(zip(segment_index, queries), key=lambda sq: sq[0]):
        kb = q.fetch_group_keys()
        _, first, counts, vals = q.fetch_groups()
        strs = {j: q.fetch_group_strings(j) for j in sj}
        for g in range(kb.shape[0]):
            key = bytes(kb[g])
            f = (int(s) << 32) | int(first[g])
            v = [int(x) for x in vals[g]]
            st = {j: bytes(strs[j][g]) for j in sj}
            cur = table.get(key)
            if cur is None:
                table[key] = [f, int(counts[g]), v, st]
                continue
            cur[0] = min(cur[0], f)
            cur[1] += int(counts[g])
            for j, (k, _) in enumerate(aggs):
                if j in sj:
                    if st[j] > cur[3][j]:
                        cur[3][j] = st[j]
                        cur[2][j] = v[j]      # (the first 8 bytes big-endian: they move with the bytes)
                elif k == MX:
                    cur[2][j] = max(cur[2][j], v[j])
                elif k == MN:
                    cur[2][j] = min(cur[2][j], v[j])
                elif k == S:
                    cur[2][j] += v[j]
                else:
                    cur[2][j] = cur[1]
    n = len(table)
    kw = queries[0].fetch_group_keys().shape[1]
    keys = np.array([list(k) for k in table], np.uint8).reshape(n, kw)
    first = np.array([e[0] for e in table.values()], np.uint64)
    counts = np.array([e[1] for e in table.values()], np.uint64)
    vals = np.array([e[2] for e in table.values()], np.int64).reshape(n, len(aggs))
    widths = {j: queries[0].seg.widths[queries[0].used_cols[aggs[j][1]]] for j in sj}
    strs = {j: np.array([list(e[3][j]) for e in table.values()], np.uint8).reshape(n, widths[j]) for j in sj}
    return keys, first, counts, vals, strs


def assert_merged(got, want, what=None):
    keys, first, counts, vals, strs = got[:5]
    wk, wf, wc, wv, ws = want
    assert keys.shape == wk.shape and np.array_equal(keys, wk), what
    assert first.tolist() == wf.tolist(), what
    assert counts.tolist() == wc.tolist(), what
    assert vals.tolist() == wv.tolist(), what
    assert sorted(strs) == sorted(ws), what
    for j in ws:
        assert strs[j].shape == ws[j].shape and np.array_equal(strs[j], ws[j]), (what, j)
        pre = [int.from_bytes(bytes(r[:8]), "big") for r in ws[j]]          # vals[g, j]: the first 8 bytes big-endian
        assert [int(x) & (2 ** 64 - 1) for x in vals[:, j]] == pre, (what, j)


# ---- the segments of the wide-key cases: key = a 16-byte name + an int8 (17 bytes), a 16-byte string to take the MAX of ---------------
SIZES = [3000, 1025, 64, 1]
AGGS = [(C, 2), (MX, 2), (S, 2), (MX, 3)]      # COUNT, MAX(int32), SUM(int32), MAX(16-byte string)
GROUP = [0, 1]


def _name(text):
    return np.frombuffer(text.ljust(16, b".")[:16], np.uint8)


# (name, k8) pairs chosen to break a merge that compares less than the whole key
PAIR_8A = (_name(b"abcdefghXaaaaaaa"), 5)          # equal in the first 8 bytes ...
PAIR_8B = (_name(b"abcdefghYaaaaaaa"), 5)          # ... differ only in byte 9
PAIR_LAST1 = (_name(b"mmmmmmmmmmmmmmmm"), 1)       # differ only in the last (17th) byte
PAIR_LAST2 = (_name(b"mmmmmmmmmmmmmmmm"), 2)
PAIR_ZERO = (np.zeros(16, np.uint8), 0)            # the all-0x00 key
PAIR_ONES = (np.full(16, 255, np.uint8), -1)       # the all-0xFF key
PAIR_ONLY1 = (_name(b"only-in-segment1"), 7)       # present in segment 1 only
PAIR_FROM2 = (_name(b"first-in-segmt-2"), 7)       # first arrival in segment 2 (then segment 3's one row)
COMMON = [PAIR_8A, PAIR_8B, PAIR_LAST1, PAIR_LAST2, PAIR_ZERO, PAIR_ONES, (_name(b"plain"), 3), (_name(b"plain"), -3)]
POOLS = [COMMON, COMMON + [PAIR_ONLY1], COMMON[:5] + [PAIR_FROM2], [PAIR_FROM2]]


def breaker_columns(rng, seg):
    """columns of segment `seg`: 0 name (16-byte string), 1 k8 (int8), 2 val (int32), 3 sname (16-byte string: a shared 8-byte
    prefix, then random bytes).  Every pair of the segment's pool occurs: the first rows walk the pool."""
    from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, RawColumn, blocks_of
    n, pool = SIZES[seg], POOLS[seg]
    pick = np.concatenate([np.arange(len(pool)), rng.integers(0, len(pool), size=n)])[:n] if n >= len(pool) else np.zeros(n, np.int64)
    pick = rng.permutation(pick)
    names = np.stack([pool[i][0] for i in pick])
    k8 = np.array([pool[i][1] for i in pick], np.int8)
    sname = rng.integers(97, 123, size=(n, 16)).astype(np.uint8)
    sname[:, :8] = ord("p")
    br = blocks_of(n, 1024)
    return [RawColumn(DENSE_STRING, 16, names, br), RawColumn(DENSE_TINYINT, 1, k8, br),
            RawColumn(DENSE_INT, 4, rng.integers(-10 ** 6, 10 ** 6, size=n).astype(np.int32), br), RawColumn(DENSE_STRING, 16, sname, br)]


def pair_key(pair):
    return bytes(pair[0]) + int(pair[1]).to_bytes(1, "little", signed=True)
