"""CPU census of the group-merge fuzz (merge_fuzz_util.py, test_gpu_merge_fuzz.py, test_gpu_merge_fuzz_loopback.py): the generator and
the whole reference side run over every seed the GPU tests use, without a device.  It asserts that the fuzz is not hollow -- several
contributing segments, keys on both sides and on one side only, groups that arrive late, every key-width class and every path of the
deal really occur -- and holds the reference against itself: under identity indices the per-segment combine must be
table_fuzz_util.expected_groups over the whole table, group by group."""
import numpy as np
import pytest

import merge_fuzz_util as F
import table_fuzz_util as U

# what the chosen seed bases give, pinned so that a later change to a generator or a default cannot hollow the fuzz out unnoticed
CASES = F.SEEDS * F.TABLES * F.QUERIES


@pytest.fixture(scope="module")
def census(oracle):
    out = []
    for seed in range(F.SEEDS):
        for ti, (t, cases) in enumerate(F.merge_cases(seed)):
            for ci, case in enumerate(cases):
                ref = F.reference(oracle, t, case)
                out.append((seed, ti, ci, t, case, ref.keep, ref))
    return out


def test_tables_and_deals_are_what_the_generator_promises(census):
    assert len(census) == CASES
    for seed, ti, ci, t, case, keep, ref in census:
        what = (seed, ti, ci)
        assert t.n_rows <= F.MAX_ROWS and sum(1 for r in t.seg_rows if r > 0) >= 2, what
        assert all(U.layout_ok(br) and sum(br) == n for br, n in zip(t.layouts, t.seg_rows)), what
        n = len(t.seg_rows)
        idx = [e.index for e in case.entries]
        assert sorted(idx) == list(range(len(idx))) and sorted(case.passed) == list(range(len(idx))), what
        assert [e.seg for e in case.entries[:n]] == list(range(n)) and not any(e.nothing or e.doubled for e in case.entries[:n]), what
        assert {e.owner for e in case.entries} == {0, 1}, what
        assert sum(e.nothing for e in case.entries) <= 1 and sum(e.doubled for e in case.entries) <= 1, what
        assert case.permuted == (idx != sorted(idx)), what
        for e in case.entries:
            assert not e.doubled or t.seg_rows[e.seg] > 0, what
        assert 1 <= len(case.aq.aggs) <= 4 and len(case.aq.group) <= 2, what
        assert case.aq.wide_keys or F.key_width(t, case.aq) <= 8, what


def test_the_combine_is_expected_groups_over_the_whole_table(census):
    """identity indices and no doubled segment: group by group the whole table's answer; any indices: its keys, counts and values --
    the merge changes the order and `first`, nothing else; a doubled segment adds exactly its own counts once more"""
    identity = 0
    for seed, ti, ci, t, case, keep, ref in census:
        what = (seed, ti, ci)
        whole = F.whole_table(t, case.aq, keep)
        doubled = [e for e in case.entries if e.doubled]
        if not doubled:
            assert sorted(m[0] for m in ref.merged) == sorted(w[0] for w in whole), what
            assert {m[0]: (m[2], m[3]) for m in ref.merged} == {w[0]: (w[2], w[3]) for w in whole}, what
            if not case.permuted:
                assert ref.merged == whole, what
                identity += 1
        else:
            once = {w[0]: w[2] for w in whole}
            again = {k: c for k, _, c, _ in ref.per_seg[doubled[0].seg]}
            assert {m[0]: m[2] for m in ref.merged} == {k: c + again.get(k, 0) for k, c in once.items()}, what
        firsts = [m[1] for m in ref.merged]
        assert firsts == sorted(set(firsts)), what                              # strictly ascending: no two groups share a first row
        index_of = {e.index: e for e in case.entries}
        for key, first, count, vals in ref.merged:                              # first names a row of a segment that holds the key
            e = index_of[first >> 32]
            assert not e.nothing and (first & 0xFFFFFFFF) < t.seg_rows[e.seg], what
        k, f, c, v, s = ref.arrays
        assert k.shape == (len(ref.merged), F.key_width(t, case.aq)) and v.shape == (len(ref.merged), len(case.aq.aggs)), what
        assert sorted(s) == sorted(F.string_aggs(t, case.aq)), what
    assert identity >= CASES // 4


def test_the_census(census):
    N = len(census)
    n = dict.fromkeys(["empty", "shared", "late", "one-sided", "<= 2", "3 .. 8", "> 8", "wide max", "permuted", "extra", "doubled",
                       "lengths differ", "a rank without groups", "refused by the narrow merge", "exactly 8"], 0)
    kinds, most, mixed, codecs = set(), 0, 0, set()
    for seed, ti, ci, t, case, keep, ref in census:
        aq = case.aq
        holders = {}                                                            # key -> the segments that hold it
        for si, groups in ref.per_seg.items():
            for g in groups:
                holders.setdefault(g[0], set()).add(si)
        contributing = [si for si, groups in ref.per_seg.items() if groups]
        lowest = min([e.index for e in case.entries if not e.nothing and ref.per_seg[e.seg]], default=0)
        n["empty"] += not ref.merged
        n["shared"] += any(len(s) >= 2 for s in holders.values())
        n["late"] += any(m[1] >> 32 > lowest for m in ref.merged)
        n["one-sided"] += len(contributing) >= 2 and any(len(s) == 1 for s in holders.values())
        kb = F.key_width(t, aq)
        n["<= 2" if kb <= 2 else "3 .. 8" if kb <= 8 else "> 8"] += 1
        n["exactly 8"] += kb == 8
        n["wide max"] += any(w > 8 for w in F.string_aggs(t, aq).values())
        n["refused by the narrow merge"] += not F.narrow_accepts(t, aq)
        n["permuted"] += case.permuted
        n["extra"] += any(e.nothing for e in case.entries)
        n["doubled"] += any(e.doubled for e in case.entries)
        n["lengths differ"] += len(ref.local[0]) != len(ref.local[1])
        n["a rank without groups"] += bool(ref.merged) and (not ref.local[0] or not ref.local[1])
        kinds |= {k for k, _ in aq.aggs}
        most = max(most, len(ref.merged))
        mixed += any(len(set(br[:-1])) > 1 for br in t.layouts if br)
        codecs |= set(t.codecs)
        assert all(any(e.owner == r for e in case.entries) for r in range(2))
    print("merge fuzz census over %d cases: %s, most groups %d" % (N, n, most))
    assert 6 * n["empty"] <= N, n
    assert 3 * n["shared"] >= 2 * N, n
    assert 3 * n["late"] >= N, n
    assert 4 * n["one-sided"] >= N, n
    assert 4 * n["<= 2"] >= N and 4 * n["3 .. 8"] >= N and 8 * n["> 8"] >= N, n
    assert 8 * n["wide max"] >= N, n
    assert most > 2048, most
    assert kinds == {"count", "min", "max", "sum"}, kinds
    assert 5 * n["permuted"] >= N and 5 * n["extra"] >= N and 5 * n["doubled"] >= N, n
    assert 2 * n["lengths differ"] >= N, n
    assert n["a rank without groups"] >= 2, n
    assert n["refused by the narrow merge"] >= N // 8 and n["exactly 8"] >= 2, n
    assert mixed >= 4 and codecs == {U.DENSE, U.PFOR, U.SNAPPY}, (mixed, codecs)


def test_the_loopback_subset_is_not_hollow(census):
    """the cases the two-rank worker walks (LOOPBACK_CASES): per key-width class -- the direct table, the hash list, the byte-key records
    -- a rank whose queries have no group and a key that both ranks hold; lists of different lengths; more than 2048 groups in the
    hash list and in the records; a doubled segment and an extra empty query"""
    seen, walked = set(), 0
    for seed, ti, ci, t, case, keep, ref in census:
        if (seed, ti, ci) not in F.LOOPBACK_CASES:
            continue
        walked += 1
        kb = F.key_width(t, case.aq)
        path = "direct" if kb <= 2 else "hash" if F.narrow_accepts(t, case.aq) else "records"
        seen.add(path)
        assert ref.merged, (seed, ti, ci)
        if not ref.local[0] or not ref.local[1]:
            seen.add(path + ": a rank without groups")
        if {m[0] for m in ref.local[0]} & {m[0] for m in ref.local[1]}:
            seen.add(path + ": a key on both ranks")
        if len(ref.local[0]) != len(ref.local[1]):
            seen.add("lengths differ")
        if len(ref.merged) > 2048:
            seen.add(path + ": more than 2048 groups")
        if any(w > 8 for w in F.string_aggs(t, case.aq).values()):
            seen.add("a wide string MAX")
        seen |= {"permuted"} if case.permuted else set()
        seen |= {"doubled"} if any(e.doubled for e in case.entries) else set()
        seen |= {"extra"} if any(e.nothing for e in case.entries) else set()
    assert walked == len(F.LOOPBACK_CASES) == len(set(F.LOOPBACK_CASES))
    want = {p + s for p in ("direct", "hash", "records") for s in ("", ": a rank without groups", ": a key on both ranks")}
    assert seen >= want | {"lengths differ", "hash: more than 2048 groups", "records: more than 2048 groups", "a wide string MAX", "permuted", "doubled", "extra"}, seen


def test_the_all_ones_table(oracle):
    """the directed table holds what its tests are there for: the all-ones key deep inside segment 0, at row 0 of segment 1, not in
    segment 2, alone in segment 3; its neighbours everywhere; grouping by (id, v) and by name is one partition"""
    t = F.OnesTable(np.random.default_rng(7))
    ones = (t.data[U.ID] == -1) & (t.data[U.V] == -1)
    assert (t.data[U.NAME][ones] == 0xFF).all() and not (t.data[U.NAME][~ones] == 0xFF).all(axis=1).any()
    per = [np.flatnonzero(ones[t.starts[si]: t.starts[si + 1]]) for si in range(4)]
    assert per[0][0] == F.ONES_DEEP and per[1][0] == 0 and per[1][-1] == 1024 and per[2].size == 0 and per[3].tolist() == [0]
    for a, b in F.NEIGHBOURS:
        assert ((t.data[U.ID] == a) & (t.data[U.V] == b)).any()
    for what, aq in F.ones_queries():
        keep = F.ones_keep(t, aq.sels)
        assert np.array_equal(keep, U.Expected(oracle, t, aq.used, aq.sels, [0]).keep(t)), what    # (the oracle reads the predicates the same way)
        whole = F.whole_table(t, aq, keep)
        parts = [(si, F.segment_groups(t, aq, keep, si)) for si in range(4)]
        assert F.combine(aq, parts) == whole, what
        keys = [w[0] for w in whole]
        ones_key = b"\xff" * 8
        assert F.key_width(t, aq) == 8 and F.narrow_accepts(t, aq)
        if what[0] == "every row":
            assert len(keys) == len(F.ONES_PAIRS) and ones_key in keys and whole[keys.index(ones_key)][1] == F.ONES_DEEP, what
        elif what[0] == "the all-ones key alone":
            assert keys == [ones_key] and whole[0][2] == int(ones.sum()), what
        else:
            assert ones_key not in keys and len(keys) >= 3, what
    by_pair = F.whole_table(t, F.ones_queries()[0][1], np.ones(t.n_rows, bool))
    by_name = F.whole_table(t, F.ones_queries()[2][1], np.ones(t.n_rows, bool))
    assert [w[1:3] for w in by_pair] == [w[1:3] for w in by_name]
    assert F.virtual_rows(t, [0, 1, 2, 3], [5, 0, 63, 0]).tolist() == [5, 3 * 1024, 5 * 1024 + 63, 6 * 1024]
