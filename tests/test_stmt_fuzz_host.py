"""CPU census of the statement fuzz (stmt_fuzz_util.py, test_gpu_stmt_fuzz.py), and the parser twins over its statements.  The generator
and the whole reference side run over the default seed set without a device.  The census asserts that the fuzz is not hollow: every
clause, every documented launch decision and every edge of the merges occurs often enough, by the reference's own account.  Every
statement the grammar can spell goes through sql.py and through imm3_sql --parse-only, which must read it as the same ADT and the same
used-column order; and the reference is held against a second witness, numpy over whole columns.

What the default seeds (16 seeds of 10 statements) give, pinned in COUNTS below so that a later change to the generator cannot hollow
the fuzz out unnoticed:
    statements: 160
    either: 1
    spellable: 79
    errors: 16
    honoured or: 15
    or run as and, differing: 10
    notmatch: 28
    in-list > 8: 28
    range on name: 11
    range on tag: 12
    first key ties across segments: 39
    limit below kept: 49
    limit above kept: 33
    zero survivors: 26
    all rows survive: 9
    having keeps none: 16
    having keeps all: 12
    group first seen in the last segment: 32
    0 groups: 10
    1 group: 15
    > 100 groups: 17
    table: 99
    segments: 44
    keyword-prefixed column: 64
    names compared as bytes: 24
(table / segments / either: predict_path over blocks of 1024; the error class has no path.)
"""
import os
import subprocess
from dataclasses import replace

import pytest

import stmt_fuzz_util as F
from immutable3_amd.sql import SQLParser

SQL = os.path.join(F.BIN, "imm3_sql")
ALL_FLAGS = {"order_by": True, "string_ranges": True, "group_order": True, "having": True}
CLI_FLAGS = ("--order-by", "--string-ranges", "--having")
MAX_PARSED = 150

COUNTS = {"statements": 160, "either": 1, "spellable": 79, "errors": 16, "honoured or": 15, "or run as and, differing": 10, "notmatch": 28,
          "in-list > 8": 28, "range on name": 11, "range on tag": 12, "first key ties across segments": 39, "limit below kept": 49,
          "limit above kept": 33, "zero survivors": 26, "all rows survive": 9, "having keeps none": 16, "having keeps all": 12,
          "group first seen in the last segment": 32, "0 groups": 10, "1 group": 15, "> 100 groups": 17, "table": 99, "segments": 44,
          "keyword-prefixed column": 64, "names compared as bytes": 24}


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    return F.make_tables(tmp_path_factory.mktemp("stmt_fuzz_host"))


@pytest.fixture(scope="module")
def census(tables):
    """[(seed, index, statement, keep mask or None, expected or None)] over the default seeds"""
    rows, _, _ = tables
    data = F.Data(rows)
    out = []
    for seed in range(F.SEEDS):
        for i, s in enumerate(F.statements(seed, data)):
            try:
                keep = F.keep_mask(rows, s)
                want = F.expected(rows, s, keep)
            except F.Refused:
                keep = want = None
            out.append((seed, i, s, keep, want))
    return out


def count_features(census, rows, seg_rows):
    """the census's counts, by the reference alone"""
    bounds = [sum(seg_rows[:k]) for k in range(1, len(seg_rows))]
    last = bounds[-1]

    def segment(i):
        return sum(i >= b for b in bounds)
    c = dict.fromkeys(("statements", "either", "spellable", "errors", "honoured or", "or run as and, differing", "notmatch", "in-list > 8",
                       "range on name", "range on tag", "first key ties across segments", "limit below kept", "limit above kept",
                       "zero survivors", "all rows survive", "having keeps none", "having keeps all", "group first seen in the last segment",
                       "0 groups", "1 group", "> 100 groups", "table", "segments", "keyword-prefixed column", "names compared as bytes"), 0)
    for (_, _, s, keep, want) in census:
        c["statements"] += 1
        c["spellable"] += F.render(s) is not None
        if s.error is not None:
            assert want is None, s
            c["errors"] += 1
            continue
        assert want is not None, s
        path = F.predict_path(s, 1024)
        c[path] += 1
        ls = F.leaves_of(s.where)
        c["keyword-prefixed column"] += "order_no" in F.used_columns(s)
        c["honoured or"] += bool(F.as_tree(s) and F.has_or(s.where))
        if F.has_or(s.where) and not F.as_tree(s):
            c["or run as and, differing"] += F.keep_mask(rows, replace(s, honour_and_or=True)) != keep if not any(l[2] in F.RANGE_OPS for l in ls) else \
                [F.tree_holds(s.where, r) for r in rows] != keep
        # the high-byte names decide something: an order key, a string maximum or a range bound on `name`, with such a name among the survivors
        by_name = ("name" in [n for (n, _) in s.order_by] or any(n in ("name_max", "name_min") for (n, _) in s.order_by) or
                   any(a in (("max", "name"), ("min", "name")) for a in s.aggs) or any(l[2] in F.RANGE_OPS and l[1] == "name" for l in ls))
        c["names compared as bytes"] += bool(by_name and any(k and not r["name"].isascii() for k, r in zip(keep, rows)))
        c["notmatch"] += any(l[2] == "notin" for l in ls)
        c["in-list > 8"] += any(l[2] in ("in", "notin") and len(l[3]) > 8 for l in ls)
        c["range on name"] += any(l[2] in F.RANGE_OPS and l[1] == "name" for l in ls)
        c["range on tag"] += any(l[2] in F.RANGE_OPS and l[1] == "tag" for l in ls)
        kept = sum(keep)
        if s.where is not None:
            c["zero survivors"] += kept == 0
            c["all rows survive"] += kept == len(rows)
        if s.kind == "project":
            if s.order_by:
                j = s.order_by[0][0]
                seen = {}
                for i, r in enumerate(rows):
                    if keep[i]:
                        seen.setdefault(r[j], set()).add(segment(i))
                c["first key ties across segments"] += any(len(v) > 1 for v in seen.values())
            total = kept
        else:
            groups = F.all_groups(rows, s, keep)
            held = [g for g in groups if s.having is None or F.having_holds(s.having, g[1])]
            if s.having is not None and groups:
                c["having keeps none"] += not held
                c["having keeps all"] += len(held) == len(groups)
            c["group first seen in the last segment"] += any(g[3] >= last for g in groups)
            c["0 groups"] += len(groups) == 0
            c["1 group"] += len(groups) == 1
            c["> 100 groups"] += len(groups) > 100
            total = len(held)
        c["limit below kept"] += 0 < s.limit < total
        c["limit above kept"] += s.limit > total
    return c


def test_census(census, tables):
    rows, _, seg_rows = tables
    assert seg_rows[1024] == [2049, 2049, 902] and seg_rows[1000] == [2001, 2001, 998]     # two blocks and the loader's one-row block; a short last one
    assert {r["state"] for r in rows[: seg_rows[1000][0]]} >= {F.FIRST_ONLY} and all(r["state"] != F.FIRST_ONLY for r in rows[seg_rows[1000][0]:])
    assert all(r["state"] != F.LAST_ONLY for r in rows[: sum(seg_rows[1024][:2])]) and any(r["state"] == F.LAST_ONLY for r in rows)
    # names with bytes >= 0x80 are in the rows, and the loader carried them into the column files as they are
    high = [n for n in F.NAMES if not n.isascii()]
    assert sorted(high) == sorted(F.HIGH_NAMES) and all(sum(r["name"] == n for r in rows) > 50 for n in high)
    for d in tables[1].values():
        with open(os.path.join(d, F.TABLE, "name_0.dat"), "rb") as f:
            dat = f.read()
        assert all(n.encode("utf-8") in dat for n in high) and len(dat) == 8 * seg_rows[int(os.path.basename(d)[4:])][0]
    c = count_features(census, rows, seg_rows[1024])
    n = c["statements"]
    assert n == F.SEEDS * F.PER_SEED
    assert 4 * c["either"] <= n - c["errors"]
    assert 3 * c["spellable"] >= n
    assert 10 * c["errors"] <= n
    for what in ("honoured or", "or run as and, differing", "notmatch", "in-list > 8", "range on name", "range on tag", "first key ties across segments",
                 "limit below kept", "limit above kept", "zero survivors", "all rows survive", "having keeps none", "having keeps all",
                 "group first seen in the last segment", "0 groups", "1 group", "> 100 groups", "keyword-prefixed column", "names compared as bytes"):
        assert c[what] >= 8, (what, c[what])
    assert c == COUNTS
    for (_, _, s, _, _) in census:                                    # what every statement keeps to
        assert len(F.used_columns(s)) <= 4, s
        assert len(s.order_by) <= (4 if s.kind == "project" else 3), s
        if s.error is None and s.kind == "project":
            assert sum(F.WIDTH[c] for (c, _) in s.order_by) <= 16, s
        if s.error is None and s.kind == "agg":
            assert 1 <= len(s.aggs) <= 4 and len(s.group) <= 2 and sum(F._order_width(s, n) for (n, _) in s.order_by) <= 12, s
            assert len({F.alias_of(a) for a in s.aggs}) == len(s.aggs), s


def test_every_error_kind_occurs_and_is_refused_by_the_reference(census):
    kinds = {s.error for (_, _, s, _, _) in census if s.error}
    assert kinds == set(F.ERRORS)


def test_numpy_agrees_with_the_plain_python_reference(census, tables):
    """the second witness: the where clause as whole-column comparisons, the groups by np.unique / bincount / ufunc.at"""
    rows, _, _ = tables
    arrs = F.column_arrays(rows)
    for (seed, i, s, keep, want) in census:
        if want is None:
            continue
        mask = F.np_mask(arrs, s)
        assert mask.tolist() == keep, (seed, i, s)
        if s.kind == "agg":
            assert F.np_groups(arrs, s, mask) == [(g[0], g[1]) for g in F.all_groups(rows, s, keep)], (seed, i, s)


def spellable(census):
    return [(seed, i, s, F.render(s)) for (seed, i, s, _, _) in census if F.render(s) is not None][:MAX_PARSED]


def test_the_python_parser_reads_every_spellable_statement_as_its_adt(census):
    n = 0
    for (seed, i, s, sql) in spellable(census):
        try:
            q = F.to_query(s)
        except ValueError:                                             # the error class: the constructors refuse, and so must the parser
            with pytest.raises(ValueError):
                SQLParser.parseAll(sql, **ALL_FLAGS)
            continue
        assert SQLParser.parseAll(sql, **ALL_FLAGS) == q, (seed, i, sql)
        n += 1
    assert n >= 40


def test_the_cpp_parser_prints_the_same_query_and_used_columns(census, tables):
    _, dirs, _ = tables
    n = 0
    for (seed, i, s, sql) in spellable(census):
        p = subprocess.run([SQL, "--parse-only", *CLI_FLAGS, "-q", sql, "-d", dirs[1024]], capture_output=True, text=True, timeout=60)
        try:
            F.to_query(s)
        except ValueError:                                             # the error class: refused here, or read alike and left to the engine to refuse
            assert p.returncode == 1 or (p.returncode == 0 and p.stdout.splitlines()[0] == F.show(s)), (sql, p.stdout)
            continue
        assert p.returncode == 0, (sql, p.stdout, p.stderr)
        lines = p.stdout.splitlines()
        assert lines[0] == F.show(s), (seed, i, sql)
        assert lines[1] == "usedColumns: " + " ".join(F.used_columns(s)), (seed, i, sql)
        n += 1
    assert n >= 40
