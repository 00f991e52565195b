"""Host suite (no GPU): what tests/test_gpu_column_pass_matrix.py relies on, checked on the generated data itself
(tests/column_pass_util.py) -- that the layouts make a wave walk full and partial tiles in every order, that every tile of every
column holds the rows the matrix is about, that the lists and ranges which hold the all-zero value select the genuine zero rows, and
that the two string references (numpy equality for Match, Python bytes order for the range) agree where they meet."""
import numpy as np
import pytest

import column_pass_util as M
import str_range_util as R
from immutable3_amd import native
from immutable3_amd.build import build_native
from int_in_util import args_largest_n, lds_largest_n


def kinds(layout):
    return ["F" if nv == M.TILE else "P" for _, _, nv in M.tiles_of(layout)]


def sequences(layout, grid):
    k = kinds(layout)
    return ["".join(k[t] for t in w) for w in M.walks(len(k), grid)]


def test_the_widths_reach_all_seven_instances_of_a_string_kernel():
    assert {M.instance_of(w) for w in M.WIDTHS} == {(1, 1, False), (2, 2, False), (3, 1, False), (4, 4, False), (4, 4, True), (4, 2, True), (4, 1, True)}
    # the tail loop: one chunk (24, 32), several at C = 1, 2 and 4 (20 is one chunk of one dword; 28: three, 40: three of two, 256: fifteen of four)
    chunks = {w: ((w // 4 - 4) // M.instance_of(w)[1], M.instance_of(w)[1]) for w in M.WIDTHS if w > 16}
    assert chunks == {20: (1, 1), 24: (1, 2), 28: (3, 1), 32: (1, 4), 40: (3, 2), 256: (15, 4)}


def test_the_library_agrees_with_the_constants_restated_here():
    build_native()
    assert args_largest_n() == M.K_MAX_MATCH
    assert all(native.plan_string_route(w, n) == 1 for w in M.WIDTHS for n in (1, M.K_MAX_MATCH, M.K_MAX_MATCH + 1))
    assert all(native.plan_string_range_route(w) == 1 for w in M.WIDTHS)
    assert lds_largest_n() > M.K_MAX_MATCH


def test_a_wave_walks_full_and_partial_tiles_in_every_order():
    for r in M.LAST_ROWS:                                   # a segment: nine full tiles and a partial one
        name = f"segment-{r}"
        assert kinds(name) == ["F"] * 9 + ["P"] and M.tiles_of(name)[-1][2] == r
        one = sequences(name, 1)
        assert one == ["FFF", "FFP", "FF", "FF"]            # one work-group: three tiles per wave, the partial one behind two full ones
        assert sequences(name, 3) == sequences(name, 0) and max(len(s) for s in one) >= 3
    rows = M.LAYOUTS["table"]
    assert 0 in rows and 1 in rows and len(M.tiles_of("table")) >= 10
    assert sorted({nv for _, _, nv in M.tiles_of("table")}) == [1, 63, 64, 65, 700, 1023, 1024]
    one = sequences("table", 1)
    assert any("FPF" in s for s in one) and any(s.startswith("PF") for s in one) and any("PP" in s for s in one)
    assert max(len(s) for s in one) >= 3 and len(one) == 4
    three = sequences("table", 3)                           # a step of 12 over 14 tiles: two waves walk two tiles, ten walk one
    assert len(three) == 12 and sorted(s for s in three if len(s) > 1) == ["FP", "PF"]
    assert kinds("table")[M.EMPTIED_TILE] == "F" and all(kinds(n)[M.EMPTIED_TILE] == "F" for n in M.LAYOUTS)


def first_difference(rows, bound, width):
    """per row, the first dword in which it differs from `bound` (width / 4: none)"""
    ne = (rows != np.frombuffer(bound, np.uint8)).reshape(rows.shape[0], width // 4, 4).any(axis=2)
    return np.where(ne.any(axis=1), ne.argmax(axis=1), width // 4)


@pytest.mark.parametrize("width", M.WIDTHS)
def test_every_tile_of_every_string_column_holds_the_rows_the_matrix_is_about(width):
    P, C, tail = M.instance_of(width)
    for layout in M.LAYOUTS:
        c = M.string_case(width, layout)
        assert sum(r.nbytes for r in c.rows) <= 10 * M.TILE * 256
        predicates = [(c.match_masks(v), what, c.zero in v) for v, what in c.lists] + [(c.range_masks(a, b), what, a == b"") for a, b, what in c.ranges]
        assert sum(z for _, _, z in predicates) == 3 and len(predicates) == 8
        assert all(len({v for v in vals if len(v) == width}) > M.K_MAX_MATCH for vals, what in c.lists if "long" in what)
        assert all(len(vals) <= M.K_MAX_MATCH for vals, what in c.lists if "short" in what)
        zero_rows = 0
        for ti, (si, r0, nv) in enumerate(M.tiles_of(layout)):
            t, age, gate = c.rows[si][r0:r0 + nv], c.age[si][r0:r0 + nv], c.gate[si][r0:r0 + nv]
            is_zero = ~t.any(axis=1)
            assert is_zero.sum() == (2 if nv == M.TILE else 0)     # the genuine zero rows: full tiles only, so never a segment's last tile
            zero_rows += int(is_zero.sum())
            for masks, what, holds_zero in predicates:
                m = masks[si][r0:r0 + nv]
                where = (width, layout, ti, what)
                assert m[0] and m[nv - 1] and age[0] > 0 and age[nv - 1] > 0, where       # survivors at row 0 and at the last valid row
                if nv > 64:
                    assert m[63] and m[64] and age[63] > 0 and age[64] > 0, where         # ... and on both sides of a word boundary
                assert m[is_zero].all() if holds_zero else not m[is_zero].any(), where    # gap 4: only these predicates see a zero
                if nv >= 5:                                                                # both outcomes of both passes
                    assert (m & (age > 0)).any() and (m & ~(age > 0)).any() and (~m & (age > 0)).any() and (~m & ~(age > 0)).any(), where
                if nv >= 700:
                    assert 0.4 < (age > 0).mean() < 0.6, where                            # the first pass keeps about half
                assert not (gate > 0).any() if ti == M.EMPTIED_TILE else (gate == age).all(), where
            if ti == M.EMPTIED_TILE:
                assert c.match_masks(c.lists[1][0])[si][r0:r0 + nv].any()                 # the string pass's answer there is not empty
            if nv == M.TILE:
                for bound in (c.lo, c.hi, c.hi2):
                    fd = first_difference(t, bound, width)
                    # rows that differ from the value / bound in one byte of each dword; wider than 16 bytes they share the prefix and
                    # leave the tail loop in every chunk, and one differs in the last byte only
                    assert set(range(width // 4)) <= set(fd.tolist()), (width, layout, ti)
                    if tail:
                        assert {(d - P) // C for d in fd.tolist() if P <= d < width // 4} == set(range((width // 4 - P) // C)), (width, layout, ti)
                        last = bound[:-1] + bytes([(bound[-1] + 1) & 0xFF])
                        assert (t == np.frombuffer(last, np.uint8)).all(axis=1).any(), (width, layout, ti)
                if tail:                                                                   # rows tied with both bounds of the shared-prefix pair
                    assert ((t[:, :16] == np.frombuffer(c.lo[:16], np.uint8)).all(axis=1) & ~c.range_masks(c.lo, c.hi2)[si][r0:r0 + nv]).any()
        assert zero_rows >= 2 * 6


@pytest.mark.parametrize("layout", list(M.LAYOUTS))
def test_every_tile_of_the_integer_columns(layout):
    build_native()
    c = M.int_case(layout)
    sizes = {"I8": 40, "ARGS": args_largest_n(), "LDS": lds_largest_n(), "GLOBAL": lds_largest_n() + 1}
    for form in M.FORMS:
        lists = c.lists(form, sizes[form])
        assert [0 in v for v, _ in lists] == [False, True]
        for values, what in lists:
            assert native.plan_int_list_form(1 if form == "I8" else 4, len(set(values))) == M.FORMS.index(form), (form, what)
            masks = c.masks(form, values)
            for ti, (si, r0, nv) in enumerate(M.tiles_of(layout)):
                v, m, age = c.column(form)[si][r0:r0 + nv], masks[si][r0:r0 + nv], c.age[si][r0:r0 + nv]
                assert m[0] and m[nv - 1] and age[0] > 0 and age[nv - 1] > 0, (form, what, ti)
                assert (v == 0).sum() == (2 if nv == M.TILE else 0)
                assert m[v == 0].all() if 0 in values else not m[v == 0].any(), (form, what, ti)
                if nv > 64:
                    assert m[63] and m[64]
                if nv >= 5:
                    assert (m & (age > 0)).any() and (m & ~(age > 0)).any() and (~m & (age > 0)).any() and (~m & ~(age > 0)).any(), (form, what, ti)
                if nv >= 63:                                                               # neighbours of a member that are no members
                    assert ((v == 6) | (v == 8)).any() and not m[(v == 6) | (v == 8)].any(), (form, what, ti)


@pytest.mark.parametrize("width", M.WIDTHS)
def test_the_match_reference_is_the_range_reference_at_a_single_value(width):
    """numpy equality (Match) against Python bytes order (the range) where they mean the same: lo == hi == v"""
    c = M.string_case(width, "table")
    rows = np.concatenate(c.rows)
    for v in (c.lo, c.hi, c.hi2, c.zero, c.out, bytes(c.pool[0]), bytes(c.pool[-1])):
        a, b = M.match_mask(rows, [v]), R.in_range(rows, v, v)
        assert a.tolist() == b.tolist() and a.any(), (width, v)
    assert not M.match_mask(rows, [c.lo[:-1], c.lo + b"x"]).any()          # values of another length select nothing
