"""GPU suite: the instance matrix of the one-column filter passes (csrc/imm3_pass.h: k_filter_str_rows, k_filter_str_range,
k_filter_int_list).  Every <P, C, TAIL> instance of the two string kernels and every form of the integer-list kernel, TABLE false and
true, runs
  * over a segment of nine full tiles and a tenth of 1, 63, 64, 65 or 1023 rows, and over a table of nine segments (1 .. 3071 rows, an
    empty one among them) whose fourteen tiles make a wave walk full -> partial -> full, partial -> full and partial -> partial;
  * under the default grid, under one work-group (four waves own every tile: three or four tiles per wave) and under three (a step
    of 12; the table's tiles 12 and 13 are second tiles), and -- segments -- under the word-at-a-time kernel (tuning variant 1);
  * alone (the bitmap line begins as all ones) and as an and_existing pass behind an int8 tile pass that keeps about half the rows of
    every tile; Match and the integer lists also behind one that keeps nothing in one whole tile;
  * with lists and ranges that hold the all-zero value (a partial tile's rows beyond its valid count compare as zeros) and with ones
    that do not, lists in the kernel arguments and in device memory.
The columns, what every tile of them holds and why are tests/column_pass_util.py's; tests/test_column_pass_host.py asserts all of it
without a device.  Expected bitmaps come from numpy and Python bytes alone (Match: byte equality with a value of exactly the width;
range: str_range_util.in_range; lists: np.isin on int64), every comparison is exact, the count is the mask's sum, and with kernel
timing on each run must have enqueued exactly 1 (alone) or 2 (behind a tile pass) select launches, so no case passes by running
another kernel.  A cell prints one line; run with -s to list the matrix."""
import pytest

import column_pass_util as M
from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, GT, MATCH, RawColumn
from immutable3_amd import native
from int_in_util import args_largest_n, lds_largest_n

pytestmark = pytest.mark.gpu
TV_GENERIC_ONLY = 1
STR_ROWS_ROUTE = 1                                          # plan_string_route / plan_string_range_route: the string pass


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    c.timing_enable(64)
    yield c
    c.close()


@pytest.fixture(scope="module")
def on_device(ctx):
    """case -> (what a query runs over: the segment, or the table of the layout's segments); uploaded once per column, closed at the end"""
    held = {}

    def get(case):
        if case not in held:
            if isinstance(case, M.StringCase):
                cols = [[RawColumn(DENSE_STRING, case.width, case.rows[s], M.blocks_of(n))] for s, n in enumerate(M.LAYOUTS[case.layout])]
            else:
                cols = [[RawColumn(DENSE_INT, 4, case.ids[s], M.blocks_of(n)), RawColumn(DENSE_TINYINT, 1, case.tiny[s], M.blocks_of(n))]
                        for s, n in enumerate(M.LAYOUTS[case.layout])]
            for s, n in enumerate(M.LAYOUTS[case.layout]):
                cols[s] += [RawColumn(DENSE_TINYINT, 1, case.age[s], M.blocks_of(n)), RawColumn(DENSE_TINYINT, 1, case.gate[s], M.blocks_of(n))]
            dsegs = [native.DeviceSegment(ctx, [c.native() for c in seg]) for seg in cols]
            table = native.DeviceTable(ctx, dsegs) if case.layout == "table" else None
            held[case] = (dsegs, table)
        dsegs, table = held[case]
        return table if table is not None else dsegs[0]

    yield get
    for dsegs, table in held.values():
        if table is not None:
            table.close()
        for d in dsegs:
            d.close()


def run(ctx, target, layout, used, sels, masks, variant, grid, launches, what):
    """one query under set_tuning(variant, grid): the bitmap of every segment, the zero padding up to the next tile (a table), the
    count, and the select launches it enqueued (launches: None under the word-at-a-time kernel)"""
    ctx.set_tuning(variant, grid)
    try:
        q = native.DeviceQuery(ctx, target, used, sels)
        ctx.timing_reset()
        q.run_select()
        enqueued = int(ctx.timing_collect(0).size)
        words, count = q.bitmap(), q.count()
        first_word = q.segment_starts()[1] if layout == "table" else None
        q.close()
    finally:
        ctx.set_tuning(0, 0)
    want = M.expected_words(masks, layout)
    if launches is not None:
        assert enqueued == launches, (what, enqueued)
    assert count == sum(int(m.sum()) for m in masks), (what, count)
    if layout != "table":
        assert words.tolist() == want[0].tolist(), what
        return
    for si, w in enumerate(want):
        at = int(first_word[si])
        assert words[at: at + w.size].tolist() == w.tolist(), (what, si)
        assert not words[at + w.size: int(first_word[si + 1])].any(), (what, si)         # up to the next tile: zeros


def matrix(ctx, target, case, column, predicates, cell):
    """every grid and position of one (kernel, instance, layout): predicates = [(cond, operand, masks per segment, what, also behind
    the emptied tile)]"""
    layout = case.layout
    plans = [(0, g) for g in M.GRIDS] + ([(TV_GENERIC_ONLY, 0)] if layout != "table" else [])
    age, gate = 2 if isinstance(case, M.IntCase) else 1, 3 if isinstance(case, M.IntCase) else 2
    for variant, grid in plans:
        for position, first in (("alone", None), ("behind a tile pass", age), ("behind a tile pass that empties a tile", gate)):
            ran = 0
            for cond, operand, masks, what, emptied in predicates:
                if first == gate and not emptied:
                    continue
                if first is None:
                    used, sels, want = [column], [(0, cond, operand)], masks
                else:
                    kept = case.age if first == age else case.gate
                    used, sels, want = [first, column], [(0, GT, 0.0), (1, cond, operand)], [m & (k > 0) for m, k in zip(masks, kept)]
                launches = None if variant else (1 if first is None else 2)
                run(ctx, target, layout, used, sels, want, variant, grid, launches, (cell, layout, variant, grid, position, what))
                ran += 1
            if ran:
                plan = "word-at-a-time" if variant else f"grid {grid or 'default'}"
                print(f"cell: {cell} | {'TABLE' if layout == 'table' else 'segment'} {layout} | {plan} | {position} | "
                      f"select launches {'-' if variant else (1 if first is None else 2)} | {ran} predicates")


@pytest.mark.parametrize("layout", list(M.LAYOUTS))
@pytest.mark.parametrize("width", M.WIDTHS)
def test_match(ctx, on_device, width, layout):
    case = M.string_case(width, layout)
    for values, _ in case.lists:
        assert native.plan_string_route(width, len(values)) == STR_ROWS_ROUTE
    predicates = [(MATCH, values, case.match_masks(values), what, what == "short, zero") for values, what in case.lists]
    assert any(m.any() for m in predicates[0][2]) and not all(m.all() for m in predicates[0][2])
    matrix(ctx, on_device(case), case, 0, predicates, "k_filter_str_rows<%d, %d, %s> width %d" % (M.instance_of(width) + (width,)))


@pytest.mark.parametrize("layout", list(M.LAYOUTS))
@pytest.mark.parametrize("width", M.WIDTHS)
def test_range(ctx, on_device, width, layout):
    case = M.string_case(width, layout)
    assert native.plan_string_range_route(width) == STR_ROWS_ROUTE
    predicates = [(native.STR_RANGE, (lo, hi), case.range_masks(lo, hi), what, False) for lo, hi, what in case.ranges]
    matrix(ctx, on_device(case), case, 0, predicates, "k_filter_str_range<%d, %d, %s> width %d" % (M.instance_of(width) + (width,)))


@pytest.mark.parametrize("layout", list(M.LAYOUTS))
@pytest.mark.parametrize("form", M.FORMS)
def test_int_list(ctx, on_device, form, layout):
    case = M.int_case(layout)
    n_values = {"I8": 40, "ARGS": args_largest_n(), "LDS": lds_largest_n(), "GLOBAL": lds_largest_n() + 1}[form]
    predicates = []
    for values, what in case.lists(form, n_values):
        assert native.plan_int_list_form(1 if form == "I8" else 4, len(set(values))) == getattr(native, "INT_LIST_" + form), (form, what)
        predicates.append((native.INT_IN, values, case.masks(form, values), what, "zero" in what))
    matrix(ctx, on_device(case), case, 1 if form == "I8" else 0, predicates, f"k_filter_int_list<{form}>")
