"""Host suite (no GPU): where a string Match goes (csrc/imm3_planner.cpp::pred_route, exported as imm3_plan_string_route), and the C
oracle's Match against a plain numpy byte compare at the widest string (the GPU suites take their expectations from the oracle)."""
import numpy as np

from conftest import DENSE_STRING, MATCH, RawColumn
from immutable3_amd import native
from immutable3_amd.build import build_native
from str_rows_util import in_lists, make_strings, pool_for

TILE, STR_ROWS, GENERIC = 0, 1, 2


def test_widths_that_are_whole_dwords_go_to_the_string_pass():
    build_native()
    for width in (4, 8, 16, 256):
        for n_match in (1, 8, 9, 40):
            assert native.plan_string_route(width, n_match) == STR_ROWS, (width, n_match)
    assert all(native.plan_string_route(w, 3) == STR_ROWS for w in range(4, 257, 4))


def test_everything_else_stays_generic():
    build_native()
    assert native.plan_string_route(2, 8) == TILE and native.plan_string_route(2, 1) == TILE
    assert native.plan_string_route(2, 9) == GENERIC
    for width in (1, 3, 5, 6, 7, 9, 255):
        assert native.plan_string_route(width, 1) == GENERIC, width
    assert native.plan_string_route(0, 1) == -1 and native.plan_string_route(257, 1) == -1 and native.plan_string_route(4, 0) == -1


def test_oracle_match_equals_numpy_byte_compare(oracle):
    for width in (16, 256):
        rng = np.random.default_rng(width)
        pool, t0, t1 = pool_for(rng, width)
        n = 2 * 1024 + 1
        v = make_strings(rng, pool, n)
        col = RawColumn(DENSE_STRING, width, v, [1024, 1024, 1])
        for values in in_lists(rng, pool, t0, t1, width):
            keep = np.zeros(n, bool)
            for val in values:
                if len(val) == width:
                    keep |= (v == np.frombuffer(val, np.uint8)).all(1)
            words, count = oracle.scan_select([col.ocol()], [(0, MATCH, values)], 1024, 1)
            bits = np.unpackbits(words.view(np.uint8), bitorder="little")
            want = np.zeros(bits.size, np.uint8)
            want[:1024] = keep[:1024]; want[1024:2048] = keep[1024:2048]; want[2048] = keep[2048]
            assert count == int(keep.sum()) and bits.tolist() == want.tolist(), (width, len(values))
