"""Host suite (no GPU): when does a table query with a `limit` take the one launch that stops at the limit?  The decision is a named
pure function (csrc/imm3_planner.cpp::table_limit_applies, exported as imm3_plan_table_limit next to imm3_plan_limit_scan): its base
case and every veto are walked here.  The chunked scan of ONE segment keeps its own decision, untouched (tests/test_host.py pins it)."""
from immutable3_amd import native
from immutable3_amd.build import build_native

CLAIM = native.TABLE_LIMIT_CLAIM_TILES
# the README-shaped table: 98 segments of 1 024 001 rows = 98 x 1001 virtual tiles, an int32 predicate column (512 work-groups)
BASE = dict(table=1, tree=0, limit=10, count_in_scan=1, single_tile_pass=1, whole=0, count_log_on=0, count_only=0, filter_variant=0,
            n_tiles=98 * 1001, grid=512)


def call(**kw):
    return native.plan_table_limit(**{**BASE, **kw})


def test_the_base_case_takes_the_stopping_launch():
    build_native()
    assert CLAIM == 32 and CLAIM % 16 == 0            # a multiple of the gather's span (16 tiles): the scanned prefix ends on a span boundary
    assert call() == 1
    assert call(limit=1) == 1 and call(limit=10 ** 12) == 1
    assert call(filter_variant=12) == 1 and call(filter_variant=15) == 1      # variants that pin other things
    assert call(grid=1536) == 1                         # (the tile pass of run_select hands in the grid it launches: at most 512 work-groups)


def test_every_veto_keeps_the_whole_select():
    build_native()
    vetoes = [dict(table=0),                            # one segment: the chunked scan's business (imm3_plan_limit_scan)
              dict(tree=1),                             # a select tree with an OR runs k_filter_expr
              dict(limit=0), dict(limit=-1),
              dict(count_in_scan=0),                    # no projection follows
              dict(single_tile_pass=0),                 # the select chain is more than one tile launch
              dict(whole=1),                            # a getter's whole select
              dict(count_log_on=1),
              dict(count_only=1),
              dict(filter_variant=7), dict(filter_variant=native.TV_NO_LIMIT_CHUNKS),
              dict(n_tiles=512 * CLAIM), dict(n_tiles=5), dict(n_tiles=0), dict(grid=0),
              dict(grid=4096)]                          # 4096 x 32 tiles claimed at once: more than the table has
    for veto in vetoes:
        assert call(**veto) == 0, veto


def test_the_size_threshold_is_one_claim_per_work_group():
    build_native()
    for grid in (1, 2, 7, 512, 1536):
        assert call(grid=grid, n_tiles=grid * CLAIM) == 0, grid
        assert call(grid=grid, n_tiles=grid * CLAIM + 1) == 1, grid


def test_the_segment_decision_still_refuses_tables():
    import ctypes
    build_native()
    L = native.load()
    L.imm3_plan_limit_scan.argtypes = [ctypes.c_int32] * 3 + [ctypes.c_int64] + [ctypes.c_int32] * 6 + [ctypes.c_int64]
    #                             whole log in_scan limit one_pass table records skip overlap variant n_tiles
    assert L.imm3_plan_limit_scan(0, 0, 1, 10, 1, 1, 0, 0, 0, 0, 98 * 1001) == 0
    assert L.imm3_plan_limit_scan(0, 0, 1, 10, 1, 0, 0, 0, 0, 0, 98 * 1001) == 1
