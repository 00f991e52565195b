// imm3_run.cpp -- the run calls of include/imm3.h (imm3_query_run, _run_select, _run_count, _join_count, _sync) and every launch
// they enqueue: the select run as one launcher per pass kind (run_select; the one-column passes -- string match, string range, integer
// list -- share fill_column_pass and launch_column_pass), the one-launch projection (run_single_pass), the
// projection behind a select (run_project: offsets scan, gather / records / the fused limit gather), and the graph-capture
// bookkeeping around a run.  Query creation, the getters (which settle what a run left undone through run_select, launch_project
// and join_total: imm3_api_internal.h) and aggregation (run_agg shares its argument filling with the group getters) are
// imm3_api.cpp; the decisions between equivalent launches are pure functions in imm3_planner.cpp.
#include "../../include/imm3.h"
#include "../../include/imm3_diag.h"
#include "imm3_internal.h"

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "imm3_handles.h"
#include "imm3_api_internal.h"

using namespace imm3;

// ---------------------------------------------------------------------------------------------
// the select run: one launcher per pass kind
// ---------------------------------------------------------------------------------------------
void imm3::fill_colpred(const imm3_query *q, const FoldedPred &fp, ColPred &cp) {
    std::memset(&cp, 0, sizeof(cp));
    const SegCol &sc = q->seg->cols[(size_t)fp.seg_col];
    cp.data = col_flat(sc);
    cp.kind = fp.kind;
    cp.width = fp.width;
    cp.lo = (int32_t)fp.lo;
    cp.hi = (int32_t)fp.hi;
    cp.n_match = (int32_t)fp.match.size();
    cp.negated = fp.negated ? 1 : 0;
    cp.match_in_args = (fp.kind == KIND_STR && !fp.d_blob) ? 1 : 0;
    cp.match_blob = fp.d_blob;
    if (fp.has_range) { // the bounds, byte for byte, on the device: lo' then hi' (upload_match_blobs)
        cp.range = 1;
        cp.match_in_args = 0;
        cp.n_match = 0;
    }
    if (fp.kind != KIND_STR && fp.has_list) { // IMM3_INT_IN: the set (int8) or the probe table (int32: upload_match_blobs)
        cp.list = 1;
        cp.n_match = 0;
        std::memcpy(cp.match, fp.list_set, sizeof(fp.list_set));
        if (fp.kind == KIND_I32 && int_list_form(fp.width, pred_list_count(fp)) == INT_LIST_ARGS) { // no table: the values themselves, a shorter list repeating its first
            cp.list = 2;
            int32_t vals[kMaxMatch];
            for (size_t m = 0; m < (size_t)kMaxMatch; ++m) vals[m] = fp.list[m < fp.list.size() ? m : 0];
            std::memcpy(cp.match, vals, sizeof(vals));
        }
        cp.list_empty = fp.list_empty;
        cp.list_mask = fp.list_mask;
        cp.list_shift = fp.list_shift;
        cp.list_max_probe = fp.kind == KIND_I32 && fp.d_blob ? fp.list_max_probe : 0; // (no table: no step)
    }
    if (cp.match_in_args) {
        for (size_t m = 0; m < fp.match.size(); ++m) {
            uint64_t v = 0;
            for (int b = 0; b < fp.width; ++b) v |= (uint64_t)(uint8_t)fp.match[m][(size_t)b] << (8 * b);
            cp.match[m] = v;
        }
    }
}

// join: make `s` wait for this query's count reduce on the aux stream (no-op when it ran on the main stream)
int imm3::join_total(imm3_query *q, hipStream_t s) {
    if (q->total_on_aux) HIPCHK(hipStreamWaitEvent(s, q->ev_total_done, 0));
    return IMM3_OK;
}

// One select run: what run_select knows before the first pass, and what the passes leave for the ones behind them.  The launchers
// below take (q, run) and nothing else of run_select's.
struct SelectRun {
    unsigned mode = SEL_DEFAULT;                                           // SelectMode bits, and three of them by name
    bool overlap_total = false, count_in_scan = false, count_only = false;
    int fv = 0;                // the tuning variant, read once
    hipStream_t s = nullptr;   // the context's stream
    SelectChain chain;         // (empty for a select tree)
    bool tree_tile = false;    // a select tree that runs through the tile kernel
    bool skip_bitmap = false;  // a count-only run of ONE launch: no bitmap is stored
    bool chunked = false;      // the one tile launch runs as the chunks of a limit scan
    int pass = 0;              // launches so far: every pass behind the first ANDs into the bitmap in memory
    int grid = 1;              // work-groups of the last launch: that many block_partials for the count reduce
    bool count_done = false;   // the filter kernel's last work-group has written total / n_emit
};

// the tail every select kernel's arguments share; a pass of the chain (not a tree) also says whether it ANDs into the bitmap
template <class Args> static void fill_bitmap_tail(const imm3_query *q, Args &a) {
    a.n_rows = q->n_rows;
    a.n_words = q->n_words;
    a.n_tiles = q->n_tiles;
    a.bitmap = q->d_bitmap;
    a.block_partials = q->d_block_partials;
}
template <class Args> static void fill_pass_tail(const imm3_query *q, const SelectRun &run, Args &a) {
    a.and_existing = run.pass > 0;
    fill_bitmap_tail(q, a);
}

static int tile_kind_bytes(int kind) { return kind == TK_I32 ? 4 : ((kind == TK_S2 || kind == TK_H16) ? 2 : (kind == TK_I8 ? 1 : 0)); } // (TK_H16: what the scan streams, the plane)

// what filter_grid asks about a tile launch's columns: an int32 column among them, else the bytes per row of the narrow ones -- and the
// lone high-half plane, which streams TK_S2's two bytes per row but wants twice its work-groups (filter_grid: kPlaneGrid)
struct TileGridHint {
    bool any_i32 = false;
    int narrow_bytes = 0;
    bool lone_plane = false;
};
static TileGridHint tile_grid_hint(const int32_t *kinds) {
    TileGridHint h;
    for (int k = 0; k < kMaxTileCols; ++k) {
        h.any_i32 |= kinds[k] == TK_I32;
        if (kinds[k] != TK_I32) h.narrow_bytes += tile_kind_bytes(kinds[k]);
    }
    h.lone_plane = kinds[0] == TK_H16 && kinds[1] == TK_NONE; // (sorted: nothing behind a TK_NONE)
    return h;
}

// (diagnostics: bench.py's instrumented pass)  The device-clock stamps of a launch of `grid` work-groups: the next free slot, or null
// when the stamps are off or used up.
static unsigned long long *claim_stamp_slot(imm3_ctx *ctx, int grid) {
    if (!ctx->d_stamps) return nullptr;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->d_stamps || ctx->stamp_used >= ctx->stamp_slots) return nullptr;
    unsigned long long *slot = ctx->d_stamps + (size_t)ctx->stamp_used * kMaxFilterGrid * 2;
    ctx->stamp_grids.push_back(grid);
    ++ctx->stamp_used;
    return slot;
}

static LimitScanInputs limit_scan_inputs(const imm3_query *q, const SelectRun &run) {
    LimitScanInputs li;
    li.whole = run.mode & SEL_WHOLE;
    li.count_log_on = q->count_log_on;
    li.count_in_scan = run.count_in_scan;
    li.limit = q->limit;
    li.single_tile_pass = run.chain.single_tile_pass;
    li.table = q->table != nullptr;
    li.records = q->d_stage_rec != nullptr;
    li.skip_bitmap = run.skip_bitmap;
    li.overlap_total = run.overlap_total;
    li.filter_variant = run.fv;
    li.n_tiles = q->n_tiles;
    return li;
}

static TableLimitInputs table_limit_inputs(const imm3_query *q, const SelectRun &run) {
    TableLimitInputs ti;
    ti.table = q->table != nullptr;
    ti.tree = q->is_expr;
    ti.limit = q->limit;
    ti.count_in_scan = run.count_in_scan;
    ti.single_tile_pass = run.chain.single_tile_pass;
    ti.whole = run.mode & SEL_WHOLE;
    ti.count_log_on = q->count_log_on;
    ti.count_only = run.count_only;
    ti.filter_variant = run.fv;
    ti.n_tiles = q->n_tiles;
    ti.grid = std::min(run.grid, kTableLimitMaxGrid); // (narrow columns like 1536 work-groups for a whole scan; here they would claim half of a 100 M-row table before the first run is done)
    return ti;
}

// the tree's terms through the tile kernel (k_filter_expr)
static int launch_tree_tile(imm3_query *q, SelectRun &run) {
    imm3_ctx *ctx = q->ctx;
    ExprTileArgs a;
    std::memset(&a, 0, sizeof(a));
    for (int k = 0; k < kMaxTileCols; ++k) a.kinds[k] = q->expr_kinds[k];
    a.n_terms = (int32_t)q->expr_terms.size();
    for (int ti = 0; ti < a.n_terms; ++ti)
        for (int k = 0; k < kMaxTileCols && a.kinds[k] != TK_NONE; ++k) {
            const FoldedPred *fp = pred_on(q->expr_terms[(size_t)ti], q->expr_seg_col[k]);
            if (fp) {
                fill_tile_col(q, *fp, a.cols[ti][k], a.kinds[k]);
                a.use[ti] |= 1u << k;
            } else a.cols[ti][k].data = col_flat(q->seg->cols[(size_t)q->expr_seg_col[k]]); // (not tested in this term)
        }
    if (q->table) { // address the columns through the tile table (cols[..].data is not read)
        a.tile_rows = q->table->d_tile_rows;
        for (int k = 0; k < kMaxTileCols && a.kinds[k] != TK_NONE; ++k) a.tile_ptrs[k] = (const void *const *)q->table->d_tile_ptrs[(size_t)q->expr_seg_col[k]];
    }
    fill_bitmap_tail(q, a);
    if (run.skip_bitmap) a.bitmap = nullptr;
    const TileGridHint hint = tile_grid_hint(a.kinds);
    run.grid = filter_grid(q->n_tiles, false, hint.any_i32, ctx->grid_blocks, hint.narrow_bytes);
    if (!run.overlap_total && run.fv != TV_COUNT_BY_K_TOTAL && (run.grid <= 512 || run.fv != TV_COUNT_SMALL_GRID)) {
        a.finish = q->d_total;
        run.count_done = true;
    }
    LaunchTimer t(ctx, 0);
    if (!launch_filter_expr(a, run.grid, run.s, t.start, t.stop)) return fail(IMM3_ERR_ARG, "internal: no tree kernel for this column combination");
    q->expr_form_ran = 0;
    return IMM3_OK;
}

// ... and word at a time (k_filter_expr_generic)
static int launch_tree_generic(imm3_query *q, SelectRun &run) {
    imm3_ctx *ctx = q->ctx;
    ExprGenericArgs a;
    std::memset(&a, 0, sizeof(a));
    a.preds = q->d_expr_preds;
    a.term_start = q->d_expr_term_start;
    a.n_terms = (int32_t)q->expr_terms.size();
    fill_bitmap_tail(q, a);
    a.word_row_base = q->d_word_row_base;
    a.word_nvalid = q->d_word_nvalid;
    run.grid = filter_grid(q->n_words, true, false, ctx->grid_blocks);
    LaunchTimer t(ctx, 0);
    bool negated = false;
    for (const ColPred &cp : q->h_expr_preds) negated = negated || cp.negated;
    launch_filter_expr_generic(a, negated, run.grid, run.s, t.start, t.stop);
    q->expr_form_ran = 1;
    return IMM3_OK;
}

// the tree's terms, one launch (imm3_expr.hip); `limit` is the gather's to honour
static int launch_tree_pass(imm3_query *q, SelectRun &run) {
    const int rc = run.tree_tile ? launch_tree_tile(q, run) : launch_tree_generic(q, run);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    ++run.pass;
    return IMM3_OK;
}

// what hi16_eligible (imm3_hi16_plan.h) asks about the int32 predicate `fp` of a tile pass over `take`; creation (imm3_api.cpp:
// place_hi16) asks the same with the run-time facts left false
imm3::Hi16Inputs imm3::hi16_inputs(const imm3_query *q, const FoldedPred &fp, const std::vector<const FoldedPred *> &take) {
    Hi16Inputs in;
    in.table = q->table != nullptr;
    in.tree = q->is_expr;
    in.ragged = q->ragged;
    in.dense_int = q->seg->cols[(size_t)fp.seg_col].codec == IMM3_DENSE_INT;
    in.has_list = fp.has_list;
    in.has_plane = fp.d_hi16 != nullptr;
    for (const FoldedPred *p : take) {
        const int tk = tile_kind(*p);
        in.n_i32 += tk == TK_I32;
        in.n_i8 += tk == TK_I8;
        in.n_s2 += tk == TK_S2;
    }
    return in;
}

// The pass's int32 column becomes TK_H16 -- the scan reads its 16-bit high-half plane, 2 bytes per row, and the full column only where a
// half does not decide -- when hi16_eligible says so.  The kinds stay sorted (tile_kind_rank): the plane goes behind an int8 column.
static void take_hi16_plane(imm3_query *q, const SelectRun &run, const std::vector<const FoldedPred *> &take, TileArgs &a) {
    for (int k = 0; k < (int)take.size() && k < kMaxTileCols; ++k) {
        if (a.kinds[k] != TK_I32) continue;
        const FoldedPred &fp = *take[(size_t)k];
        if (!fp.d_hi16) return; // (creation found or made no plane: nothing to decide)
        Hi16Inputs in = hi16_inputs(q, fp, take);
        in.stages = a.stage_rec != nullptr;
        in.chunked = run.chunked || (q->limit > 0 && run.count_in_scan && !(run.mode & SEL_WHOLE)); // (the select of a projection with a limit: its chunks, or the one launch of a segment the first chunk covers)
        in.pinned_i32 = run.fv == TV_I32_SCAN;
        if (!hi16_eligible(in)) return;
        TileCol &c = a.cols[k];
        tile_col_set_full(c, c.data);
        c.data = fp.d_hi16;
        const Hi16Bounds b = hi16_bounds(c.lo, c.hi);
        c.match[0] = b.possible_first;
        c.match[1] = b.possible_count;
        c.match[2] = b.certain_first;
        c.match[3] = b.certain_count;
        tile_col_set_refined(c, q->d_total + kFinishHi16Refined);
        a.kinds[k] = TK_H16;
        for (int j = k; j + 1 < kMaxTileCols && tile_kind_rank(a.kinds[j + 1]) < tile_kind_rank(a.kinds[j]); ++j) {
            std::swap(a.kinds[j], a.kinds[j + 1]);
            std::swap(a.cols[j], a.cols[j + 1]);
        }
        q->hi16_ran = true;
        return; // (one int32 column per instance)
    }
}

// The arguments of one tile pass over the columns of `take`, and with them what the pass decides for the run: whether it stages
// survivor records, stores a bitmap, reduces the count itself; run.grid is the grid of a launch over the whole segment.
static int fill_tile_args(imm3_query *q, SelectRun &run, const std::vector<const FoldedPred *> &take, TileArgs &a) {
    imm3_ctx *ctx = q->ctx;
    std::memset(&a, 0, sizeof(a));
    const int n = (int)take.size();
    for (int k = 0; k < kMaxTileCols; ++k) a.kinds[k] = TK_NONE;
    for (int k = 0; k < n; ++k) {
        const FoldedPred &fp = *take[(size_t)k];
        if (q->table) a.tile_ptrs[k] = (const void *const *)q->table->d_tile_ptrs[(size_t)fp.seg_col];
        a.kinds[k] = tile_kind(fp);
        fill_tile_col(q, fp, a.cols[k], a.kinds[k]);
    }
    if (run.chain.single_tile_pass && q->d_stage_rec && !run.skip_bitmap && !(run.mode & SEL_PLAIN)) { // the columns are in the order the records were laid out for (same sort)
        bool same = true;
        for (int k = 0; k < kMaxTileCols; ++k) same = same && a.kinds[k] == q->stage_kinds[k] && (k >= n || take[(size_t)k]->seg_col == q->stage_seg_col[k]);
        if (!same) return fail(IMM3_ERR_ARG, "internal: staged record layout does not match the tile launch");
        a.stage_rec = q->d_stage_rec;
        a.tile_start = q->d_tile_start;
        a.wave_cap = q->stage_wave_cap;
        a.max_slots = q->stage_max_slots;
        q->run.stage_written = true;
    }
    take_hi16_plane(q, run, take, a);
    a.ablate = tile_ablation(run.fv); // (tools' build only)
    fill_pass_tail(q, run, a);
    // A records run whose offsets scan follows (imm3_query_run of a projection) stores NO bitmap: the records carry the positions
    // and the scan takes the tiles' counts from the arenas (round 5: 12.5 MB of 128-byte line stores in between the streaming
    // loads, and 12.5 MB read back by k_scan -- C4 107 -> 100 us).  imm3_query_bitmap materialises it on demand.  TV_EAGER_BITMAP: off.
    q->run.bitmap_lazy = q->run.stage_written && run.count_in_scan && !q->count_log_on && run.fv != TV_EAGER_BITMAP;
    if (q->run.bitmap_lazy) {
        a.bitmap = nullptr;
        q->run.bitmap_valid = false;
    }
    a.tile_rows = q->table ? q->table->d_tile_rows : nullptr; // table query: address the columns through the tile table
    const TileGridHint hint = tile_grid_hint(a.kinds);
    run.grid = filter_grid(q->n_tiles, false, hint.any_i32, ctx->grid_blocks, hint.narrow_bytes, hint.lone_plane); // (no column at all: the store-only kernel also likes 1536 groups, 9.9 vs 17.2 us)
    if (q->run.stage_written) run.grid = q->stage_grid; // fixed at creation: the arena layout depends on it
    // A select chain that is ONE tile pass also reduces its count in the kernel (one relaxed atomic per work-group into a
    // two-level tally, finish_add): no k_total launch.  TV_COUNT_BY_K_TOTAL = never; TV_COUNT_SMALL_GRID = only at <= 512 work-groups (what
    // round 1 did: with a single tally the 1536 atomics of a narrow-column launch cost more than the launch they saved).
    if (run.chain.single_tile_pass && !run.overlap_total && run.fv != TV_COUNT_BY_K_TOTAL && (run.grid <= 512 || run.fv != TV_COUNT_SMALL_GRID)) {
        a.finish = q->d_total;
        run.count_done = true;
    }
    // bitmap lines parked in LDS and stored in bursts: no staging (whose LDS and 2048 work-groups
    // leave no room for 32 KiB more per group); TV_PLAN_PINNED switches it off
    // (64 lines = 32 KiB per work-group at <= 4 groups per CU; 16 lines = 8 KiB for the 1536-group narrow-column kernels)
    a.defer_lines = (run.fv == TV_PLAN_PINNED || q->run.bitmap_lazy) ? 0 : (q->run.stage_written ? 16 : (run.grid <= 1024 ? kDeferLines : 16)); // (no bitmap, no lines to park)
    if (run.skip_bitmap) { // count-only: the kernel instance that stores nothing (the count is reduced in the kernel)
        a.bitmap = nullptr;
        a.defer_lines = 0;
    }
    return IMM3_OK;
}

// A table query with a limit: ONE launch whose work-groups claim runs of tiles in ascending order and stop claiming once the
// finished runs hold `limit` rows (k_filter_table_limit); it publishes count, rows to emit and the scanned prefix itself.
static int launch_tile_table_limit(imm3_query *q, SelectRun &run, TileArgs &a, int grid) {
    imm3_ctx *ctx = q->ctx;
    run.grid = grid;
    a.stamps = claim_stamp_slot(ctx, run.grid);
    a.finish = q->d_total;
    a.defer_lines = 0;
    LaunchTimer t(ctx, 0);
    if (!launch_filter_table_limit(a, run.grid, run.s, t.start, t.stop)) return fail(IMM3_ERR_ARG, "internal: no tile kernel for this column combination");
    HIPCHK(hipGetLastError());
    run.count_done = true;
    q->run.select_partial = true; // (the offsets scan and the gather stop at finish[kFinishLimitTiles]; the getters' whole select: settle_whole_select)
    return IMM3_OK;
}

// The limit scan: this launch in chunks that end at tiles 1024, 8192, 32 768, ... (limit_chunk_ends); each adds to the running
// count and scanned-tile words.
static int launch_tile_chunks(imm3_query *q, SelectRun &run, const TileArgs &a) {
    imm3_ctx *ctx = q->ctx;
    (void)claim_stamp_slot(ctx, run.grid); // (the slot of the whole launch; the chunks write no stamps)
    const TileGridHint hint = tile_grid_hint(a.kinds);
    const LimitChunks chunks = limit_chunk_ends(q->n_tiles);
    int64_t tile0 = 0; // the chunk's first tile: the end of the chunk before it
    for (int i = 0; i < chunks.n; ++i) {
        const int64_t tiles = chunks.end[i] - tile0;
        TileArgs c = a;
        for (int k = 0; k < kMaxTileCols; ++k)
            if (c.kinds[k] != TK_NONE) c.cols[k].data = (const uint8_t *)a.cols[k].data + tile0 * kTileRows * tile_kind_bytes(a.kinds[k]);
        c.bitmap = a.bitmap + tile0 * kTileWords;
        c.n_rows = std::min<int64_t>(tiles * kTileRows, q->n_rows - tile0 * kTileRows);
        c.n_words = (c.n_rows + 63) / 64;
        c.n_tiles = (c.n_words + kTileWords - 1) / kTileWords;
        c.finish = q->d_total;
        c.chunked = tile0 == 0 ? 2 : 1; // (the first chunk starts the running words over)
        c.stamps = nullptr;
        const int cgrid = filter_grid(c.n_tiles, false, hint.any_i32, ctx->grid_blocks, hint.narrow_bytes);
        c.defer_lines = run.fv == TV_PLAN_PINNED ? 0 : (cgrid <= 1024 ? kDeferLines : 16);
        LaunchTimer t(ctx, 0);
        if (!launch_filter_tile(c, cgrid, run.s, t.start, t.stop)) return fail(IMM3_ERR_ARG, "internal: no tile kernel for this column combination");
        HIPCHK(hipGetLastError());
        tile0 = chunks.end[i];
    }
    run.count_done = true;
    q->run.select_partial = true;
    return IMM3_OK;
}

static int launch_tile_plain(imm3_query *q, SelectRun &run, TileArgs &a) {
    imm3_ctx *ctx = q->ctx;
    a.stamps = claim_stamp_slot(ctx, run.grid);
    LaunchTimer t(ctx, 0);
    if (!launch_filter_tile(a, run.grid, run.s, t.start, t.stop)) return fail(IMM3_ERR_ARG, "internal: no tile kernel for this column combination");
    HIPCHK(hipGetLastError());
    return IMM3_OK;
}

// One tile pass (k_filter_tile): up to kMaxTileCols predicate columns.  `limit` stops the scan (Project.scala:73-80;
// Engine.scala:166,253-258: the reference's workers stall on the full queue once the consumer has its rows) -- over a table inside one
// launch (table_limit_applies), over one uniform segment as chunks of growing size (limit_scan_applies: run.chunked); every chunk
// first looks at the rows selected so far (a device word) and leaves at once when the limit has been reached -- nothing is read, no
// bitmap line written.  Enqueued blindly: no host wait.  TV_NO_LIMIT_CHUNKS: both off.
static int launch_tile_pass(imm3_query *q, SelectRun &run, const std::vector<const FoldedPred *> &take) {
    TileArgs a;
    int rc = fill_tile_args(q, run, take, a);
    if (rc) return rc;
    const TableLimitInputs ti = table_limit_inputs(q, run); // (decided before the stamp slot is claimed: the slot's grid is the launch's)
    if (table_limit_applies(ti)) rc = launch_tile_table_limit(q, run, a, ti.grid);
    else if (run.chunked) rc = launch_tile_chunks(q, run, a);
    else rc = launch_tile_plain(q, run, a);
    if (rc) return rc;
    ++run.pass;
    return IMM3_OK;
}

// A PFOR_INT pass: one compressed column per launch, decoded in LDS and compared in registers (k_filter_pfor)
static int launch_pfor_pass(imm3_query *q, SelectRun &run, const FoldedPred &fp) {
    imm3_ctx *ctx = q->ctx;
    const SegCol &sc = q->seg->cols[(size_t)fp.seg_col];
    PforArgs a;
    std::memset(&a, 0, sizeof(a));
    a.data = sc.d_data;
    a.block_off = sc.d_block_off;
    a.n_blocks = (int64_t)sc.block_rows.size();
    a.lo = (int32_t)fp.lo;
    a.hi = (int32_t)fp.hi;
    fill_pass_tail(q, run, a);
    a.status = (uint32_t *)(q->d_total + 2);
    // VALU/LDS-latency bound, 5 waves per SIMD resident: the finest grid balances best (measured 83 us at 2048
    // work-groups, 76 us at 4096, 100 M rows)
    run.grid = filter_grid(q->n_tiles, true, false, ctx->grid_blocks > 0 ? ctx->grid_blocks.load() : kMaxFilterGrid);
    {
        LaunchTimer t(ctx, 0);
        launch_filter_pfor(a, run.grid, run.s, t.start, t.stop);
    }
    HIPCHK(hipGetLastError());
    ++run.pass;
    return IMM3_OK;
}

// ---- the one-column passes (ColumnPassArgs, imm3_internal.h): one predicate's column per launch, a segment or a table's tile table.
// Each launcher below fills only what is its kernel's own and names its grid.
// the pass's head: the column of `fp`, flat and through the table's tile table, and the pass tail
static void fill_column_pass(const imm3_query *q, const SelectRun &run, const FoldedPred &fp, ColumnPassArgs &p) {
    p.data = col_flat(q->seg->cols[(size_t)fp.seg_col]);
    p.width = fp.width;
    fill_pass_tail(q, run, p);
    if (q->table) {
        p.tile_rows = q->table->d_tile_rows;
        p.tile_ptrs = (const void *const *)q->table->d_tile_ptrs[(size_t)fp.seg_col];
    }
}

// the pass's launch, `grid` work-groups under the select launch's timer; `refused`: what to say when the launcher takes no such arguments
template <class Args>
static int launch_column_pass(imm3_query *q, SelectRun &run, const Args &a, int grid, bool (*launch)(const Args &, int, hipStream_t, hipEvent_t, hipEvent_t), const char *refused) {
    run.grid = grid;
    {
        LaunchTimer t(q->ctx, 0);
        if (!launch(a, run.grid, run.s, t.start, t.stop)) return fail(IMM3_ERR_ARG, refused);
    }
    HIPCHK(hipGetLastError());
    ++run.pass;
    return IMM3_OK;
}

// The string pass of a range (k_filter_str_range)
static int launch_str_range_pass(imm3_query *q, SelectRun &run, const FoldedPred &fp) {
    StrRangeArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_column_pass(q, run, fp, a.pass);
    std::memcpy(a.lo, fp.range_lo4, sizeof(a.lo));
    std::memcpy(a.hi, fp.range_hi4, sizeof(a.hi));
    if (!fp.d_blob) return fail(IMM3_ERR_ARG, "internal: a string range without its bounds on the device");
    a.tails = (const uint32_t *)(fp.d_blob + 2 * (size_t)fp.width); // (behind the byte-for-byte bounds: str_range_pack)
    return launch_column_pass(q, run, a, str_rows_grid(q->n_tiles, q->ctx->grid_blocks), launch_filter_str_range, "internal: no string range kernel for this column width");
}

// A string pass (k_filter_str_rows): a column whose width is a multiple of 4
static int launch_str_rows_pass(imm3_query *q, SelectRun &run, const FoldedPred &fp) {
    if (fp.has_range) return launch_str_range_pass(q, run, fp);
    StrRowsArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_column_pass(q, run, fp, a.pass);
    a.n_match = (int32_t)fp.match.size();
    a.values = (const uint32_t *)fp.d_blob;
    if (!a.values) // (upload_match_blobs: width <= 8 and <= kMaxMatch values)
        for (size_t m = 0; m < fp.match.size() && m < (size_t)kMaxMatch; ++m) std::memcpy(a.inl[m], fp.match[m].data(), std::min<size_t>((size_t)fp.width, sizeof(a.inl[m])));
    return launch_column_pass(q, run, a, str_rows_grid(q->n_tiles, q->ctx->grid_blocks), launch_filter_str_rows, "internal: no string kernel for this column width");
}

// A list pass (k_filter_int_list): an int32 / int8 column with a folded IMM3_INT_IN list
static int launch_int_list_pass(imm3_query *q, SelectRun &run, const FoldedPred &fp) {
    IntListArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_column_pass(q, run, fp, a.pass);
    a.form = int_list_form(fp.width, pred_list_count(fp));
    a.lo = (int32_t)fp.lo;
    a.hi = (int32_t)fp.hi;
    if (a.form == INT_LIST_I8) std::memcpy(a.set, fp.list_set, sizeof(a.set));
    else if (a.form == INT_LIST_ARGS) {
        a.n_values = (int32_t)fp.list.size();
        for (size_t m = 0; m < (size_t)kMaxMatch; ++m) a.inl[m] = fp.list[m < fp.list.size() ? m : 0]; // (the kernel compares all kMaxMatch: a shorter list repeats its first value)
    } else {
        if (!fp.d_blob) return fail(IMM3_ERR_ARG, "internal: an integer list without its table on the device");
        a.table = (const int32_t *)fp.d_blob;
        a.mask = fp.list_mask;
        a.shift = fp.list_shift;
        a.max_probe = fp.list_max_probe;
        a.empty = fp.list_empty;
    }
    return launch_column_pass(q, run, a, int_list_grid(q->n_tiles, q->ctx->grid_blocks, fp.width), launch_filter_int_list, "internal: no integer list kernel for these arguments");
}

// A word-at-a-time pass (k_filter_generic) over up to kMaxPredCols of the chain's generic predicates from `first` on (none at all:
// the query without predicates on a layout the tile kernel does not take)
static int launch_generic_pass(imm3_query *q, SelectRun &run, size_t first) {
    imm3_ctx *ctx = q->ctx;
    FilterArgs a;
    std::memset(&a, 0, sizeof(a));
    const size_t take = std::min<size_t>(kMaxPredCols, run.chain.generic.size() - first);
    for (size_t i = 0; i < take; ++i) fill_colpred(q, *run.chain.generic[first + i], a.cols[i]);
    a.ncols = (int32_t)take;
    fill_pass_tail(q, run, a);
    a.word_row_base = q->d_word_row_base;
    a.word_nvalid = q->d_word_nvalid;
    run.grid = filter_grid(q->n_words, true, false, ctx->grid_blocks);
    {
        LaunchTimer t(ctx, 0);
        launch_filter_generic(a, run.grid, run.s, t.start, t.stop);
    }
    HIPCHK(hipGetLastError());
    ++run.pass;
    return IMM3_OK;
}

// The last pass's per-workgroup partials -> selected-row count (+ rows ProjectOp will emit): k_total
static int launch_count_reduce(imm3_query *q, const SelectRun &run) {
    imm3_ctx *ctx = q->ctx;
    TotalArgs ta;
    std::memset(&ta, 0, sizeof(ta));
    ta.block_partials = q->d_block_partials;
    ta.n_partials = run.grid;
    ta.total = q->d_total;
    ta.n_emit = q->d_n_emit;
    ta.limit = q->limit;
    hipStream_t ts = run.s;
    if (run.overlap_total) {
        // nothing downstream on the main stream needs the count: reduce it on the aux stream so the next scan
        // starts right behind this one (saves the reduce kernel and two dependent-launch gaps per step)
        {
            std::lock_guard<std::mutex> lk(ctx->mu);
            if (!ctx->aux) HIPCHK(hipStreamCreateWithFlags(&ctx->aux, hipStreamNonBlocking));
        }
        if (!q->ev_filter_done) {
            HIPCHK(hipEventCreateWithFlags(&q->ev_filter_done, hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&q->ev_total_done, hipEventDisableTiming));
        }
        HIPCHK(hipEventRecord(q->ev_filter_done, run.s));
        HIPCHK(hipStreamWaitEvent(ctx->aux, q->ev_filter_done, 0));
        ts = ctx->aux;
    }
    {
        LaunchTimer t(ctx, 3);
        launch_total(ta, ts, t.start, t.stop);
    }
    if (run.overlap_total) {
        HIPCHK(hipEventRecord(q->ev_total_done, ctx->aux));
        q->total_on_aux = true;
    }
    return IMM3_OK;
}

// ScanOp -> SelectOp*: the bitmap and the count of the query's predicates, one launcher per pass of the chain
int imm3::run_select(imm3_query *q, unsigned mode) {
    imm3_ctx *ctx = q->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    SelectRun run;
    run.mode = mode;
    run.overlap_total = mode & SEL_OVERLAP_TOTAL;
    run.count_in_scan = mode & SEL_COUNT_IN_SCAN;
    run.count_only = mode & SEL_COUNT_ONLY;
    run.s = ctx->stream;
    {   // the previous run's reduce may still be reading block_partials / writing total on the aux stream
        const int jrc = join_total(q, run.s);
        if (jrc) return jrc;
        q->total_on_aux = false;
    }
    q->run.offsets_valid = false; // (a new bitmap)
    q->run.select_partial = false;
    q->hi16_ran = false;
    q->run.agg_select_skipped = false; // (... and a new count: a fused aggregation's select is no longer owed -- behind imm3_query_run_count imm3_query_bitmap refuses, it does not run the chain)
    if (q->always_false || q->n_tiles == 0) {
        // an empty interval / empty IN-list clears every bit; nothing to read
        HIPCHK(hipMemsetAsync(q->d_total, 0, 2 * sizeof(unsigned long long), run.s)); // (an always-false query logs nothing)
        HIPCHK(hipMemsetAsync(q->d_bitmap, 0, (size_t)std::max<int64_t>(q->n_tiles * kTileWords, 1) * sizeof(uint64_t), run.s));
        q->run.ran_select = true;
        q->run.bitmap_valid = true;
        q->run.ran_single_pass = false;
        return IMM3_OK;
    }
    // (planned on every run: the tuning variant may have changed since creation)
    if (!q->is_expr) run.chain = plan_select_chain(q); // (a select tree is ONE launch of its own: no chain)
    if (q->expr_universal) q->expr_form_ran = run.chain.tile_passes.empty() ? 1 : 0; // (a tree that selects every row: the NoSelect scan, tile or word at a time)
    // (a table has no word-at-a-time kernel.  Creation has refused the predicates that need it; what is left here is the tools'
    // TV_GENERIC_ONLY tuning variant, which sends every predicate there)
    if (q->table && !run.chain.generic.empty()) return fail(IMM3_ERR_ARG, kTableGenericRefusal);
    run.fv = ctx->filter_variant;
    q->run.stage_written = false;
    q->run.bitmap_lazy = false;
    q->run.ran_single_pass = false;
    run.tree_tile = q->is_expr && q->expr_tile_ok && run.fv != TV_GENERIC_ONLY;
    // (a table has no generic kernel, so the tools' TV_GENERIC_ONLY tuning variant has nothing to run for a table tree: imm3_diag.h)
    if (q->is_expr && q->table && !run.tree_tile)
        return fail(IMM3_ERR_ARG, "a select tree over a table runs through the tile kernel only (the generic-only tuning variant "
                                  "does not apply to a table); use per-segment queries");
    // exactly ONE launch in the whole select chain: only then may that launch publish the count (and append to the count
    // log) itself, and only then are the survivors' values staged
    run.skip_bitmap = run.count_only && (run.chain.single_tile_pass || run.tree_tile) && !q->table && !run.overlap_total && run.fv != TV_COUNT_BY_K_TOTAL;
    q->run.bitmap_valid = !run.skip_bitmap;
    run.chunked = limit_scan_applies(limit_scan_inputs(q, run)); // (launch_tile_pass)
    int rc = IMM3_OK;
    if (q->is_expr) rc = launch_tree_pass(q, run);
    for (size_t i = 0; !rc && i < run.chain.tile_passes.size(); ++i) rc = launch_tile_pass(q, run, run.chain.tile_passes[i]);
    if (rc) return rc;
    q->run.has_pfor_pass = !run.chain.pfor.empty();
    for (size_t i = 0; !rc && i < run.chain.pfor.size(); ++i) rc = launch_pfor_pass(q, run, *run.chain.pfor[i]);
    for (size_t i = 0; !rc && i < run.chain.str_passes.size(); ++i) rc = launch_str_rows_pass(q, run, *run.chain.str_passes[i]);
    for (size_t i = 0; !rc && i < run.chain.list_passes.size(); ++i) rc = launch_int_list_pass(q, run, *run.chain.list_passes[i]);
    const bool need_empty_generic = q->preds.empty() && run.pass == 0;
    for (size_t gi = 0; !rc && (gi < run.chain.generic.size() || (need_empty_generic && run.pass == 0)); gi += kMaxPredCols) rc = launch_generic_pass(q, run, gi);
    if (rc) return rc;
    q->run.count_pending_scan = !run.count_done && run.count_in_scan;
    if (!run.count_done && !run.count_in_scan) rc = launch_count_reduce(q, run);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    q->run.ran_select = true;
    return IMM3_OK;
}

// the SELECT-list columns as the unpacking kernels take them: gathered columns first, then the ones the record carries
// (every mention of a staged column reads the record; the plan counts only the first as riding in it: proj_rides_in_records)
static int fill_emit_cols(const imm3_query *q, EmitCol *out, int &n_out) {
    std::vector<EmitCol> gathered, staged;
    for (size_t j = 0; j < q->proj.size(); ++j) {
        const int32_t sci = q->used[(size_t)q->proj[j]];
        const SegCol &sc = q->seg->cols[(size_t)sci];
        EmitCol c;
        std::memset(&c, 0, sizeof(c));
        c.dst = q->d_proj[j];
        c.width = sc.width;
        c.rec_dword = -1;
        for (int k = 0; k < kMaxTileCols; ++k)
            if (q->stage_seg_col[k] == sci) {
                const RecField f = rec_layout(q->stage_kinds, k);
                c.rec_dword = f.dword;
                c.rec_shift = f.shift;
            }
        if (c.rec_dword < 0) { c.src = col_flat(sc); gathered.push_back(c); }
        else staged.push_back(c);
    }
    int n = 0;
    for (const auto &c : gathered) out[n++] = c;
    for (const auto &c : staged) out[n++] = c;
    n_out = n;
    return (int)gathered.size();
}

void imm3::fill_tile_col(const imm3_query *q, const FoldedPred &fp, TileCol &c, int kind) {
    c.data = col_flat(q->seg->cols[(size_t)fp.seg_col]);
    c.lo = (int32_t)fp.lo;
    c.hi = (int32_t)fp.hi;
    if (kind == TK_S2) {
        c.n_match = (int32_t)fp.match.size();
        c.negated = fp.negated ? 1 : 0;
        for (size_t m = 0; m < fp.match.size(); ++m)
            c.match[m] = (uint32_t)(uint8_t)fp.match[m][0] | ((uint32_t)(uint8_t)fp.match[m][1] << 8);
    }
}

// Per-device state of the single-pass projection kernel, whose work-groups wait on each other and therefore must own the
// device while they run (imm3_project.hip): launches of all contexts of a device are chained through one event -- each
// starts behind the previous one, stream side, no host wait -- and a device word holds the running launch's ticket for
// whatever the host cannot order (graph replays, other processes on the same GPU).  Internal synchronisation state, guarded
// by its mutex; it lives as long as the process.
namespace {
struct SinglePassDevice {
    std::mutex mu;
    hipEvent_t last = nullptr;            // recorded behind the last launch
    unsigned long long *d_lock = nullptr; // the ticket word
};
SinglePassDevice g_single_pass[kMaxDevices];
} // namespace

static int single_pass_device(int device, SinglePassDevice **out) {
    if (device < 0 || device >= kMaxDevices) return fail(IMM3_ERR_ARG, "device index out of range");
    SinglePassDevice &d = g_single_pass[device];
    std::lock_guard<std::mutex> lk(d.mu);
    if (!d.d_lock) {
        void *p = nullptr;
        HIPCHK(hipMalloc(&p, 64));
        HIPCHK(hipMemset(p, 0, 64));
        d.d_lock = (unsigned long long *)p;
        HIPCHK(hipEventCreateWithFlags(&d.last, hipEventDisableTiming));
    }
    *out = &d;
    return IMM3_OK;
}

#ifdef IMM3_ABLATE
int imm3::single_pass_lock_word(int device, unsigned long long **out) {
    SinglePassDevice *dev = nullptr;
    const int rc = single_pass_device(device, &dev);
    if (rc) return rc;
    *out = dev->d_lock;
    return IMM3_OK;
}
#endif

// the one launch's predicate columns (and the SELECT-list columns streamed with them), in the order the plan laid out
static int single_pass_pred_cols(const imm3_query *q, ProjectArgs &a) {
    for (int k = 0; k < kMaxTileCols; ++k) {
        a.kinds[k] = q->stage_kinds[k];
        if (a.kinds[k] == TK_NONE) continue;
        const FoldedPred *fp = nullptr;
        for (const auto &p : q->preds)
            if (p.seg_col == q->stage_seg_col[k]) fp = &p;
        for (const auto &p : q->sp_pass) // (a streamed SELECT-list column: every value passes)
            if (p.seg_col == q->stage_seg_col[k]) fp = &p;
        if (!fp) return fail(IMM3_ERR_ARG, "internal: single-pass plan lost a predicate column");
        fill_tile_col(q, *fp, a.cols[k], a.kinds[k]);
    }
    return IMM3_OK;
}

// a communicator may have been attached or destroyed since the plan was made: the grid follows, and so does the planned P
// (a P the host has lowered for dense survivors stays: it is below either plan)
static void single_pass_follow_comms(imm3_query *q, hipStream_t s) {
    const int32_t want_plan = q->sp_P_plan_for[single_pass_reserves(q) ? 1 : 0];
    if (!q->sp_P_fixed && !q->ctx->capture && want_plan > 0 && want_plan != q->sp_P_plan) {
        const bool at_plan = q->sp_P == q->sp_P_plan;
        q->sp_P_plan = want_plan;
        if (at_plan || q->sp_P > want_plan) {
            if (hipMemsetAsync(q->d_desc, 0, q->sp_trash_off, s) == hipSuccess) single_pass_set_P(q, want_plan); // (hygiene, as in single_pass_pick_P)
            else (void)hipGetLastError();
        }
    }
    q->sp_grid = single_pass_run_grid(q);
}

// SELECT-list columns: the first mention of a predicate column comes out of the records, everything else is gathered
static int single_pass_select_list(const imm3_query *q, ProjectArgs &a) {
    int ng = 0;
    for (size_t j = 0; j < q->proj.size(); ++j) {
        const int32_t sci = q->used[(size_t)q->proj[j]];
        const SegCol &sc = q->seg->cols[(size_t)sci];
        int k_pred = -1;
        for (int k = 0; k < kMaxTileCols; ++k)
            if (q->stage_seg_col[k] == sci && !a.pred_dst[k]) { k_pred = k; break; }
        if (k_pred >= 0) a.pred_dst[k_pred] = q->d_proj[j];
        else {
            if (ng >= kMaxEmitGather || q->table) return fail(IMM3_ERR_ARG, "internal: single-pass plan has too many gathered columns");
            a.gather[ng].dst = q->d_proj[j];
            a.gather[ng].src = col_flat(sc);
            a.gather[ng].width = sc.width;
            ++ng;
        }
    }
    a.n_gather = ng;
    return IMM3_OK;
}

// ScanOp -> SelectOp* -> ProjectOp in one launch (k_filter_project): bitmap, count and the projected rows
static int run_single_pass(imm3_query *q) {
    imm3_ctx *ctx = q->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    {
        const int jrc = join_total(q, s);
        if (jrc) return jrc;
        q->total_on_aux = false;
    }
    // The rows are written by the filter kernel itself, so their arrays exist before the count does: the caller's
    // reservation, else room for every row of the segment (pooled: allocated once).  A reservation that turns out too
    // small is answered from the bitmap when the rows are fetched (settle_rows).
    if (!q->reserved && q->cap_rows < (uint64_t)q->n_rows) {
        const int rc = ensure_row_capacity(q, (uint64_t)q->n_rows);
        if (rc) return rc;
    }
    ProjectArgs a;
    std::memset(&a, 0, sizeof(a));
    int arc = single_pass_pred_cols(q, a);
    if (arc) return arc;
    single_pass_follow_comms(q, s);
    a.P = q->sp_P;
    a.n_rows = q->n_rows;
    if (q->table) {
        if (!q->d_tile_desc) return fail(IMM3_ERR_STATE, "internal: table query planned as one launch without its tile descriptors");
        a.tile_desc = q->d_tile_desc;
        a.n_rows = q->n_tiles * kTileRows; // (virtual rows: what the tiles span; the kernel takes a tile's valid rows from its descriptor)
    }
    a.n_tiles = q->n_tiles;
    a.n_spans = q->sp_spans;
    a.n_rounds = (q->sp_spans + q->sp_grid - 1) / q->sp_grid;
    a.bitmap = q->d_bitmap;
    a.finish = q->d_total;
    a.desc = (unsigned long long *)((uint8_t *)q->d_desc + q->sp_desc_off);
    a.round_total = q->d_desc;
    a.round_ctr = (uint32_t *)(q->d_desc + q->sp_rounds_max);
    a.trash = (uint8_t *)q->d_desc + q->sp_trash_off;
    a.cap_rows = q->cap_rows;
    a.row_index = q->d_row_index;
    arc = single_pass_select_list(q, a);
    if (arc) return arc;
    a.ablate = project_ablation(ctx->filter_variant); // (tools' build only: a mask -- 1 no unpack, 2 no chained scan, 4 no records, 16 no output stores, 32 plain instead of non-temporal stores in the straight copy of fully surviving dense ranges)
    a.max_polls = ctx->fault_max_polls; // (tools' build only: imm3_ctx_inject_fault)
    a.fault_wg = ctx->fault_wg;
    a.fault_span = ctx->fault_span;
    a.stamps = claim_stamp_slot(ctx, q->sp_grid);
    SinglePassDevice *dev = nullptr;
    {
        const int drc = single_pass_device(ctx->device, &dev);
        if (drc) return drc;
    }
    a.device_lock = dev->d_lock;
    {
        std::lock_guard<std::mutex> lk(dev->mu); // (wait - launch - record is one step: the next launcher waits for THIS launch)
        const bool chained = !ctx->capture;      // (a capture cannot depend on an event recorded outside it: the device lock covers replays)
        if (chained) HIPCHK(hipStreamWaitEvent(s, dev->last, 0));
        {
            LaunchTimer t(ctx, 0);
            const bool launched = q->table ? launch_filter_project_table(a, q->sp_grid, s, t.start, t.stop) : launch_filter_project(a, q->sp_grid, s, t.start, t.stop);
            if (!launched) return fail(IMM3_ERR_ARG, "internal: no single-pass kernel for this column combination");
        }
        HIPCHK(hipGetLastError());
        if (chained) HIPCHK(hipEventRecord(dev->last, s));
    }
    q->run.stage_written = false;
    q->run.count_pending_scan = false;
    q->run.has_pfor_pass = false;
    q->run.ran_select = true;
    q->run.bitmap_valid = true;
    q->run.ran_project = true;
    q->run.ran_single_pass = true;
    q->run.sp_verified = false;
    q->run.offsets_valid = false;
    return IMM3_OK;
}

// ProjectOp from the survivor records the select launch staged
static int launch_emit_records(imm3_query *q) {
    imm3_ctx *ctx = q->ctx;
    EmitArgs e;
    std::memset(&e, 0, sizeof(e));
    e.stage = q->d_stage_rec;
    e.tile_start = q->d_tile_start;
    e.wave_cap = q->stage_wave_cap;
    e.n_waves = (int64_t)q->stage_grid * kWavesPerBlock;
    e.main_tiles = q->stage_main_tiles;
    e.max_slots = q->stage_max_slots;
    e.T = q->stage_T;
    e.ablate = emit_ablation(ctx->filter_variant); // (tools' build only)
    e.tile_offsets = q->d_tile_offsets;
    e.chunk_sums = q->d_chunk_sums;
    e.n_tiles = q->n_tiles;
    e.cap_rows = q->cap_rows;
    e.row_index = q->d_row_index;
    e.R = rec_layout(q->stage_kinds, -1).dwords;
    int n_cols = 0;
    const int n_gather = fill_emit_cols(q, e.cols, n_cols);
    e.n_cols = n_cols;
    LaunchTimer t(ctx, 2);
    launch_emit(e, n_gather, 0, ctx->stream, t.start, t.stop);
    HIPCHK(hipGetLastError());
    return IMM3_OK;
}

int imm3::launch_project(imm3_query *q) {
    imm3_ctx *ctx = q->ctx;
    hipStream_t s = ctx->stream;
    q->run.order_valid = false; // (the rows are emitted again: whoever does that orders them again -- run_query, settle_rows)
    if (q->run.stage_written) return launch_emit_records(q);
    GatherArgs g;
    std::memset(&g, 0, sizeof(g));
    g.bitmap = q->d_bitmap;
    g.tile_offsets = q->d_tile_offsets;
    g.chunk_sums = q->d_chunk_sums;
    g.n_tiles = q->n_tiles;
    g.n_words = q->n_words;
    g.limit = q->limit;
    g.cap_rows = q->cap_rows;
    g.n_staged_tiles = 0;
    g.word_row_base = q->d_word_row_base;
    g.tile_rows = q->table ? q->table->d_tile_rows : nullptr;
    g.scanned_tiles = q->run.select_partial ? q->d_total + kFinishLimitTiles : nullptr;
    // more SELECT-list columns than one launch carries: gather in groups (row indices written by the first)
    size_t done = 0;
    const size_t np = q->proj.size();
    do {
        const size_t take = std::min<size_t>(kMaxProj, np - done);
        g.row_index = done == 0 ? q->d_row_index : nullptr;
        g.n_proj = (int32_t)take;
        for (size_t j = 0; j < take; ++j) {
            const SegCol &sc = q->seg->cols[(size_t)q->used[(size_t)q->proj[done + j]]];
            g.proj[j].src = col_flat(sc);
            g.proj[j].tile_ptrs = q->table ? (const void *const *)q->table->d_tile_ptrs[(size_t)q->used[(size_t)q->proj[done + j]]] : nullptr;
            g.proj[j].dst = q->d_proj[done + j];
            g.proj[j].width = sc.width;
            g.proj[j].staged = nullptr;
        }
        {
            LaunchTimer t(ctx, 2);
            launch_gather(g, 0, s, t.start, t.stop);
        }
        HIPCHK(hipGetLastError());
        done += take;
    } while (done < np);
    return IMM3_OK;
}

// A small limit behind a limit scan: the offsets scan and the gather in ONE launch over the scanned tiles (k_limit_gather).
// `select id ... limit 10`: 7 + 9 us of k_scan + k_gather -> ~5.  TV_LIMIT_NO_FUSED_GATHER: off.
constexpr int kLimitGatherGrid = 256;
static bool limit_gather_applies(const imm3_query *q) {
    if (!q->run.select_partial || !(q->limit > 0) || q->limit > kLimitGatherMaxRows || q->table || q->d_word_row_base || q->run.stage_written || q->ctx->filter_variant == TV_LIMIT_NO_FUSED_GATHER) return false;
    if (q->n_chunks > (int64_t)kLimitGatherGrid * kLimitGatherMaxChunks || q->proj.size() > (size_t)kMaxProj || !q->d_limit_state) return false;
    for (int32_t pj : q->proj) {
        const SegCol &sc = q->seg->cols[(size_t)q->used[(size_t)pj]];
        if (!col_flat(sc) || (sc.width != 1 && sc.width != 2 && sc.width != 4)) return false;
    }
    return true;
}
static int launch_limit_gather_for(imm3_query *q) {
    imm3_ctx *ctx = q->ctx;
    LimitGatherArgs g;
    std::memset(&g, 0, sizeof(g));
    g.bitmap = q->d_bitmap;
    g.finish = q->d_total;
    g.wg_state = q->d_limit_state;
    g.n_tiles = q->n_tiles;
    g.limit = q->limit;
    g.cap_rows = q->cap_rows;
    g.row_index = q->d_row_index;
    g.n_proj = (int32_t)q->proj.size();
    g.fault_wg = ctx->fault_wg;        // (tools' build only: imm3_ctx_inject_fault)
    g.max_polls = ctx->fault_max_polls;
    for (size_t j = 0; j < q->proj.size(); ++j) {
        const SegCol &sc = q->seg->cols[(size_t)q->used[(size_t)q->proj[j]]];
        g.proj[j].src = col_flat(sc);
        g.proj[j].dst = q->d_proj[j];
        g.proj[j].width = sc.width;
    }
    LaunchTimer t(ctx, 2);
    launch_limit_gather(g, (int)std::min<int64_t>(kLimitGatherGrid, std::max<int64_t>(q->n_chunks, 1)), ctx->stream, t.start, t.stop);
    HIPCHK(hipGetLastError());
    return IMM3_OK;
}

// the offsets scan behind a select of the same run (k_scan): tile offsets, chunk sums and, where the select left it to the scan, the count
static int launch_offsets_scan(imm3_query *q) {
    imm3_ctx *ctx = q->ctx;
    ScanArgs sa;
    std::memset(&sa, 0, sizeof(sa));
    sa.bitmap = q->d_bitmap;
    sa.tile_offsets = q->d_tile_offsets;
    sa.chunk_sums = q->d_chunk_sums;
    sa.n_tiles = q->n_tiles;
    sa.finish = q->run.count_pending_scan ? q->d_total : nullptr;
    sa.scanned_tiles = q->run.select_partial ? q->d_total + kFinishLimitTiles : nullptr;
    if (q->run.stage_written && q->run.bitmap_lazy) { // no bitmap was stored: the tiles' counts come from the records' start table
        sa.rec_tile_start = q->d_tile_start;
        sa.rec_n_waves = (int64_t)q->stage_grid * kWavesPerBlock;
        sa.rec_main_tiles = q->stage_main_tiles;
        sa.rec_max_slots = q->stage_max_slots;
        sa.rec_T = q->stage_T;
    }
    {
        LaunchTimer t(ctx, 1);
        launch_scan(sa, ctx->stream, t.start, t.stop);
    }
    HIPCHK(hipGetLastError());
    q->run.offsets_valid = true;
    return IMM3_OK;
}

// for the cost model, where the survivors are, from the offsets scan's per-chunk counts of a first run that selected `total` rows
static void note_survivor_density(imm3_query *q, unsigned long long total, const std::vector<uint32_t> &chunk_counts) {
    if (chunk_counts.empty() || !(total > 0)) return;
    const double chunk_rows = (double)kChunkTiles * kTileRows;
    double sum = 0.0, sum_sq = 0.0, sum_full = 0.0;
    for (size_t i = 0; i < chunk_counts.size(); ++i) {
        const double c = (double)chunk_counts[i];
        sum += c;
        sum_sq += c * c;
        if (c >= chunk_rows) sum_full += c;
    }
    if (sum > 0.0) {
        q->plan_density.sigma = (double)total / (double)std::max<int64_t>(q->n_rows, 1);
        q->plan_density.sloc = std::min(1.0, std::max(q->plan_density.sigma, sum_sq / (sum * chunk_rows)));
        q->plan_density.full = sum_full / sum;
        q->plan_have_density = true;
    }
}

static int run_project(imm3_query *q) {
    imm3_ctx *ctx = q->ctx;
    hipStream_t s = ctx->stream;
    if (q->n_tiles > 0 && limit_gather_applies(q)) {
        if (!q->d_row_index) {
            const int rc = ensure_row_capacity(q, 1);
            if (rc) return rc;
        }
        const int rc = launch_limit_gather_for(q);
        if (rc) return rc;
        q->run.offsets_valid = false; // (no offsets scan has run on this bitmap)
        q->run.ran_project = true;
        q->run.limit_gather_ran = true;
        return IMM3_OK;
    }
    q->run.limit_gather_ran = false;
    if (q->n_tiles > 0) {
        const int rc = launch_offsets_scan(q);
        if (rc) return rc;
    }
    if (!(q->limit > 0) && !q->reserved && !q->d_row_index) {
        // Unlimited projection, no reservation, FIRST run: the output size is the count -> one synchronisation.  The arrays get
        // an eighth of headroom and every later run of the query writes into them without asking: a steady-state projecting
        // query never synchronises (a run that outgrows them is detected when its rows are fetched, and emitted again).
        unsigned long long total = 0;
        HIPCHK(hipMemcpyAsync(&total, q->d_total, sizeof(total), hipMemcpyDeviceToHost, s));
        // ... and, for the cost model, where the survivors are: the offsets scan's per-chunk counts (256 tiles each; 1.5 KB for 100 M
        // rows) say how densely they sit where they sit and how many of them in fully surviving chunks -- the whole segment, where
        // the sample at creation saw 0.5 % of it (a range of a sorted key between two sample chunks showed it nothing)
        std::vector<uint32_t> chunk_counts;
        if (!q->plan_pinned && !q->table && q->n_chunks > 0 && q->n_chunks <= (1 << 20) && q->run.offsets_valid) {
            chunk_counts.resize((size_t)q->n_chunks);
            HIPCHK(hipMemcpyAsync(chunk_counts.data(), q->d_chunk_sums, chunk_counts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipStreamSynchronize(s));
        ++q->run_syncs;
        note_survivor_density(q, total, chunk_counts);
        {   // enough survivors for the gathered columns to be streamed instead?  Then this run is done again as one launch
            const int src = single_pass_stream_columns(q, total);
            if (src) return src;
            if (q->single_pass) return run_single_pass(q);
            if (single_pass_restore_wanted(q, total)) {
                q->sp_restore_pending = true; // (from the next run on)
                q->sp_restore_survivors = total;
            }
            records_drop_if_narrow(q, total); // (this run's rows then come from the bitmap)
            if (!q->d_stage_rec && q->run.bitmap_lazy) { // ... which the staging launch did not store: the select chain runs once more, plainly (the offsets stand: same counts)
                const int prc = run_select(q, SEL_WHOLE);
                if (prc) return prc;
                q->run.offsets_valid = true;
            }
        }
        const unsigned long long want = std::min<unsigned long long>((unsigned long long)std::max<int64_t>(q->n_rows, 1), total + total / 8 + 1024);
        const int rc = ensure_row_capacity(q, want);
        if (rc) return rc;
    } else if (!q->d_row_index) {
        const int rc = ensure_row_capacity(q, 1);
        if (rc) return rc;
    }
    if (q->n_tiles > 0) {
        const int rc = launch_project(q);
        if (rc) return rc;
    }
    q->run.ran_project = true;
    return IMM3_OK;
}

// ORDER BY behind the rows as last emitted (imm3_order.hip): key build, the radix select when a limit is set, one LSD pass per key
// byte, apply.  Every launch reads the row count and what the launches before it decided from device words: enqueued blindly.
int imm3::run_order(imm3_query *q) {
    imm3_ctx *ctx = q->ctx;
    hipStream_t s = ctx->stream;
    if (!q->ordered) return IMM3_OK;
    if (q->n_tiles <= 0) { // (nothing was emitted and no row-count word was written: the ordered result is empty)
        q->run.order_valid = true;
        return IMM3_OK;
    }
    {
        const int rc = ensure_order_buffers(q);
        if (rc) return rc;
    }
    OrderArgs a;
    std::memset(&a, 0, sizeof(a));
    a.n_emit = q->d_n_emit;
    a.cap_rows = q->cap_rows;
    a.limit = q->order_limit;
    a.n_cols = (int32_t)q->order_keys.size();
    for (int c = 0; c < a.n_cols; ++c) {
        const imm3_order_key &k = q->order_keys[(size_t)c];
        const SegCol &sc = q->seg->cols[(size_t)q->used[(size_t)q->proj[(size_t)k.proj]]];
        a.cols[c].src = q->d_proj[(size_t)k.proj];
        a.cols[c].width = sc.width;
        a.cols[c].kind = sc.vcodec == IMM3_DENSE_INT ? KIND_I32 : (sc.vcodec == IMM3_DENSE_TINYINT ? KIND_I8 : KIND_STR);
        a.cols[c].descending = k.descending ? 1 : 0;
    }
    a.key_bytes = q->order_key_bytes;
    a.key_words = (q->order_key_bytes + 3) / 4;
    a.force_full = ctx->filter_variant == TV_ORDER_FULL_SORT ? 1 : (ctx->filter_variant == TV_ORDER_SELECT_ALWAYS ? 2 : 0); // (0: the device decides)
    for (int b = 0; b < 2; ++b) {
        a.keys[b] = q->d_order_keys[b];
        a.perm[b] = q->d_order_perm[b];
    }
    a.state = q->d_order_state;
    a.counts = q->d_order_counts;
    a.diff = q->d_order_diff;
    a.tally = q->d_order_tally;
    LaunchTimer t(ctx, 7); // (one record for the whole order: from its first kernel's start to its last one's end)
    launch_order_keys(a, s, t.start, nullptr);
    if (q->order_limit > 0) launch_order_select(a, s, nullptr, nullptr);
    for (int p = a.key_bytes - 1; p >= 0; --p) { // least significant byte first
        a.byte_pos = p;
        launch_order_pass(a, s, nullptr, nullptr);
    }
    HIPCHK(hipGetLastError());
    OrderApplyArgs ap;
    std::memset(&ap, 0, sizeof(ap));
    ap.perm[0] = q->d_order_perm[0];
    ap.perm[1] = q->d_order_perm[1];
    ap.state = q->d_order_state;
    ap.key_bytes = a.key_bytes;
    const size_t np = q->proj.size();
    size_t done = 0;
    do { // more SELECT-list columns than one launch carries: in groups, as the gather (the row indices with the first)
        const size_t take = std::min<size_t>(kMaxProj, np - done);
        ap.row_index = done == 0 ? q->d_row_index : nullptr;
        ap.row_index_out = q->d_order_row_index;
        ap.n_cols = (int32_t)take;
        for (size_t j = 0; j < take; ++j) {
            ap.cols[j].src = q->d_proj[done + j];
            ap.cols[j].dst = q->d_order_proj[done + j];
            ap.cols[j].width = q->seg->cols[(size_t)q->used[(size_t)q->proj[done + j]]].width;
        }
        done += take;
        launch_order_apply(ap, s, nullptr, done >= np ? t.stop : nullptr);
    } while (done < np);
    HIPCHK(hipGetLastError());
    ++q->order_launches;
    q->run.order_valid = true;
    return IMM3_OK;
}

// a run recorded into an open capture: nothing in it may synchronise, allocate or use a second stream
static int capture_admit(imm3_query *q) {
    imm3_ctx *ctx = q->ctx;
    if (!ctx->capture) return IMM3_OK;
    if (q->ordered) return fail(IMM3_ERR_STATE, "an ordered query (imm3_query_set_order) cannot be run inside a graph capture: graph replay of ordered queries is not supported");
    if (ctx->filter_variant == TV_COUNT_ON_AUX) return fail(IMM3_ERR_STATE, "tuning variant 2 (count reduce on the aux stream) cannot be captured");
    const bool sp = q->single_pass && !q->proj.empty() && !q->always_false && q->n_tiles > 0; // (writes its rows without knowing the count)
    if (!q->proj.empty() && !(q->limit > 0) && !q->reserved && !sp && !q->d_row_index)
        return fail(IMM3_ERR_STATE, "an unlimited projection sizes its output from the count on its first run (a synchronisation): run it once, or call imm3_query_reserve_rows, before capturing it");
    if (sp && !q->reserved && q->cap_rows < (uint64_t)q->n_rows)
        return fail(IMM3_ERR_STATE, "run the query once (or reserve rows) before capturing it: its output buffers are allocated on first use");
    if (!q->proj.empty() && !q->d_row_index) return fail(IMM3_ERR_STATE, "run the query once (or reserve rows) before capturing it: its output buffers are allocated on first use");
    auto &qs = ctx->capture->queries;
    if (std::find(qs.begin(), qs.end(), q) == qs.end()) {
        qs.push_back(q);
        ctx->capture->states.emplace_back();
        ctx->capture->live.push_back(q->run);
    }
    return IMM3_OK;
}

// the run has been recorded: what it leaves in the handle is what every replay of the graph leaves (imm3_graph_launch)
static int capture_note(imm3_query *q, int rc) {
    imm3_ctx *ctx = q->ctx;
    if (rc || !ctx->capture) return rc;
    auto &qs = ctx->capture->queries;
    const auto it = std::find(qs.begin(), qs.end(), q);
    if (it == qs.end()) return rc;
    ctx->capture->states[(size_t)(it - qs.begin())] = q->run;
    return rc;
}

// The three run calls: the context's capture gate held for the whole run, the run admitted into an open capture and noted there
// (capture_note); `plan` is what the call launches.
static int run_entry(imm3_query *q, int (*plan)(imm3_query *)) {
    if (!q) return fail(IMM3_ERR_ARG, "query is null");
    CTX_LIVE_RUN(q->ctx);
    const int ca = capture_admit(q);
    if (ca) return ca;
    q->run.ran_project = false;
    q->run.rows_moved = false;
    return capture_note(q, plan(q));
}

extern "C" int imm3_query_run_select(imm3_query *q) {
    return run_entry(q, [](imm3_query *r) { return run_select(r, r->ctx->filter_variant == TV_COUNT_ON_AUX ? SEL_OVERLAP_TOTAL : SEL_DEFAULT); });
}

extern "C" int imm3_query_run_count(imm3_query *q) {
    return run_entry(q, [](imm3_query *r) { return run_select(r, SEL_COUNT_ONLY); });
}

extern "C" int imm3_query_join_count(imm3_query *q) {
    if (!q) return fail(IMM3_ERR_ARG, "query is null");
    CTX_LIVE(q->ctx);
    HIPCHK(hipSetDevice(q->ctx->device));
    return imm3::join_query_count(q);
}

static int run_query(imm3_query *q) {
    // Reducing the count on the aux stream (TV_COUNT_ON_AUX) measured SLOWER on MI355X / ROCm 7.2 (75.6 vs 67.1 us
    // per step: the cross-queue event packets cost more than the two same-queue launch gaps they remove), so the
    // default keeps the reduce on the main stream.
    if (q->sp_restore_pending && !q->ctx->capture) {
        const int rrc = single_pass_restore(q, q->sp_restore_survivors);
        if (rrc) return rrc;
    }
    if (q->single_pass && !q->proj.empty() && !q->always_false && q->n_tiles > 0) {
        const int src = run_single_pass(q);
        return src ? src : run_order(q);
    }
    const bool select_only = q->proj.empty() && !q->is_agg && q->ctx->filter_variant == TV_COUNT_ON_AUX;
    const bool count_in_scan = !q->proj.empty() && q->n_tiles > 0 && !q->always_false && q->ctx->filter_variant != TV_COUNT_BY_K_TOTAL;
    int rc = IMM3_OK;
    q->run.agg_select_skipped = agg_run_fuses(q);
    if (q->run.agg_select_skipped) q->run.ran_select = true; // (bitmap and count on demand: settle_agg_select)
    else rc = run_select(q, (select_only ? SEL_OVERLAP_TOTAL : SEL_DEFAULT) | (count_in_scan ? SEL_COUNT_IN_SCAN : SEL_DEFAULT));
    if (rc) return rc;
    if (!q->proj.empty()) rc = run_project(q);
    if (!rc && q->ordered) rc = run_order(q);
    if (!rc && q->is_agg) rc = run_agg(q);
    return rc;
}

extern "C" int imm3_query_run(imm3_query *q) { return run_entry(q, run_query); }

extern "C" int imm3_query_sync(imm3_query *q) {
    if (!q) return fail(IMM3_ERR_ARG, "query is null");
    CTX_LIVE(q->ctx);
    HIPCHK(hipSetDevice(q->ctx->device));
    HIPCHK(hipStreamSynchronize(q->ctx->stream));
    if (q->ctx->aux) HIPCHK(hipStreamSynchronize(q->ctx->aux));
    return IMM3_OK;
}
