// imm3_planner.cpp -- which plan a projection takes and with what geometry (round 5: split off imm3_api.cpp, which keeps the C
// ABI's validation and getters; the launches of a run are imm3_run.cpp).  Everything here is host arithmetic plus the one sampling
// launch at query creation:
//   * the one-launch projection's geometry: tiles per wave and span (P) per grid, the grid a run may use while a communicator
//     is attached, the descriptor allocation (single_pass_setup, single_pass_run_grid, single_pass_adapt);
//   * the cost model's decisions between the one launch, survivor records and the bitmap path (imm3_plan.h) on an estimate --
//     the sample at creation, a reservation -- or on a run's count (single_pass_stream_columns, records_drop_if_narrow,
//     single_pass_drop_if_narrow, single_pass_restore);
//   * whether a projection with a `limit` scans in chunks (limit_scan_applies) and where the chunks end (limit_chunk_ends) or, over a
//     table, in one launch that stops (table_limit_applies);
//   * the select chain's passes (plan_select_chain) and the plan query creation makes for a projection (plan_projection).
// The reference has no planner to mirror: its Engine builds ScanOp -> SelectOp* -> ProjectOp per segment unconditionally
// (engine/src/main/scala/immutabledb/engine/Engine.scala:158-196); these are choices between equivalent executions of that chain.
#include "../../include/imm3.h"
#include "../../include/imm3_diag.h"
#include "imm3_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "imm3_handles.h"
#include "imm3_api_internal.h"

namespace imm3 {

// `limit` stops the scan (Project.scala:73-80; Engine.scala:166,253-258): a projection with a limit whose select chain is ONE tile
// launch over one uniform segment runs that launch as chunks of growing size (launch_tile_chunks, imm3_run.cpp).  Not when the caller wants
// the whole segment's count anyway (`whole`: a getter settling a partial scan; a count log), not for a select-only run
// (count_in_scan false: no projection follows), not for tables, records plans or count-only runs, not under the tuning variants that
// pin the old launches (7: k_total, 14: no chunks), and not for segments the first chunk already covers.
bool limit_scan_applies(const LimitScanInputs &in) {
    if (in.whole || in.count_log_on || !in.count_in_scan || !(in.limit > 0) || !in.single_tile_pass) return false;
    if (in.table || in.records || in.skip_bitmap || in.overlap_total) return false;
    if (in.filter_variant == TV_COUNT_BY_K_TOTAL || in.filter_variant == TV_NO_LIMIT_CHUNKS) return false;
    return in.n_tiles > kLimitFirstChunkTiles;
}

// Chunks of a limit scan: they end at tiles 1024, 8192, 32 768, 131 072, ... (x 4) and at the segment's end -- four launches for
// 100 M rows.  A `limit 10` is usually met in the first megarow: the chunks behind it cost their dispatch only (1 - 4 us each, which
// is why there are few of them); a limit met at 5 % of the segment stops at 8 %; one met in the second half scans everything, as a
// whole select would.  Multiples of kChunkTiles (the offsets scan's unit), but for the last end.
LimitChunks limit_chunk_ends(int64_t n_tiles) {
    static_assert(kLimitFirstChunkTiles % kChunkTiles == 0 && kLimitSecondEndTiles % kChunkTiles == 0, "a chunk of the limit scan ends where a chunk of the offsets scan does");
    LimitChunks c;
    for (int64_t end = kLimitFirstChunkTiles; end < n_tiles; end = end == kLimitFirstChunkTiles ? kLimitSecondEndTiles : end * 4) {
        c.end[c.n++] = end;
        if (end > INT64_MAX / 4) break; // (no further end fits an int64_t: 27 entries at the most)
    }
    if (n_tiles > 0) c.end[c.n++] = n_tiles;
    return c;
}

// The same over a TABLE (all segments a GPU owns: what both Engines build for a multi-segment table) is ONE launch that stops itself
// (k_filter_table_limit, imm3_kernels.hip: runs of kTableLimitClaimTiles tiles claimed in ascending order until the runs that are
// done have selected `limit` rows).  A flat query only (a select tree with an OR or a NOT runs k_filter_expr), with a projection behind it
// (count_in_scan), a select chain of one tile launch, not for a getter's whole select, a count log or a count-only run, not under
// the tuning variants that pin the old launches (7, 14: the whole select stays reachable for comparison) -- and only when the table
// has more tiles than the launch's work-groups claim at once: below that every tile is claimed before the first run is done.
bool table_limit_applies(const TableLimitInputs &in) {
    if (!in.table || in.tree || !(in.limit > 0) || !in.count_in_scan || !in.single_tile_pass) return false;
    if (in.whole || in.count_log_on || in.count_only) return false;
    if (in.filter_variant == TV_COUNT_BY_K_TOTAL || in.filter_variant == TV_NO_LIMIT_CHUNKS) return false;
    return in.grid > 0 && in.n_tiles > (int64_t)in.grid * kTableLimitClaimTiles;
}

int tile_kind(const FoldedPred &fp) {
    if (fp.kind != KIND_STR && fp.has_list) return TK_NONE; // (a folded IMM3_INT_IN list: a pass of its own, k_filter_int_list)
    if (fp.kind == KIND_I32) return TK_I32;
    if (fp.kind == KIND_I8) return TK_I8;
    if (fp.kind == KIND_STR && fp.width == 2 && !fp.match.empty() && fp.match.size() <= (size_t)kMaxTileMatch) return TK_S2;
    return TK_NONE;
}

// A string predicate the string pass takes (imm3_strmatch.hip): a row is a whole number of dwords, 4 .. 256 bytes; any IN-list
// (k_filter_str_rows) or a byte-order range (k_filter_str_range; str_range_route says the same of the width).
bool str_rows_pred(const FoldedPred &fp) {
    if (fp.kind == KIND_STR && fp.has_range) return !fp.pfor && str_range_route(fp.width) == 1;
    return fp.kind == KIND_STR && !fp.pfor && str_rows_width_ok(fp.width) && !fp.match.empty();
}

// Which kernel a folded predicate goes to on a uniform layout: 0 the tile kernel, 1 k_filter_str_rows, 2 the word-at-a-time kernel
// (the only one a table does not have), 3 k_filter_int_list (an int32 / int8 predicate with a list; a table has its instances).
int pred_route(const FoldedPred &fp) {
    if (fp.kind != KIND_STR && fp.has_list) return 3;
    if (tile_kind(fp) != TK_NONE) return 0;
    return str_rows_pred(fp) ? 1 : 2;
}

SelectChain plan_select_chain(const imm3_query *q) {
    // Uniform layouts: numeric and 2-byte-string predicates go through the tile kernel, string predicates on columns whose width is
    // a multiple of 4 through k_filter_str_rows (one column per launch); everything else -- other string widths, long IN-lists on
    // 2-byte columns, ragged layouts -- through the word-at-a-time kernel, up to 4 columns per launch.  Every pass after the first
    // ANDs into the bitmap in memory.
    const bool tiles = !q->ragged && q->ctx->filter_variant != TV_GENERIC_ONLY;
    SelectChain c;
    std::vector<const FoldedPred *> tile_preds;
    for (const auto &p : q->preds) {
        if (p.pfor) c.pfor.push_back(&p);
        else if (tiles && pred_route(p) == 0) tile_preds.push_back(&p);
        else if (tiles && pred_route(p) == 1) c.str_passes.push_back(&p);
        else if (tiles && pred_route(p) == 3) c.list_passes.push_back(&p);
        else c.generic.push_back(&p);
    }
    std::stable_sort(tile_preds.begin(), tile_preds.end(),
                     [](const FoldedPred *x, const FoldedPred *y) { return tile_kind(*x) < tile_kind(*y); });
    // up to 3 columns per launch, numeric kinds first (sorted), at most one 2-byte string column per launch -- so two string
    // predicates are two passes even when only two columns are filtered
    while (!tile_preds.empty()) {
        std::vector<const FoldedPred *> take;
        int n_s2 = 0;
        for (size_t i = 0; i < tile_preds.size() && take.size() < (size_t)kMaxTileCols; ++i) {
            const int tk = tile_kind(*tile_preds[i]);
            if (tk == TK_S2 && n_s2 == 1) continue;
            take.push_back(tile_preds[i]);
            n_s2 += tk == TK_S2;
        }
        for (const FoldedPred *fp : take) tile_preds.erase(std::find(tile_preds.begin(), tile_preds.end(), fp));
        c.tile_passes.push_back(take);
    }
    if (q->preds.empty() && tiles) c.tile_passes.emplace_back();
    c.single_tile_pass = c.generic.empty() && c.pfor.empty() && c.str_passes.empty() && c.list_passes.empty() && c.tile_passes.size() == 1; // (a string or list pass: the bitmap path, as with a generic pass)
    return c;
}

// ---- single-pass projection: tiles per wave and span (P) ----
// CUs a one-launch plan leaves free while a communicator is attached to its context: ONE PER XCD.  The kernel wants every CU (one
// work-group per CU, all resident); the kernel RCCL launches for the count all-reduce of the pass before cannot share a CU with such
// a work-group (ncclDevKernel_Generic for gfx950: 512 threads x 256 vector registers and 37 664 bytes of LDS, beside 3 waves x 131
// registers per SIMD and 140 KB) -- so with all 256 CUs taken it waits until a work-group LEAVES, i.e. for the whole pass, and when
// it wins the race instead, one work-group of the pass starts late by the collective's duration and the pass ends that much later.
// Work-groups go to the XCDs round-robin BEFORE the dispatcher knows where there is room, so a free CU only helps on the XCD the
// collective's work-group is sent to: four free CUs (grid 252: XCDs 0-3 full) changed nothing, one per XCD does (tools/overlap_probe.py,
// profiles/r05_overlap.txt; the table is in DESIGN section 8).
constexpr int kXcds = 8;
constexpr int kCommReservedCUs = kXcds;
bool single_pass_reserves(const imm3_query *q) {
    return q->ctx->comms_attached.load(std::memory_order_relaxed) > 0 && q->ctx->filter_variant != TV_NO_CU_RESERVATION && q->sp_max_grid > 4 * kCommReservedCUs;
}
int32_t single_pass_run_grid(const imm3_query *q) {
    const int64_t g = single_pass_reserves(q) ? q->sp_max_grid - kCommReservedCUs : q->sp_max_grid;
    return (int32_t)std::max<int64_t>(1, std::min<int64_t>(g, q->sp_spans));
}
void single_pass_set_P(imm3_query *q, int32_t P) {
    const int64_t tiles_per_span = (int64_t)P * kProjectStreamers;
    q->sp_P = P;
    q->sp_spans = (q->n_tiles + tiles_per_span - 1) / tiles_per_span;
    q->sp_grid = single_pass_run_grid(q);
}
// The host has learnt how many rows survive (a count it fetched together with the number of ranges that outgrew their LDS
// ring, dense_ranges; or a reservation, dense_ranges < 0): later runs use a P at which a range's survivors fill about 45 %
// of a streamer's ring -- the streamers then keep compacting while the writers unpack, and no range outgrows its ring (a
// range that does is unpacked from the source columns row by row: several times slower per row than from records).
// Survivors are taken to sit in the dense ranges when there were any (a sorted key: half the table survives, all of it
// in one half); when not even two tiles of such a range fit a ring the planned P stays -- there the row-by-row path
// beats short ranges.  Measured at 100 M rows: 50 % survivors of an int8 column, evenly spread: P = 14 (the plan, made
// for ~10 %) 386 us, P = 3 164 us (three launches: 180-208); 28 % of int8 + int32: P = 6 506 us, P = 2 190 us (242);
// id > 5e7 on the sorted key: P = 7 232-269 us, P = 2 364 us, P = 1 426 us (338).  A run recorded in a graph keeps the P
// it was recorded with (the descriptors' layout does not depend on P).
// sigma: survivors per row WHERE THERE ARE SURVIVORS (the local density: what a range has to hold); `sure`: measured by a run
void single_pass_pick_P(imm3_query *q, double sigma, bool sure) {
    if (!q->single_pass || q->sp_P_fixed || !(sigma > 0.0)) return;
    const int R = project_rec_dwords(q->stage_kinds);
    const double ring_records = (double)kProjectRingBytes / (4.0 * R);
    const double per_tile = std::min(1.0, sigma) * kTileRows;
    const double fill = per_tile * q->sp_P / ring_records;
    if (!sure && fill >= 0.3 && fill <= 0.6) return; // (close enough: P does not flip between an estimate and the count)
    int64_t P = (int64_t)(0.45 * ring_records / per_tile);
    if (P < 2) P = (int64_t)(0.9 * ring_records / per_tile); // (nearly every row survives: whatever still fits)
    if (P < 2) P = q->sp_P_plan;
    P = std::min<int64_t>(P, q->sp_P_plan);
    if ((int32_t)P == q->sp_P) return;
    // The descriptors are tagged with the run counter (26 bits): leave no tag behind in places the new P does not rewrite every
    // run (stream order: after the runs so far, before the next one).  Hygiene, not correctness -- an alias would need 2^26 runs --
    // so a failed memset only means the old P stays.
    if (hipMemsetAsync(q->d_desc, 0, q->sp_trash_off, q->ctx->stream) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    single_pass_set_P(q, (int32_t)P);
}
void single_pass_adapt(imm3_query *q, uint64_t survivors, int64_t dense_ranges) {
    if (!q->single_pass || q->sp_P_fixed || q->n_rows <= 0 || survivors == 0) return;
    if (dense_ranges < 0 && q->sp_have_stats) return; // (a reservation says less than a run did)
    if (dense_ranges >= 0) q->sp_have_stats = true;
    double sigma = (double)survivors / (double)q->n_rows;
    const double n_ranges = (double)q->sp_spans * kProjectStreamers;
    const bool clustered = dense_ranges > 0 && (double)dense_ranges > 0.02 * n_ranges;
    if (clustered) sigma = std::min(1.0, sigma * n_ranges / (double)dense_ranges);
    single_pass_pick_P(q, sigma, dense_ranges > 0);
}

// Plans the one-launch projection for the tile columns in q->stage_kinds: P, the grid, the descriptor allocation.
// q->single_pass stays false when the kernel cannot run here (no instance, no resident work-group).
int single_pass_setup(imm3_query *q) {
    imm3_ctx *ctx = q->ctx;
    const int R = project_rec_dwords(q->stage_kinds);
    int64_t tile_bytes = 0;
    for (int k = 0; k < kMaxTileCols; ++k)
        tile_bytes += (q->stage_kinds[k] == TK_I32 ? 4 : (q->stage_kinds[k] == TK_S2 ? 2 : (q->stage_kinds[k] == TK_I8 ? 1 : 0))) * (int64_t)kTileRows;
    // Tiles per wave and span (P).  Large enough that a span's prefix (a ~10 us chain through three other work-groups)
    // and its unpacking fit in the time the streamers need for the next spans; small enough that three ranges of
    // ~10 % survivors fit a streamer's LDS ring -- the streamers then never wait for a writer -- and that the last
    // round, whose prefix nothing overlaps, is short.  Within that window P is the value that fills the last round of
    // spans best (spans are dealt round-robin to one work-group per CU).  Measured on C3 (100 M rows, R = 2): P = 6-8
    // 127-133 us, P = 12 143 us, P = 4 154 us.
    int maxg = project_max_grid(q->stage_kinds, 0);
    if (ctx->grid_blocks > 0) maxg = std::min(maxg, ctx->grid_blocks.load());
    const int64_t ring_records = kProjectRingBytes / (4 * R);
    int64_t p_hi = std::max<int64_t>(4, std::min<int64_t>(16, ring_records / 3 / 85));
    if (tile_bytes > 0) p_hi = std::max<int64_t>(4, std::min<int64_t>(p_hi, (60 * 1024) / tile_bytes));
    // Spans go to the work-groups in ROUNDS of one span each, and a round takes the time of its P tiles whether all work-groups have a
    // span in it or one: the launch costs rounds x P tile times (+ a prefix chain per round), and the rounds are quantised by the
    // grid.  100 M rows on 256 CUs: P = 6 -> 7.95 rounds -> 8 x 6 = 48 tile times (47.7 is the floor); on 248 CUs (a CU per XCD left
    // to a communicator) P = 6 -> 8.2 rounds -> 9 x 6 = 54, P = 5 -> 9.85 -> 10 x 5 = 50.  So P is planned per grid: the candidate
    // (two below the ceiling the ring and the register sets allow, never under 4) with the fewest tile times, the larger P on a tie.
    auto plan_P = [&](int64_t grid) -> int64_t {
        int64_t best_P = p_hi;
        double best = 1e300;
        for (int64_t p = p_hi; p >= std::max<int64_t>(4, p_hi - 2) && grid > 0; --p) {
            const int64_t spans = (q->n_tiles + p * kProjectStreamers - 1) / (p * kProjectStreamers);
            const int64_t rounds = (spans + grid - 1) / grid;
            const double cost = (double)rounds * ((double)p + 0.35); // (+ the part of a round's prefix chain and ring hand-offs that nothing hides)
            if (cost < best - 1e-9) { best = cost; best_P = p; }
        }
        return best_P;
    };
    int64_t P = plan_P(maxg);
    const int64_t P_reserved = plan_P(maxg > 4 * kCommReservedCUs ? maxg - kCommReservedCUs : maxg);
    const bool fixed = fixed_P(ctx->filter_variant) > 0;
    if (fixed) P = fixed_P(ctx->filter_variant);
    if (maxg < 1 || q->n_tiles < 1) return IMM3_OK;
    // One allocation: round totals and round counters first (at the same place whatever P a run uses), then the span
    // descriptors of the smallest P a run may use, then one 64-byte trash line per writer wave.  The plan is committed only
    // once the allocation stands (a query whose descriptors could not be allocated keeps the three launches).
    const int64_t spans_max = (q->n_tiles + kProjectMinP * kProjectStreamers - 1) / (kProjectMinP * kProjectStreamers);
    const int64_t grid_min = std::max<int64_t>(1, std::min<int64_t>(maxg > 4 * kCommReservedCUs ? maxg - kCommReservedCUs : maxg, spans_max)); // (the smallest grid a run may use: single_pass_run_grid)
    const size_t rounds_max = (size_t)((spans_max + grid_min - 1) / grid_min);
    const size_t desc_off = (rounds_max * (sizeof(unsigned long long) + sizeof(uint32_t)) + 255) / 256 * 256;
    const size_t desc_bytes = desc_off + (size_t)spans_max * sizeof(unsigned long long);
    const size_t trash_off = (desc_bytes + 255) / 256 * 256;
    void *d = nullptr;
    HIPCHK(pool_alloc(ctx, &d, trash_off + (size_t)maxg * kProjectWriters * 64));
    const hipError_t me = hipMemsetAsync(d, 0, desc_bytes, ctx->stream); // (pooled memory: another query's descriptors)
    if (me != hipSuccess) {
        pool_release(ctx, d);
        HIPCHK(me);
    }
    if (q->table && !q->d_tile_desc) { // the launch's view of the tile table: one descriptor per tile (built on the device from the table's per-column pointers)
        void *td = nullptr;
        const hipError_t te = pool_alloc(ctx, &td, (size_t)q->n_tiles * sizeof(ProjectTile));
        if (te != hipSuccess) {
            pool_release(ctx, d);
            HIPCHK(te);
        }
        const void *const *tp[kMaxTileCols] = {nullptr, nullptr, nullptr};
        for (int k = 0; k < kMaxTileCols; ++k)
            if (q->stage_kinds[k] != TK_NONE && q->stage_seg_col[k] >= 0) tp[k] = (const void *const *)q->table->d_tile_ptrs[(size_t)q->stage_seg_col[k]];
        launch_project_tile_desc(q->table->d_tile_rows, tp[0], tp[1], tp[2], (ProjectTile *)td, q->n_tiles, ctx->stream);
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) {
            pool_release(ctx, d);
            pool_release(ctx, td);
            HIPCHK(le);
        }
        q->d_tile_desc = (ProjectTile *)td;
    }
    q->d_desc = (unsigned long long *)d;
    q->sp_rounds_max = rounds_max;
    q->sp_desc_off = desc_off;
    q->sp_trash_off = trash_off;
    q->single_pass = true;
    q->sp_P_fixed = fixed;
    q->sp_max_grid = maxg;
    q->sp_P_plan_for[0] = (int32_t)P;
    q->sp_P_plan_for[1] = fixed ? (int32_t)P : (int32_t)P_reserved;
    q->sp_P_plan = q->sp_P_plan_for[single_pass_reserves(q) ? 1 : 0];
    single_pass_set_P(q, q->sp_P_plan);
    return IMM3_OK;
}

// ---- the cost model's view of a query (imm3_plan.h) ----
// Where the survivors are, given a count (or an estimate of one): the sample taken at creation knows how they are spread (survivors
// per row where there are survivors, and how many sit in fully surviving stretches); without it they are taken as spread evenly.
PlanDensity plan_density_for(const imm3_query *q, uint64_t survivors) {
    PlanDensity d;
    d.sigma = q->n_rows > 0 ? std::min(1.0, (double)survivors / (double)q->n_rows) : 0.0;
    d.sloc = d.sigma;
    d.full = 0.0;
    if (q->plan_have_density) { // (how densely the survivors sit where they sit is the data's property: a better count does not change it)
        d.sloc = std::min(1.0, std::max(d.sigma, q->plan_density.sloc));
        d.full = q->plan_density.full;
    }
    return d;
}
// the plan a query would fall back to from the one launch, and its predicted cost: records when a predicate column is projected
// and they are predicted cheaper than the bitmap path
double plan_cost_three_launches(const imm3_query *q, const PlanDensity &d, bool records_possible, bool *use_records) {
    const double c = plan_cost('C', q->plan_shape, d);
    const double b = records_possible ? plan_cost('B', q->plan_shape, d) : 1e30;
    if (use_records) *use_records = b < c;
    return std::min(b, c);
}

// The survivor records' buffers go back to the pool (a graph that recorded a run on them is stale now).
static void records_release(imm3_query *q) {
    graphs_mark_stale(q->ctx, q);
    pool_release(q->ctx, q->d_stage_rec);
    pool_release(q->ctx, q->d_tile_start);
    q->d_stage_rec = nullptr;
    q->d_tile_start = nullptr;
    q->run.stage_written = false;
}

// A projection with gathered SELECT-list columns was planned as three launches (records -> k_scan -> k_emit).  Now the host
// knows how many rows survive: when that is enough for a gather to touch most 128-byte lines of the column anyway, the
// column is STREAMED instead -- it joins the one-launch kernel as a tile column whose predicate every value passes, and its
// values ride in the records like a predicate column's.  (`select id, age ... where age > 18 and age < 30`, 11 % of 100 M rows:
// 123 us against 174; at 3 % the three launches win.)  Called outside a capture, before the query's row arrays exist or
// from imm3_query_reserve_rows; the records' buffers go back to the pool.
int single_pass_stream_columns(imm3_query *q, uint64_t survivors) {
    imm3_ctx *ctx = q->ctx;
    if (!q->alt_ok || q->single_pass || ctx->capture || q->n_rows <= 0) return IMM3_OK;
    if (ctx->filter_variant != TV_STREAM_ALWAYS) {
        if (q->plan_pinned) return IMM3_OK;
        const PlanDensity d = plan_density_for(q, survivors);
        const double now = q->d_stage_rec ? std::min(plan_cost('B', q->plan_shape, d), plan_cost('C', q->plan_shape, d)) : plan_cost('C', q->plan_shape, d);
        if (!(plan_cost('A', q->plan_shape, d) < kPlanKeepMargin * now)) return IMM3_OK;
    }
    int32_t keep_kinds[kMaxTileCols], keep_cols[kMaxTileCols];
    for (int k = 0; k < kMaxTileCols; ++k) {
        keep_kinds[k] = q->stage_kinds[k];
        keep_cols[k] = q->stage_seg_col[k];
        q->stage_kinds[k] = q->alt_kinds[k];
        q->stage_seg_col[k] = q->alt_seg_col[k];
    }
    const int rc = single_pass_setup(q);
    if (rc || !q->single_pass) { // (cannot run here: the three launches stay)
        for (int k = 0; k < kMaxTileCols; ++k) {
            q->stage_kinds[k] = keep_kinds[k];
            q->stage_seg_col[k] = keep_cols[k];
        }
        q->alt_ok = false;
        return rc;
    }
    records_release(q);
    q->alt_ok = false;
    single_pass_adapt(q, survivors, -1);
    return IMM3_OK;
}

// Survivor records planned, but the bitmap path is predicted cheaper for this many survivors (the staging instance of the filter
// kernel costs 10-35 us per 100 M rows more than the plain one, plus the records' bytes; it buys the emit kernel the projected
// predicate columns: age > 97 -> id, age at 1 %: 75 us with records, 65 without; id > 9e7 -> id, age: 152 / 140; state in (8
// values) -> id, state, age: 277 / 243).  The records' buffers go back to the pool.
void records_drop_if_narrow(imm3_query *q, uint64_t survivors) {
    imm3_ctx *ctx = q->ctx;
    if (q->single_pass || !q->d_stage_rec || q->plan_pinned || ctx->capture || ctx->filter_variant == TV_RECORDS_ALWAYS ||
        ctx->filter_variant == TV_NO_ONE_LAUNCH || q->n_rows <= 0) return;
    const PlanDensity d = plan_density_for(q, survivors);
    if (!(plan_cost('C', q->plan_shape, d) < kPlanKeepMargin * plan_cost('B', q->plan_shape, d))) return;
    records_release(q);
    q->alt_ok = false; // (settled: three launches from the bitmap)
}

// Survivor records (k_filter_tile STAGE -> k_emit) for the tile columns in q->stage_kinds.  Every wave of the staging launch
// writes its records to its own arena, so the launch geometry is fixed here: 768 work-groups (3 per CU: an 8 KiB record
// buffer per wave), grid-stride over groups of T tiles.
int records_setup(imm3_query *q) {
    imm3_ctx *ctx = q->ctx;
    const int R = rec_layout(q->stage_kinds, -1).dwords;
    const int T = filter_tile_group(q->stage_kinds);
    // 3 per CU (~52 KiB of LDS each); 4 per CU for a lone 2-byte-string column (1-dword records, 4 KiB record buffers: C4's
    // filter 50.5 -> 46.6 us).  Measured per shape: a lone int8 column at 1024 lost 8 us, an int32 column 7 us.
    const bool lone_s2 = q->stage_kinds[0] == TK_S2 && q->stage_kinds[1] == TK_NONE;
    const int cap = ctx->grid_blocks > 0 ? std::min(ctx->grid_blocks.load(), kMaxFilterGrid) : (R == 1 && lone_s2 ? 1024 : 768);
    const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((q->n_tiles + kWavesPerBlock - 1) / kWavesPerBlock, cap));
    const int64_t n_waves = grid * kWavesPerBlock;
    const int64_t n_groups = T > 0 ? (q->n_rows / kTileRows) / T : 0;
    const int64_t main_tiles = n_groups * T;
    const int64_t max_slots = ((n_groups + n_waves - 1) / n_waves) * T + (q->n_tiles - main_tiles + n_waves - 1) / n_waves;
    if (T > 0 && max_slots <= kMaxArenaSlots) {
        q->stage_grid = (int32_t)grid;
        q->stage_T = T;
        q->stage_max_slots = (int32_t)std::max<int64_t>(max_slots, 1) + 1; // (+ 1: behind a wave's tile starts sits its arena's end -- the last tile's length, for an offsets scan without a bitmap)
        q->stage_wave_cap = (int64_t)q->stage_max_slots * kTileRows; // (skewing the arena bases off their 128 KiB-aligned stride changed nothing)
        q->stage_main_tiles = main_tiles;
        void *d = nullptr;
        HIPCHK(pool_alloc(ctx, &d, (size_t)n_waves * (size_t)q->stage_wave_cap * 4 * (size_t)R + 256));
        q->d_stage_rec = (uint8_t *)d;
        HIPCHK(pool_alloc(ctx, &d, (size_t)n_waves * (size_t)q->stage_max_slots * sizeof(uint32_t) + 256));
        q->d_tile_start = (uint32_t *)d;
    }
    return IMM3_OK;
}

// The one launch planned, but three launches are predicted cheaper for this many survivors.  The one-launch kernel costs ~23 us +
// 0.6-0.85 us per million rows whatever the columns' widths (it is bound by instructions per row, DESIGN finding 21), and its
// writers walk stretches of mostly-surviving rows at ~1.5 us per million rows and column; the plain filter over 1- and 2-byte
// columns takes 21-45 us per 100 M rows and k_gather ~2.5 us per million survivors.  So: narrow predicate columns alone take
// filter -> offsets scan -> gather until many rows survive (select age ... where age > 98, 1 %: 89 us in one launch, 53 in three);
// small segments take it nearly always (4 M rows: 27 us against 16-20); and C3's shape takes it again above ~50 % survivors spread
// evenly (60 %: 373 us in one launch, 329 in three).  A projected string column with few survivors is better staged in records than
// gathered (state = CA -> state, 2 %: 62 us with records, 75 from the bitmap): the cheaper of the two is taken.
void single_pass_drop_if_narrow(imm3_query *q, uint64_t survivors) {
    imm3_ctx *ctx = q->ctx;
    if (!q->single_pass || !q->sp_pass.empty() || q->sp_P_fixed || q->plan_pinned || ctx->capture || ctx->filter_variant == TV_ONE_LAUNCH_GATHERS ||
        ctx->filter_variant == TV_RECORDS_ALWAYS || q->n_rows <= 0) return;
    const PlanDensity d = plan_density_for(q, survivors);
    bool use_records = false;
    const double other = plan_cost_three_launches(q, d, ctx->filter_variant != TV_NO_RECORDS && !q->table, &use_records); // (a table has no survivor records: the bitmap path)
    if (!(other < kPlanKeepMargin * plan_cost('A', q->plan_shape, d))) return;
    graphs_mark_stale(ctx, q);
    q->single_pass = false;
    q->sp_model_dropped = true; // (the first count may bring it back: single_pass_restore)
    pool_release(ctx, q->d_desc);
    q->d_desc = nullptr;
    pool_release(ctx, q->d_tile_desc);
    q->d_tile_desc = nullptr;
    if (use_records && !q->d_stage_rec) {
        if (records_setup(q) != IMM3_OK || !q->d_tile_start) { // (no memory for the records: the bitmap path needs none)
            pool_release(ctx, q->d_stage_rec);
            q->d_stage_rec = nullptr;
            (void)hipGetLastError();
        }
    }
}

// ... and back: the one launch was left on an estimate (the sample, or the guess made for a segment too small to sample), and the
// first run's count says it is the cheaper plan after all (a small segment most of whose rows survive: 4 M rows, 60 %: 27 us in
// one launch, 37 in three; a range of the sorted key that the sample's chunks missed).
bool single_pass_restore_wanted(const imm3_query *q, uint64_t survivors) {
    const imm3_ctx *ctx = q->ctx;
    if (q->single_pass || !q->sp_model_dropped || q->plan_pinned || ctx->capture || ctx->filter_variant == TV_NO_ONE_LAUNCH ||
        ctx->filter_variant == TV_NO_RECORDS || q->n_rows <= 0) return false;
    const PlanDensity d = plan_density_for(q, survivors);
    const double now = q->d_stage_rec ? plan_cost('B', q->plan_shape, d) : plan_cost('C', q->plan_shape, d);
    return plan_cost('A', q->plan_shape, d) < kPlanKeepMargin * now;
}
// (the run that read the count finishes on the plan it started with -- its filter and offsets scan are done, the gather is the
// smaller part -- and the NEXT run takes the one launch: the switch happens at the start of that run)
int single_pass_restore(imm3_query *q, uint64_t survivors) {
    imm3_ctx *ctx = q->ctx;
    q->sp_restore_pending = false;
    if (q->single_pass || !q->sp_model_dropped || q->plan_pinned || ctx->capture) return IMM3_OK;
    const int rc = single_pass_setup(q);
    if (rc || !q->single_pass) return rc; // (cannot run here: the three launches stay)
    records_release(q);
    q->sp_model_dropped = false;
    q->sp_narrow_checked = true; // (decided on a count: no second look)
    single_pass_adapt(q, survivors, -1);
    return IMM3_OK;
}

// A look at the data before the first run: the select chain's count over eight evenly spaced chunks of 64 tiles (0.5 % of
// 100 M rows, eight count-only launches of the scan+select kernel and one strided copy, inside query creation, which ends with
// a stream synchronisation anyway: + 0.05-0.15 ms on a creation of 0.35-0.6 ms; tools/first_run.py).  Most queries run ONCE (the reference's Engine plans, runs and drops a pipeline per statement),
// so what later runs learn from a count -- P, streamed SELECT-list columns -- the first run gets from the sample.  Survivors
// per row are also taken per chunk: weighted by the chunks' own survivors they give the density where the survivors ARE,
// which tells a sorted key's all-or-nothing ranges (keep the planned P: unpack_dense) from the same number of survivors
// spread evenly (shorter ranges).

// the sample's tile table for one column of the segment (cached on the segment: the sampled tiles are the segment's, not the query's)
int sample_tile_ptrs(imm3_ctx *ctx, const imm3_segment *cseg, int32_t col, int64_t n_full, void ***out, uint32_t **rows_out) {
    imm3_segment *seg = const_cast<imm3_segment *>(cseg);
    // The device allocations and copies happen OUTSIDE the segment's lock (they wait for the device: query creations on one
    // segment would queue up behind them); the lock only covers looking the tables up and publishing them.  Two creations that
    // race for the same column both build a table and the loser's is freed.
    bool have_rows = false, have_ptrs = false;
    {
        std::lock_guard<std::mutex> g(seg->layout_mu);
        if (seg->sample_full_tiles >= 0 && seg->sample_full_tiles != n_full) return fail(IMM3_ERR_STATE, "internal: the segment's sample was laid out for another row count");
        have_rows = seg->d_sample_rows != nullptr;
        have_ptrs = seg->d_sample_ptrs.find(col) != seg->d_sample_ptrs.end();
    }
    void *new_rows = nullptr, *new_ptrs = nullptr;
    if (!have_rows) {
        std::vector<uint32_t> rows((size_t)kSampleTiles, (uint32_t)kTileRows);
        HIPCHK(hipMalloc(&new_rows, rows.size() * sizeof(uint32_t)));
        const hipError_t e = hipMemcpy(new_rows, rows.data(), rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(new_rows); HIPCHK(e); }
    }
    if (!have_ptrs) {
        const SegCol &sc = seg->cols[(size_t)col];
        std::vector<const void *> ptrs((size_t)kSampleTiles);
        for (int i = 0; i < kSampleChunks; ++i) {
            int64_t tile0 = (int64_t)((2 * i + 1) * n_full / (2 * kSampleChunks)) - kSampleChunkTiles / 2;
            tile0 = std::max<int64_t>(0, std::min<int64_t>(tile0, n_full - kSampleChunkTiles));
            for (int64_t t = 0; t < kSampleChunkTiles; ++t)
                ptrs[(size_t)(i * kSampleChunkTiles + t)] = col_flat(sc) + (size_t)(tile0 + t) * kTileRows * (size_t)sc.width;
        }
        hipError_t e = hipMalloc(&new_ptrs, ptrs.size() * sizeof(void *));
        if (e == hipSuccess) e = hipMemcpy(new_ptrs, ptrs.data(), ptrs.size() * sizeof(void *), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(new_rows); (void)hipFree(new_ptrs); HIPCHK(e); }
    }
    void *drop_rows = nullptr, *drop_ptrs = nullptr;
    {
        std::lock_guard<std::mutex> g(seg->layout_mu);
        if (new_rows) {
            if (!seg->d_sample_rows) { seg->d_sample_rows = (uint32_t *)new_rows; seg->sample_full_tiles = n_full; }
            else drop_rows = new_rows;
        }
        auto it = seg->d_sample_ptrs.find(col);
        if (new_ptrs) {
            if (it == seg->d_sample_ptrs.end()) it = seg->d_sample_ptrs.emplace(col, (void **)new_ptrs).first;
            else drop_ptrs = new_ptrs;
        }
        *out = it->second;
        *rows_out = seg->d_sample_rows;
    }
    (void)hipFree(drop_rows);
    (void)hipFree(drop_ptrs);
    (void)ctx;
    return IMM3_OK;
}

static int single_pass_sample(imm3_query *q) {
    imm3_ctx *ctx = q->ctx;
    const int64_t n_full = q->table ? q->n_tiles : q->n_rows / kTileRows; // (a table's sample may hold a segment's partial last tile: the kernel's rolled path)
    const bool undecided = q->single_pass || q->alt_ok || q->d_stage_rec;
    if (!undecided || q->sp_P_fixed || q->plan_pinned || ctx->filter_variant == TV_NO_SAMPLE || n_full < 4096) return IMM3_OK; // (below ~4 M rows the sample costs what it saves)
    if (q->table && !q->table->d_sample_rows) return IMM3_OK;
    // ONE count-only launch of the scan+select kernel's table instance over the sample's tile table (round 3: eight launches, a
    // memset and a strided copy): 128 work-groups, one tile per wave, so that work-groups 16 i .. 16 i + 15 hold chunk i's count
    // in their partials.
    TileArgs a;
    std::memset(&a, 0, sizeof(a));
    bool any = false;
    for (int k = 0; k < kMaxTileCols; ++k) {
        a.kinds[k] = q->stage_kinds[k];
        if (a.kinds[k] == TK_NONE) continue;
        const FoldedPred *fp = pred_on(q->preds, q->stage_seg_col[k]);
        if (!fp) return IMM3_OK; // (a streamed column already: nothing left to decide)
        if (is_compressed(q->seg->cols[(size_t)fp->seg_col].codec) && !q->seg->cols[(size_t)fp->seg_col].d_dense) return IMM3_OK;
        fill_tile_col(q, *fp, a.cols[k], a.kinds[k]);
        void **ptrs = nullptr;
        uint32_t *rows = nullptr;
        if (q->table) { // (made with the table: imm3_table_create)
            ptrs = q->table->d_sample_ptrs[(size_t)fp->seg_col];
            rows = q->table->d_sample_rows;
        } else {
            const int rc = sample_tile_ptrs(ctx, q->seg, fp->seg_col, n_full, &ptrs, &rows);
            if (rc) return rc;
        }
        a.tile_ptrs[k] = (const void *const *)ptrs;
        a.tile_rows = rows;
        any = true;
    }
    if (!any) return IMM3_OK; // (no predicate: every row survives, the plan for that is the dense path at the planned P)
    a.n_rows = (int64_t)kSampleTiles * kTileRows;
    a.n_words = (int64_t)kSampleTiles * kTileWords;
    a.n_tiles = kSampleTiles;
    a.bitmap = nullptr; // count-only
    a.block_partials = q->d_block_partials;
    a.finish = nullptr;
    constexpr int kGrid = kSampleTiles / kWavesPerBlock; // 128: wave w of the launch takes tile w
    if (!launch_filter_tile(a, kGrid, ctx->stream, nullptr, nullptr)) return IMM3_OK;
    HIPCHK(hipGetLastError());
    uint32_t partials[kGrid] = {0};
    HIPCHK(hipMemcpyAsync(partials, q->d_block_partials, sizeof(partials), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const double chunk_rows = (double)(kSampleChunkTiles * kTileRows);
    double sum = 0.0, sum_sq = 0.0, sum_full = 0.0;
    for (int i = 0; i < kSampleChunks; ++i) {
        double c = 0.0;
        for (int b = 0; b < kGrid / kSampleChunks; ++b) {
            const double part = (double)partials[i * (kGrid / kSampleChunks) + b];
            c += part;
            if (part >= (double)(kWavesPerBlock * kTileRows)) sum_full += part; // (a work-group's eight tiles, every row of them)
        }
        sum += c;
        sum_sq += c * c;
    }
    // (nothing in the sample: fewer than one row in 130 000 survives, or they all sit between the sample's chunks -- the plans for
    // very few survivors are compared; the first count corrects a miss)
    const double sigma = std::max(sum, 0.5) / (chunk_rows * kSampleChunks), sigma_local = sum > 0.0 ? sum_sq / (sum * chunk_rows) : sigma;
    q->plan_density.sigma = sigma;
    q->plan_density.sloc = std::max(sigma, std::min(1.0, sigma_local));
    q->plan_density.full = sum > 0.0 ? sum_full / sum : 0.0;
    q->plan_have_density = true;
    const uint64_t estimate = (uint64_t)(sigma * (double)q->n_rows);
    const int rc = single_pass_stream_columns(q, estimate);
    if (rc) return rc;
    records_drop_if_narrow(q, estimate);
    single_pass_drop_if_narrow(q, estimate);
    if (sum > 0.0) single_pass_pick_P(q, sigma_local, false);
    return IMM3_OK;
}

// ---- the plan query creation makes for a projection ----
// The SELECT-list entries whose values ride in the records (and in the one launch's): the first mention of each predicate column;
// every other entry is gathered.  (fill_emit_cols, imm3_run.cpp, lets a later mention of a staged column read the record too: the
// plan counts it as gathered -- one rule for both would change which launches run.)
static std::vector<bool> proj_rides_in_records(imm3_query *q) {
    std::vector<bool> rides(q->proj.size(), false);
    for (size_t j = 0; j < q->proj.size(); ++j) {
        const int32_t sci = q->used[(size_t)q->proj[j]];
        bool first = true;
        for (size_t i = 0; i < j; ++i) first &= q->used[(size_t)q->proj[i]] != sci;
        rides[j] = first && pred_on(q->preds, sci) != nullptr;
    }
    return rides;
}

// The alternative the first count may switch to (single_pass_stream_columns): every gathered column of the SELECT list (first
// mentions; dense int32 / int8) as a tile column that lets every value pass.
static void plan_stream_alternative(imm3_query *q, const std::vector<const FoldedPred *> &order) {
    std::vector<FoldedPred> pass;
    for (int32_t pj : q->proj) {
        const int32_t sci = q->used[(size_t)pj];
        bool have = false;
        for (const FoldedPred *fp : order) have |= fp->seg_col == sci;
        for (const FoldedPred &fp : pass) have |= fp.seg_col == sci;
        if (have) continue;
        const SegCol &sc = q->seg->cols[(size_t)sci];
        const bool dense_int = (sc.codec == IMM3_DENSE_INT && sc.width == 4) || (sc.codec == IMM3_DENSE_TINYINT && sc.width == 1);
        if (!dense_int || !col_flat(sc)) return;
        pass.push_back(unfolded_pred(sci, sc.codec, sc.width));
    }
    if (pass.empty() || order.size() + pass.size() > (size_t)kMaxTileCols) return;
    q->sp_pass = pass;
    std::vector<const FoldedPred *> all(order);
    for (const FoldedPred &fp : q->sp_pass) all.push_back(&fp);
    std::stable_sort(all.begin(), all.end(), [](const FoldedPred *x, const FoldedPred *y) { return tile_kind(*x) < tile_kind(*y); });
    bool any4 = false, any_s2 = false;
    for (int k = 0; k < kMaxTileCols; ++k) {
        q->alt_kinds[k] = (size_t)k < all.size() ? tile_kind(*all[(size_t)k]) : (int)TK_NONE;
        q->alt_seg_col[k] = (size_t)k < all.size() ? all[(size_t)k]->seg_col : -1;
        any_s2 |= q->alt_kinds[k] == TK_S2;
    }
    for (const FoldedPred &fp : q->sp_pass) any4 |= fp.width == 4;
    // Whether they ARE streamed is the cost model's call once the survivors are known (single_pass_stream_columns: the
    // sample at creation, a reservation or the first count).  Measured at 100 M rows (one launch / three launches):
    // age < 10 -> id, 10 %: 117 / 123 us; 3 %: 107 / 79; 30 %: 204 / 168; 99 %: 534 / 372 -- a window around 10 %.
    // Not with a string predicate (the 2-byte match streams at 74 us with the one-launch kernel's 8 streaming waves per
    // CU against 47), and not for 1-byte columns alone (their gather reads every line of the column from ~3 % on and
    // still costs 33 us at 10 %).
    q->alt_ok = any4 && !any_s2;
}

// The plans of an unlimited projection whose select chain is ONE tile launch (<= 3 predicate columns of int32 / int8 / 2-byte
// string, at most one string; none is also fine: the record is then the position alone), `order` its columns: survivor records
// (k_filter_tile STAGE -> k_emit), the one launch, the streamed alternative.  The SELECT list must be 1-, 2- and 4-byte columns,
// at most kMaxEmitGather of them gathered.
// A table query (every segment the GPU owns as one scan unit) takes the ONE-LAUNCH plan under the same conditions when no
// SELECT-list column has to be gathered (round 5; its TABLE instances walk the tile table); survivor records and streamed
// gathers are one-segment plans, the bitmap path is a table's other plan.
static int plan_one_tile_pass(imm3_query *q, const std::vector<const FoldedPred *> &order) {
    const int fv = q->ctx->filter_variant;
    const std::vector<bool> rides = proj_rides_in_records(q);
    int n_gather = 0;
    int n_pred_proj = 0;         // predicate columns in the SELECT list whose values ride in the records ...
    bool pred_proj_wide = false; // ... and whether one of them is wider than a byte
    for (size_t j = 0; j < q->proj.size(); ++j) {
        const int32_t w = q->seg->cols[(size_t)q->used[(size_t)q->proj[j]]].width;
        if (w != 1 && w != 2 && w != 4) return IMM3_OK;
        n_gather += !rides[j];
        n_pred_proj += rides[j];
        pred_proj_wide |= rides[j] && w > 1;
    }
    if (n_gather > kMaxEmitGather || (q->table && (n_gather > 0 || fv == TV_NO_ONE_LAUNCH))) return IMM3_OK;
    for (size_t k = 0; k < order.size(); ++k) {
        q->stage_kinds[k] = tile_kind(*order[k]);
        q->stage_seg_col[k] = order[k]->seg_col;
    }
    PlanShape &ps = q->plan_shape; // what the cost model needs to know (imm3_plan.h)
    ps = PlanShape();
    ps.n_rows = q->n_rows;
    for (size_t k = 0; k < order.size() && ps.n_pred < kPlanMaxCols; ++k, ++ps.n_pred) {
        ps.pred_width[ps.n_pred] = order[k]->width;
        ps.pred_match[ps.n_pred] = tile_kind(*order[k]) == TK_S2 ? (int32_t)order[k]->match.size() : 0;
    }
    for (size_t j = 0; j < q->proj.size() && ps.n_proj < kPlanMaxCols; ++j, ++ps.n_proj) {
        ps.proj_width[ps.n_proj] = q->seg->cols[(size_t)q->used[(size_t)q->proj[j]]].width;
        ps.proj_is_pred[ps.n_proj] = rides[j];
    }
    ps.rec_bytes = 4 * rec_layout(q->stage_kinds, -1).dwords;
    q->plan_pinned = fv == TV_PLAN_PINNED;
    // Single pass (k_filter_project): the filter kernel writes the rows itself.  Only when every SELECT-list column is a predicate
    // column (its values ride in the records): gathers issued by the four writer waves of a CU are latency-bound (C4 154 us against
    // 118 us with the emit kernel's 2048 work-groups).
    if (fv != TV_NO_ONE_LAUNCH && (n_gather == 0 || fv == TV_ONE_LAUNCH_GATHERS)) {
        const int rc = single_pass_setup(q);
        if (rc) return rc;
    }
    if (!q->single_pass && n_gather > 0 && fv != TV_NO_ONE_LAUNCH && !q->table) plan_stream_alternative(q, order);
    // Survivor records pay when the predicate columns' values are wanted: the staging instances of the filter kernel cost
    // 12 (string) to 33 us (int8) per 100 M rows more than the plain ones, and buy the emit kernel the projected predicate
    // columns.  When none is projected they buy nothing -- state in (5 values) -> age, 10 %: 120 us with records, 87 without
    // (filter -> offsets scan -> gather from the bitmap); age in (18, 30) -> id, 11 %: 167 / 122; 3 %: 106 / 79.
    q->records_narrow_only = n_pred_proj > 0 && !pred_proj_wide;
    if (q->single_pass || q->table || (n_gather > 0 && n_pred_proj == 0 && fv != TV_RECORDS_ALWAYS)) return IMM3_OK; // (no survivor records in HBM)
    return records_setup(q);
}

int plan_projection(imm3_query *q) {
    if (q->is_expr) return IMM3_OK; // a select tree: the bitmap path (k_scan + k_gather) -- no records, no one launch, no sample
    // (anything but an unlimited projection whose select chain is ONE tile launch takes the bitmap path, which needs no set-up)
    if (!q->proj.empty() && q->limit <= 0 && !q->always_false && q->n_rows > 0 && q->ctx->filter_variant != TV_NO_RECORDS &&
        q->proj.size() <= (size_t)kMaxProj) {
        const SelectChain chain = plan_select_chain(q); // (a ragged layout, TV_GENERIC_ONLY: no tile pass)
        if (chain.single_tile_pass) {
            const int rc = plan_one_tile_pass(q, chain.tile_passes[0]);
            if (rc) return rc;
        }
    }
    const int rc = single_pass_sample(q); // (the one synchronisation a creation may contain: segments of 4 M rows and more, undecided plans)
    if (rc) return rc;
    // No sample (a segment below 4 M rows -- there the sample costs what it saves): the plans are compared for one survivor in
    // ten, spread evenly; the first count corrects it.  (At 4 M rows the bitmap path wins nearly every shape: the one launch
    // starts at ~27 us, three small launches at 16-20.)
    if (!q->plan_have_density && !q->plan_pinned && !q->sp_P_fixed && q->ctx->filter_variant != TV_NO_SAMPLE && q->plan_shape.n_rows > 0 &&
        (q->single_pass || q->alt_ok || q->d_stage_rec)) {
        const uint64_t guess = (uint64_t)(q->n_rows / 10);
        const int rc2 = single_pass_stream_columns(q, guess);
        if (rc2) return rc2;
        records_drop_if_narrow(q, guess);
        single_pass_drop_if_narrow(q, guess);
    }
    return IMM3_OK;
}

} // namespace imm3

using namespace imm3;

// diagnostics: the cost model's prediction for a shape (tests hold it against immutable3_amd/plan_model.py; tools print it)
extern "C" int imm3_plan_predict(int64_t n_rows, const int32_t *pred_width, const int32_t *pred_match, int32_t n_pred, const int32_t *proj_width,
                                 const int32_t *proj_is_pred, int32_t n_proj, int32_t rec_bytes, double sigma, double sloc, double full, double *out_abc) {
    if (n_pred < 0 || n_pred > kPlanMaxCols || n_proj < 0 || n_proj > kPlanMaxCols || !out_abc || (n_pred > 0 && (!pred_width || !pred_match)) ||
        (n_proj > 0 && (!proj_width || !proj_is_pred)))
        return fail(IMM3_ERR_ARG, "bad argument");
    PlanShape ps;
    ps.n_rows = n_rows;
    ps.n_pred = n_pred;
    for (int i = 0; i < n_pred; ++i) { ps.pred_width[i] = pred_width[i]; ps.pred_match[i] = pred_match[i]; }
    ps.n_proj = n_proj;
    for (int i = 0; i < n_proj; ++i) { ps.proj_width[i] = proj_width[i]; ps.proj_is_pred[i] = proj_is_pred[i] != 0; }
    ps.rec_bytes = rec_bytes;
    PlanDensity d;
    d.sigma = sigma;
    d.sloc = sloc;
    d.full = full;
    out_abc[0] = plan_cost('A', ps, d);
    out_abc[1] = plan_cost('B', ps, d);
    out_abc[2] = plan_cost('C', ps, d);
    return IMM3_OK;
}

// diagnostics: the limit-scan decision as the library makes it (a pure function of these inputs; tests/test_host.py walks it)
extern "C" int imm3_plan_limit_scan(int32_t whole, int32_t count_log_on, int32_t count_in_scan, int64_t limit, int32_t single_tile_pass, int32_t table, int32_t records,
                                    int32_t skip_bitmap, int32_t overlap_total, int32_t filter_variant, int64_t n_tiles) {
    LimitScanInputs in;
    in.whole = whole != 0;
    in.count_log_on = count_log_on != 0;
    in.count_in_scan = count_in_scan != 0;
    in.limit = limit;
    in.single_tile_pass = single_tile_pass != 0;
    in.table = table != 0;
    in.records = records != 0;
    in.skip_bitmap = skip_bitmap != 0;
    in.overlap_total = overlap_total != 0;
    in.filter_variant = filter_variant;
    in.n_tiles = n_tiles;
    return limit_scan_applies(in) ? 1 : 0;
}

// diagnostics: the chunk ends of a limit scan over n_tiles tiles (limit_chunk_ends; tests/test_limit_chunks_host.py walks them)
extern "C" int imm3_plan_limit_chunks(int64_t n_tiles, int64_t *ends_out, int32_t cap) {
    const LimitChunks c = limit_chunk_ends(n_tiles);
    for (int i = 0; i < c.n && i < cap && ends_out; ++i) ends_out[i] = c.end[i];
    return c.n;
}

// diagnostics: the same for the limit-aware table launch (table_limit_applies; tests/test_table_limit_host.py walks it)
extern "C" int imm3_plan_table_limit(int32_t table, int32_t tree, int64_t limit, int32_t count_in_scan, int32_t single_tile_pass, int32_t whole, int32_t count_log_on,
                                     int32_t count_only, int32_t filter_variant, int64_t n_tiles, int32_t grid) {
    TableLimitInputs in;
    in.table = table != 0;
    in.tree = tree != 0;
    in.limit = limit;
    in.count_in_scan = count_in_scan != 0;
    in.single_tile_pass = single_tile_pass != 0;
    in.whole = whole != 0;
    in.count_log_on = count_log_on != 0;
    in.count_only = count_only != 0;
    in.filter_variant = filter_variant;
    in.n_tiles = n_tiles;
    in.grid = grid;
    return table_limit_applies(in) ? 1 : 0;
}

// diagnostics: which kernel a string Match goes to (pred_route; tests/test_str_rows_host.py walks it): 0 the tile kernel (2-byte
// strings, <= 8 values), 1 k_filter_str_rows (a width that is a multiple of 4), 2 the word-at-a-time kernel (what a table refuses)
extern "C" int imm3_plan_string_route(int32_t width, int32_t n_match) {
    if (width < 1 || width > IMM3_STRING_MAX_WIDTH || n_match < 1) return -1;
    FoldedPred fp;
    fp.kind = KIND_STR;
    fp.width = width;
    fp.match.assign((size_t)n_match, std::string((size_t)width, 'x'));
    return pred_route(fp);
}
