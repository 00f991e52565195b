/*
 * imm3_diag.h -- measurement and tuning hooks of libimm3.so.  NOT part of the drop-in boundary (include/imm3.h): nothing
 * a GpuScanOp / GpuSelectOp / GpuProjectOp binds lives here.  bench.py, tools/ and the roofline tests use them to time
 * kernels with HIP events, to cross-check that timing against the device clock, to measure the GPU's read-only
 * streaming ceiling, and to A/B kernel variants.
 */
#ifndef IMM3_DIAG_H
#define IMM3_DIAG_H

#include "imm3.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- live kernel timing (HIP events on the context's stream) ----
 * When enabled, every kernel launch of this context is bracketed by an event pair.
 * kernel ids: 0 = scan+select, 1 = offsets scan, 2 = compact+gather, 3 = count reduce, 4 = group-by aggregation,
 *             5 = PFOR_INT / snappy column decode, 6 = refine pass of a MAX over a string wider than 8 bytes (one per pass),
 *             7 = ORDER BY of an ordered query: ONE record per order, from its first kernel's start to its last one's end,
 *             8 = ORDER BY over groups (imm3_query_set_group_order): ONE record per ordered settle, from the small launch's start (or
 *                 the radix path's key launch's) to the end of the launch that writes the ordered groups,
 *             9 = a view of merged groups (imm3_comm_merge_groups_view): ONE record per view, from the small launch's start (or the
 *                 radix path's key launch's) to the end of the launch that writes the ordered records,
 *             10 = the mark pass of an IMM3_AGG_COUNT_DISTINCT aggregate (one per such aggregate), 11 = the clear of its pair set. */
int imm3_ctx_timing_enable(imm3_ctx *ctx, int32_t max_records);
int imm3_ctx_timing_reset(imm3_ctx *ctx);
/* Only launches whose kernel id has its bit set in `kernel_mask` are bracketed (default: all). */
int imm3_ctx_timing_mask(imm3_ctx *ctx, uint32_t kernel_mask);
/* Synchronises, then writes up to cap durations (ms) of launches of `kernel_id`, oldest first. */
int imm3_ctx_timing_collect(imm3_ctx *ctx, int32_t kernel_id, float *ms_out, int32_t cap, int32_t *n_out);

/* Cross-check of the event timing: when enabled, every tile-kernel launch also records, per work-group, the 100 MHz
 * device clock at entry and exit; collect() returns per launch (last work-group's exit - first work-group's entry) in
 * ms, oldest first.  Diagnostics only (bench.py's instrumented pass); costs two stores per work-group. */
int imm3_ctx_devclock_enable(imm3_ctx *ctx, int32_t max_launches);
int imm3_ctx_devclock_collect(imm3_ctx *ctx, float *ms_out, int32_t cap, int32_t *n_out);
/* The raw stamps of one recorded launch (100 MHz ticks): [2 b] / [2 b + 1] = entry / exit of work-group b; the tools' build of
 * the single-pass kernel adds per-range stamps behind them. */
int imm3_ctx_devclock_raw(imm3_ctx *ctx, int32_t launch, uint64_t *out, int32_t n);

/* Empirical read-only streaming ceiling of this GPU: times a kernel that only reads `bytes` (non-temporal dword loads,
 * same tiling and grid as the scan+select kernel, three rotated buffers) and returns the median GB/s over `iters`. */
int imm3_ctx_measure_read_gbps(imm3_ctx *ctx, uint64_t bytes, int32_t iters, double *gbps);

/* Tuning knobs (0 = default): filter variant, grid size in workgroups.  For experiments/bench.
 * variant 1 = word-at-a-time kernel only (a select tree over an imm3_table has no such kernel: under variant 1 its run calls
 * answer IMM3_ERR_ARG), 2 = count reduce on the aux stream, 3 = no survivor staging,
 * 4 = stage int32 columns only, 5 = PFOR_INT predicates read the decoded column instead of the compressed blocks,
 * 7 = reduce the count with a separate k_total launch instead of inside the filter kernel,
 * 6 = projections never use the one-launch kernel, 8 = they use it with gathered SELECT-list columns too, 9 = gathered int32
 * columns are streamed through it whatever the selectivity, 10 = no sampled selectivity estimate at query creation (the plan
 * then adapts from the first run's count on), 11 = survivor records are staged even when no predicate column is projected,
 * 12 = the plan made at creation stands whatever the cost model predicts (tests of one plan's kernels; P still adapts) and no
 * bitmap lines are parked in LDS, 13 = a one-launch select chain reduces its count inside the filter kernel only at <= 512
 * work-groups (default: at every grid), 14 = a `limit` query scans the whole segment in one launch instead of in chunks behind a limit-reached word, and the whole table instead of stopping at the limit (decided per run),
 * 15 = a small limit behind a limit scan takes k_scan + k_gather instead of the one fused launch (k_limit_gather),
 * 16 = one-launch projections use every CU even while a communicator whose collectives launch kernels is attached (default: one
 * CU per XCD is left to the collective's kernel), 17 = an aggregation's select chain runs as its own launch instead of inside the
 * aggregation launch, 18 = group keys wider than 8 bytes hash to 3 bits, so that distinct keys collide by construction (tests of
 * the exactness of the key compare), 19 = a projection through survivor records stores its bitmap in the staging launch (default: the bitmap is
 * materialised when imm3_query_bitmap asks), 23 = an ordered query with a limit sorts every row (no radix select: the
 * yardstick of tests/test_gpu_zz_perf_order.py), 24 = it takes the radix select whenever the limit is below the survivors (both also
 * pin the radix path of imm3_query_set_group_order), 25 = an ordered aggregation takes the radix path whatever its group count (no
 * one-work-group launch: the yardstick of tests/test_gpu_zz_perf_group_order.py), 26 = int32 range predicates scan the column itself (no
 * 16-bit high-half plane is made at creation or read by a run: A/B runs of the tools), 20 - 22 and 34 - 35 = ablation switches of k_filter_tile and k_emit (tools' build,
 * libimm3_ablate.so, only), 50 + mask = ablation mask of k_filter_project (tools' build), 100 + AggForm = the aggregation starts at
 * that kernel form, 140 and above = aggregation ablations (tools' build), 200 + P = fixed tiles per range.  The names of these
 * numbers are csrc/imm3_handles.h's TuningVariant. */
int imm3_ctx_set_tuning(imm3_ctx *ctx, int32_t filter_variant, int32_t grid_blocks);

/* The projection planner's cost model (csrc/imm3_plan.h): predicted microseconds of one run's kernels under plan A (one launch), B
 * (survivor records) and C (the bitmap path) for a query shape -- predicate columns' widths and IN-list sizes, the SELECT list's
 * widths and which of its entries are predicate columns, the bytes of a survivor record -- with sigma = survivors per row, sloc =
 * survivors per row where there are survivors, full = share of the survivors in fully surviving stretches.  out_abc: 3 values. */
int imm3_plan_predict(int64_t n_rows, const int32_t *pred_width, const int32_t *pred_match, int32_t n_pred, const int32_t *proj_width,
                      const int32_t *proj_is_pred, int32_t n_proj, int32_t rec_bytes, double sigma, double sloc, double full, double *out_abc);

/* How the library planned a query (tests assert the path they mean to exercise; tools print it).
 * out[0] = 1 when an unlimited projection runs as ONE launch (k_filter_project: the filter kernel writes the rows), else 0;
 * out[1] = tiles per wave per span (P: lowered by the library once a getter has seen how many rows a run selected); out[2] = work-groups of that launch; out[3] = spans;
 * out[4] = 1 when the projection goes through survivor records in HBM (filter -> k_scan -> k_emit), else 0;
 * out[5] = dwords per survivor record; out[6] = 1 when the last run used the single-pass launch; out[7] = how often
 * imm3_query_run has waited for the device so far (an unreserved unlimited projection: once, on its first run);
 * out[8] / out[9] = single-pass runs of this query whose rows a getter had to gather from the bitmap because the launch gave up on
 * them: a look-back wait timed out (the query keeps the bitmap path from then on) / another launch of the kernel owned the device
 * (that run only); out[10] = runs whose small-limit gather (k_limit_gather) ran into its look-back poll cap, so that a getter
 * gathered the rows again with k_scan + k_gather.
 * Ordered queries (imm3_query_set_order), the tail: out[11] / out[12] = ordered runs, as far as a row getter has settled them, that
 * took the radix select in front of the sort (0 < limit, survivors >= 4 x limit) / that sorted every row; out[13] = times the order
 * has been enqueued (once per run, once more whenever a getter had to emit the rows again).
 * out[14] = 1 when a pass of the last select run scanned an int32 column over its 16-bit high-half plane (the TK_H16 tile kind), 0 when
 * every int32 predicate read the column itself.  n <= 15 values. */
int imm3_query_plan(const imm3_query *q, int64_t *out, int32_t n);

/* imm3_query_hi16_refined: *refined = 1 when a FULL tile of a plane scan of this query (out[14] above) has compared full values -- held a
 * row whose half does not decide and that no other column had failed: the refine -- in a run since the last call, else 0 (the rolled
 * last tile of a segment reads the column itself and does not count).  The word is set on the device by such a tile; the call waits
 * for the context's stream, reads it and clears it.  IMM3_ERR_STATE while a graph capture is open.
 * imm3_segment_hi16_plane: the plane of column `col` as k_hi16_build wrote it.  *state: 0 = no query has asked for one yet, 1 = it is
 * there (up to cap_rows halves are copied to `out` when out is not null), -1 = the column gets none; min_max = {smallest, largest}
 * half as the build reduced them ({32767, -32768} before any build). */
int imm3_query_hi16_refined(imm3_query *q, int32_t *refined);
int imm3_segment_hi16_plane(const imm3_segment *seg, int32_t col, int16_t *out, int64_t cap_rows, int32_t *state, int32_t *min_max);

/* imm3_query_agg_form: the kernel form of an aggregation's last launch (csrc/imm3_internal.h's AggForm: 0 = lanes (63 keys), 1 = lanes
 * (127 keys), 2 = direct, 3 = tile, 4 = general), after any re-run from a later form that a full per-work-group table forced; -1
 * before the first run.  IMM3_ERR_ARG for a query that is not an aggregation. */
int imm3_query_agg_form(const imm3_query *q, int32_t *form);

/* imm3_query_group_order_path: the path the last ordered settle of an aggregation took (imm3_query_set_group_order; a getter orders
 * the groups): 0 = none (no order set, or no getter has asked since the last run or change of order), 1 = the one-work-group launch
 * (k_group_order_small: up to 2048 groups), 2 = the radix path sorting every group, 3 = the radix path with the radix select in front
 * (0 < limit, groups >= 4 x limit).  IMM3_ERR_ARG for a query that is not an aggregation. */
#define IMM3_GROUP_ORDER_SMALL_MAX 2048
int imm3_query_group_order_path(const imm3_query *q, int32_t *path);

/* imm3_comm_merge_view_path: the path the last imm3_comm_merge_groups_view on this communicator took, with the values above: 0 = none
 * (no view yet, a failed call, or an empty merged list), 1 = the one-work-group launch (up to 2048 merged groups), 2 = the radix path
 * sorting every kept group, 3 = the radix path with the radix select in front. */
int imm3_comm_merge_view_path(const imm3_comm *c, int32_t *path);

/* imm3_merge_view_plan_json: the host-only plan of a view of merged groups, without a device or a handle.  The aggregation's shape
 * is given as plain values (column kinds: 0 = int32, 1 = int8, 2 = string); json_out receives, NUL-terminated,
 *   {"seg_bytes":S,"user_bytes":U,"key_bytes":U+S+4,"canonical_bytes":N,"hash":"<16 hex digits>"}
 * -- S the tie's segment bytes for `largest_segment_index`, the hash that of the canonical bytes (keys, program, limit) the ranks vote
 * on.  `needed` (may be NULL) the bytes that takes; cap = 0 only asks for `needed`.  Errors as imm3_comm_merge_groups_view's: a bad key
 * or leaf, or the refusal that begins with IMM3_MERGE_VIEW_REFUSED. */
int imm3_merge_view_plan_json(int32_t n_group, const int32_t *group_kind, const int32_t *group_width, int32_t n_aggs, const int32_t *agg_kind,
                              const int32_t *agg_col_kind, const int32_t *agg_col_width, const imm3_group_view *view, uint32_t largest_segment_index,
                              char *json_out, int64_t cap, int64_t *needed);

/* imm3_query_group_filter_stats: what the device's filter did in the last settled view of an aggregation with a filter set
 * (imm3_query_set_group_filter): *groups_in = the dense groups it evaluated, *groups_kept = those the program kept (before the limit),
 * both read back from the device's count words.  Zeros when no filter is set or the view is stale (no getter has asked since the last
 * run or change of filter / order).  A filtered settle reports its path through imm3_query_group_order_path like an ordered one.
 * IMM3_ERR_ARG for a null argument or a query that is not an aggregation. */
int imm3_query_group_filter_stats(const imm3_query *q, uint64_t *groups_in, uint64_t *groups_kept);

/* imm3_group_filter_check: imm3_query_set_group_filter's argument checks on plain values, no query and no device: the n_aggs aggregates'
 * kinds (IMM3_AGG_*) and their columns' kinds (0 = int32, 1 = int8, 2 = string), then the leaves and the program.  is_agg == 0 stands
 * for a query that is no aggregation.  Returns what the entry point would return; the message is imm3_last_error's.  With
 * count_vals != NULL and an accepted program it also evaluates it on ONE group -- count_vals[0] = the count, count_vals[1 .. 4] = the
 * four values -- with the evaluator the kernels run, and stores 0 / 1 in *kept. */
int imm3_group_filter_check(int32_t is_agg, const int32_t *agg_kind, const int32_t *agg_col_kind, int32_t n_aggs, const imm3_group_filter_leaf *leaves,
                            int32_t n_leaves, const int32_t *prog, int32_t n_prog, const int64_t *count_vals, int32_t *kept);

/* imm3_query_expr_form: which kernel the last select launch of a select-tree query (an IMM3_EXPR_OR or IMM3_EXPR_NOT in its program) ran: 0 = the tile
 * form (k_filter_expr), 1 = the generic form (k_filter_expr_generic); -1 before the first launch, for a tree that selects nothing
 * (no launch at all) and for every other query.  A tree that selects EVERY row runs the NoSelect scan: 0 when that is the tile
 * kernel's launch, 1 when it is the word-at-a-time kernel's (ragged layouts). */
int imm3_query_expr_form(const imm3_query *q, int32_t *form);

/* imm3_expr_normalize: the normal form of a select tree, without a device or a handle (tests hold the terms' truth table against the
 * tree's).  Columns are given by codec and width; a leaf's `column` indexes them.  json_out receives, NUL-terminated,
 *   [[{"col":c,"lo":l,"hi":h} | {"col":c,"match":["<hex bytes>", ...]} | {"col":c,"not_match":[...]}, ...], ...]     one inner list per term
 * ("not_match": a negated IN-list, the exclusions of a complemented Match; a tree that selects every row is [[]], one that selects nothing [])
 * `needed` (may be NULL) the bytes that takes; cap = 0 only asks for `needed`.  Errors as at query creation; a normal form of
 * more than 64 terms is IMM3_ERR_ARG. */
int imm3_expr_normalize(const int32_t *col_codec, const int32_t *col_width, int32_t n_cols, const imm3_select *leaves, int32_t n_leaves,
                        const int32_t *prog, int32_t n_prog, char *json_out, int64_t cap, int64_t *needed);

/* ---- fault injection into the single-pass projection kernel (k_filter_project, csrc/imm3_project.hip) ----
 * The kernel's work-groups wait on each other; what happens when such a wait does not resolve must be exercised on a device.
 * imm3_ctx_inject_fault: in every later single-pass launch of this context, work-group `work_group` never announces its
 * `span`-th span (so the round of spans it belongs to never completes), and look-back waits give up after `max_polls` polls
 * (0 = the shipped cap, ~0.1-0.2 s).  work_group = -1 switches the fault off.  Only the TOOLS' build of the library carries the
 * code (make -C immutable3_amd/csrc ablate -> lib/libimm3_ablate.so); the shipped library answers IMM3_ERR_STATE to anything
 * but "off".
 * imm3_ctx_debug_device_lock: overwrites the per-device ticket word that keeps two launches of the kernel from sharing the
 * device (0 = free) and returns what it held; with a foreign ticket in place every launch finds the device busy.  Synchronises
 * the context's stream first.  TOOLS' build only, like the fault injection (round 4 shipped it: any caller could have parked every
 * one-launch query of a device, in every context, on its fallback); the shipped library answers IMM3_ERR_STATE. */
/* imm3_comm_debug_standin (tools' build; the shipped library answers IMM3_ERR_STATE to anything but "off"): from now on every
 * imm3_comm_allreduce_count of this communicator first launches, on the communicator's stream, `work_groups` work-groups of a kernel
 * with the footprint of RCCL's all-reduce kernel (512 threads, 256 vector registers per lane, 37 664 bytes of LDS) that spin for
 * `spin_us` microseconds: what a multi-rank collective puts on the device beside the next pass's scans, measurable on one GPU
 * (tools/overlap_probe.py).  work_groups = 0 switches it off. */
/* imm3_plan_limit_scan: does a projection with a `limit` scan in chunks that stop once the limit is reached (1) or as one whole
 * select (0)?  The library's own decision (csrc/imm3_planner.cpp: limit_scan_applies) as a pure function of its inputs -- no device,
 * no handle: tests walk it. */
int imm3_plan_limit_scan(int32_t whole, int32_t count_log_on, int32_t count_in_scan, int64_t limit, int32_t single_tile_pass, int32_t table, int32_t records,
                         int32_t skip_bitmap, int32_t overlap_total, int32_t filter_variant, int64_t n_tiles);
/* imm3_plan_limit_chunks: the chunks such a scan runs as over a segment of n_tiles tiles (csrc/imm3_planner.cpp: limit_chunk_ends,
 * pure): returns their number (at most 32) and writes the first `cap` chunk ends -- the tile a chunk stops before -- to ends_out,
 * ascending: 1024, 8192, 32 768, ... (x 4) while below n_tiles, then n_tiles itself.  n_tiles <= 0: no chunk. */
int imm3_plan_limit_chunks(int64_t n_tiles, int64_t *ends_out, int32_t cap);
/* imm3_plan_table_limit: does a projection with a `limit` over an imm3_table run its select as the one launch that stops at the limit
 * (1: k_filter_table_limit -- work-groups claim runs of 32 virtual tiles in ascending order and stop claiming once the finished runs
 * have selected `limit` rows) or as the whole select (0)?  csrc/imm3_planner.cpp: table_limit_applies, pure like the decision above.
 * 1 needs: a table; a flat query (tree = 0: no IMM3_EXPR_OR / IMM3_EXPR_NOT); limit > 0; a projection behind the select (count_in_scan); a select chain
 * of one tile launch; not a getter's whole select; no count log; not a count-only run; not tuning variant 7 or 14; and
 * n_tiles > grid * 32, `grid` being the launch's work-groups. */
int imm3_plan_table_limit(int32_t table, int32_t tree, int64_t limit, int32_t count_in_scan, int32_t single_tile_pass, int32_t whole, int32_t count_log_on,
                          int32_t count_only, int32_t filter_variant, int64_t n_tiles, int32_t grid);
/* imm3_plan_string_route: which kernel a Match on a string column of `width` bytes with `n_match` IN-list values goes to on a uniform
 * layout (csrc/imm3_planner.cpp: pred_route, pure): 0 = the tile kernel (2-byte columns, at most 8 values), 1 = k_filter_str_rows (a
 * width that is a multiple of 4, 4 .. 256, any IN-list), 2 = the word-at-a-time kernel -- the one an imm3_table does not have, so
 * 2 is what a table query refuses at creation.  -1: width outside 1 .. IMM3_STRING_MAX_WIDTH or an empty list. */
int imm3_plan_string_route(int32_t width, int32_t n_match);
/* imm3_plan_string_range_route: the same for an IMM3_STR_RANGE leaf (neither empty nor full) on a string column of `width` bytes:
 * 1 = the string pass (k_filter_str_range: widths 4, 8, ... 256), 2 = the word-at-a-time kernel (every other width in 1 .. 256: what
 * a table refuses), -1 outside. */
int imm3_plan_string_range_route(int32_t width);
/* IMM3_INT_IN (csrc/imm3_int_list_plan.cpp, pure).  imm3_plan_int_list_table: the open-addressing table query creation builds for
 * `n` int32 values (any order, duplicates count once): *n_slots slots (a power of two, >= 16 and >= 2 x the distinct values), empty
 * slots holding *empty (an int32 the list does not hold), values inserted in ascending order by linear probing from the home slot
 * (the top bits of (uint32_t)v * 0x9E3779B1), *max_probe = the longest insertion distance + 1 -- the step bound of every probe.  With
 * cap == 0 only the three figures are returned; else slots_out takes the slots (cap >= *n_slots, or IMM3_ERR_ARG).
 * imm3_plan_int_list_form: the form of k_filter_int_list a folded list of n values takes on a column of `width` bytes: 0 = int8 (a
 * 256-bit set, any n), 1 = int32, the values as kernel arguments, 2 = int32, the table copied into LDS, 3 = int32, the table in
 * device memory; -1: width not 1 or 4, n outside 0 .. IMM3_INT_IN_MAX_VALUES.
 * imm3_plan_int_list_probe: the kernels' probe on the host (the same inline code): 1 = v is found within max_probe steps, 0 = not,
 * -1 = n_slots is no power of two in 16 .. 2^25. */
int imm3_plan_int_list_table(const int32_t *values, int64_t n, int32_t *slots_out, int64_t cap, int64_t *n_slots, int32_t *empty, int32_t *max_probe);
int imm3_plan_int_list_form(int32_t width, int64_t n);
int imm3_plan_int_list_probe(const int32_t *slots, int64_t n_slots, int32_t empty, int32_t max_probe, int32_t v);
/* Integer sets built from selections (imm3_int_set_create; csrc/imm3_int_set_plan.cpp is pure, the rest needs a device).
 * imm3_plan_int_set_scratch_slots: the slots of the scratch table a build inserts into, for `selected_rows` selected rows whose values
 * span [min, max] under a cap of `cap` distinct values: imm3_plan_int_list_table's slot rule (a power of two, >= 16, >= 2 x) applied to
 * min(selected_rows, max - min + 1, cap), 16 for no rows or min > max; -1: cap outside 0 .. IMM3_INT_IN_MAX_VALUES.
 * imm3_int_set_create_capped: imm3_int_set_create with `max_values` (1 .. IMM3_INT_IN_MAX_VALUES) in the cap's place: more distinct
 * values than that give the IMM3_ERR_ARG of "too many distinct values" at a size a test can afford.
 * imm3_int_set_table: the set's probe table as it stands on the device -- *n_slots slots (0 for an empty set), what a free slot holds,
 * the step bound of every probe, the 256-bit set of the values in -128 .. 127 (8 words), and whether the host built the table (the set
 * holds INT32_MIN and INT32_MAX).  With cap == 0 only the figures are returned; else slots_out takes the slots (cap >= *n_slots). */
int64_t imm3_plan_int_set_scratch_slots(int64_t selected_rows, int32_t min, int32_t max, int64_t cap);
int imm3_int_set_create_capped(imm3_ctx *ctx, imm3_query *const *sources, const int32_t *columns, int32_t n_sources, int64_t max_values, imm3_int_set **out);
int imm3_int_set_table(imm3_int_set *s, int32_t *slots_out, int64_t cap, int64_t *n_slots, int32_t *empty, int32_t *max_probe, uint32_t *set256, int32_t *host_route);
/* The 16-bit high-half plane of a DENSE_INT column (csrc/imm3_hi16_plan.cpp, pure).  imm3_plan_hi16_bounds: the closed interval
 * [lo, hi] over the halves v >> 16 as two windows of 16-bit wrap-around arithmetic, out4 = {possible_first, possible_count,
 * certain_first, certain_count}: a half h is in a window when (uint16_t)(h - first) < count; outside the possible window a row fails,
 * inside the certain window it passes, in between its full value is compared.
 * imm3_plan_hi16_class: what that says of one half (-32768 .. 32767; -1 outside): 0 = fails, 1 = passes, 2 = undecided.
 * imm3_plan_hi16_span_ok: 1 when a column whose halves span min_half .. max_half keeps its plane (at least 64 distinct halves).
 * imm3_plan_hi16_eligible: 1 when a tile pass's int32 predicate scans the plane.  flags: bit 0 the query is over a table, 1 it is a
 * select tree, 2 the layout is ragged, 3 the column is DENSE_INT, 4 the folded predicate is an IN-list, 5 the pass stages survivor
 * records, 6 it is a chunk of a limit scan, 7 the column has a plane, 8 the tuning variant pins the int32 scan; n_i32 / n_i8 / n_s2:
 * the pass's columns by kind. */
int imm3_plan_hi16_bounds(int32_t lo, int32_t hi, uint32_t *out4);
int imm3_plan_hi16_class(int32_t lo, int32_t hi, int32_t half);
int imm3_plan_hi16_span_ok(int32_t min_half, int32_t max_half);
int imm3_plan_hi16_eligible(uint32_t flags, int32_t n_i32, int32_t n_i8, int32_t n_s2);
/* imm3_plan_distinct_capacity: the entries of an IMM3_AGG_COUNT_DISTINCT aggregate's pair set (csrc/imm3_distinct_plan.cpp:
 * distinct_capacity, pure) for a query over `rows` rows with a packed group key of `key_bytes` bytes and a value column of `width`
 * bytes: the power of two at or above 2 x min(rows, min(rows, 256^key_bytes) x 256^width), at least 1024.  -1: more than 2^28 (what
 * creation refuses); -2: rows < 0, key_bytes < 0 or width outside 1 .. 4. */
int64_t imm3_plan_distinct_capacity(int64_t rows, int32_t key_bytes, int32_t width);
struct imm3_comm;
int imm3_comm_debug_standin(struct imm3_comm *comm, int32_t work_groups, uint32_t spin_us);
int imm3_ctx_inject_fault(imm3_ctx *ctx, int32_t work_group, int32_t span, uint32_t max_polls);
int imm3_ctx_debug_device_lock(imm3_ctx *ctx, uint64_t value, uint64_t *previous);

#ifdef __cplusplus
}
#endif
#endif /* IMM3_DIAG_H */
