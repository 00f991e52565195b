// imm3_api_internal.h -- what imm3_api.cpp (the C ABI but for the run calls: validation, creation, getters, aggregation), imm3_run.cpp
// (the run calls and their launches), imm3_planner.cpp (plans and their geometry) and imm3_expr_norm.cpp (select trees) share: only
// what crosses between them.  Internal to libimm3: nothing here is part of include/imm3.h.
#pragma once

#include "imm3_handles.h"

// Entry into a context (imm3_sync.h): the call passes the context's capture gate -- shared, so calls of any number of
// threads run side by side; while ANOTHER thread has a graph capture open it waits here until that capture ends.
// (Declares a scope guard: one use per function scope.)
#define CTX_LIVE_RUN(c)                                                                           \
    if (!(c)) return fail(IMM3_ERR_ARG, "ctx is null");                                           \
    imm3::GateScope imm3_gate_scope_(&(c)->gate);                                                 \
    if ((c)->closed) return fail(IMM3_ERR_STATE, "the context of this handle has been destroyed")
// every entry point but the run calls: not while THIS thread's graph capture is open (most of them synchronise or allocate)
#define CTX_LIVE(c)                                                                               \
    CTX_LIVE_RUN(c);                                                                              \
    if ((c)->capture) return fail(IMM3_ERR_STATE, "a graph capture is open on this context: only imm3_query_run / imm3_query_run_select and imm3_ctx_capture_end are accepted")

namespace imm3 {

// ---- imm3_api.cpp ----
hipError_t pool_alloc(imm3_ctx *ctx, void **out, size_t bytes);      // the context's caching allocator (stream-ordered reuse)
void pool_release(imm3_ctx *ctx, void *p);
void graphs_mark_stale(imm3_ctx *ctx, const imm3_query *q);          // recorded graphs that replay this query point at buffers that are about to move
int ensure_row_capacity(imm3_query *q, uint64_t rows);               // the projection's output arrays, for at least `rows` rows
extern const char *const kTableGenericRefusal;                       // a table has no word-at-a-time kernel: the refusal's text, at creation and at a run
int run_agg(imm3_query *q);                                          // ProjectAggOp behind (or fused with) the select: the aggregation launch
bool agg_run_fuses(const imm3_query *q);                             // ... which evaluates the select chain itself: no run_select
int query_bitmap_current(imm3_query *q);                             // the select bitmap of the whole selection on the device, as imm3_query_bitmap settles it (and a run where none was stored)
int segment_dense_column(imm3_ctx *ctx, const imm3_segment *seg, int32_t col); // the decoded form of a PFOR_INT / snappy column, made on first need

// ---- imm3_int_set_api.cpp: integer sets built from selections (imm3_int_set_create) and their leaf, IMM3_INT_IN_SET ----
imm3_int_set *int_set_retain(imm3_int_set *s);
void int_set_release(imm3_int_set *s);
int int_set_check_leaf(imm3_ctx *ctx, int32_t n_match, const uint8_t *handle); // the leaf's own checks: one handle, live, of this context
extern const char *const kIntSetOneListRefusal;                       // a column with a set leaf takes no other IMM3_INT_IN / IMM3_INT_IN_SET leaf
extern const char *const kTreeIntSetRefusal;                          // a program with an OR or a NOT takes no IMM3_INT_IN_SET leaf

// Hands out one event pair per launch when timing is on; the launcher stamps it with the kernel's own
// start and end (hipExtLaunchKernelGGL), so elapsed time == kernel duration as rocprofv3 reports it.
struct LaunchTimer {
    hipEvent_t start = nullptr, stop = nullptr;
    LaunchTimer(imm3_ctx *ctx, int32_t id) {
        if (!ctx->timing.load(std::memory_order_relaxed) || ctx->capture || !((ctx->timing_mask.load(std::memory_order_relaxed) >> id) & 1u)) return;
        std::lock_guard<std::mutex> lk(ctx->mu); // (diagnostics only: the lock is taken when timing is on)
        if (ctx->used < ctx->pool.size()) {
            TimingRecord &rec = ctx->pool[ctx->used++];
            rec.kernel_id = id;
            start = rec.start;
            stop = rec.stop;
        }
    }
};

// ---- imm3_run.cpp ----
// What a caller of run_select wants, OR-ed together; SEL_DEFAULT: store the bitmap, reduce the count on the main stream.
enum SelectMode : unsigned {
    SEL_DEFAULT = 0,
    SEL_OVERLAP_TOTAL = 1u << 0, // nothing on the main stream needs the count: reduce it on the aux stream (TV_COUNT_ON_AUX)
    SEL_COUNT_IN_SCAN = 1u << 1, // a projection follows on the same stream; its offsets scan publishes the count (no k_total launch)
    SEL_COUNT_ONLY = 1u << 2,    // the caller wants selected.size alone -- a chain that is ONE tile launch then stores no bitmap
    SEL_WHOLE = 1u << 3,         // never in chunks (the getters' full select)
    SEL_PLAIN = 1u << 4,         // stage no survivor records: the bitmap is what the caller wants (settle_lazy_bitmap)
};
int run_select(imm3_query *q, unsigned mode);                        // ScanOp -> SelectOp*: bitmap and count; mode: SelectMode bits
int launch_project(imm3_query *q);                                   // the gather behind an offsets scan: from the records a run staged, else from the bitmap
int run_order(imm3_query *q);                                        // an ordered query: key build, select / sort, apply behind the rows as last emitted (enqueued, no host wait)
int join_total(imm3_query *q, hipStream_t s);                        // make `s` wait for the count reduce on the aux stream
void fill_colpred(const imm3_query *q, const FoldedPred &fp, ColPred &cp);
void fill_tile_col(const imm3_query *q, const FoldedPred &fp, TileCol &c, int kind);
Hi16Inputs hi16_inputs(const imm3_query *q, const FoldedPred &fp, const std::vector<const FoldedPred *> &take); // what hi16_eligible asks of a tile pass's int32 predicate (imm3_run.cpp)
#ifdef IMM3_ABLATE
int single_pass_lock_word(int device, unsigned long long **out);     // the device's ticket word of the single-pass kernel (imm3_ctx_debug_device_lock)
#endif

// scalar rules shared with the reference (JVM d2i / i2b): Select.scala:65,73; SURVEY Appendix A.1 rule 5
inline int32_t jvm_d2i(double d) {
    if (d != d) return 0;
    if (d >= 2147483647.0) return INT32_MAX;
    if (d <= -2147483648.0) return INT32_MIN;
    return (int32_t)d;
}
inline int32_t jvm_d2b(double d) { return (int32_t)(int8_t)(uint8_t)((uint32_t)jvm_d2i(d) & 0xFFu); }

// ---- imm3_expr_norm.cpp: select trees (imm3_query_create_expr) ----
struct ExprCol { int32_t seg_col, vcodec, width; };   // the column a leaf is on: segment column, its DENSE_* value codec, bytes per value
typedef std::vector<FoldedPred> ExprTerm;             // a conjunction: at most one folded predicate per column
int leaf_pred(int32_t seg_col, int32_t vcodec, int32_t width, const imm3_select &leaf, FoldedPred &out); // one leaf alone
void merge_pred(FoldedPred &into, const FoldedPred &other);                                             // ... AND another on the same column
bool pred_empty(const FoldedPred &p);                                                                    // no value passes
bool pred_unconstrained(const FoldedPred &p);                                                            // every value passes
int expr_check_program(const int32_t *prog, int32_t n_prog, int32_t n_leaves, bool *has_or, bool *has_not); // IMM3_ERR_ARG: malformed; the out-flags (may be null): an IMM3_EXPR_OR / an IMM3_EXPR_NOT in it
int expr_normalize(const std::vector<ExprCol> &leaf_cols, const imm3_select *leaves, int32_t n_leaves, const int32_t *prog, int32_t n_prog,
                   std::vector<ExprTerm> &terms);

// ---- imm3_order_args.cpp: the argument checks of imm3_query_set_order, over plain values ----
int order_check_args(bool is_agg, int32_t n_proj, const int32_t *proj_widths, int64_t create_limit, bool has_run,
                     const imm3_order_key *keys, int32_t n_keys, int64_t limit, int32_t *key_bytes_out);

// ---- imm3_group_order_api.cpp: the ordered view of an aggregation's groups (imm3_query_set_group_order) ----
void group_order_release(imm3_query *q);                              // its buffers back to the pool (query destruction; grown dense arrays)
int group_order_settle(imm3_query *q, uint32_t *n_groups);            // settle the groups, order them on the device: *n_groups = min(groups, limit)
int group_order_fetch_groups(imm3_query *q, uint64_t *keys, uint32_t *first_row, uint64_t *counts, int64_t *vals, uint32_t max_groups);
int group_order_fetch_strings(imm3_query *q, int32_t agg, uint8_t *out, uint32_t max_groups); // `agg` checked by the caller
int group_order_fetch_keys(imm3_query *q, uint8_t *out, uint32_t max_groups);

// ---- imm3_str_range.cpp: IMM3_STR_RANGE over plain values ----
int str_range_check_leaf(int32_t n_match, const uint8_t *bytes, const int32_t *lens, int32_t width);   // the leaf's own checks (width <= 0: not held against a column)
void str_range_pad(const uint8_t *lo, int32_t lo_len, const uint8_t *hi, int32_t hi_len, int32_t width, std::string &lo_out, std::string &hi_out);
bool str_range_empty(const std::string &lo, const std::string &hi);                                      // lo' > hi'
bool str_range_full(const std::string &lo, const std::string &hi);                                       // every row passes
bool str_range_holds(const std::string &lo, const std::string &hi, const std::string &v);
void str_range_intersect(std::string &lo, std::string &hi, const std::string &lo2, const std::string &hi2);
void str_range_filter_match(const std::string &lo, const std::string &hi, std::vector<std::string> &match);
bool str_range_successor(std::string &v);
bool str_range_predecessor(std::string &v);
int str_range_route(int32_t width);
void str_range_pack(const std::string &lo, const std::string &hi, std::vector<uint8_t> &blob, uint32_t lo4[4], uint32_t hi4[4]);
extern const char *const kTreeIntInRefusal;                           // imm3_expr_norm.cpp: a program with an OR or a NOT takes no IMM3_INT_IN leaf
extern const char *const kTableRangeRefusal;                       // a table has no word-at-a-time kernel: a range on a width the string pass does not take

// ---- imm3_planner.cpp ----
constexpr int kSampleChunks = 8;                                      // the sample a plan is made on: eight chunks of 64 tiles spread over the segment / table
constexpr int64_t kSampleChunkTiles = 64;
constexpr int kSampleTiles = kSampleChunks * (int)kSampleChunkTiles;
constexpr int64_t kLimitFirstChunkTiles = 1024;                       // a limit scan's first chunk ends here, the second at
constexpr int64_t kLimitSecondEndTiles = 8192;                        // ... this tile, every later one at 4 x the end before it
constexpr int kLimitMaxChunks = 32;                                   // (27 such ends fit an int64_t)

int tile_kind(const FoldedPred &fp);
bool str_rows_pred(const FoldedPred &fp);
int pred_route(const FoldedPred &fp);
int32_t single_pass_run_grid(const imm3_query *q);
bool single_pass_reserves(const imm3_query *q);
void single_pass_set_P(imm3_query *q, int32_t P);
void single_pass_pick_P(imm3_query *q, double sigma, bool sure);
void single_pass_adapt(imm3_query *q, uint64_t survivors, int64_t dense_ranges);
int single_pass_setup(imm3_query *q);
PlanDensity plan_density_for(const imm3_query *q, uint64_t survivors);
double plan_cost_three_launches(const imm3_query *q, const PlanDensity &d, bool records_possible, bool *use_records);
int single_pass_stream_columns(imm3_query *q, uint64_t survivors);
void records_drop_if_narrow(imm3_query *q, uint64_t survivors);
int records_setup(imm3_query *q);
void single_pass_drop_if_narrow(imm3_query *q, uint64_t survivors);
bool single_pass_restore_wanted(const imm3_query *q, uint64_t survivors);
int single_pass_restore(imm3_query *q, uint64_t survivors);

// The select chain's passes as run_select (imm3_run.cpp) enqueues them, from the query's folded predicates and the tuning variant read NOW: tile passes
// of up to kMaxTileCols columns (numeric kinds first, at most one 2-byte string each; a query without predicates is one tile pass
// with zero columns), then one k_filter_pfor pass per fused PFOR_INT predicate, then one k_filter_str_rows pass per string predicate
// on a column whose width is a multiple of 4, then the word-at-a-time passes.
struct SelectChain {
    std::vector<std::vector<const FoldedPred *>> tile_passes;
    std::vector<const FoldedPred *> pfor, str_passes, list_passes, generic; // (list_passes: IMM3_INT_IN, k_filter_int_list, one column per launch)
    bool single_tile_pass = false; // exactly ONE launch in the whole chain: its column order is the records' and the one launch's
};
SelectChain plan_select_chain(const imm3_query *q);
int plan_projection(imm3_query *q); // query creation: the projection's plan (records, one launch, streamed alternative), then the sample

struct LimitScanInputs {
    bool whole = false, count_log_on = false, count_in_scan = false, single_tile_pass = false, table = false, records = false, skip_bitmap = false, overlap_total = false;
    int64_t limit = 0, n_tiles = 0;
    int filter_variant = 0;
};
bool limit_scan_applies(const LimitScanInputs &in);
struct LimitChunks {
    int n = 0;                        // chunks; end[0 .. n) ascending, end[n - 1] == n_tiles
    int64_t end[kLimitMaxChunks] = {}; // the tile a chunk ends before (the next chunk's first tile)
};
LimitChunks limit_chunk_ends(int64_t n_tiles); // a limit scan's chunks over a segment of n_tiles tiles (none for an empty one)

// A projection with a `limit` over a TABLE: one limit-aware launch whose work-groups claim runs of tiles and stop claiming at the
// limit (k_filter_table_limit), or the whole select as before?
struct TableLimitInputs {
    bool table = false, tree = false, count_in_scan = false, single_tile_pass = false, whole = false, count_log_on = false, count_only = false;
    int64_t limit = 0, n_tiles = 0;
    int filter_variant = 0, grid = 0; // grid: work-groups of the launch
};
bool table_limit_applies(const TableLimitInputs &in);

} // namespace imm3
