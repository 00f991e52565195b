// imm3_api_internal.h -- what imm3_api.cpp (the C ABI: validation, launches, getters) and imm3_planner.cpp (plans and their
// geometry) share.  Internal to libimm3: nothing here is part of include/imm3.h.
#pragma once

#include "imm3_handles.h"

namespace imm3 {

// ---- imm3_api.cpp ----
hipError_t pool_alloc(imm3_ctx *ctx, void **out, size_t bytes);      // the context's caching allocator (stream-ordered reuse)
void pool_release(imm3_ctx *ctx, void *p);
void graphs_mark_stale(imm3_ctx *ctx, const imm3_query *q);          // recorded graphs that replay this query point at buffers that are about to move
void fill_tile_col(const imm3_query *q, const FoldedPred &fp, TileCol &c, int kind);

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
int expr_check_program(const int32_t *prog, int32_t n_prog, int32_t n_leaves, bool *has_or);             // IMM3_ERR_ARG: malformed
int expr_normalize(const std::vector<ExprCol> &leaf_cols, const imm3_select *leaves, int32_t n_leaves, const int32_t *prog, int32_t n_prog,
                   std::vector<ExprTerm> &terms);

// ---- imm3_planner.cpp ----
constexpr int kSampleChunks = 8;                                      // the sample a plan is made on: eight chunks of 64 tiles spread over the segment / table
constexpr int64_t kSampleChunkTiles = 64;
constexpr int kSampleTiles = kSampleChunks * (int)kSampleChunkTiles;
constexpr int64_t kLimitFirstChunkTiles = 1024;                       // a limit scan's first chunk (the next ones are 8 x, 4 x, 4 x ... larger)

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

// The select chain's passes as run_select enqueues them, from the query's folded predicates and the tuning variant read NOW: tile passes
// of up to kMaxTileCols columns (numeric kinds first, at most one 2-byte string each; a query without predicates is one tile pass
// with zero columns), then one k_filter_pfor pass per fused PFOR_INT predicate, then one k_filter_str_rows pass per string predicate
// on a column whose width is a multiple of 4, then the word-at-a-time passes.
struct SelectChain {
    std::vector<std::vector<const FoldedPred *>> tile_passes;
    std::vector<const FoldedPred *> pfor, str_passes, generic;
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

// A projection with a `limit` over a TABLE: one limit-aware launch whose work-groups claim runs of tiles and stop claiming at the
// limit (k_filter_table_limit), or the whole select as before?
struct TableLimitInputs {
    bool table = false, tree = false, count_in_scan = false, single_tile_pass = false, whole = false, count_log_on = false, count_only = false;
    int64_t limit = 0, n_tiles = 0;
    int filter_variant = 0, grid = 0; // grid: work-groups of the launch
};
bool table_limit_applies(const TableLimitInputs &in);

} // namespace imm3
