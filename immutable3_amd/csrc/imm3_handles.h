// imm3_handles.h -- the handle structs behind include/imm3.h, shared by the translation units of the C ABI
// (imm3_api.cpp: creation + getters; imm3_run.cpp: the run and its launches; imm3_planner.cpp: plans; imm3_comm.cpp: the RCCL count reduce; imm3_merge_*.cpp: the cross-rank merges).  Private to csrc/.
#pragma once

#include "../../include/imm3.h"
#include "imm3_internal.h"
#include "imm3_plan.h"
#include "imm3_sync.h"

#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

// ---------------------------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------------------------
namespace imm3 {
int fail(int code, const std::string &msg); // sets the calling thread's imm3_last_error() text (imm3_api.cpp)
}
using imm3::fail;

#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess)                                                                     \
            return fail(IMM3_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e));      \
    } while (0)

// ---------------------------------------------------------------------------------------------
// handles
// ---------------------------------------------------------------------------------------------
struct TimingRecord {
    int32_t kernel_id;
    hipEvent_t start, stop;
};

// Lifetimes.  Every handle is reference counted: the caller's handle holds one reference, and every handle created
// FROM it holds another (segment / table / query / comm -> context; table -> its segments; query -> its segment or
// table).  imm3_*_destroy marks the handle closed and drops the caller's reference; the memory behind it goes when
// the last dependant is destroyed, so handles may be destroyed in ANY order (a JVM finalizer or a Python __del__ run
// by the garbage collector gives no order).  Work submitted through a handle whose context has been destroyed fails
// with IMM3_ERR_STATE; destroying the same handle twice while dependants keep it alive does too.
struct imm3_graph;
struct HipBlockBackend {
    static int alloc(void **p, size_t bytes) { return (int)hipMalloc(p, bytes); }
    static void free(void *p) { (void)hipFree(p); }
};
namespace imm3 {
// Tuning variants (imm3_ctx_set_tuning, include/imm3_diag.h): each pins one decision for A/B runs and tests.  The numbers are the
// interface -- tests and tools/ pass them as integers.  Read where the decision is made (creation or run), so a query created under
// one variant may run under another.
enum TuningVariant : int {
    TV_DEFAULT = 0,
    TV_GENERIC_ONLY = 1,        // every predicate through the word-at-a-time kernel: no tile launch, no PFOR_INT pass, no records / one launch
    TV_COUNT_ON_AUX = 2,        // select-only runs reduce the count on the aux stream (cannot be captured)
    TV_NO_RECORDS = 3,          // no survivor records and no one launch at creation, and the cost model never picks either
    TV_PFOR_DECODED = 5,        // PFOR_INT predicates read the decoded column instead of the compressed blocks
    TV_NO_ONE_LAUNCH = 6,       // projections never take the one launch (nor streamed columns); the cost model keeps survivor records
    TV_COUNT_BY_K_TOTAL = 7,    // the count by a k_total launch: none in the filter kernel or the offsets scan, no count-only instance, no limit chunks
    TV_ONE_LAUNCH_GATHERS = 8,  // the one launch with gathered SELECT-list columns too, and the cost model never leaves it
    TV_STREAM_ALWAYS = 9,       // gathered int32 columns streamed through the one launch whatever the prediction
    TV_NO_SAMPLE = 10,          // no sample and no guess at creation: the plan adapts from the first run's count on
    TV_RECORDS_ALWAYS = 11,     // survivor records even when no predicate column is projected; the cost model drops neither them nor the one launch
    TV_PLAN_PINNED = 12,        // the plan made at creation stands whatever the cost model says (P still adapts); also: no bitmap lines parked in LDS
    TV_COUNT_SMALL_GRID = 13,   // a one-launch select chain reduces its count in the kernel only at <= 512 work-groups
    TV_NO_LIMIT_CHUNKS = 14,    // a `limit` query scans the whole segment in one launch (a table query: the whole table)
    TV_LIMIT_NO_FUSED_GATHER = 15, // a small limit takes k_scan + k_gather instead of k_limit_gather
    TV_NO_CU_RESERVATION = 16,  // one-launch projections use every CU while a communicator is attached
    TV_AGG_SELECT_LAUNCH = 17,  // an aggregation's select chain runs as its own launch, not inside the aggregation launch
    TV_AGG_WEAK_HASH = 18,      // group keys wider than 8 bytes hash to 3 bits: distinct keys collide by construction (tests of the key compare)
    TV_EAGER_BITMAP = 19,       // a projection through survivor records stores its bitmap in the staging launch
    TV_ORDER_FULL_SORT = 23,    // an ordered query with a limit sorts every row: no radix select in front of the sort
    TV_ORDER_SELECT_ALWAYS = 24, // ... takes the radix select whenever the limit is below the survivors (the threshold sweep of tools/order_bench.py)
    TV_GROUP_ORDER_RADIX = 25,  // an ordered aggregation (imm3_query_set_group_order) takes the radix path whatever the group count: no one-work-group launch
    TV_I32_SCAN = 26,           // int32 range predicates scan the column itself: no high-half plane is made or read (A/B runs of the tools)
    TV_TILE_ABLATION = 20,      // 20 .. 22: k_filter_tile's ablation switches (tools' build only)
    TV_EMIT_ABLATION = 34,      // 34 .. 35: k_emit's ablation switches (tools' build only)
    TV_PROJECT_ABLATION = 50,   // 50 + mask (mask <= 255): k_filter_project's ablation mask (tools' build only)
    TV_AGG_FORM = 100,          // 100 + AggForm: the aggregation's form chain starts at that form
    TV_AGG_ABLATION = 140,      // 140 and above: ablation (variant - 100) of the aggregation kernels (tools' build only)
    TV_FIXED_P = 200,           // 200 + P (1 <= P <= kProjectMaxP): the one launch takes P tiles per range, never adapted
};
// the ranges: what the variant passes on to a launch or the planner (0, or -1 for the form, when the variant is not in the range)
inline int tile_ablation(int v) { return v >= TV_TILE_ABLATION && v <= TV_TILE_ABLATION + 2 ? v : 0; }
inline int emit_ablation(int v) { return v >= TV_EMIT_ABLATION && v <= TV_EMIT_ABLATION + 1 ? v : 0; }
inline int project_ablation(int v) { return v >= TV_PROJECT_ABLATION && v <= TV_PROJECT_ABLATION + 255 ? v - TV_PROJECT_ABLATION : 0; }
inline int agg_form_variant(int v) { return v >= TV_AGG_FORM && v <= TV_AGG_FORM + AGG_FORM_GENERAL ? v - TV_AGG_FORM : -1; }
inline int agg_ablation(int v) { return v >= TV_AGG_ABLATION ? v - TV_AGG_FORM : 0; }
inline int fixed_P(int v) { return v > TV_FIXED_P && v <= TV_FIXED_P + kProjectMaxP ? v - TV_FIXED_P : 0; }
} // namespace imm3

// Threading: see imm3_sync.h.  A context may be used by any number of threads at once; `gate` serialises a graph capture
// against the other threads' calls, `mu` guards the small mutable state below, the buffer pool has its own lock.
struct imm3_ctx {
    std::atomic<int> refs{1};
    std::atomic<bool> closed{false}; // imm3_ctx_destroy has run: streams, events and the buffer pool are gone
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    imm3::CaptureGate gate;
    std::mutex mu;                  // guards aux / copy creation, pinned, the timing and stamp records, graphs, d_xpow8
    hipStream_t aux = nullptr;      // count reduce of select-only runs: overlaps the next scan on `stream`
    hipStream_t copy = nullptr;     // host -> HBM staging of segments: never on the query stream, so staging overlaps queries
    std::map<void *, int> pinned;   // host ranges pinned in place for asynchronous staging, by start address, with a use count
    std::atomic<int> filter_variant{0}; // imm3::TuningVariant
    std::atomic<int> grid_blocks{0};
    std::atomic<bool> timing{false};
    std::atomic<uint32_t> timing_mask{0xFFFFFFFFu};
    std::vector<TimingRecord> pool; // pre-created event pairs (mu)
    size_t used = 0;                // (mu)
    imm3::BlockPool<HipBlockBackend> blocks; // per-query device buffers, reused in stream order
    // device-clock stamps (diagnostics): slot i = kMaxFilterGrid {start, end} pairs for the i-th tile launch (mu)
    unsigned long long *d_stamps = nullptr;
    int32_t stamp_slots = 0, stamp_used = 0;
    std::vector<int32_t> stamp_grids;
    uint32_t *d_xpow8 = nullptr;    // snappy CRC-32C check: x^(8 n) mod P for n = 0 .. 32768 (mu)
    imm3_graph *capture = nullptr;  // open stream capture (imm3_ctx_capture_begin .. _end), else null; owned by the capturing thread (gate)
    std::vector<imm3_graph *> graphs; // graphs recorded on this context that have not been destroyed yet (mu)
    // fault injection into k_filter_project (imm3_ctx_inject_fault, imm3_diag.h): read by the tools' build of the kernel only
    std::atomic<int> comms_attached{0}; // communicators created on this context and not yet destroyed: one-launch plans leave CUs for their kernels (imm3_planner.cpp: single_pass_run_grid)
    std::atomic<int> fault_wg{-1}, fault_span{-1};
    std::atomic<uint32_t> fault_max_polls{0};
};

// What a run leaves in the query handle for the getters: which outputs exist and how they have to be settled (imm3_api.cpp: settle).
// Every flag that describes the last run lives here and nowhere else.  A graph keeps the record each recorded query had after its
// (last) recorded run and puts it back whole at every imm3_graph_launch: a replay IS that run again, whatever direct runs, fallbacks
// or getters did to the handle in between.  Counters, diagnostics, stream bookkeeping and the plan are not run results: they stay
// in imm3_query, and a replay does not rewind them.
struct QueryRunState {
    bool ran_select = false, ran_project = false;
    bool bitmap_valid = false;       // the last run stored the selection bitmap (a count-only run does not)
    bool has_pfor_pass = false;      // a k_filter_pfor pass may flag malformed blocks in the status word
    bool count_pending_scan = false; // the last select run left the count to the projection's offsets scan
    bool select_partial = false;     // the last select pass was a limit scan in chunks: the bitmap and the count cover the tiles scanned until
                                     // the limit was reached (finish[kFinishLimitTiles]); imm3_query_count / _bitmap run the whole select first
    bool offsets_valid = false;      // d_tile_offsets / d_chunk_sums describe the last run's bitmap (an offsets scan has run since)
    bool stage_written = false;      // the last select run filled the records
    bool bitmap_lazy = false;        // ... and stored NO bitmap (a records run of imm3_query_run: the records carry the positions, the offsets scan counts them): imm3_query_bitmap runs the select chain then
    bool ran_agg = false;
    bool agg_select_skipped = false; // the last run fused the select into the aggregation launch: bitmap and count do not exist until a getter asks (settle_agg_select)
    bool limit_gather_ran = false;   // the last projection was k_limit_gather's one launch: settle_rows looks at its give-up tag
    bool ran_single_pass = false;    // the last run went through k_filter_project ...
    bool sp_verified = false;        // ... and its status word has been read since (rows complete, or gathered again from the bitmap)
    bool group_order_valid = false;  // an ordered and / or filtered aggregation (imm3_query_set_group_order, _set_group_filter): "the view is current" -- the ordered group arrays hold the view of the last run's groups (a run clears it: run_agg)
    bool rows_moved = false;         // the row arrays were allocated anew behind the last projection (imm3_query_reserve_rows): settle_rows emits its rows again
    bool order_valid = false;        // an ordered query (imm3_query_set_order): the ordered arrays hold the order of the rows as last emitted (every re-emit clears it: launch_project)
};

// A recorded sequence of query runs (hipGraph): launching it enqueues every kernel of those runs with one call.
struct imm3_graph {
    imm3_ctx *ctx = nullptr;              // retained
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    std::vector<imm3_query *> queries;    // the queries whose runs were recorded (not retained: destroying one makes the graph stale)
    std::vector<QueryRunState> states;    // per query: its run state after the recorded run
    std::vector<QueryRunState> live;      // per query: its run state when the capture first admitted it -- nothing executes during a capture, so
                                          // imm3_ctx_capture_end puts it back: until a launch the handle describes the last run that EXECUTED
    bool stale = false;
};

static inline bool is_snappy(int32_t c) { return c == IMM3_SNAPPY_INT || c == IMM3_SNAPPY_TINYINT || c == IMM3_SNAPPY_STRING; }
static inline bool is_compressed(int32_t c) { return c == IMM3_PFOR_INT || is_snappy(c); }
// the DENSE_* codec whose decoded vectors a column's values are (type dispatch of ScanOp / SelectOp / ProjectAggOp)
static inline int32_t value_codec(int32_t c) {
    if (c == IMM3_PFOR_INT || c == IMM3_SNAPPY_INT) return IMM3_DENSE_INT;
    if (c == IMM3_SNAPPY_TINYINT) return IMM3_DENSE_TINYINT;
    if (c == IMM3_SNAPPY_STRING) return IMM3_DENSE_STRING;
    return c;
}

struct SegCol {
    int32_t codec = 0, width = 0;
    int32_t vcodec = 0;                // value_codec(codec)
    uint8_t *d_data = nullptr;
    bool owned = false;
    uint64_t bytes = 0;
    std::vector<int32_t> offsets;
    // PFOR_INT (imm3_codec.hip) / snappy (imm3_snappy.hip): the blocks stay compressed in d_data
    std::vector<int32_t> block_rows;   // the rows each block declares (PFOR: its count word; snappy: uncompressed bytes / width)
    int32_t in_cap = 0, out_cap = 0;   // snappy: LDS bytes k_snappy_decode needs for the largest block / chunk
    int64_t rows = 0;
    bool tile_aligned = false;         // every block but the last holds exactly 1024 rows: block k == bitmap tile k
    uint32_t *d_block_off = nullptr;   // n_blocks + 1 byte offsets
    uint32_t *d_row_base = nullptr;    // n_blocks + 1 first rows
    uint8_t *d_dense = nullptr;        // decoded int32 column, made on first need (Project, aggregation, ragged, table)
    // DENSE_INT: the 16-bit high-half plane, int16[rows] = (int16_t)(v >> 16), made the first time a query's plan wants it
    // (ensure_hi16, imm3_api.cpp; guarded by the segment's decode_mu) and kept for the segment's life.  hi16_state: 0 = not asked
    // yet, 1 = d_hi16 is there, -1 = the column gets none (its halves span fewer than kHi16MinSpan values, or no memory)
    uint8_t *d_hi16 = nullptr;
    int32_t hi16_state = 0;
    int32_t hi16_min = 32767, hi16_max = -32768; // the halves' span as the build reduced it (diagnostics: imm3_segment_hi16_plane)
};

// Batches of one segment as ScanOp yields them (Scan.scala:55,72; Segment.scala:159-168): block k of the FIRST used column holds
// size[k] rows, its BitSet starts at word word_off[k] of the segment's bitmap.  The same for every query whose first used column is
// the same, so it is computed once per (segment, first column) and shared (a 100 M-row segment has 97 657 batches: three vectors
// of that length per query were most of a query's creation time).  oid = k * table.blockSize is the caller's parameter: not stored.
struct SegLayout {
    std::vector<int32_t> size;
    std::vector<int64_t> word_off; // within the segment's own bitmap
    int64_t rows = 0, words = 0;
    bool ragged = false;
};

struct imm3_segment {
    std::atomic<int> refs{1};
    std::atomic<bool> closed{false};
    imm3_ctx *ctx = nullptr;
    std::vector<SegCol> cols;
    uint64_t device_bytes = 0;
    std::vector<void *> registered;    // host ranges pinned in place for an asynchronous create (unpinned by imm3_segment_wait)
    hipEvent_t ready = nullptr;        // recorded on the context's copy stream behind the last column's copy
    std::atomic<bool> ready_pending{false}; // the copies may still be in flight: consumers make their stream wait for `ready`
    std::mutex decode_mu;              // guards the lazy d_dense of PFOR_INT columns and the lazy d_hi16 of DENSE_INT ones
    std::mutex layout_mu;              // guards the two caches below
    std::map<int32_t, std::shared_ptr<const SegLayout>> layouts; // by first used column
    std::map<std::pair<int32_t, int32_t>, bool> same_blocks;     // (first column, other column) -> holds the same rows in the same blocks (checked once)
    // the selectivity sample of query creation (single_pass_sample): a tile table over 8 evenly spaced chunks of 64 full tiles, one
    // pointer array per column (made on first need), so that the sample is ONE launch of the table instance of the scan+select kernel
    std::map<int32_t, void **> d_sample_ptrs; // by column
    uint32_t *d_sample_rows = nullptr;        // kSampleTiles x 1024
    int64_t sample_full_tiles = -1;           // the full tiles the table was laid out for
};

// the flat, fixed-width form of a column (what every kernel but k_filter_pfor reads)
static inline const uint8_t *col_flat(const SegCol &sc) { return is_compressed(sc.codec) ? sc.d_dense : sc.d_data; }

struct imm3_table { // all segments of one table as one scan unit: the tile table
    std::atomic<int> refs{1};
    std::atomic<bool> closed{false};
    imm3_ctx *ctx = nullptr;
    std::vector<const imm3_segment *> segs;
    std::vector<int64_t> seg_rows;     // rows per segment
    std::vector<int64_t> tile_start;   // n_segs + 1: first (virtual) tile of each segment
    int64_t n_tiles = 0, n_rows = 0;
    uint32_t *d_tile_rows = nullptr;   // valid rows per tile
    std::vector<void **> d_tile_ptrs;  // per column: device array of per-tile pointers
    // the sample a query's plan is made on (single_pass_sample, imm3_planner.cpp): eight chunks of 64 tiles spread over the table
    uint32_t *d_sample_rows = nullptr;     // valid rows of the sampled tiles (null: the table is too small to sample)
    std::vector<void **> d_sample_ptrs;    // per column: the sampled tiles' pointers
    // batches of all segments (every column shares one block layout: checked at creation), built once: a query over 98
    // README-style segments otherwise spends ~0.4 ms of host time re-deriving them
    std::vector<int32_t> batch_size, batch_k; // rows; index of the batch within its segment (oid = k * table.blockSize)
    std::vector<int64_t> batch_word_off;
    std::vector<int32_t> seg_first_batch;     // n_segs + 1
    std::vector<int64_t> seg_first_word;      // n_segs + 1
};

// A device-resident integer set (imm3_int_set_create; imm3_int_set_api.cpp builds it, imm3_intset.hip holds the kernels; DESIGN.md
// §3d).  Immutable once created.  Reference counted like every handle: the caller's handle holds one reference, every query created
// with an IMM3_INT_IN_SET leaf on it another.  What it holds is exactly what a folded IMM3_INT_IN list gives the kernels: the probe
// table (IntListTable's fields), the 256-bit set of its values in -128 .. 127, and -- at most kMaxMatch values -- the values themselves.
struct imm3_int_set {
    std::atomic<int> refs{1};
    std::atomic<bool> closed{false};
    imm3_ctx *ctx = nullptr;               // retained
    int64_t n = 0;                         // distinct values
    int32_t min = 0, max = 0;              // their extremes (0, 0 when n == 0)
    int32_t *d_table = nullptr;            // n > 0: int_list_slots(n) slots (pool memory of ctx)
    uint32_t mask = 0, shift = 0, max_probe = 0;
    int32_t empty = 0;
    uint32_t set256[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<int32_t> small;            // n <= kMaxMatch: the values, ascending (such a set is an ordinary short list on the host)
    bool host_route = false;               // diagnostics: the table was built on the host (the set holds INT32_MIN and INT32_MAX)
};

struct FoldedPred { // all SelectOp leaves on one segment column, folded
    int32_t seg_col = 0;
    int32_t kind = 0, width = 0;
    int64_t lo = 0, hi = 0;                // numeric closed interval
    bool has_list = false;                 // numeric: AND a member of `list` (IMM3_INT_IN leaves, folded: imm3_int_list_plan.cpp); never in a program with an OR or a NOT
    std::vector<int32_t> list;             // ... ascending, each value once, all inside [lo, hi] = [its minimum, its maximum]; an empty folded list is lo > hi
    uint32_t list_set[8] = {0, 0, 0, 0, 0, 0, 0, 0};                  // ... int8: the 256-bit membership set (upload_match_blobs)
    uint32_t list_mask = 0, list_shift = 0, list_max_probe = 0;        // ... int32: the probe table at d_blob (IntListTable)
    int32_t list_empty = 0;
    const imm3_int_set *set = nullptr;     // ... an IMM3_INT_IN_SET leaf: the list lives in this shared set (kept alive by imm3_query::sets).  A set of more than kMaxMatch values
                                           // leaves `list` EMPTY: d_blob is the set's table (not owned), the count is the set's (pred_list_count); a smaller one IS `list`
    std::vector<std::string> match;        // string: surviving IN-list values (each exactly width bytes)
    bool negated = false;                  // string, select trees only: `match` are EXCLUSIONS -- every value but these passes (a complemented Match)
    bool has_range = false;                // string: a byte-order range INSTEAD of an IN-list (IMM3_STR_RANGE; `match` is empty, never negated):
    std::string range_lo, range_hi;        // ... the padded bounds, `width` bytes each, lo' <= row <= hi' (imm3_str_range.cpp)
    uint32_t range_lo4[4] = {0, 0, 0, 0}, range_hi4[4] = {0, 0, 0, 0}; // ... their first 16 bytes as the string pass's kernel arguments (str_range_pack)
    uint8_t *d_blob = nullptr;             // device copy when it does not fit the kernel arguments
    bool pfor = false;                     // PFOR_INT column evaluated on its compressed blocks (k_filter_pfor)
    const uint8_t *d_hi16 = nullptr;       // int32 interval: the column's high-half plane as creation found or made it (SegCol::d_hi16), null: none
};
// The predicate no leaf has narrowed yet, for a column of DENSE_* codec `codec`: an int32 / int8 interval every value passes; a
// string's IN-list is the first leaf's.
static inline FoldedPred unfolded_pred(int32_t seg_col, int32_t codec, int32_t width) {
    FoldedPred fp;
    fp.seg_col = seg_col;
    fp.width = width;
    if (codec == IMM3_DENSE_INT) { fp.kind = imm3::KIND_I32; fp.lo = INT32_MIN; fp.hi = INT32_MAX; }
    else if (codec == IMM3_DENSE_TINYINT) { fp.kind = imm3::KIND_I8; fp.lo = -128; fp.hi = 127; }
    else fp.kind = imm3::KIND_STR;
    return fp;
}
// the list lives in a shared set and only there (more than kMaxMatch values: no host copy)
static inline bool pred_list_shared(const FoldedPred &fp) { return fp.set && fp.set->n > (int64_t)imm3::kMaxMatch; }
// the values a numeric predicate's folded list holds, as int_list_form wants them: the set's own count where the list is shared (the
// interval may cut it further: the probe does not mind)
static inline int64_t pred_list_count(const FoldedPred &fp) { return pred_list_shared(fp) ? fp.set->n : (int64_t)fp.list.size(); }
// the folded predicate on segment column `sci` (at most one per column), or null
static inline FoldedPred *pred_on(std::vector<FoldedPred> &preds, int32_t sci) {
    for (auto &p : preds)
        if (p.seg_col == sci) return &p;
    return nullptr;
}

struct imm3_query {
    imm3_ctx *ctx = nullptr;
    const imm3_segment *seg = nullptr;   // the segment (table queries: the first one, for the schema)
    const imm3_table *table = nullptr;   // table query: columns are addressed through the tile table
    int32_t table_block_size = 0;   // table.blockSize as given at creation (oid of a batch = index in its segment * blockSize)
    std::vector<int32_t> used;     // segment column index of each used column
    std::vector<int32_t> proj;     // index into `used`
    int64_t limit = 0;
    // layout (Scan.scala:55-60): shared with every query of the segment that has the same first used column (null: table query)
    std::shared_ptr<const SegLayout> layout;
    int64_t n_rows = 0, n_words = 0, n_tiles = 0, n_chunks = 0;
    bool ragged = false;
    bool always_false = false;
    std::vector<FoldedPred> preds;
    std::vector<imm3_int_set *> sets;   // the sets of this query's IMM3_INT_IN_SET leaves, retained until the query goes
    // device buffers
    uint64_t *d_bitmap = nullptr;
    uint32_t *d_tile_offsets = nullptr, *d_chunk_sums = nullptr, *d_block_partials = nullptr;
    unsigned long long *d_limit_state = nullptr; // k_limit_gather: per-work-group survivor counts, tagged with the run (small limits only)
    unsigned long long *d_total = nullptr, *d_n_emit = nullptr; // adjacent: d_n_emit = d_total + 1; d_total + 2 = status word
    std::vector<unsigned long long> h_init; // host image of the whole finish block at creation (copied asynchronously: lives with the query)
    std::vector<uint32_t> h_word_row_base;  // ragged layouts: host images of the per-word row map (same reason)
    std::vector<uint8_t> h_word_nvalid;
    uint32_t *d_word_row_base = nullptr;
    uint8_t *d_word_nvalid = nullptr;
    uint32_t *d_row_index = nullptr;
    std::vector<uint8_t *> d_proj;
    uint64_t cap_rows = 0;
    bool reserved = false;
    QueryRunState run;             // what the last run left for the getters
    uint32_t run_syncs = 0;        // times imm3_query_run had to wait for the device (diagnostics: imm3_query_plan)
    // group-by aggregation
    bool is_agg = false;
    std::vector<int32_t> group_cols;           // index into `used`
    std::vector<imm3_aggregate> aggs;
    uint32_t agg_mask = 0;
    unsigned long long *d_akeys = nullptr, *d_acounts = nullptr, *d_okeys = nullptr, *d_ocounts = nullptr;
    uint32_t *d_afirst = nullptr, *d_ofirst = nullptr, *d_ameta = nullptr; // d_ameta: {n_groups, overflow}
    long long *d_avals = nullptr, *d_ovals = nullptr;
    // per aggregate that is a string MAX wider than 8 bytes (else null): the refine passes' alive bitmap and chunk table (AggCol)
    uint64_t *d_alive[imm3::kMaxAggs] = {nullptr, nullptr, nullptr, nullptr};
    unsigned long long *d_chunks[imm3::kMaxAggs] = {nullptr, nullptr, nullptr, nullptr};
    // per IMM3_AGG_COUNT_DISTINCT aggregate (else null / 0): its pair set and the set's entries (imm3_distinct_plan.h)
    unsigned long long *d_dset[imm3::kMaxAggs] = {nullptr, nullptr, nullptr, nullptr};
    uint64_t dset_entries[imm3::kMaxAggs] = {0, 0, 0, 0};
    uint32_t out_cap = 0;
    bool agg_wide_key = false;         // group key wider than 8 bytes (the _wide entry points): tables hold tags (AggArgs::wide_key)
    bool agg_fusable = false;          // the select chain is closed intervals over <= 2 dense int8 / int32 columns of one uniform segment (or empty): the aggregation kernel can evaluate it itself
    uint64_t limit_gather_gave_up = 0; // times settle_rows found k_limit_gather's give-up tag and gathered the rows again with k_scan + k_gather
    int32_t agg_first_form = imm3::AGG_FORM_LANES; // first kernel form to try: raised past the forms this query's keys overflowed
    int32_t agg_form_ran = -1;         // diagnostics (imm3_query_agg_form): the AggForm the last aggregation launch ran, -1 before any
    // select-only runs: the count reduce goes to ctx->aux, fenced by these events
    hipEvent_t ev_filter_done = nullptr, ev_total_done = nullptr;
    bool total_on_aux = false;
    // survivor records (k_filter_tile STAGE instances -> k_emit): an unlimited projection over one uniform segment whose
    // select chain is ONE tile launch
    uint8_t *d_stage_rec = nullptr;
    int32_t stage_kinds[imm3::kMaxTileCols] = {imm3::TK_NONE, imm3::TK_NONE, imm3::TK_NONE}; // of the staged launch, in its column order
    int32_t stage_seg_col[imm3::kMaxTileCols] = {-1, -1, -1};                                 // segment column of each
    // the staging launch's geometry (fixed at creation: the arena layout depends on it)
    uint32_t *d_tile_start = nullptr;
    int32_t stage_grid = 0, stage_T = 1, stage_max_slots = 0;
    int64_t stage_wave_cap = 0, stage_main_tiles = 0;
    // single-pass projection (k_filter_project, imm3_project.hip): planned at creation for the same queries as the records
    bool single_pass = false;
    int32_t sp_P = 0, sp_grid = 0;          // tiles per wave per span; work-groups (all resident: they wait on each other)
    int64_t sp_spans = 0;                   // spans of 8 * P tiles
    int32_t sp_P_plan = 0, sp_max_grid = 0; // P as planned without knowing the selectivity (the ceiling of the adapted P); resident work-groups
    int32_t sp_P_plan_for[2] = {0, 0};      // ... for the whole chip / with a CU per XCD left to a communicator's kernels (single_pass_run_grid): the rounds of spans are quantised by the grid
    bool sp_P_fixed = false;                // P was set by the tuning hook: never adapted
    // the alternative plan of a projection with gathered columns: those columns streamed as always-true tile columns
    std::vector<FoldedPred> sp_pass;        // (once switched: part of the single-pass plan)
    bool alt_ok = false;
    int32_t alt_kinds[3] = {3, 3, 3}, alt_seg_col[3] = {-1, -1, -1};
    bool records_narrow_only = false;       // the projected predicate columns are all 1 byte wide (few survivors: the bitmap path beats the records)
    bool sp_narrow_checked = false;         // the first count has been looked at by the cost model ("leave the one launch?")
    imm3::PlanShape plan_shape;             // what the cost model (imm3_plan.h) needs to know of this query
    imm3::PlanDensity plan_density;         // where the survivors are: from the sample at creation (plan_have_density), else a default
    bool plan_have_density = false;
    bool sp_restore_pending = false;        // ... and it does: the next run sets the one launch up again
    uint64_t sp_restore_survivors = 0;
    bool sp_model_dropped = false;          // the cost model took this query off the one launch on an estimate: the first count may bring it back
    bool plan_pinned = false;               // tuning 12 at creation: the plan made there stands whatever the cost model says (tests of one plan's kernels)
    bool sp_have_stats = false;             // a run's count and dense-range tally have been seen (a reservation's estimate no longer moves P)
    size_t sp_rounds_max = 0;               // rounds at the smallest P: d_desc = {round totals, round counters, span descriptors (smallest P), trash lines}
    size_t sp_desc_off = 0;                 // byte offset of the span descriptors in d_desc's allocation
    unsigned long long *d_desc = nullptr;   // per-span descriptors of the chained scan
    size_t sp_trash_off = 0;                // byte offset of the writers' trash lines in d_desc's allocation
    imm3::ProjectTile *d_tile_desc = nullptr; // table queries: one descriptor per tile of the table for the launch's columns (k_filter_project's TABLE instances)
    // select tree (imm3_query_create_expr / _table_expr, an OR or a NOT in it): the selection is the OR of these terms, ONE launch of imm3_expr.hip's
    // tile or generic kernel (a table: the tile kernel's TABLE instance, or the query is refused); q->preds stays empty, the projection takes the bitmap path and an aggregation reads the bitmap
    bool is_expr = false;
    std::vector<std::vector<FoldedPred>> expr_terms;
    bool expr_tile_ok = false;              // the tile form can take the terms (uniform layout, <= 8 terms over <= 3 tile columns of an instantiated kind combination)
    int32_t expr_kinds[imm3::kMaxTileCols] = {imm3::TK_NONE, imm3::TK_NONE, imm3::TK_NONE}; // of the tile launch, sorted
    int32_t expr_seg_col[imm3::kMaxTileCols] = {-1, -1, -1};                                  // segment column of each
    std::vector<imm3::ColPred> h_expr_preds; // generic form: host images of the terms' predicates and their starts (copied asynchronously: live with the query)
    std::vector<int32_t> h_expr_term_start;
    imm3::ColPred *d_expr_preds = nullptr;
    int32_t *d_expr_term_start = nullptr;
    int32_t expr_form_ran = -1;             // diagnostics (imm3_query_expr_form): 0 = tile, 1 = generic, -1 before any launch
    bool hi16_ran = false;                  // diagnostics (imm3_query_plan): a pass of the last select run scanned a high-half plane (TK_H16)
    bool expr_universal = false;            // the tree's normal form is the one term without a predicate: every row -- the query is the NoSelect form (is_expr stays false)
    bool count_log_on = false;              // imm3_query_log_counts is installed: every run logs the segment's count (a limit query then scans whole)
    // ORDER BY (imm3_query_set_order; imm3_order.hip): the projected rows ordered behind every emit, into arrays of their own
    bool ordered = false;
    std::vector<imm3_order_key> order_keys;   // proj: index into `proj`
    int64_t order_limit = 0;                  // <= 0: every row
    int32_t order_key_bytes = 0;
    uint32_t *d_order_keys[2] = {nullptr, nullptr}, *d_order_perm[2] = {nullptr, nullptr}; // ping-pong, sized with the row arrays
    uint32_t *d_order_state = nullptr, *d_order_counts = nullptr, *d_order_diff = nullptr, *d_order_tally = nullptr;
    uint32_t *d_order_row_index = nullptr;
    std::vector<uint8_t *> d_order_proj;
    uint64_t order_cap_rows = 0;              // rows the order's buffers were sized for
    uint64_t order_select_runs = 0, order_full_runs = 0, order_launches = 0, order_counted = 0; // settled ordered runs that took the radix select / sorted every row; times the order was enqueued (imm3_query_plan)
    // ORDER BY over groups (imm3_query_set_group_order; imm3_group_order.hip, imm3_group_order_api.cpp): applied when a getter settles the groups
    bool group_ordered = false;
    std::vector<imm3_group_order_key> group_order_keys;
    int64_t group_order_limit = 0;            // <= 0: every group
    imm3::GroupOrderLayout group_order_layout{};
    imm3::GroupOrderArgs go{};                 // the ordered arrays (dst_*), the gathered wide keys / strings (src_keyb, src_str) and the radix path's key column, as the kernels take them
    uint32_t *d_go_keys[2] = {nullptr, nullptr}, *d_go_perm[2] = {nullptr, nullptr}; // radix path: the order's ping-pong buffers and tables, made on first need
    uint32_t *d_go_state = nullptr, *d_go_counts = nullptr, *d_go_diff = nullptr, *d_go_tally = nullptr;
    std::vector<void *> go_allocs;            // every pool buffer of the group order (released with the query, or when out_cap has grown)
    uint32_t go_cap = 0;                      // groups the buffers were sized for (out_cap then)
    bool go_radix_bufs = false;
    uint32_t go_n_out = 0;                    // groups of the ordered view, min(groups, limit)
    int32_t go_path = 0;                      // diagnostics (imm3_query_group_order_path): the GroupOrderPath of the last ordered settle
    // HAVING (imm3_query_set_group_filter): the view of the groups is filter, then order, then limit; run.group_order_valid says the view is current
    bool group_filtered = false;
    imm3::GroupFilterArgs gf{};               // the checked program; map: the radix path's kept position -> dense index (made with the radix buffers)
    uint64_t gf_groups_in = 0, gf_groups_kept = 0; // diagnostics (imm3_query_group_filter_stats): the last filtered settle's counts
    uint32_t sp_abandoned_runs = 0, sp_busy_runs = 0; // single-pass runs whose rows were gathered from the bitmap instead: a prefix never came / the device was busy (imm3_query_plan)
};


// reference counting (imm3_api.cpp)
namespace imm3 {
void ctx_retain(imm3_ctx *c);
void ctx_release(imm3_ctx *c);
int join_query_count(imm3_query *q); // settle the query's count word for device-side consumers on the context's stream (enqueued, no host wait)
int query_groups(imm3_query *q, uint32_t *n_groups);  // the aggregation's dense group list is complete in q->d_o* (synchronises)
int ensure_order_buffers(imm3_query *q);              // an ordered query's buffers, for the capacity of its row arrays
void query_agg_args(const imm3_query *q, AggArgs &a); // the kernels' view of an aggregation query (launch_group_keys / launch_strmax_collect behind query_groups)
}
