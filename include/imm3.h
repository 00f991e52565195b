/*
 * imm3.h -- C ABI of the MI355X-native scan / filter / project path of immutable3.
 *
 * This is the drop-in boundary.  The reference (markosski/immutable3) has NO FFI: the path sits
 * behind Scala traits (engine/src/main/scala/immutabledb/engine/operator/Operator.scala:14-28)
 * and three factories wired in Engine.execute (engine/.../engine/Engine.scala:167-173):
 *     ScanOp.mkScanOp(sm, table)        engine/.../operator/Scan.scala:10-15
 *     SelectOp.mkSelectOp(col, cond)    engine/.../operator/Select.scala:5-12
 *     ProjectOp.mkProjectOp(cols,limit) engine/.../operator/Project.scala:8-15
 * The entry points below are what a JNI shim for GpuScanOp / GpuSelectOp / GpuProjectOp binds
 * (INTEGRATION.md shows the Scala + JNI side).  Plain pointers and sizes only; no torch types.
 *
 * Threading: the reference calls the path from a FixedThreadPool(cpuCount), one PipelineThread per segment
 * (Engine.scala:176-180, 247-262; SqlCli.scala:64).  The contract here (csrc/imm3_sync.h; tests/test_gpu_threads.py runs
 * it with 8 threads, tests/test_host_threads.py runs the host pieces under -fsanitize=thread):
 *   - every entry point may be called from any thread; there is no process-wide mutable state except the thread-local
 *     error text;
 *   - a CONTEXT may be used by any number of threads at once (the Scala binding gives every PipelineThread of a device
 *     the same one): its buffer pool, lazily made streams and diagnostics records are guarded inside; the work of all
 *     threads lands on the context's one stream in call order;
 *   - SEGMENTS and TABLES are immutable once created and may be read by any number of queries, threads and contexts of
 *     the same device (a query's context need not be the context that staged its segment);
 *   - ONE imm3_query / imm3_graph / imm3_comm is used by one thread at a time (a PipelineThread owns its iterator
 *     chain), and nothing else may still be inside a call on a handle that is being destroyed;
 *   - a graph capture is exclusive: imm3_ctx_capture_begin ... _end belong to ONE thread, and calls of other threads on
 *     that context wait meanwhile.
 * Worker threads that want their kernels to overlap on the device take one context each (a context = a stream) over the
 * shared segments.
 *
 * Errors: the reference throws Exception(msg) (Scan.scala:49, Select.scala:22,41,80,118,156).
 * Here every call returns an int status (0 = ok) and imm3_last_error() returns the message for
 * the calling thread; a JNI shim turns non-zero into ThrowNew(java/lang/Exception, msg).
 *
 * Citations: core/ = core/src/main/scala/immutabledb, engine/ = engine/src/main/scala/immutabledb.
 */
#ifndef IMM3_H
#define IMM3_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IMM3_ABI_VERSION 1

/* CodecType (core/codec/Codec.scala:21-24), in enumeration order.
 * IMM3_PFOR_INT: blocks as PFORCodecInt.encode writes them (core/codec/PFORCodec.scala:19-31: big-endian words of
 * JavaFastPFOR 0.1.10's IntegratedIntCompressor.compress + 8 zero bytes).  The reference dispatches the codec
 * (Column.scala:61, Scan.scala:37-39) but its decode throws on every block (PFORCodec.scala:43-50); this library
 * decodes the blocks on the GPU (csrc/imm3_codec.hip), a documented departure from the reference's failure. */
enum { IMM3_PFOR_INT = 0, IMM3_DENSE_INT = 1, IMM3_DENSE_TINYINT = 2, IMM3_DENSE_STRING = 3 };

/* EXTENSION (not CodecType values): columns whose blocks are what SnappyCodec.encode writes
 * (core/codec/SnappyCodec.scala:15-43: iq80 snappy 0.4 SnappyOutputStream framing -- "snappy\0", then per <= 32768
 * input bytes a flag, a 2-byte big-endian payload length, the masked CRC-32C of the input, and the stored or
 * raw-Snappy payload).  The reference defines the encoder only: `decode = ???` (SnappyCodec.scala:45), no CodecType
 * names the codec and nothing instantiates it, so a reference table cannot declare such a column; the ids sit outside
 * the enumeration's range on purpose.  Values decode to int32 / int8 / fixed-width strings exactly as the DENSE_*
 * codecs of the same type; blocks are decompressed on the GPU (csrc/imm3_snappy.hip), checksums verified. */
enum { IMM3_SNAPPY_INT = 16, IMM3_SNAPPY_TINYINT = 17, IMM3_SNAPPY_STRING = 18 };

/* SelectCondition (core/Query.scala:3-9) */
enum { IMM3_MATCH = 0, IMM3_NOTMATCH = 1, IMM3_EQ = 2, IMM3_GT = 3, IMM3_LT = 4, IMM3_NOOP = 5 };
/* EXTENSION (not a SelectCondition value): a closed byte-order range on a STRING column, the order ORDER BY sorts by and the string
 * MAX aggregate maximises by -- unsigned, byte-wise, from the first byte.  A leaf with this cond has n_match == 2: match_bytes holds
 * `lo` followed by `hi`, match_lens their lengths, each 0 .. width.  It selects the rows whose `width` bytes r satisfy
 * lo' <= r <= hi', where lo' is lo padded to `width` with 0x00 and hi' is hi padded with 0xFF: {lo = "Jo", hi = "Jo"} is the prefix
 * test, {lo = "M", hi = ""} is "from M on", {"", ""} selects every row, lo' > hi' selects none.  No null semantics, no collation.
 * Errors: n_match != 2, null pointers or a bound longer than the column: IMM3_ERR_ARG, the message says which; a leaf on an int32 /
 * int8 column: "Unsupported column vector" iff the segment has >= 1 batch, as for Match on such a column.
 * Every creator that takes `sels` or `leaves` accepts the leaf.  Leaves on one column fold: two ranges to their intersection, a range
 * and a Match to the IN-list's values inside the range (an ordinary Match from there on).  Uniform layouts run a range on a column of
 * 4, 8, ... IMM3_STRING_MAX_WIDTH bytes through a string pass of its own (k_filter_str_range, beside Match's; a table too), any
 * other width, ragged layouts and the generic-only tuning variant through the word-at-a-time kernel; a TABLE refuses a range on
 * those other widths at creation (IMM3_ERR_ARG, a message of its own).
 * OUT OF SCOPE: a select-tree program that has an IMM3_EXPR_OR or an IMM3_EXPR_NOT *and* an IMM3_STR_RANGE leaf is refused at creation
 * with IMM3_ERR_ARG (segment and table alike; not an IMM3_TABLE_TREE_REFUSED refusal: per-segment queries would be refused the same
 * way) -- the normal form would need complemented ranges and ranges with exclusions. */
enum { IMM3_STR_RANGE = 6 };
/* EXTENSION (not a SelectCondition value): an IN-list on an int32 or int8 column -- `id in (3, 17, 4096)`.  A leaf with this cond
 * carries n_match values in match_bytes, each a 4-byte little-endian two's-complement int32; match_lens may be NULL and `value` is
 * ignored.  It selects the rows whose value is a member of the list.  Membership is exact on integers: there is no d.toByte /
 * d.toInt narrowing, and on an int8 column a value outside -128 .. 127 is no member of anything and is dropped, the way a Match value
 * of the wrong length is.  Duplicates count once; n_match == 0 selects no row.  n_match runs up to IMM3_INT_IN_MAX_VALUES (2^24: the
 * probe table of such a list has 2^25 four-byte slots, 128 MiB of device memory per query).
 * Errors: a negative count, a null match_bytes with n_match > 0, or a count above the cap: IMM3_ERR_ARG, the message says which; a
 * leaf on a STRING column: "Unsupported column vector" iff the segment has >= 1 batch.  IMM3_MATCH on an int column keeps its error.
 * Every creator that takes `sels` or `leaves` accepts the leaf.  Leaves on one column fold: a list and GT / LT / EQ leaves to the
 * list's values inside the interval, two lists to their intersection; an empty folded list selects nothing.  Uniform layouts and
 * tables run a folded list through a pass of its own (k_filter_int_list, one column per launch: a 256-bit set for int8, the values as
 * kernel arguments up to 8 of them, else an open-addressing table probed from LDS or from device memory); ragged layouts and the
 * generic-only tuning variant test the same set, values or table in the word-at-a-time kernel.
 * OUT OF SCOPE: a select-tree program that has an IMM3_EXPR_OR or an IMM3_EXPR_NOT *and* an IMM3_INT_IN leaf is refused at creation
 * with IMM3_ERR_ARG (segment and table alike; not an IMM3_TABLE_TREE_REFUSED refusal) -- NOT IN and lists inside disjunctions need
 * negated lists and intervals with exclusions in the normal form.  The JNI / Scala binding does not carry the leaf. */
enum { IMM3_INT_IN = 7 };
#define IMM3_INT_IN_MAX_VALUES (1 << 24)
/* EXTENSION (not a SelectCondition value): `id in (sub-query)`, the semi-join -- membership in a device-resident integer set built
 * on the GPU from other queries' selections (imm3_int_set_create, below).  A leaf with this cond has n_match == 1 and match_bytes ==
 * the imm3_int_set * itself (the handle, not bytes it points at); match_lens and `value` are ignored.  It selects the rows of an
 * int32 or int8 column whose value is a member of the set; on an int8 column only the set's values in -128 .. 127 are members
 * (IMM3_INT_IN's rule).  The query RETAINS the set: destroying the set while queries use it is legal.
 * Errors (IMM3_ERR_ARG): n_match != 1, a null handle, a set of another context; a destroyed set: IMM3_ERR_STATE; a leaf on a STRING
 * column: "Unsupported column vector" iff the segment has >= 1 batch.
 * Every creator that takes `sels` or `leaves` accepts the leaf.  GT / LT / EQ leaves on the same column fold to their interval,
 * intersected with the set's [min, max]; an empty intersection, like an empty set, selects nothing.  A column with a set leaf takes NO
 * other IMM3_INT_IN / IMM3_INT_IN_SET leaf (IMM3_ERR_ARG, one fixed message, whatever the sizes: the intersection of two
 * device-resident sets is not built).  The pass that probes it is IMM3_INT_IN's (k_filter_int_list and the word-at-a-time kernels read
 * the set's table, 256-bit set or, up to 8 values, its host copy), so what holds for a list -- the bitmap path, no fused
 * aggregation, `limit` bounding the gather, table launches, graph capture of the consumer's runs -- holds for the set.
 * OUT OF SCOPE: a select-tree program that has an IMM3_EXPR_OR or an IMM3_EXPR_NOT and this leaf is refused at creation (IMM3_ERR_ARG, a
 * fixed message of its own, not an IMM3_TABLE_TREE_REFUSED refusal): NOT IN (sub-query) and the leaf under OR.  Also out of scope:
 * string or multi-column sets, sets shared across contexts or ranks, correlated sub-queries; the JNI / Scala binding does not carry it. */
enum { IMM3_INT_IN_SET = 8 };

/* status codes */
enum {
    IMM3_OK = 0,
    IMM3_ERR_UNSUPPORTED_CONDITION = 1, /* "Unsupported condition: ..."   Select.scala:22            */
    IMM3_ERR_UNSUPPORTED_VECTOR = 2,    /* "Unsupported column vector"    Select.scala:41,80,118,156 */
    IMM3_ERR_NO_CODEC = 3,              /* "No implementation for ..."    Scan.scala:49              */
    IMM3_ERR_LAYOUT = 4,                /* block tables the reference would fault on / mis-join      */
    IMM3_ERR_ARG = 5,                   /* bad handle / index / null pointer                         */
    IMM3_ERR_DEVICE = 6,                /* HIP runtime error (message carries hipGetErrorString)     */
    IMM3_ERR_STATE = 7                  /* result requested before imm3_query_run(); destroyed context */
};

typedef struct imm3_ctx imm3_ctx;         /* device + stream + scratch                                   */
typedef struct imm3_segment imm3_segment; /* one segment's columns resident in HBM (SegmentManager role) */
typedef struct imm3_table imm3_table;     /* all resident segments of one table: scanned by ONE launch    */
typedef struct imm3_query imm3_query;     /* one PipelineThread: ScanOp -> SelectOp* -> ProjectOp        */
typedef struct imm3_graph imm3_graph;     /* a recorded sequence of query runs (hipGraph)                */
typedef struct imm3_int_set imm3_int_set; /* a device-resident set of int32 values built from selections  */

/* One column of one segment as the reference stores it: `<col>_<id>.dat` bytes + the
 * `blockOffset` array of `<col>_<id>.meta` (core/storage/Segment.scala:33-58, 154-181;
 * core/storage/SegmentManager.scala:81-111) + the codec of core/Column.scala:18,57-63. */
typedef struct {
    int32_t codec;                /* IMM3_DENSE_INT / _TINYINT / _STRING / IMM3_PFOR_INT           */
    int32_t width;                /* bytes per value: 4, 1, or dtypeAttrs("size") for strings      */
    const void *dat;              /* host pointer to the (mmap'd) .dat bytes                       */
    uint64_t dat_bytes;
    const int32_t *block_offsets; /* N+1 byte offsets, first 0 (SegmentMeta.blockOffsets)          */
    int32_t n_offsets;
} imm3_column;

/* One SelectOp leaf (engine/.../operator/Select.scala:14-23).  Leaves are applied in array order,
 * which is the order PipelineThread.runOps composes them (Engine.scala:237-245); the AND/OR tag is
 * ignored there, so a flat list of leaves is a CONJUNCTION -- through every entry point that takes `sels`, whatever tree the
 * leaves came from.  A tree whose AND / OR tags are honoured is described by the leaves plus a program: see the select trees
 * below (the _expr entry points). */
typedef struct {
    int32_t column;             /* index into the query's used-column list                           */
    int32_t cond;               /* IMM3_GT / IMM3_LT / IMM3_EQ / IMM3_MATCH / IMM3_STR_RANGE / IMM3_INT_IN / IMM3_INT_IN_SET (others -> error) */
    double value;               /* GT/LT/EQ operand as the Query ADT carries it (core/Query.scala:6-8);
                                   narrowed per column type INSIDE the library: Int column d.toInt,
                                   TinyInt column d.toByte (Select.scala:65,73)                      */
    const uint8_t *match_bytes; /* MATCH: the IN-list values, concatenated; STR_RANGE: lo, then hi; INT_IN: the values; INT_IN_SET: the imm3_int_set * itself */
    const int32_t *match_lens;  /* MATCH: byte length of each value; STR_RANGE: of lo and of hi       */
    int32_t n_match;
} imm3_select;

/* ---- library ---- */
int imm3_abi_version(void);
const char *imm3_last_error(void); /* thread-local; valid until the next failing call on this thread */
int imm3_device_count(int *count);

/* ---- context: device id + stream ---- */
/* stream: a hipStream_t to launch on, or NULL to create one (non-blocking).  NULL is also what HIP calls the legacy
 * default stream, so that stream cannot be named here: a caller that wants its own work ordered with the library's
 * passes a real stream (and enqueues on it), or synchronises through imm3_ctx_sync / imm3_query_sync.
 * Handles may be destroyed in any order: a context outlives, internally, the segments / tables / queries / comms made
 * from it, a segment the tables and queries that read it.  Calls through a handle whose context was destroyed fail
 * with IMM3_ERR_STATE. */
int imm3_ctx_create(int device, void *stream, imm3_ctx **out);
int imm3_ctx_destroy(imm3_ctx *ctx);
int imm3_ctx_sync(imm3_ctx *ctx);
int imm3_ctx_stream(imm3_ctx *ctx, void **stream_out);

/* ---- graphs: the reference's Engine starts one PipelineThread per segment for every query it executes
 * (Engine.scala:176-196); here a host that runs the same set of queries again and again -- the segments of a table, pass
 * after pass -- records their runs once and replays them with ONE call: a hipGraph of every kernel of those runs, which
 * removes the per-launch host cost and the gaps between the kernels.
 *   imm3_ctx_capture_begin(ctx); imm3_query_run(q0); imm3_query_run(q1); ...; imm3_ctx_capture_end(ctx, &g);
 *   imm3_graph_launch(g);   -- asynchronous on the context's stream, like the runs it stands for; results are read
 *                              through the queries as after imm3_query_run
 * Between begin and end the context accepts only imm3_query_run / imm3_query_run_select (nothing executes then: the
 * runs are recorded) -- every other call returns IMM3_ERR_STATE.  A recorded run must not need the host: an unlimited
 * projection has to have rows reserved (imm3_query_reserve_rows), and every recorded query must have run once before (its
 * buffers are allocated on first use).  A PROJECTING query is recorded -- whichever of the two calls -- only once its row arrays
 * exist: after an executed imm3_query_run or a reservation (a query created with a limit has them from creation).  A run that is
 * refused inside a capture leaves its query as it was; imm3_ctx_capture_end then closes the capture as after any other.
 * Between imm3_ctx_capture_end and the first imm3_graph_launch a recorded query describes THE LAST RUN THAT EXECUTED, exactly as if
 * nothing had been recorded: its getters answer for that run (IMM3_ERR_STATE where none has executed).  Every launch then leaves
 * the query as the recorded run would: the getters answer for the recorded run, whatever runs or getters came in between -- except
 * that the groups of an aggregation stay readable behind a replayed imm3_query_run_select once any imm3_query_run has executed.
 * Destroying a recorded query makes the graph stale (launch: IMM3_ERR_STATE, the queries stay as they were); so does anything that
 * moves a recorded query's buffers: imm3_query_reserve_rows, row arrays that a getter had to grow. */
int imm3_ctx_capture_begin(imm3_ctx *ctx);
int imm3_ctx_capture_end(imm3_ctx *ctx, imm3_graph **out);
int imm3_graph_launch(imm3_graph *g);
int imm3_graph_destroy(imm3_graph *g);

/* ---- segment: what SegmentManager.getSegment(id, table, col) hands to ScanOp, for every column
 * of one segment id, staged into HBM once and kept resident (the reference keeps the mmaps for the
 * process lifetime, SegmentManager.scala:22,81-87).  The library owns the device copy; the host
 * buffers may be unmapped after the call returns. ---- */
int imm3_segment_create(imm3_ctx *ctx, const imm3_column *cols, int32_t ncols, imm3_segment **out);
/* same, but `dat` fields are DEVICE pointers that stay owned by the caller (no copy).  Each must be 16-byte aligned and
 * readable for 16 KiB past dat_bytes: the partial last tile of a column is read as a whole tile (1024 rows x width),
 * and the aggregation / gather kernels fetch the aligned dword around a narrow value. */
int imm3_segment_wrap_device(imm3_ctx *ctx, const imm3_column *cols, int32_t ncols, imm3_segment **out);
/* Asynchronous staging: returns as soon as the copies are enqueued on the context's copy stream (never the query stream:
 * staging a segment overlaps queries on the others); the host buffers must stay mapped until imm3_segment_wait()
 * returns (the reference's mmaps live as long as the SegmentManager).  Queries created on the segment order
 * themselves behind the copies by themselves. */
int imm3_segment_create_async(imm3_ctx *ctx, const imm3_column *cols, int32_t ncols, imm3_segment **out);
int imm3_segment_wait(imm3_segment *seg);
int imm3_segment_destroy(imm3_segment *seg);
int imm3_segment_bytes(const imm3_segment *seg, uint64_t *device_bytes);

enum { IMM3_AGG_COUNT = 0, IMM3_AGG_MIN = 1, IMM3_AGG_MAX = 2, IMM3_AGG_SUM = 3, IMM3_AGG_COUNT_DISTINCT = 5 };
/* IMM3_AGG_COUNT_DISTINCT: the number of distinct values of `column` among the group's selected rows -- `select state,
 * count(distinct age) from t group by state`.  (5, not 4: kinds 4 and 9 are what callers and tests feed as "an unknown kind" and stay
 * unknown, the decision IMM3_EXPR_NOT = -4 records.)  All eight aggregation creators take it; up to four may stand in one query,
 * beside any other aggregate.  Columns: int32, int8 and STRING columns of 1 .. 4 bytes -- a value is its raw bytes, and distinct raw
 * bytes are distinct values; a wider string column is refused at creation with IMM3_ERR_ARG.  The figure is EXACT: each such
 * aggregate owns a device-resident open-addressing set of (group slot << 32 | value) entries, the power of two at or above
 * 2 x min(rows, bound on groups x 256^width) and at least 1024 of them (imm3_plan_distinct_capacity, imm3_diag.h), refused with
 * IMM3_ERR_ARG above 2^28 entries.  A run clears the sets, aggregates (always the general kernel form: the fast forms and the fused
 * select decline the kind), then walks the select bitmap once per such aggregate; a recorded run replays all of it.  Over an
 * imm3_table the figure counts over ALL segments.  The getters return it as the aggregate's int64 value (imm3_query_fetch_groups and
 * its ordered form); ORDER BY over groups takes it as an 8-byte key, a group filter as a value leaf -- over a string column too.
 * Counts of distinct values do not add: every imm3_comm_merge_groups* entry point refuses a query that carries the kind.
 * OUT OF SCOPE: values wider than 4 bytes; a getter for the sets themselves, and with it exact merges across queries and ranks; a
 * set in LDS for narrow value domains; the fast aggregation forms carrying the kind; the JNI / Scala binding. */
/* widest STRING column that IMM3_AGG_MAX takes on the GPU path (bytes) */
#define IMM3_STRING_MAX_WIDTH 256
/* widest group key (the sum of the group columns' widths) that the _wide aggregation entry points take (bytes) */
#define IMM3_GROUP_KEY_MAX_WIDTH 256
typedef struct {
    int32_t kind;
    int32_t column;
} imm3_aggregate;

/* ---- table: every segment of one table (SegmentManager.getSegments, SegmentManager.scala:108-111) as ONE scan unit.
 * The reference fans out one PipelineThread per segment (Engine.scala:176-180) and merges on the consumer thread;
 * a README-style table (block 1024 x segment 1000) has ~1 M rows per segment, so 100 M rows are ~98 segments and a
 * per-segment launch sequence is launch-bound.  A table query runs the same fused kernels over a TILE TABLE (per
 * 1024-row tile: valid rows + one pointer per column) that spans all segments: one scan+select launch, one
 * compaction, rows / groups in ascending (segment, row) order -- exactly what Engine.execute returns.
 * Requires every segment to have the uniform layout (all columns cut into the same blocks, every non-final block
 * a multiple of 64 rows); otherwise IMM3_ERR_LAYOUT and the caller falls back to per-segment queries.
 * The segments stay owned by the caller and must outlive the table. ---- */
int imm3_table_create(imm3_ctx *ctx, const imm3_segment *const *segs, int32_t n_segs, imm3_table **out);
int imm3_table_destroy(imm3_table *t);
/* Table flavours of imm3_query_create / imm3_query_create_agg (same arguments, `seg` replaced by `table`).
 * Layout getters cover all segments in order (batches of segment 0, then segment 1, ...; oid restarts per segment);
 * imm3_query_segment_starts gives, per segment, its first batch and its first word in the bitmap.
 * `limit` > 0 STOPS THE SCAN of a table projection too (Project.scala:73-80; Engine.scala:166,253-258: the workers of the segments
 * behind the limit stall on the full queue): when the select is one tile launch over a table of more tiles than that launch's
 * work-groups claim at once, the work-groups take runs of 32 virtual tiles in ascending order and stop once the finished runs
 * hold `limit` rows.  The getters then answer exactly as behind a segment's stopped scan: imm3_query_row_count and
 * imm3_query_fetch_rows give the first `limit` survivors in (segment, row) order; imm3_query_count, imm3_query_bitmap,
 * imm3_query_join_count and a count log give the WHOLE table's figures (the whole select runs first; a logged query never stops);
 * imm3_query_segment_starts and imm3_query_locate_rows are unchanged.  Behind imm3_query_run the device-side bitmap and count
 * (imm3_query_device_ptr 0, 1) cover the scanned prefix only.  A select tree with an IMM3_EXPR_OR or IMM3_EXPR_NOT scans the whole table.
 * PREDICATES A TABLE TAKES: GT / LT / EQ on int32 and int8 columns; Match on a 2-byte string column with at most 8 IN-list values
 * (the tile kernel); Match on a string column whose width is a multiple of 4, 4 .. IMM3_STRING_MAX_WIDTH bytes, with an IN-list of
 * any length (one more launch per such column over the tile table, ANDed into the bitmap; a query with one takes the bitmap plan:
 * offsets scan then gather, no stop at a `limit`, an aggregation reads the bitmap).  STILL REFUSED, at creation, with IMM3_ERR_ARG
 * and a message that says so: Match on a string column of any other width (1, 3, 5, ...) and on a 2-byte column with more than 8
 * values -- a table has no word-at-a-time kernel; the caller runs per-segment queries. */
int imm3_query_create_table(imm3_ctx *ctx, const imm3_table *table,
                            const int32_t *used_cols, int32_t n_used,
                            const imm3_select *sels, int32_t n_sels,
                            const int32_t *proj, int32_t n_proj, int64_t limit,
                            int32_t table_block_size, imm3_query **out);
int imm3_query_create_table_agg(imm3_ctx *ctx, const imm3_table *table,
                                const int32_t *used_cols, int32_t n_used,
                                const imm3_select *sels, int32_t n_sels,
                                const int32_t *group_cols, int32_t n_group,
                                const imm3_aggregate *aggs, int32_t n_aggs,
                                int32_t table_block_size, imm3_query **out);
/* n_segments + 1 entries each (last = totals); any pointer may be NULL */
int imm3_query_segment_starts(const imm3_query *q, int32_t *n_segments, int32_t *first_batch, int64_t *first_word);
/* Row indices of a TABLE query are virtual (tile * 1024 + position); this maps them to (segment, row in segment). */
int imm3_query_locate_rows(const imm3_query *q, const uint32_t *row_index, uint64_t n, uint32_t *segment_out, uint32_t *row_out);

/* ---- query: one PipelineThread (Engine.scala:235-262) over one segment ----
 *   used_cols   indices into the segment's columns, in Engine.getColumns order (Engine.scala:85-106);
 *               the FIRST one defines the batches (Scan.scala:55,72)
 *   sels        SelectOp leaves in application order (may be empty: NoSelect)
 *   proj        indices into used_cols of the SELECT-list columns in SELECT-list order
 *               (Project.scala:55-57); n_proj == 0 -> no ProjectOp (bitmap/count only)
 *   limit       Project limit; <= 0 = unlimited (Project.scala:73-80)
 *   table_block_size  Table.blockSize, only used for oid = vecCounter * blockSize (Scan.scala:60)
 * Validation mirrors the reference: NotMatch/NoOp always fail (SelectOp.iterator, Select.scala:22);
 * a condition on the wrong vector type or an unknown codec fails iff the segment has >= 1 batch. */
int imm3_query_create(imm3_ctx *ctx, const imm3_segment *seg,
                      const int32_t *used_cols, int32_t n_used,
                      const imm3_select *sels, int32_t n_sels,
                      const int32_t *proj, int32_t n_proj, int64_t limit,
                      int32_t table_block_size, imm3_query **out);
int imm3_query_destroy(imm3_query *q);

/* ---- select trees: a SelectADT (core/Query.scala:11-15: Select | And(l, r) | Or(l, r) | NoSelect) with its tags HONOURED.
 * The reference announces this and does not do it ("TODO: use AND/OR operators", Engine.scala:236,266): its runOps, and
 * every entry point above, execute an Or as an And.  Here the tree is the `leaves` array plus a POSTFIX program of int32:
 *   value >= 0         push leaf `value`
 *   IMM3_EXPR_AND      pop two, push their conjunction
 *   IMM3_EXPR_OR       pop two, push their disjunction
 *   IMM3_EXPR_NOT      pop ONE, push its complement: exactly the rows of the segment (or table) the operand does not select
 * exactly one result must remain; (age < 18 or age > 65) and state = 'CA' is leaves {LT 18, GT 65, Match CA}, program
 * {0, 1, IMM3_EXPR_OR, 2, IMM3_EXPR_AND}.  An empty program (and no leaves) is NoSelect.
 * IMM3_EXPR_NOT is what the reference's query ADT calls NotMatch (core/Query.scala) and its SelectOp throws on (Select.scala:22):
 * NotMatch(values) is written {Match leaf, IMM3_EXPR_NOT}; `state not in ('CA','NY')`, `not (age > 18 and age < 30)` and `id != 7`
 * ({EQ 7, IMM3_EXPR_NOT}) are trees like any other.  There are no null semantics, because the reference has none: Int.MinValue
 * and "\\N" are ordinary values, and the complement of a leaf holds every row the leaf does not.  A LEAF with cond IMM3_NOTMATCH or
 * IMM3_NOOP stays "Unsupported condition", always.  The operator's value is -4 on purpose: -3 has been fed to these entry points
 * as "an unknown operator" since they exist, and stays one.
 * Checks, in this order: the leaves, as imm3_query_create checks its list (NotMatch / NoOp: "Unsupported condition" always; a
 * leaf on the wrong vector type "Unsupported column vector" and an unknown codec "No implementation for ..." iff the segment
 * has >= 1 batch; thresholds narrowed per leaf); then the program -- stack underflow, more than one result, an unknown operator
 * or a leaf index out of range: IMM3_ERR_ARG (an IMM3_EXPR_NOT on an empty stack is a stack underflow).
 * A program with NEITHER IMM3_EXPR_OR NOR IMM3_EXPR_NOT is the flat list of its leaves in program order and takes exactly
 * imm3_query_create's path (same folded predicates, same plan, same kernels).  With either, the library rewrites the tree into a
 * disjunction of TERMS: NOT is pushed down to the leaves first (De Morgan over AND / OR, a double NOT cancels; NOT GT t is the
 * interval up to t, NOT LT t the one from t, NOT EQ t the two intervals around t -- two terms, an empty one dropped -- and NOT Match
 * a NEGATED IN-list, the values of the column's width as exclusions), then AND distributes over OR.  Each term is a conjunction
 * with at most one interval / IN-list / exclusion list per column (on one column IN and NOT-IN fold to the IN-list minus the
 * exclusions, two NOT-INs to the union of their exclusions; terms that select nothing and duplicates are dropped; a predicate
 * every value passes leaves its term).  A tree whose normal form is the one term WITHOUT any predicate -- `x or not x`, NOT GT
 * 1e12, NOT Match of values of the wrong length only -- selects every row and runs as the query's NoSelect form: the scan, plan
 * and kernels of a query without select leaves.
 * Any other tree's whole select is ONE launch: up to 8 terms over up to 3 int32 / int8 / 2-byte-string columns (IN-lists and
 * exclusion lists of <= 8 values) of a uniform segment through a tile kernel, anything else -- ragged layouts, other string widths
 * (the dword-multiple widths a flat select list runs through its string kernel included: a tree keeps the row-per-lane form for
 * them), longer IN-lists, more columns, 9 .. 64 terms -- through a row-per-lane kernel; more than 64 terms: IMM3_ERR_ARG.
 * PFOR_INT / snappy predicate columns are read in their decoded form.  The projection goes scan -> offsets scan -> gather (imm3_query_plan reports no one launch and no
 * records; `limit` bounds the rows emitted, the select covers the whole segment); an aggregation reads the bitmap the select
 * launch wrote.  Every run call, getter, imm3_query_log_counts and graph capture works as for any query.
 * An imm3_table takes a tree through imm3_query_create_table_expr / _table_agg_expr below. ---- */
enum { IMM3_EXPR_AND = -1, IMM3_EXPR_OR = -2, IMM3_EXPR_NOT = -4 };
int imm3_query_create_expr(imm3_ctx *ctx, const imm3_segment *seg,
                           const int32_t *used_cols, int32_t n_used,
                           const imm3_select *leaves, int32_t n_leaves, const int32_t *prog, int32_t n_prog,
                           const int32_t *proj, int32_t n_proj, int64_t limit,
                           int32_t table_block_size, imm3_query **out);
/* Group-by aggregation under a select tree: the arguments of imm3_query_create_agg_wide (group keys of 0 ..
 * IMM3_GROUP_KEY_MAX_WIDTH bytes; a key of <= 8 bytes behaves as through imm3_query_create_agg) with the tree in place of `sels`. */
int imm3_query_create_agg_expr(imm3_ctx *ctx, const imm3_segment *seg,
                               const int32_t *used_cols, int32_t n_used,
                               const imm3_select *leaves, int32_t n_leaves, const int32_t *prog, int32_t n_prog,
                               const int32_t *group_cols, int32_t n_group,
                               const imm3_aggregate *aggs, int32_t n_aggs,
                               int32_t table_block_size, imm3_query **out);

/* Select trees over an imm3_table: the arguments of imm3_query_create_expr / imm3_query_create_agg_expr with `seg` replaced by
 * `table` (the aggregation takes wide keys, as _agg_expr does).  Checks, in this order: the leaves, exactly as
 * imm3_query_create_table checks its list (every leaf, whether or not the program mentions it; the vector-type and codec checks
 * that need a batch included); then the program, with imm3_query_create_expr's errors.
 * A program with neither IMM3_EXPR_OR nor IMM3_EXPR_NOT takes exactly the path of imm3_query_create_table / _table_agg_wide: same
 * imm3_query_plan, same kernels, same results.  With either, the tree is normalised as for a segment (a tree that selects every
 * row: the table's NoSelect form) and must fit the tile form, the rules applied to the normal form AFTER negation -- at most 8 terms
 * (a complemented EQ counts as two), at most 3 predicate columns of int32 / int8 / 2-byte string (at most one of them a string),
 * IN-lists and exclusion lists of at most 8 values (a union of exclusions that grew past 8 included; NOT over a 4-byte string
 * column is "2-byte columns only").  The select over ALL segments is then ONE launch (imm3_query_expr_form reports the tile form,
 * 0).  A tree that does not fit is refused at creation with IMM3_ERR_ARG and a message that names the bound exceeded -- a table
 * has no row-per-lane kernel.  That includes a tree with an IMM3_EXPR_OR over a string column of 4, 8, ... bytes, which
 * imm3_query_create_table's flat list takes: a tree's string predicates are 2-byte columns only -- and the caller runs
 * per-segment tree queries and merges.  Every such refusal's message begins with IMM3_TABLE_TREE_REFUSED (part of the contract):
 * that prefix, not the status alone, tells "this tree does not fit a table" from a genuine argument error, which falling back would only repeat.
 * A tree that normalises to no term selects nothing.  PFOR_INT / snappy predicate columns are read in the
 * decoded form the table holds.  The projection takes the table's bitmap plan (offsets scan, then gather: imm3_query_plan reports
 * no one launch and no records); `limit` bounds the rows emitted, in ascending (segment, row) order.  An aggregation reads the
 * bitmap (never fused).  imm3_query_segment_starts, imm3_query_locate_rows, imm3_query_run_count (a table run always stores its
 * bitmap), imm3_query_log_counts, graph capture and replay and every getter work as for any table query. */
#define IMM3_TABLE_TREE_REFUSED "a select tree over a table takes "
int imm3_query_create_table_expr(imm3_ctx *ctx, const imm3_table *table,
                                 const int32_t *used_cols, int32_t n_used,
                                 const imm3_select *leaves, int32_t n_leaves, const int32_t *prog, int32_t n_prog,
                                 const int32_t *proj, int32_t n_proj, int64_t limit,
                                 int32_t table_block_size, imm3_query **out);
int imm3_query_create_table_agg_expr(imm3_ctx *ctx, const imm3_table *table,
                                     const int32_t *used_cols, int32_t n_used,
                                     const imm3_select *leaves, int32_t n_leaves, const int32_t *prog, int32_t n_prog,
                                     const int32_t *group_cols, int32_t n_group,
                                     const imm3_aggregate *aggs, int32_t n_aggs,
                                     int32_t table_block_size, imm3_query **out);

/* ---- group-by aggregation: ProjectAggOp (engine/.../operator/ProjectAggregate.scala:115-227) over the rows the
 * SelectOps keep.  CountAggr / MinDoubleAggr / MaxDoubleAggr / MaxStringAggr (:22-112), and the sum that AvgDoubleAggr
 * (:60-75) divides by its counter (the group's count).
 *   group_cols  indices into used_cols, in the order their values are joined into the group key (the reference
 *               joins them in batch-column order with "_", :151-156); total width <= 8 bytes on this path
 *   aggs        {kind, column (index into used_cols)}; MIN/MAX/SUM on INT/TINYINT (PFOR_INT included), MAX on STRING
 *               (1 .. IMM3_STRING_MAX_WIDTH bytes; wider: IMM3_ERR_ARG), COUNT on any.  MIN or SUM on a STRING column: IMM3_ERR_UNSUPPORTED_VECTOR "bad aggregator for
 *               this data type" iff the segment has >= 1 batch (:205-214)
 * Groups come back in first-seen order (the reference's LinkedHashMap order): ascending first selected row. ---- */
int imm3_query_create_agg(imm3_ctx *ctx, const imm3_segment *seg,
                          const int32_t *used_cols, int32_t n_used,
                          const imm3_select *sels, int32_t n_sels,
                          const int32_t *group_cols, int32_t n_group,
                          const imm3_aggregate *aggs, int32_t n_aggs,
                          int32_t table_block_size, imm3_query **out);
/* The same with group keys of 0 .. IMM3_GROUP_KEY_MAX_WIDTH bytes (still at most 4 group columns; wider: IMM3_ERR_ARG).  The
 * arguments are those of imm3_query_create_agg / imm3_query_create_table_agg.  A key of <= 8 bytes takes exactly the path of those
 * (validation, plan, kernels, results).  A wider key is compared byte for byte on the device; imm3_query_fetch_groups then gives
 * its first 8 bytes and imm3_query_fetch_group_keys the whole key.  The merges refuse a query with such a key; see
 * imm3_comm_merge_groups_wide. */
int imm3_query_create_agg_wide(imm3_ctx *ctx, const imm3_segment *seg,
                               const int32_t *used_cols, int32_t n_used,
                               const imm3_select *sels, int32_t n_sels,
                               const int32_t *group_cols, int32_t n_group,
                               const imm3_aggregate *aggs, int32_t n_aggs,
                               int32_t table_block_size, imm3_query **out);
int imm3_query_create_table_agg_wide(imm3_ctx *ctx, const imm3_table *table,
                                     const int32_t *used_cols, int32_t n_used,
                                     const imm3_select *sels, int32_t n_sels,
                                     const int32_t *group_cols, int32_t n_group,
                                     const imm3_aggregate *aggs, int32_t n_aggs,
                                     int32_t table_block_size, imm3_query **out);
int imm3_query_group_count(imm3_query *q, uint32_t *n_groups);
/* The shape of an aggregation query's result rows: group columns, aggregates (the stride of `vals` in imm3_query_fetch_groups and
 * imm3_comm_merge_groups[_all]), bytes of the packed group key.  A binding sizes its buffers from THIS, not from what its caller
 * believes (IMM3_ERR_ARG for a query that is not an aggregation). */
int imm3_query_agg_shape(const imm3_query *q, int32_t *n_group_cols, int32_t *n_aggs, int32_t *key_bytes);
/* keys: the group columns' raw bytes packed little-endian in group_cols order; first_row: lowest selected row of
 * the group; counts: selected rows of the group; vals[g * n_aggs + j]: COUNT -> the count, MIN/MAX numeric -> the
 * int32 value sign-extended, SUM -> the exact int64 sum of the group's selected values (<= 2^32 rows x 2^31: no
 * overflow), MAX string -> the value's bytes packed big-endian (a column wider than 8 bytes: its FIRST 8 bytes packed
 * big-endian; the whole value comes from imm3_query_fetch_group_strings).  Sorted by first_row -- or, behind imm3_query_set_group_order,
 * in that order and cut to its limit (imm3_query_group_count, _fetch_group_strings and _fetch_group_keys likewise).
 * A group key wider than 8 bytes (the _wide entry points): keys[g] holds its FIRST 8 bytes little-endian -- the same packing as a
 * narrow key's, so distinct groups may share keys[g]; the whole key comes from imm3_query_fetch_group_keys. */
int imm3_query_fetch_groups(imm3_query *q, uint64_t *keys, uint32_t *first_row, uint64_t *counts, int64_t *vals,
                            uint32_t max_groups);
/* The exact value of the string MAX aggregate `agg` (index into aggs) of every group: the column's width in bytes per group
 * (out[g * width .. g * width + width)), the byte-lexicographic maximum (String.compareTo for ASCII).  Groups in the order of
 * imm3_query_fetch_groups; any width, narrow columns included.  IMM3_ERR_ARG when `agg` is out of range or is not a MAX over
 * a STRING column. */
int imm3_query_fetch_group_strings(imm3_query *q, int32_t agg, uint8_t *out, uint32_t max_groups);
/* The packed group key of every group: the group columns' raw bytes in group_cols order, key_bytes (imm3_query_agg_shape) per group
 * (out[g * key_bytes .. g * key_bytes + key_bytes)).  Groups in the order of imm3_query_fetch_groups; any key width, narrow keys
 * included (there: byte for byte the u64 keys, little-endian).  IMM3_ERR_ARG for a query that is not an aggregation,
 * IMM3_ERR_STATE before its first run. */
int imm3_query_fetch_group_keys(imm3_query *q, uint8_t *out, uint32_t max_groups);

/* Pre-size the projected-row buffers so that not even the FIRST imm3_query_run() has to wait for the count.  Without it an
 * unlimited projection sizes them once: a query whose SELECT list is predicate columns only (it runs as ONE launch that
 * writes the rows itself) gets room for every row of the segment; any other one synchronises on its first run to read the
 * count and keeps the arrays (with an eighth of headroom) for every later run -- a steady-state projecting query never
 * synchronises.  A run that outgrows the arrays, reserved or not, is detected when its rows are fetched and emitted again.
 * Called BEHIND a run, the call may move the arrays; the rows of that run stay readable (imm3_query_row_count / _fetch_rows emit
 * them again into the new arrays), device pointers 2 and 16+j fetched before the call are void. */
int imm3_query_reserve_rows(imm3_query *q, uint64_t rows);

/* ---- ORDER BY: the "sort" core/Query.scala:27 announces above ProjectADT ("// add sort") and the reference does not have.
 * Called on a PROJECTING query from any of the four creators (imm3_query_create, _create_expr, _create_table, _create_table_expr),
 * before that query's first run; every later run then orders its projected rows on the device, behind the projection on the
 * context's stream (no host synchronisation beyond the projection's own), and the row getters answer in that order.
 *   keys    1 .. IMM3_ORDER_MAX_KEYS entries, keys[0] most significant; proj = index into the query's SELECT list (`proj` of the
 *           creator), descending != 0 reverses THAT key only.  The key columns' widths sum to at most IMM3_ORDER_KEY_MAX_WIDTH bytes.
 *   limit   > 0: the first `limit` rows of the ordered result (applied AFTER the order); <= 0: every row.
 * Order: lexicographic over the keys.  int32 and int8 columns compare as signed integers (PFOR_INT / snappy columns are projected
 * decoded: the same); STRING columns byte-wise unsigned, first byte most significant (String.compareTo for ASCII: the rule of the
 * string MAX aggregate).  Rows whose keys are ALL equal stay in ascending row order -- (segment, row) of a table, i.e. the virtual
 * row index -- under descending keys too: the result is a pure function of the data, bit-exact from run to run.  No null semantics:
 * Int.MinValue and "\\N" are ordinary values.
 * Getters of an ordered query: imm3_query_row_count = min(survivors, limit); imm3_query_fetch_rows = the ordered rows (row index
 * and every SELECT-list column, permuted together).  imm3_query_count, _bitmap, _join_count, _segment_starts and _locate_rows are
 * untouched: they describe the select, not the order.  The ordered rows live in arrays of their own (imm3_query_device_ptr
 * IMM3_PTR_ORDER_*); ids 2, 3 and 16+j keep meaning the unordered projection.
 * Errors: IMM3_ERR_ARG -- n_keys outside 1 .. 4, a `proj` out of range or repeated, key columns wider than 16 bytes together, a
 * query without a SELECT list or an aggregation, a query that was CREATED with a limit > 0 (a creation-time limit stops the scan
 * -- the reference's unordered Project.scala:73-80 -- and an order over the prefix it happened to emit has no meaning: create the
 * query with limit <= 0 and pass the limit here; the message says so);
 * IMM3_ERR_STATE -- the query has already run.  imm3_query_run of an ordered query inside imm3_ctx_capture_begin .. _end:
 * IMM3_ERR_STATE (graph replay of ordered queries is not supported).
 * Merging the ordered results of several queries -- segments, tables, ranks -- is imm3_comm_merge_ordered.
 * Aggregation results are ordered by imm3_query_set_group_order below.
 * OUT OF SCOPE: order keys outside the SELECT list, graph capture of ordered runs. ---- */
typedef struct { int32_t proj; int32_t descending; } imm3_order_key;   /* proj: index into the query's SELECT list */
#define IMM3_ORDER_MAX_KEYS 4
#define IMM3_ORDER_KEY_MAX_WIDTH 16   /* sum of the key columns' widths, bytes */
int imm3_query_set_order(imm3_query *q, const imm3_order_key *keys, int32_t n_keys, int64_t limit);

/* ---- ORDER BY over groups: `select state, count(id), max(age) from t group by state order by id_count desc limit 10`.
 * Called on an AGGREGATION query from any of the eight aggregation creators (segment or table, flat or _expr, narrow or _wide), before
 * or after runs: nothing in imm3_query_run depends on it (graph capture and replay of aggregation runs are unaffected).  The order is
 * applied on the device when a getter settles the groups; imm3_query_group_count, _fetch_groups, _fetch_group_strings and
 * _fetch_group_keys then answer in that order, cut to `limit`, and copy only those groups to the host.  A run, another call of this
 * function, or a re-collect into grown arrays invalidates the ordered view: the next getter orders again.  With a filter set
 * (imm3_query_set_group_filter below) the view is filter, then order, then limit: the order and the limit apply to the groups kept.
 *   keys   1 .. IMM3_ORDER_MAX_KEYS entries, keys[0] most significant.  kind IMM3_GROUP_ORDER_GROUP_COL: index = a place in the
 *           creator's group_cols; kind IMM3_GROUP_ORDER_AGG: index = a place in its aggs.  descending != 0 reverses THAT key only.
 *           n_keys == 0 removes the order: the getters answer in first-seen order again, exactly as on a query never ordered.
 *   limit   > 0: the first `limit` groups of the order (imm3_query_group_count = min(groups, limit)); <= 0: every group.
 * Order: the rule of imm3_query_set_order -- lexicographic over the keys, no null semantics.  int32 / int8 group columns and MIN / MAX
 * over such columns compare as signed integers, COUNT as an unsigned count, SUM as a signed int64, string group columns and string
 * MAX values byte-wise unsigned over their whole width.  Groups whose keys are ALL equal stay in first-seen order (ascending first
 * selected row; a table: the virtual row, i.e. (segment, row)) under descending keys too: the result is a pure function of the data.
 * The keys' normalised widths -- group column: its width; COUNT 5; MIN / MAX on int32 4, on int8 1; SUM 8; string MAX: the column's
 * width -- sum to at most IMM3_GROUP_ORDER_KEY_MAX_WIDTH bytes.
 * imm3_comm_merge_groups* read the group tables and ignore the order.
 * Errors (IMM3_ERR_ARG, the message names the cause): not an aggregation query, n_keys outside 0 .. 4, an unknown kind, an index out
 * of range, the same (kind, index) twice, key bytes above 12 (a 16-byte group column cannot be a key).
 * Merged results are ordered on the device by imm3_comm_merge_groups_view.
 * OUT OF SCOPE: ordering by an average, key bytes beyond 12. ---- */
enum { IMM3_GROUP_ORDER_GROUP_COL = 0, IMM3_GROUP_ORDER_AGG = 1 };
typedef struct { int32_t kind; int32_t index; int32_t descending; } imm3_group_order_key;
#define IMM3_GROUP_ORDER_KEY_MAX_WIDTH 12
int imm3_query_set_group_order(imm3_query *q, const imm3_group_order_key *keys, int32_t n_keys, int64_t limit);

/* ---- HAVING: `select state, count(id), max(age) from t group by state having id_count > 1000 order by id_count desc limit 10`.
 * A predicate over the groups' aggregates, evaluated on the device when a getter settles the groups.  Called on an AGGREGATION query
 * from any of the eight aggregation creators, before or after runs: like the group order, nothing in imm3_query_run depends on it.
 * The view of the groups is FILTER, then ORDER, then LIMIT: with a filter set, imm3_query_group_count, _fetch_groups,
 * _fetch_group_strings and _fetch_group_keys answer over the groups the program keeps -- in the order of imm3_query_set_group_order
 * cut to its limit if one is set (imm3_query_group_count = min(groups kept, limit)), else in first-seen order (ascending first_row),
 * the order the unfiltered getters give -- and copy only the answered groups to the host.  A run, a call of this function or of
 * imm3_query_set_group_order, or a re-collect into grown arrays invalidates the view: the next getter builds it again.
 *   leaves  0 .. IMM3_GROUP_FILTER_MAX_LEAVES.  agg: a place in the creator's aggs, or IMM3_GROUP_FILTER_COUNT: the group's
 *           selected-row count, whether or not a COUNT aggregate exists.  cond: IMM3_GT / IMM3_LT / IMM3_EQ -- strict >, strict <, ==.
 *           value is compared exactly in int64: with a COUNT the count, with MIN / MAX on int32 / int8 the sign-extended value, with
 *           SUM the exact int64 sum.  average != 0 (a SUM aggregate only) compares sum / count as a rational, by
 *           sum <cond> value * count in int64 -- the HAVING on an average; groups have count >= 1, and value must lie in
 *           [-2^31, 2^31 - 1], so that with count < 2^32 the product cannot overflow.
 *   prog    0 .. IMM3_GROUP_FILTER_MAX_PROG entries, postfix over leaf indices with IMM3_EXPR_AND / IMM3_EXPR_OR / IMM3_EXPR_NOT,
 *           checked like a select tree's program (same messages).  n_leaves == 0 && n_prog == 0 removes the filter: the getters then
 *           answer exactly as on a query never filtered.
 * imm3_comm_merge_groups* read the dense group tables and ignore the filter, as they ignore the order.
 * Errors (IMM3_ERR_ARG, the message names the cause): a null query, not an aggregation query, n_leaves outside 0 .. 8, n_prog outside
 * 0 .. 32 or 0 with leaves given, a malformed program, agg out of range, a MAX over a STRING column, average on anything but a SUM or
 * with a value outside [-2^31, 2^31 - 1], an unknown cond.
 * OUT OF SCOPE: leaves on group columns (that is the select's job), leaves on string MAX values, non-integer thresholds, aggregates
 * that are not in the query's aggs, JNI / Scala bindings (merged results are filtered on the device by imm3_comm_merge_groups_view). ---- */
#define IMM3_GROUP_FILTER_MAX_LEAVES 8
#define IMM3_GROUP_FILTER_MAX_PROG   32
#define IMM3_GROUP_FILTER_COUNT      (-1)
typedef struct { int32_t agg; int32_t average; int32_t cond; int64_t value; } imm3_group_filter_leaf;
int imm3_query_set_group_filter(imm3_query *q, const imm3_group_filter_leaf *leaves, int32_t n_leaves, const int32_t *prog, int32_t n_prog);

/* Enqueue the whole pipeline on the context's stream.  n_proj == 0: the scan+select kernel (selection bitmap + count).
 * Unlimited projection whose SELECT list is predicate columns only (one of them an int32 column, or >= 30 % of the rows
 * surviving), one uniform segment: ONE launch -- scan + select +
 * project (csrc/imm3_project.hip: the filter kernel writes the rows in ascending order itself).  Otherwise: scan+select
 * (staging a record per survivor when a predicate column is projected), then an offsets scan and compact+gather -- unless enough rows survive for the other SELECT-list columns to be streamed
 * through that one launch as well (dense int32 columns, from 4 % survivors on; no string predicate): decided from a sample
 * counted at query creation (segments of 4 M rows and more), a reservation, or the first run's count.  Asynchronous except for the first run of an unreserved unlimited projection
 * (see above).  May be called repeatedly on the same query. */
int imm3_query_run(imm3_query *q);
/* Only the ScanOp -> SelectOp* part (selection bitmap + count). */
int imm3_query_run_select(imm3_query *q);
/* ScanOp -> SelectOp* for the count alone: `vec.selected.size` summed over the batches (what a count(*)-style consumer of
 * the pipeline reads, Engine.scala:190-196) without materialising the BitSets.  A select chain that is one fused launch then
 * stores no bitmap at all -- on a narrow column the 1/8 byte per row of bitmap is a fifth of the kernel -- and
 * imm3_query_bitmap fails with IMM3_ERR_STATE until the next full run (of any query: also of an aggregation whose last
 * imm3_query_run fused its select, and behind a projection); any other chain runs as imm3_query_run_select.  "Full run" is
 * imm3_query_run, imm3_query_run_select or a launch of a graph that recorded either. */
int imm3_query_run_count(imm3_query *q);
int imm3_query_sync(imm3_query *q);
/* The selected-row count of a select-only run is reduced on the context's auxiliary stream so that it overlaps the
 * next scan.  Host getters wait for it by themselves; a DEVICE consumer of imm3_query_device_ptr(q, 1) that runs on
 * the context's main stream calls this first: it makes the main stream wait (stream-side, no host block).  After a projection
 * with a `limit` whose scan stopped early (imm3_query_run on a limit query) the count word holds the scanned prefix's count: this
 * call then runs the whole select first, like imm3_query_count and imm3_comm_allreduce_count, so that what the device consumer reads
 * behind it is the segment's count. */
int imm3_query_join_count(imm3_query *q);

/* Device-side log of the selected-row count of every later run of this query: run k (counted from this call) stores its
 * count at device_log[k] while k < capacity, from the kernel that produces the count -- no copy kernel, no host call
 * per run.  For consumers that reduce many runs' counts in one collective (bench.py's count all-reduce over RCCL).
 * device_log = NULL switches the log off. */
int imm3_query_log_counts(imm3_query *q, uint64_t *device_log, uint64_t capacity);

/* ---- results ---- */
/* Batches as ScanOp yields them (FilledColumnVectorBatch, core/DataVector.scala:24-31): */
int imm3_query_layout(const imm3_query *q, int32_t *n_batches, int64_t *total_words, int64_t *n_rows);
/* per batch: size (rows), oid, and the offset of its BitSet words in the batch-major bitmap
 * (ceil(size/64) words per batch; bit i of a batch <-> word i>>6, bit i&63 = mutable.BitSet) */
int imm3_query_batches(const imm3_query *q, int32_t *batch_size, int32_t *batch_oid, int64_t *batch_word_off);
int imm3_query_count(imm3_query *q, uint64_t *selected_rows);               /* sum of selected.size (the whole segment's, also behind a run that stopped at its limit) */
int imm3_query_bitmap(imm3_query *q, uint64_t *words_out, int64_t n_words); /* device -> host copy     */
/* Rows ProjectOp emits for this segment, in emission order (batch order, ascending position): */
int imm3_query_row_count(imm3_query *q, uint64_t *rows);
/* row_index_out: segment-global row number of each emitted row (may be NULL);
 * col_out[j]: packed values of projected column j, width bytes per row (int32 LE / int8 / raw bytes) */
int imm3_query_fetch_rows(imm3_query *q, uint32_t *row_index_out, void *const *col_out, uint64_t max_rows);

/* Device-resident results for callers that stay on the GPU (RCCL count reduce, chained kernels).
 * which: 0 = bitmap (uint64 words), 1 = total count (one uint64), 2 = row indices (uint32),
 *        3 = emitted row count (one uint64), 4 = status word (one uint64), 16+j = projected column j.
 *        Ordered queries (imm3_query_set_order) only -- on any other query these ids are what they always were (an unknown id, or
 *        16+j of a very long SELECT list) --, null before the first run: IMM3_PTR_ORDER_ROW_INDEX (0x1000) = ordered row indices
 *        (uint32), IMM3_PTR_ORDER_ROW_COUNT (0x1001) = ordered row count, min(survivors, limit) (one uint64), IMM3_PTR_ORDER_COLUMN
 *        (0x2000) + j = ordered projected column j; complete behind every imm3_query_run whose unordered rows (2, 16+j) are -- after
 *        a run that outgrew its arrays or gave up on its rows, imm3_query_row_count orders again.
 * What a device-side consumer may rely on behind a run, without any host getter in between:
 *   - bitmap (0), count (1) and emitted row count (3) are exact after EVERY run.  In particular the one-launch projection
 *     (csrc/imm3_project.hip), whose work-groups wait on each other, degrades to "count + bitmap" when such a wait does not
 *     resolve or when another launch of that kernel owns the device: the counts that meet in imm3_comm_allreduce_count
 *     (Engine.scala:190-196) are right whatever happened to the rows;
 *   - row indices (2) and projected columns (16+j) of a one-launch projection are complete only if the status word (4) shows
 *     neither bit 1 (a prefix never came) nor bit 2 (device busy) FOR THAT RUN: bits 8..31 of the word are the run's tag,
 *     (run counter - 1) & 0xFFFFFF with the run counter at count pointer + 8 words.  The host getters (imm3_query_row_count /
 *     _fetch_rows) check this themselves and gather the rows from the bitmap when needed; a consumer that reads the row arrays
 *     on the device calls imm3_query_row_count first (it waits for the run) or checks the word.  Pointers 2 and 16+j change
 *     when the output arrays grow (a reservation that was too small): fetch them again after imm3_query_row_count;
 *   - a query with limit > 0 stops scanning once `limit` rows are selected (ProjectIterator.hasNext, Project.scala:73-80: the
 *     reference never looks at batches behind the limit either): behind imm3_query_run its bitmap (0) and count (1) cover the
 *     scanned prefix of the segment only -- the rows (2, 3, 16+j) are complete.  imm3_query_count, imm3_query_bitmap,
 *     imm3_query_run_select / _run_count, imm3_query_log_counts and imm3_comm_allreduce_count give the whole segment's: the host
 *     getters run the whole select when the last run stopped early;
 *   - the BITMAP (0) is written by imm3_query_run_select always, and by imm3_query_run whenever the plan reads it; two plans do
 *     not: an unlimited projection that goes through survivor records (the records carry the positions; imm3_query_plan out[4])
 *     and an aggregation whose select chain rides in the aggregation launch.  imm3_query_bitmap materialises it on demand (the
 *     select chain runs once more); a DEVICE consumer of pointer 0 calls imm3_query_run_select.  The COUNT (1) is exact behind
 *     every imm3_query_run -- except for such an aggregation, where imm3_query_join_count / imm3_query_count produce it. */
#define IMM3_PTR_ORDER_ROW_INDEX 0x1000
#define IMM3_PTR_ORDER_ROW_COUNT 0x1001
#define IMM3_PTR_ORDER_COLUMN 0x2000
int imm3_query_device_ptr(imm3_query *q, int32_t which, void **ptr);

/* ---- multi-GPU: the count reduce.  Segments shard one per GPU -- segment s belongs to GPU s mod G -- and
 * every GPU runs its own PipelineThreads (Engine.scala:176-180); bitmaps, row lists and oids stay where they were
 * produced.  The ONE exchange is the selected-row count, summed over the GPUs with one 8-byte
 * ncclAllReduce(sum, ncclUint64) over RCCL / xGMI, ordered behind the scans that produce the counts.
 * RCCL is bound at run time (librccl.so.1, or the library the environment variable IMM3_RCCL_LIB names -- the test suite's
 * two-rank loopback transport); a single-GPU host never needs it.  While a communicator of more than one rank is attached to a
 * context, that context's one-launch projections leave one CU per XCD to the collective's kernel.
 *   one process per GPU : rank 0 calls imm3_comm_unique_id, the host hands the 128 bytes to every rank (any channel:
 *                         a file, a socket, a key-value store), every rank calls imm3_comm_create
 *   one process, G GPUs : imm3_comm_create_all over one context per device (the JVM host's shape: one Engine, one
 *                         GpuSegmentManager per device); collectives through imm3_comm_allreduce_count_all ---- */
#define IMM3_COMM_ID_BYTES 128
typedef struct imm3_comm imm3_comm;
int imm3_comm_unique_id(uint8_t *id_out /* IMM3_COMM_ID_BYTES */);
int imm3_comm_create(imm3_ctx *ctx, int32_t world, int32_t rank, const uint8_t *id, imm3_comm **out);
int imm3_comm_create_all(imm3_ctx *const *ctxs, int32_t n, imm3_comm **out /* n handles */);
int imm3_comm_destroy(imm3_comm *c);
int imm3_comm_info(const imm3_comm *c, int32_t *world, int32_t *rank);
/* Streams: a collective runs on the communicator's OWN stream.  It starts after everything enqueued so far on the
 * context's stream, and the context's stream does not wait for it: the next pass's scans overlap the message.
 * imm3_comm_sync blocks the host until the communicator's stream is idle; imm3_comm_join makes the context's stream
 * wait for the last collective (stream side, no host block) -- for a device consumer of the reduced words. */
int imm3_comm_sync(imm3_comm *c);
int imm3_comm_join(imm3_comm *c);
/* In-place sum of n device words over the ranks (asynchronous). */
int imm3_comm_allreduce_u64(imm3_comm *c, uint64_t *device_buf, uint64_t n);
/* The selected-row counts of this rank's queries (each already run on the communicator's context) are summed on the
 * device, then all-reduced over the ranks.  device_out: where the global count lands (a device word; NULL = a word the
 * communicator owns); host_out: if not NULL the call waits and also returns the value to the host. */
int imm3_comm_allreduce_count(imm3_comm *c, imm3_query *const *queries, int32_t n_queries, uint64_t *device_out, uint64_t *host_out);
/* Single-process flavour: comms[i] drives device i with its queries[i][0 .. n_queries[i]); one thread issues all G
 * collectives inside a group.  host_out (may be NULL) receives the global count. */
int imm3_comm_allreduce_count_all(imm3_comm *const *comms, int32_t n_comms, imm3_query *const *const *queries,
                                  const int32_t *n_queries, uint64_t *host_out);

/* ---- multi-GPU: the group-by merge.  ProjectAggregateQueueOp (engine/.../operator/ProjectAggregateQueue.scala:9-55) merges
 * the per-segment group maps by key: counts add, max / min combine, the first arrival keeps its place.  Here every rank
 * brings the aggregation queries of ITS segments (each already run; same group columns and aggregates everywhere, at least
 * one per rank), segment_index[i] = the global index of the segment queries[i] ran on, and every rank receives the merged
 * table in first-seen order -- ascending (segment, first selected row): the reference's arrival order is a race, this is
 * the order Engine.execute would produce with one thread.  Keys of <= 2 bytes travel as element-wise all-reduces of a
 * direct-indexed table (sum on counts, min on segment << 32 | row, max / min on each aggregate); wider keys are merged in a
 * device hash table per rank, exchanged as an ncclAllGather of the ranks' group lists and merged again on the device.  One rank:
 * the same merge over that rank's queries, no collective.
 *   keys / counts / vals as imm3_query_fetch_groups; first[g] = segment << 32 | first selected row of the group there.
 * A query with a MAX over a STRING column wider than 8 bytes, or with a group key wider than 8 bytes (imm3_query_create_agg_wide), is
 * refused (IMM3_ERR_ARG): such maxima and keys are not merged here; see imm3_comm_merge_groups_wide.
 * Synchronous (the merged table is returned to the host). */
int imm3_comm_merge_groups(imm3_comm *c, imm3_query *const *queries, const int32_t *segment_index, int32_t n_queries,
                           uint64_t *keys, uint64_t *first, uint64_t *counts, int64_t *vals, uint32_t max_groups, uint32_t *n_groups);
/* Single-process flavour: comms[i] brings queries[i][0 .. n_queries[i]) with segment_index[i][...]; the tables are merged inside this
 * process.  Only a communicator's CONTEXT is read (no collective runs), so any communicators with one context each do: those of
 * imm3_comm_create_all (one context per device), or a world-of-one communicator per context, several of them on one device included.
 * comms[i]'s queries must have been created on its context.  The same holds for the two _all merges below. */
int imm3_comm_merge_groups_all(imm3_comm *const *comms, int32_t n_comms, imm3_query *const *const *queries,
                               const int32_t *const *segment_index, const int32_t *n_queries,
                               uint64_t *keys, uint64_t *first, uint64_t *counts, int64_t *vals, uint32_t max_groups, uint32_t *n_groups);

/* ---- multi-GPU: the group-by merge by BYTE key.  The same merge for any aggregation query that has been run: a group key of
 * 0 .. IMM3_GROUP_KEY_MAX_WIDTH bytes (narrow or wide entry points), any mix of COUNT / MIN / MAX / SUM, MAX over a STRING column of
 * 1 .. IMM3_STRING_MAX_WIDTH bytes; queries over a segment and over a table may be mixed.  Every (query, group) becomes one record
 * on the device, the records are merged in a hash table keyed by the key's bytes, and with more than one rank the ranks' merged
 * lists are exchanged with ncclAllGather and merged again.
 *   key_bytes_out[g * key_bytes ..) the whole packed key as imm3_query_fetch_group_keys lays it out (key_bytes from
 *                                   imm3_query_agg_shape; a key of <= 8 bytes: the u64 key little-endian)
 *   first[g]                        segment << 32 | first selected row of the group there.  A query over a TABLE brings ONE
 *                                   segment_index entry for the whole table, and a group it brings carries that index << 32 | the
 *                                   group's first VIRTUAL row of the table (tile * 1024 + position, what imm3_query_fetch_groups
 *                                   gives; imm3_query_locate_rows on that query maps it to (segment, row)): the table's groups
 *                                   keep their (segment, row) order among themselves and sort against other queries' groups by
 *                                   the table's one index
 *   counts[g], vals[g * n_aggs + j] as imm3_query_fetch_groups (a string MAX wider than 8 bytes: its first 8 bytes big-endian)
 *   str_out                         NULL, or n_aggs pointers: str_out[j] receives `width` bytes per group when aggregate j is a MAX
 *                                   over a STRING column (any width) and must be NULL for every other aggregate
 * Any output pointer may be NULL.  *n_groups is the total even when max_groups is smaller; max_groups groups are written, in
 * ascending `first` (segment, then first row) -- the order of imm3_comm_merge_groups, whose result this equals for queries that one
 * accepts.  Counts and SUM add, numeric MIN / MAX combine as signed int64, a string MAX is the byte-lexicographic maximum over the
 * whole width.  IMM3_ERR_ARG: a null query, one that is not an aggregation, queries (of this rank or of different ranks) that differ
 * in key_bytes, in the number or kind of their aggregates or in the width of a string MAX column, a non-NULL str_out[j] for another
 * aggregate; IMM3_ERR_STATE: a query that has not been run.  All of these are found before the first collective and reach every
 * rank: no rank is left waiting.  At most 2^30 groups enter a merge.  Synchronous. */
int imm3_comm_merge_groups_wide(imm3_comm *c, imm3_query *const *queries, const int32_t *segment_index, int32_t n_queries,
                                uint8_t *key_bytes_out, uint64_t *first, uint64_t *counts, int64_t *vals,
                                uint8_t *const *str_out, uint32_t max_groups, uint32_t *n_groups);
/* Single-process flavour (communicators as for imm3_comm_merge_groups_all): per communicator the one-rank merge on its context, then
 * one merge by byte key inside this process. */
int imm3_comm_merge_groups_wide_all(imm3_comm *const *comms, int32_t n_comms, imm3_query *const *const *queries,
                                    const int32_t *const *segment_index, const int32_t *n_queries,
                                    uint8_t *key_bytes_out, uint64_t *first, uint64_t *counts, int64_t *vals,
                                    uint8_t *const *str_out, uint32_t max_groups, uint32_t *n_groups);

/* ---- multi-GPU: a VIEW of the merged groups ("Views of merged groups"):
 * `select count(id) from t group by name having id_count > 1000 order by id_count desc limit 10` when several queries -- segments
 * sharded over ranks, several contexts, a table mixed with segments -- bring the groups.  The merge of imm3_comm_merge_groups_wide,
 * unchanged, then FILTER, then ORDER, then LIMIT over its merged list on the device: only the groups of the view cross to the host.
 * Queries, segment_index, the output arrays and their packing are imm3_comm_merge_groups_wide's.
 *   view->order    0 .. IMM3_ORDER_MAX_KEYS keys under the rule of imm3_query_set_group_order (kinds, normal form, user bytes <=
 *                  IMM3_GROUP_ORDER_KEY_MAX_WIDTH; an average is no key), checked against queries[0]'s shape.  n_order == 0: first-arrival
 *                  order, ascending `first`.  A COUNT key stays 5 bytes: merged counts of 2^40 or more are outside the contract.
 *   view->leaves / prog   the rule of imm3_query_set_group_filter; n_prog == 0: every group is kept.  Leaves compare in 128 bits, so an
 *                  `average` leaf (sum <cond> value * count) is exact for merged counts of 2^32 and more.
 *   view->limit    > 0: the first `limit` groups of the order (of first arrival without one); <= 0: none.  Every value is accepted.
 *   *n_groups      min(groups kept, limit): the groups of the view, reported even when max_groups is smaller; max_groups of them are written
 *   *n_kept        (may be NULL) the groups the filter kept, before the limit
 * TIES: groups whose user keys are all equal come in ascending `first` (segment << 32 | first row), the arrival order of the merge.
 * The order's key is 16 bytes, so the tie takes 4 bytes of row plus S bytes of segment, S = the bytes the largest segment_index entry
 * of ANY rank needs (0 when it is 0, 1 up to 255, 2 up to 65535, 3, 4).  A view with user bytes + 4 + S > 16, or with more than 2^30
 * merged groups, is REFUSED: IMM3_ERR_ARG with a message that begins with IMM3_MERGE_VIEW_REFUSED (part of the contract), on every rank
 * in the same call, before any list is exchanged.  A caller that sees the prefix calls imm3_comm_merge_groups_wide and orders on the
 * host.  Any other IMM3_ERR_ARG is an argument error: a null view, a bad key or leaf (the messages of the two setters), the errors of
 * imm3_comm_merge_groups_wide; IMM3_ERR_STATE: a query that has not been run.  All ranks must bring the same view: ranks whose views
 * differ (keys, program, limit) all get IMM3_ERR_ARG "the ranks' views of the merged groups differ ...".  Every such error reaches
 * every rank before the first exchange of lists: no rank is left waiting, and the communicator stays usable.
 * An empty view (no order, no filter, no limit) gives imm3_comm_merge_groups_wide's result byte for byte.  Synchronous.
 * OUT OF SCOPE: ordering by an average, more than 12 user key bytes, views through imm3_comm_merge_groups (this entry accepts every
 * query that one does). ---- */
typedef struct {
    const imm3_group_order_key *order; int32_t n_order;            /* 0: first-arrival order (ascending `first`) */
    const imm3_group_filter_leaf *leaves; int32_t n_leaves;
    const int32_t *prog; int32_t n_prog;                           /* 0: every group is kept */
    int64_t limit;                                                 /* <= 0: none */
} imm3_group_view;
#define IMM3_MERGE_VIEW_REFUSED "a view of merged groups takes "
int imm3_comm_merge_groups_view(imm3_comm *c, imm3_query *const *queries, const int32_t *segment_index, int32_t n_queries,
                                const imm3_group_view *view, uint8_t *key_bytes_out, uint64_t *first, uint64_t *counts, int64_t *vals,
                                uint8_t *const *str_out, uint32_t max_groups, uint32_t *n_groups, uint64_t *n_kept);
/* Single-process flavour (communicators as for imm3_comm_merge_groups_all).  imm3_comm_merge_groups_wide_all finishes its merge on the
 * host, and so does this: the view is computed ON THE HOST, under the same rule (same keys, ties, refusals and results). */
int imm3_comm_merge_groups_view_all(imm3_comm *const *comms, int32_t n_comms, imm3_query *const *const *queries,
                                    const int32_t *const *segment_index, const int32_t *n_queries, const imm3_group_view *view,
                                    uint8_t *key_bytes_out, uint64_t *first, uint64_t *counts, int64_t *vals,
                                    uint8_t *const *str_out, uint32_t max_groups, uint32_t *n_groups, uint64_t *n_kept);

/* ---- multi-GPU: the merge of ORDERED results ("Merging ordered results").  Every rank brings the ordered
 * projecting queries of its own segments (at least one): each has had imm3_query_set_order called and has been run on the
 * communicator's context; all of them, on every rank, have the same SELECT-list shape (number of columns, widths, kinds) and the
 * same order keys (proj and descending, in the same sequence).  Every rank passes the same `limit`.
 *   segment_index   flattened: a query over a segment consumes one entry, its global segment index; a query over an imm3_table
 *                   consumes as many entries as the table has segments, in the table's segment order: the global indices of those
 *                   segments (with s mod G sharding they are not consecutive, and they need not ascend).  All entries of one rank are
 *                   >= 0 and pairwise distinct; distinctness across ranks is the caller's contract and is not checked.
 * Result, the same on every rank: all rows of all queries ordered by (normalised key of imm3_query_set_order, global segment, row in
 * segment), then the first `limit` of them when limit > 0 -- exactly the rows, and the tie order, of ONE ordered imm3_table query over
 * all the segments in global order.
 *   segment_out[i]  the global segment of row i
 *   row_out[i]      the row in that segment (a table query's rows: what imm3_query_locate_rows gives, not the virtual index)
 *   col_out[j]      `width` bytes per row of SELECT-list column j, as imm3_query_fetch_rows packs them
 * Any output pointer may be NULL.  *n_rows is the merged total after the limit even when max_rows is smaller; max_rows rows are written.
 * The limit rule: with limit > 0 every query's own order limit must be <= 0 or >= limit, with limit <= 0 every query's own limit must
 * be <= 0 (a list cut shorter may lack rows the merge needs); a table query whose global indices do not ascend must have no limit
 * of its own (its ties were cut in table order).
 * IMM3_ERR_ARG: a null query, one that is not an ordered projection, queries (of this rank or of different ranks) that differ in
 * SELECT-list shape, order keys or limit, a violated limit rule, a negative or repeated segment index on this rank, more than 2^30
 * rows entering a merge; IMM3_ERR_STATE: a query that has not been run.  All of these are found before the first collective and
 * reach every rank: the failing rank returns its own error, the others "another rank failed"; no rank is left waiting and the
 * communicator stays usable.  Synchronous.  Cost: every record is ranked by binary search in every other list -- made for the top-k
 * case (at most limit rows per list); an unlimited merge of millions of rows is exact but latency-bound. */
int imm3_comm_merge_ordered(imm3_comm *c, imm3_query *const *queries, const int32_t *segment_index, int32_t n_queries,
                            int64_t limit, uint32_t *segment_out, uint32_t *row_out, void *const *col_out,
                            uint64_t max_rows, uint64_t *n_rows);
/* Single-process flavour (communicators as for imm3_comm_merge_groups_all): per communicator the one-rank merge on its context, cut to
 * `limit`, then one merge of their lists inside this process. */
int imm3_comm_merge_ordered_all(imm3_comm *const *comms, int32_t n_comms, imm3_query *const *const *queries,
                                const int32_t *const *segment_index, const int32_t *n_queries,
                                int64_t limit, uint32_t *segment_out, uint32_t *row_out, void *const *col_out,
                                uint64_t max_rows, uint64_t *n_rows);

/* ---- integer sets built on the device from selections: IN (sub-query), the semi-join (csrc/imm3_intset.hip) ----
 * imm3_int_set_create: the set of the DISTINCT values that column columns[i] (an index into that query's used-column list, as
 * imm3_select.column is) takes among the rows sources[i] selects, united over the n_sources sources.  A source is any
 * non-aggregation query of this context (flat, tree, segment or table); its column is int32 or int8 of any codec (PFOR_INT / snappy
 * columns are read decoded, int8 values are sign-extended).  The set is the WHOLE selection's: a source's `limit`, order and SELECT
 * list play no part.  Each source's bitmap is made current first the way imm3_query_bitmap does (a lazy bitmap, a limit scan that
 * stopped early, a count-only last run or a query never run: its select chain runs).  That is a visible effect on the SOURCE: a source
 * whose chain had to run is afterwards in the state imm3_query_run_select leaves -- imm3_query_count / _bitmap answer for the whole
 * selection (a query never run now counts as run; rows a projection emitted before stay what they were), exactly as after the
 * getters imm3_query_bitmap / imm3_query_count settle such a query.  No buffer of the source moves, so a graph that recorded the
 * source's runs stays valid, and replaying it puts the recorded run's state back as always.  Sources are NOT retained and may be
 * destroyed afterwards.  The call synchronises and reads back a small header (count, minimum, maximum, probe bound, overflow flag, the
 * 256-bit set of the values in -128 .. 127); the values stay on the device, with two exceptions: a set of at most 8 values is
 * also copied to the host (it is probed as a short list), and a set that holds BOTH INT32_MIN and INT32_MAX is rebuilt on the host
 * (no sentinel just outside [min, max] is free).  Under an open stream capture it fails with IMM3_ERR_STATE, as every creation does
 * (it allocates, launches and waits); capture the consumers' runs instead.
 * Errors, IMM3_ERR_ARG with the cause in the message: n_sources < 1 or null arrays, a null source, a source of another context, an
 * aggregation source, a column index out of range, more than IMM3_INT_IN_MAX_VALUES distinct values; a string column:
 * IMM3_ERR_UNSUPPORTED_VECTOR ("Unsupported column vector").  "Too many distinct values" is found early: the insert pass keeps a
 * running count and stops every walk once the cap is passed, so the refusal costs about what a build of IMM3_INT_IN_MAX_VALUES values
 * costs, whatever the number of rows.
 * imm3_int_set_destroy drops the caller's reference (queries created with the set keep it alive).
 * imm3_int_set_info: the number of distinct values, their extremes (0, 0 when empty) and the form an int32 consumer probes it in
 * (imm3_diag.h: imm3_plan_int_list_form).  imm3_int_set_values: the values, ascending, each once (a getter: copied from the device and
 * sorted on the host); cap < n_values: IMM3_ERR_ARG. */
int imm3_int_set_create(imm3_ctx *ctx, imm3_query *const *sources, const int32_t *columns, int32_t n_sources, imm3_int_set **out);
int imm3_int_set_destroy(imm3_int_set *s);
int imm3_int_set_info(const imm3_int_set *s, int64_t *n_values, int32_t *min, int32_t *max, int32_t *form);
int imm3_int_set_values(imm3_int_set *s, int32_t *out, int64_t cap);

/* ---- write side of the PFOR_INT codec (host code, no device involved) ----
 * PFORCodecInt.encode (core/codec/PFORCodec.scala:19-31), which SegmentWriter.flush applies to each block of a PFOR_INT
 * column (core/storage/Segment.scala:115-122).  imm3_pfor_encode_block: one block of n_values little-endian int32 ->
 * the bytes appended to the .dat.  imm3_pfor_encode_column: a whole column cut into blocks of block_rows values (the
 * last one shorter); offsets_out receives the n_blocks + 1 byte offsets of the .meta blockOffset table. */
uint64_t imm3_pfor_encode_bound(int32_t n_values);
int imm3_pfor_encode_block(const int32_t *values, int32_t n_values, void *out, uint64_t cap, uint64_t *bytes_out);
int imm3_pfor_encode_column(const int32_t *values, uint64_t n_values, int32_t block_rows, void *out, uint64_t cap,
                            int32_t *offsets_out, uint64_t *bytes_out);

/* Write side of the snappy block format (host code): SnappyCodec.encode of one storage block's raw value bytes. */
uint64_t imm3_snappy_encode_bound(uint64_t n_bytes);
int imm3_snappy_encode_block(const void *bytes, uint64_t n_bytes, void *out, uint64_t cap, uint64_t *bytes_out);

#ifdef __cplusplus
}
#endif
#endif /* IMM3_H */
