// imm3_int_set_api.cpp -- integer sets built on the device from selections (include/imm3.h: imm3_int_set_create and its getters;
// DESIGN.md §3d): the handle, the order of the device passes (imm3_intset.hip) with the host's decisions between them
// (imm3_int_set_plan.cpp), and the checks of the IMM3_INT_IN_SET leaf that query creation (imm3_api.cpp) calls.
//
// One build: stats over every source (minimum, maximum, selected rows) -> the host picks `empty` and sizes the scratch table T0 ->
// fill + insert over every source -> the host reads the distinct count -> rehash into the final table of int_list_slots(n) slots when
// that is smaller than T0 (else T0 IS the final table), the same pass making the 256-bit set -> T0 back to the pool.  Three small
// header reads; the values never visit the host, but for a set of at most kMaxMatch values (its 16-slot table is read: it is probed as
// a short list) and for a set that holds both INT32_MIN and INT32_MAX (the host route below).
#include "../../include/imm3.h"
#include "../../include/imm3_diag.h"
#include "imm3_internal.h"

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "imm3_handles.h"
#include "imm3_api_internal.h"
#include "imm3_int_set_plan.h"

using namespace imm3;

// ---------------------------------------------------------------------------------------------
// the handle
// ---------------------------------------------------------------------------------------------
static void int_set_free(imm3_int_set *s) {
    if (!s) return;
    imm3_ctx *ctx = s->ctx;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        pool_release(ctx, s->d_table); // (no synchronisation: the pool reuses a block in stream order, as for a query's buffers)
        ctx_release(ctx);
    }
    delete s;
}
imm3_int_set *imm3::int_set_retain(imm3_int_set *s) {
    ref_retain(s->refs);
    return s;
}
void imm3::int_set_release(imm3_int_set *s) {
    if (s && ref_release(s->refs)) int_set_free(s);
}

int imm3::int_set_check_leaf(imm3_ctx *ctx, int32_t n_match, const uint8_t *handle) {
    if (n_match != 1) return fail(IMM3_ERR_ARG, "IntInSet: n_match is " + std::to_string(n_match) + ", an IMM3_INT_IN_SET leaf carries exactly one set (n_match == 1)");
    if (!handle) return fail(IMM3_ERR_ARG, "IntInSet without a set: match_bytes (the imm3_int_set handle) is null");
    const imm3_int_set *s = (const imm3_int_set *)handle;
    if (s->closed) return fail(IMM3_ERR_STATE, "IntInSet: the set has been destroyed");
    if (s->ctx != ctx) return fail(IMM3_ERR_ARG, "IntInSet: the set belongs to another context (sets are not shared across contexts)");
    return IMM3_OK;
}

// ---------------------------------------------------------------------------------------------
// the build
// ---------------------------------------------------------------------------------------------
namespace {

struct SetSource {
    imm3_query *q;
    IntSetSource args;
};

int read_header(imm3_ctx *ctx, const uint32_t *d_header, uint32_t *h) {
    HIPCHK(hipMemcpyAsync(h, d_header, ISH_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return IMM3_OK;
}

IntSetTable table_args(int32_t *slots, uint32_t n_slots, int32_t empty) {
    IntSetTable t;
    t.slots = slots;
    t.mask = n_slots - 1;
    uint32_t log2 = 0;
    while ((1u << log2) < n_slots) ++log2;
    t.shift = 32 - log2;
    t.empty = empty;
    return t;
}

int too_many(int64_t cap) {
    return fail(IMM3_ERR_ARG, "imm3_int_set_create: too many distinct values (more than " + std::to_string(cap) +
                                  (cap == kIntListMaxValues ? ", IMM3_INT_IN_MAX_VALUES)" : ", the cap given)"));
}

// pool blocks of one build that do not outlive it (or do, once handed over: keep())
struct Scratch {
    imm3_ctx *ctx;
    std::vector<void *> blocks;
    explicit Scratch(imm3_ctx *c) : ctx(c) {}
    ~Scratch() { for (void *p : blocks) pool_release(ctx, p); }
    hipError_t alloc(void **p, size_t bytes) {
        const hipError_t e = pool_alloc(ctx, p, bytes);
        if (e == hipSuccess) blocks.push_back(*p);
        return e;
    }
    void release(void *p) {
        blocks.erase(std::remove(blocks.begin(), blocks.end(), p), blocks.end());
        pool_release(ctx, p);
    }
    void keep(void *p) { blocks.erase(std::remove(blocks.begin(), blocks.end(), p), blocks.end()); }
};

int int_set_create_impl(imm3_ctx *ctx, imm3_query *const *sources, const int32_t *columns, int32_t n_sources, int64_t cap, imm3_int_set **out) {
    if (!out) return fail(IMM3_ERR_ARG, "out is null");
    *out = nullptr;
    if (n_sources < 1) return fail(IMM3_ERR_ARG, "imm3_int_set_create: n_sources is " + std::to_string(n_sources) + ", a set needs at least one source");
    if (!sources || !columns) return fail(IMM3_ERR_ARG, "imm3_int_set_create: null sources / columns array");
    if (cap < 1 || cap > kIntListMaxValues) return fail(IMM3_ERR_ARG, "imm3_int_set_create: the value cap is outside 1 .. IMM3_INT_IN_MAX_VALUES");
    CTX_LIVE(ctx); // (refuses an open capture: the build allocates, launches and waits)
    for (int32_t i = 0; i < n_sources; ++i) {
        const imm3_query *q = sources[i];
        const std::string who = "imm3_int_set_create: source " + std::to_string(i);
        if (!q) return fail(IMM3_ERR_ARG, who + " is null");
        if (q->ctx != ctx) return fail(IMM3_ERR_ARG, who + " belongs to another context");
        if (q->is_agg) return fail(IMM3_ERR_ARG, who + " is an aggregation query: a set is built from a selection");
        if (columns[i] < 0 || columns[i] >= (int32_t)q->used.size()) return fail(IMM3_ERR_ARG, who + ": column index " + std::to_string(columns[i]) + " is out of range of its used columns");
        const SegCol &sc = q->seg->cols[(size_t)q->used[(size_t)columns[i]]];
        if (sc.vcodec == IMM3_DENSE_STRING) return fail(IMM3_ERR_UNSUPPORTED_VECTOR, "Unsupported column vector");
        if (!((sc.vcodec == IMM3_DENSE_INT && sc.width == 4) || (sc.vcodec == IMM3_DENSE_TINYINT && sc.width == 1)))
            return fail(IMM3_ERR_ARG, who + ": the column is neither int32 nor int8");
    }
    HIPCHK(hipSetDevice(ctx->device));

    // every source's bitmap current, its column flat; sources without a row take no part
    std::vector<SetSource> srcs;
    for (int32_t i = 0; i < n_sources; ++i) {
        imm3_query *q = sources[i];
        int rc = query_bitmap_current(q);
        if (rc) return rc;
        if (q->n_words <= 0 || q->n_rows <= 0) continue;
        const int32_t sci = q->used[(size_t)columns[i]];
        if (!q->table) { rc = segment_dense_column(ctx, q->seg, sci); if (rc) return rc; }
        const SegCol &sc = q->seg->cols[(size_t)sci];
        SetSource s;
        s.q = q;
        std::memset(&s.args, 0, sizeof(s.args));
        s.args.bitmap = q->d_bitmap;
        s.args.n_words = q->n_words;
        s.args.n_rows = q->n_rows;
        s.args.width = sc.width;
        if (q->table) {
            s.args.tile_ptrs = (const void *const *)q->table->d_tile_ptrs[(size_t)sci];
            s.args.tile_rows = q->table->d_tile_rows;
            if (!s.args.tile_ptrs || !s.args.tile_rows) return fail(IMM3_ERR_ARG, "internal: a table source without its tile table");
        } else {
            s.args.data = col_flat(sc);
            if (!s.args.data) return fail(IMM3_ERR_ARG, "internal: a source column without its flat form");
            if (q->ragged) {
                s.args.word_row_base = q->d_word_row_base;
                s.args.word_nvalid = q->d_word_nvalid;
                if (!s.args.word_row_base || !s.args.word_nvalid) return fail(IMM3_ERR_ARG, "internal: a ragged source without its word map");
            }
        }
        srcs.push_back(s);
    }

    std::unique_ptr<imm3_int_set, void (*)(imm3_int_set *)> set(new imm3_int_set(), int_set_free);
    set->ctx = ctx;
    ctx_retain(ctx);
    set->max_probe = 1;
    Scratch scratch(ctx);
    void *p = nullptr;
    HIPCHK(scratch.alloc(&p, ISH_WORDS * sizeof(uint32_t)));
    uint32_t *d_header = (uint32_t *)p;
    uint32_t h[ISH_WORDS];
    hipStream_t s = ctx->stream;

    // 1. stats
    launch_int_set_init(d_header, s);
    for (const SetSource &src : srcs) {
        launch_int_set_stats(src.args, d_header, s, nullptr, nullptr);
    }
    HIPCHK(hipGetLastError());
    int rc = read_header(ctx, d_header, h);
    if (rc) return rc;
    unsigned long long rows = 0;
    std::memcpy(&rows, h + ISH_ROWS_LO, sizeof(rows));
    int32_t mn, mx;
    std::memcpy(&mn, h + ISH_MIN, sizeof(mn));
    std::memcpy(&mx, h + ISH_MAX, sizeof(mx));
    if (rows == 0 || mn > mx) { // the empty set: no table, no value -- a consumer selects nothing
        *out = set.release();
        return IMM3_OK;
    }

    // 2. the sentinel and the scratch table.  No free int32 just outside [min, max]: the host route -- the device builds the set WITHOUT
    // INT32_MAX (which then is the free sentinel), the host reads that table's values, adds INT32_MAX and builds the final table itself
    int32_t empty = 0;
    const bool host_route = !int_set_pick_empty(mn, mx, &empty);
    if (host_route) empty = INT32_MAX;
    const uint32_t slots0 = int_set_scratch_slots((int64_t)std::min<unsigned long long>(rows, (unsigned long long)INT64_MAX), mn, mx, cap);
    if (slots0 < kIntListMinSlots) return fail(IMM3_ERR_ARG, "internal: no scratch table for these figures");
    HIPCHK(scratch.alloc(&p, (size_t)slots0 * sizeof(int32_t)));
    const IntSetTable t0 = table_args((int32_t *)p, slots0, empty);
    launch_int_set_fill(t0, s);
    for (SetSource &src : srcs) {
        src.args.has_skip = host_route ? 1 : 0;
        src.args.skip = INT32_MAX;
        launch_int_set_insert(src.args, t0, (uint32_t)(cap - (host_route ? 1 : 0)), d_header, s, nullptr, nullptr);
    }
    HIPCHK(hipGetLastError());
    rc = read_header(ctx, d_header, h);
    if (rc) return rc;
    const int64_t n0 = (int64_t)h[ISH_COUNT0];
    if (h[ISH_OVERFLOW] || n0 + (host_route ? 1 : 0) > cap) return too_many(cap); // (a full table: its insert left, nothing hangs; the scratch goes back to the pool)

    if (host_route) {
        std::vector<int32_t> slots((size_t)slots0), values;
        HIPCHK(hipMemcpyAsync(slots.data(), t0.slots, (size_t)slots0 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        int_set_table_values(slots.data(), (int64_t)slots0, empty, true, INT32_MAX, values);
        scratch.release(t0.slots);
        IntListTable t;
        int_list_build_table(values, t);
        HIPCHK(scratch.alloc(&p, t.slots.size() * sizeof(int32_t)));
        HIPCHK(hipMemcpyAsync(p, t.slots.data(), t.slots.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s)); // (the host image goes away with this scope)
        scratch.keep(p);
        set->d_table = (int32_t *)p;
        set->n = (int64_t)values.size();
        set->min = values.front();
        set->max = values.back();
        set->mask = t.mask;
        set->shift = t.shift;
        set->max_probe = t.max_probe;
        set->empty = t.empty;
        set->host_route = true;
        std::vector<int32_t> small8;
        for (int32_t v : values)
            if (v >= -128 && v <= 127) small8.push_back(v);
        int_list_set256(small8, set->set256);
        if (set->n <= (int64_t)kMaxMatch) set->small = values;
        *out = set.release();
        return IMM3_OK;
    }

    // 3. the final table: T0 itself when it already has int_list_slots(n) slots, else one rehash into a table of that size; the same
    // pass makes the 256-bit set
    const uint32_t slots1 = int_list_slots(n0);
    IntSetTable fin = t0;
    IntSetTable to = table_args(nullptr, kIntListMinSlots, empty);
    if (slots1 < slots0) {
        HIPCHK(scratch.alloc(&p, (size_t)slots1 * sizeof(int32_t)));
        to = table_args((int32_t *)p, slots1, empty);
        launch_int_set_fill(to, s);
        fin = to;
    }
    launch_int_set_rehash(t0, to, d_header, s, nullptr, nullptr);
    HIPCHK(hipGetLastError());
    rc = read_header(ctx, d_header, h);
    if (rc) return rc;
    if (to.slots) {
        if (h[ISH_OVERFLOW] || (int64_t)h[ISH_COUNT1] != n0) return fail(IMM3_ERR_DEVICE, "internal: the rehash of an integer set lost values");
        scratch.release(t0.slots);
    }
    set->n = n0;
    set->min = mn;
    set->max = mx;
    set->mask = fin.mask;
    set->shift = fin.shift;
    set->empty = empty;
    set->max_probe = to.slots ? h[ISH_PROBE1] : h[ISH_PROBE0];
    std::memcpy(set->set256, h + ISH_SET256, sizeof(set->set256));
    if (n0 <= (int64_t)kMaxMatch) { // at most 8 values in 16 slots: read them -- on the host such a set is an ordinary short list
        int32_t few[kIntListMinSlots];
        if (fin.mask + 1 != kIntListMinSlots) return fail(IMM3_ERR_DEVICE, "internal: a short set in a long table");
        HIPCHK(hipMemcpyAsync(few, fin.slots, sizeof(few), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        int_set_table_values(few, (int64_t)kIntListMinSlots, empty, false, 0, set->small);
        if ((int64_t)set->small.size() != n0) return fail(IMM3_ERR_DEVICE, "internal: a short set's table does not hold its values");
    }
    scratch.keep(fin.slots);
    set->d_table = fin.slots;
    *out = set.release();
    return IMM3_OK;
}

} // namespace

extern "C" int imm3_int_set_create(imm3_ctx *ctx, imm3_query *const *sources, const int32_t *columns, int32_t n_sources, imm3_int_set **out) {
    return int_set_create_impl(ctx, sources, columns, n_sources, kIntListMaxValues, out);
}

// diagnostics (include/imm3_diag.h): the same build with a lower cap on the distinct values -- the overflow path at a small size
extern "C" int imm3_int_set_create_capped(imm3_ctx *ctx, imm3_query *const *sources, const int32_t *columns, int32_t n_sources, int64_t max_values, imm3_int_set **out) {
    return int_set_create_impl(ctx, sources, columns, n_sources, max_values, out);
}

extern "C" int imm3_int_set_destroy(imm3_int_set *s) {
    if (!s) return IMM3_OK;
    if (s->closed.exchange(true)) return fail(IMM3_ERR_STATE, "integer set destroyed twice");
    int_set_release(s);
    return IMM3_OK;
}

extern "C" int imm3_int_set_info(const imm3_int_set *s, int64_t *n_values, int32_t *min, int32_t *max, int32_t *form) {
    if (!s) return fail(IMM3_ERR_ARG, "set is null");
    if (s->closed) return fail(IMM3_ERR_STATE, "the set has been destroyed");
    if (n_values) *n_values = s->n;
    if (min) *min = s->min;
    if (max) *max = s->max;
    if (form) *form = int_list_form(4, s->n);
    return IMM3_OK;
}

// the table as it stands on the device (diagnostics, and the values' getter)
static int fetch_table(imm3_int_set *s, std::vector<int32_t> &slots) {
    slots.clear();
    if (!s->d_table) return IMM3_OK;
    slots.resize((size_t)s->mask + 1);
    HIPCHK(hipSetDevice(s->ctx->device));
    HIPCHK(hipMemcpyAsync(slots.data(), s->d_table, slots.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s->ctx->stream));
    HIPCHK(hipStreamSynchronize(s->ctx->stream));
    return IMM3_OK;
}

extern "C" int imm3_int_set_values(imm3_int_set *s, int32_t *out, int64_t cap) {
    if (!s) return fail(IMM3_ERR_ARG, "set is null");
    if (s->closed) return fail(IMM3_ERR_STATE, "the set has been destroyed");
    if (cap < s->n || (s->n > 0 && !out)) return fail(IMM3_ERR_ARG, "imm3_int_set_values: out holds fewer than the set's " + std::to_string(s->n) + " values");
    CTX_LIVE(s->ctx);
    std::vector<int32_t> slots, values;
    const int rc = fetch_table(s, slots);
    if (rc) return rc;
    int_set_table_values(slots.data(), (int64_t)slots.size(), s->empty, false, 0, values);
    if ((int64_t)values.size() != s->n) return fail(IMM3_ERR_DEVICE, "internal: the set's table does not hold its values");
    if (s->n) std::memcpy(out, values.data(), values.size() * sizeof(int32_t));
    return IMM3_OK;
}

extern "C" int imm3_int_set_table(imm3_int_set *s, int32_t *slots_out, int64_t cap, int64_t *n_slots, int32_t *empty, int32_t *max_probe, uint32_t *set256, int32_t *host_route) {
    if (!s) return fail(IMM3_ERR_ARG, "set is null");
    if (s->closed) return fail(IMM3_ERR_STATE, "the set has been destroyed");
    if (cap < 0 || (cap > 0 && !slots_out)) return fail(IMM3_ERR_ARG, "bad argument");
    CTX_LIVE(s->ctx);
    const int64_t n = s->d_table ? (int64_t)s->mask + 1 : 0;
    if (n_slots) *n_slots = n;
    if (empty) *empty = s->empty;
    if (max_probe) *max_probe = (int32_t)s->max_probe;
    if (set256) std::memcpy(set256, s->set256, sizeof(s->set256));
    if (host_route) *host_route = s->host_route ? 1 : 0;
    if (cap == 0) return IMM3_OK;
    if (cap < n) return fail(IMM3_ERR_ARG, "slots_out is too small");
    std::vector<int32_t> slots;
    const int rc = fetch_table(s, slots);
    if (rc) return rc;
    if (n) std::memcpy(slots_out, slots.data(), slots.size() * sizeof(int32_t));
    return IMM3_OK;
}
