// imm3_merge_ordered.cpp -- imm3_comm_merge_ordered and its single-process flavour.
//
// Merging ORDERED results ("Merging ordered results").  Every (query, ordered row) becomes one record whose
// first six words are its sort key (imm3_merge_order.h); this rank's lists -- one per query, already in order -- are merged by
// k_merge_order_rank and cut to the limit (the local phase, ordered_local), and with more than one rank those lists are exchanged
// with ncclAllGather -- fixed-size slots, sized by an all-reduce(max) of the list lengths -- and merged by the same kernel
// (ordered_exchange, built from the protocol of imm3_comm_internal.h).
#include "imm3_comm_internal.h"
#include "imm3_merge_order.h"

#include <algorithm>
#include <cstring>

using namespace imm3;

namespace {

MergeOrderSpec order_spec_of(const imm3_query *q) {
    MergeOrderSpec sp;
    for (int32_t p : q->proj) {
        const SegCol &sc = q->seg->cols[(size_t)q->used[(size_t)p]];
        sp.widths.push_back(sc.width);
        sp.kinds.push_back(sc.vcodec == IMM3_DENSE_INT ? KIND_I32 : (sc.vcodec == IMM3_DENSE_TINYINT ? KIND_I8 : KIND_STR));
    }
    for (const imm3_order_key &k : q->order_keys) {
        sp.key_proj.push_back(k.proj);
        sp.key_desc.push_back(k.descending ? 1 : 0);
    }
    return sp;
}

inline unsigned long long even(unsigned long long v) { return (v + 1ULL) & ~1ULL; }

// what the checks learn of this rank's queries, per query
struct OrderedInputs {
    std::vector<int32_t> n_entries; // segment_index entries the query consumes (1, or its table's segments) ...
    std::vector<size_t> entry_at;   // ... from here
    std::vector<uint64_t> n_local;  // its ordered rows
    std::vector<char> split;        // a table query whose global indices are not ascending
    unsigned long long total_local = 0;
};

// what the local phase leaves: the verdicts, the spec, and this rank's merged records cut to the limit -- `mine` of them on the
// device (d_out, in `block`) or, as the final result, in `recs` with their number in `total`
struct OrderedLocal {
    LocalVerdict verdict;
    LocalStep step;
    MergeOrderSpec sp;
    MergeOrderGeometry geo;
    int64_t limit = 0;
    DeviceBlock block;
    const uint32_t *d_out = nullptr;
    unsigned long long mine = 0;
    std::vector<uint32_t> h_meta;            // host images of the device tables: live until the stream has been synchronised
    std::vector<unsigned long long> h_lists;
    std::vector<uint32_t> recs;
    uint64_t total = 0;
    unsigned long long cut_of(unsigned long long n) const { return limit > 0 && (unsigned long long)limit < n ? (unsigned long long)limit : n; }
};

// everything this rank can get wrong on its own, before the first collective
void ordered_check(imm3_ctx *ctx, imm3_query *const *queries, const int32_t *segment_index, int32_t n_queries, int64_t limit, MergeOrderSpec &sp,
                   OrderedInputs &in, LocalVerdict &verdict) {
    const size_t nq = (size_t)std::max(n_queries, 0);
    in.n_entries.assign(nq, 1);
    in.entry_at.assign(nq, 0);
    in.n_local.assign(nq, 0);
    in.split.assign(nq, 0);
    if (n_queries == 0) verdict.fail(IMM3_ERR_ARG, "a rank joins the merge with at least one ordered query (the SELECT list and the keys come from it)");
    for (int32_t i = 0; i < n_queries && verdict.ok(); ++i) {
        const imm3_query *q = queries[i];
        if (!q) verdict.fail(IMM3_ERR_ARG, "query is null");
        else if (q->is_agg || q->proj.empty() || !q->ordered) verdict.fail(IMM3_ERR_ARG, "not an ordered projection (imm3_query_set_order on a projecting query)");
        else if (q->ctx != ctx) verdict.fail(IMM3_ERR_ARG, "the query runs on another context than the communicator");
    }
    for (int32_t i = 0; i < n_queries && verdict.ok(); ++i)
        if (!queries[i]->run.ran_project) verdict.fail(IMM3_ERR_STATE, "imm3_query_run has not been called");
    if (verdict.ok()) {
        sp = order_spec_of(queries[0]);
        for (int32_t i = 1; i < n_queries && verdict.ok(); ++i)
            if (!(order_spec_of(queries[i]) == sp)) verdict.fail(IMM3_ERR_ARG, "the queries differ in their SELECT lists (columns, widths, kinds) or in their order keys");
    }
    if (verdict.ok()) {
        std::vector<int64_t> own(nq);
        size_t at = 0;
        for (size_t i = 0; i < nq; ++i) {
            own[i] = queries[i]->order_limit;
            in.n_entries[i] = queries[i]->table ? (int32_t)queries[i]->table->segs.size() : 1;
            in.entry_at[i] = at;
            at += (size_t)in.n_entries[i];
        }
        std::string why;
        if (!merge_order_check(limit, own.data(), in.n_entries.data(), n_queries, segment_index, &why)) verdict.fail(IMM3_ERR_ARG, why);
        for (size_t i = 0; i < nq && verdict.ok(); ++i)
            for (int32_t e = 1; e < in.n_entries[i]; ++e)
                if (segment_index[in.entry_at[i] + (size_t)e] < segment_index[in.entry_at[i] + (size_t)e - 1]) in.split[i] = 1;
    }
    for (size_t i = 0; i < nq && verdict.ok(); ++i) { // (waits for the run; orders again when the arrays were outgrown)
        const int rrc = imm3_query_row_count(queries[i], &in.n_local[i]);
        if (rrc) verdict.fail(rrc, imm3_last_error());
        in.total_local += in.n_local[i];
    }
    if (verdict.ok() && in.total_local > kMergeOrderMaxRows) verdict.fail(IMM3_ERR_ARG, "too many rows to merge (more than 2^30 enter the merge)");
}

// one query's ordered rows -> records at `recs` (pa: where the rows' segments come from, set by the caller)
void pack_query(const imm3_query *q, const OrderedLocal &L, MergeOrderPackArgs pa, uint32_t *recs, uint32_t n_rows, hipStream_t s, LocalStep &step) {
    const MergeOrderSpec &sp = L.sp;
    pa.n_keys = (int32_t)q->order_keys.size();
    pa.key_bytes = q->order_key_bytes;
    for (int k = 0; k < pa.n_keys; ++k) {
        const int32_t pj = q->order_keys[(size_t)k].proj;
        pa.keys[k].src = q->d_order_proj[(size_t)pj];
        pa.keys[k].width = sp.widths[(size_t)pj];
        pa.keys[k].kind = sp.kinds[(size_t)pj];
        pa.keys[k].descending = q->order_keys[(size_t)k].descending ? 1 : 0;
    }
    pa.row_index = q->d_order_row_index;
    pa.n_rows = n_rows;
    pa.rec_words = L.geo.rec_words;
    pa.recs = recs;
    const size_t np = q->proj.size();
    for (size_t done = 0; done < np && step.ok;) { // more SELECT-list columns than one launch carries: in groups (the key with the first)
        const size_t take = std::min<size_t>(kMaxProj, np - done);
        pa.with_key = done == 0;
        pa.n_cols = (int32_t)take;
        for (size_t j = 0; j < take; ++j) {
            pa.cols[j].src = q->d_order_proj[done + j];
            pa.cols[j].width = sp.widths[done + j];
            pa.cols[j].rec_off = L.geo.col_off[done + j];
        }
        done += take;
        launch_merge_order_pack(pa, s);
        step(hipGetLastError(), "merge pack");
    }
}

// The local merge's one allocation, in 32-bit words: {input records, a split query's records in its own order, merged records, total
// word, list table, per table query: tile starts + global indices, a split query's per-segment counts}
struct OrderedLayout {
    int32_t n_lists = 0;
    unsigned long long list_cap = 0, meta_u32 = 0;
    unsigned long long w_in = 0, w_tmp = 0, w_out = 0, w_total = 0, w_lists = 0, w_meta = 0, w_counts = 0, w_end = 0;
};
OrderedLayout ordered_layout(imm3_query *const *queries, int32_t n_queries, const OrderedInputs &in, unsigned long long R, unsigned long long mine) {
    OrderedLayout y;
    unsigned long long split_rows = 0, split_segs = 0;
    for (int32_t i = 0; i < n_queries; ++i) {
        const size_t u = (size_t)i;
        y.n_lists += in.split[u] ? in.n_entries[u] : 1;
        y.list_cap = std::max<unsigned long long>(y.list_cap, in.n_local[u]);
        if (in.split[u]) { split_rows = std::max<unsigned long long>(split_rows, in.n_local[u]); split_segs = std::max<unsigned long long>(split_segs, (unsigned long long)in.n_entries[u]); }
        if (queries[i]->table) y.meta_u32 += 2ULL * (unsigned long long)in.n_entries[u] + 2ULL;
    }
    y.w_tmp = y.w_in + in.total_local * R;
    y.w_out = y.w_tmp + split_rows * R;
    y.w_total = y.w_out + mine * R;
    y.w_lists = y.w_total + 2;
    y.w_meta = y.w_lists + 4ULL * (unsigned long long)y.n_lists;
    y.w_counts = y.w_meta + even(y.meta_u32);
    y.w_end = y.w_counts + even(split_segs);
    return y;
}

// The device work of the local phase over the allocation d1: the list table and the tables' lookups, every query packed (a split
// query moved into per-segment lists), the lists merged and cut.  Whatever fails goes into L.step.
void ordered_device_merge(imm3_query *const *queries, const int32_t *segment_index, int32_t n_queries, const OrderedInputs &in, const OrderedLayout &y,
                          uint32_t *d1, hipStream_t s, OrderedLocal &L) {
    LocalStep &step = L.step;
    const size_t R = (size_t)L.geo.rec_words;
    step(hipMemsetAsync(d1, 0, (size_t)y.w_end * sizeof(uint32_t), s), "merge buffer clear"); // (pad words: records are bit-exact images)
    L.h_lists.assign(2 * (size_t)y.n_lists, 0ULL);
    L.h_meta.assign((size_t)even(y.meta_u32), 0u);
    std::vector<size_t> meta_at((size_t)n_queries, 0), list_at((size_t)n_queries, 0);
    {
        size_t m = 0, l = 0;
        unsigned long long rec_at = 0;
        for (int32_t i = 0; i < n_queries; ++i) {
            const imm3_query *q = queries[i];
            const size_t u = (size_t)i;
            list_at[u] = l;
            if (!in.split[u]) { // (a split query's entries are written by its move launch)
                L.h_lists[2 * l] = y.w_in + rec_at * R;
                L.h_lists[2 * l + 1] = in.n_local[u];
            }
            l += in.split[u] ? (size_t)in.n_entries[u] : 1;
            rec_at += in.n_local[u];
            if (!q->table) continue;
            meta_at[u] = m;
            const int32_t ns = in.n_entries[u];
            for (int32_t t = 0; t <= ns; ++t) L.h_meta[m + (size_t)t] = (uint32_t)q->table->tile_start[(size_t)t];
            for (int32_t t = 0; t < ns; ++t) L.h_meta[m + (size_t)ns + 1 + (size_t)t] = (uint32_t)segment_index[in.entry_at[u] + (size_t)t];
            m += 2 * (size_t)ns + 2;
        }
    }
    if (step.ok) step(hipMemcpyAsync(d1 + y.w_lists, L.h_lists.data(), L.h_lists.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, s), "merge list table");
    if (step.ok && !L.h_meta.empty()) step(hipMemcpyAsync(d1 + y.w_meta, L.h_meta.data(), L.h_meta.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s), "merge table lookups");
    unsigned long long rec_at = 0;
    for (int32_t i = 0; i < n_queries && step.ok; ++i) {
        const imm3_query *q = queries[i];
        const size_t u = (size_t)i;
        const uint64_t n = in.n_local[u];
        if (!n) continue;
        MergeOrderPackArgs pa;
        std::memset(&pa, 0, sizeof(pa));
        if (q->table) {
            pa.n_tsegs = in.n_entries[u];
            pa.tile_start = d1 + y.w_meta + meta_at[u];
            pa.global_index = pa.tile_start + pa.n_tsegs + 1;
        } else pa.segment = (uint32_t)segment_index[in.entry_at[u]];
        pack_query(q, L, pa, d1 + (in.split[u] ? y.w_tmp : y.w_in + rec_at * R), (uint32_t)n, s, step);
        if (in.split[u] && step.ok) {
            MergeOrderSplitArgs sa;
            std::memset(&sa, 0, sizeof(sa));
            sa.src = d1 + y.w_tmp;
            sa.dst = d1;
            sa.dst_word = y.w_in + rec_at * R;
            sa.n_rows = (uint32_t)n;
            sa.n_tsegs = in.n_entries[u];
            sa.rec_words = (int32_t)R;
            sa.global_index = pa.global_index;
            sa.counts = d1 + y.w_counts;
            sa.lists = (unsigned long long *)(d1 + y.w_lists) + 2 * list_at[u];
            launch_merge_order_split(sa, s); // (the next split query reuses the records behind this launch: same stream)
            step(hipGetLastError(), "merge split");
        }
        rec_at += n;
    }
    if (step.ok && in.total_local) {
        MergeOrderArgs ma;
        std::memset(&ma, 0, sizeof(ma));
        ma.recs = d1;
        ma.buf_words = y.w_tmp; // (the input records only)
        ma.lists = (const unsigned long long *)(d1 + y.w_lists);
        ma.n_lists = y.n_lists;
        ma.rec_words = (int32_t)R;
        ma.list_cap = (uint32_t)y.list_cap;
        ma.cut = (uint32_t)L.mine;
        ma.out = d1 + y.w_out;
        ma.out_total = (unsigned long long *)(d1 + y.w_total);
        launch_merge_order_rank(ma, s);
        step(hipGetLastError(), "merge rank");
    }
    if (step.ok) step(hipStreamSynchronize(s), "merge of this rank's lists");
}

// This rank's part: the checks into the verdict, every query's rows packed into records, the lists merged and cut to the limit.
// Returns non-zero when the call ends here -- a context that cannot be used (before anything collective), or, with `to_host`,
// whatever went wrong: the caller then meets no other rank, and the result is in L.recs / L.total.
int ordered_local(imm3_ctx *ctx, imm3_query *const *queries, const int32_t *segment_index, int32_t n_queries, int64_t limit, bool to_host, OrderedLocal &L) {
    imm3::GateScope gate(&ctx->gate);
    if (ctx->closed) return fail(IMM3_ERR_STATE, "the context of this communicator has been destroyed");
    if (ctx->capture) return fail(IMM3_ERR_STATE, "a graph capture is open on this context");
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    L.limit = limit;
    OrderedInputs in;
    ordered_check(ctx, queries, segment_index, n_queries, limit, L.sp, in, L.verdict);
    if (!L.verdict.ok()) return to_host ? merge_local_result(L.verdict, L.step) : IMM3_OK;
    L.geo = merge_order_geometry(L.sp.widths);
    L.mine = L.cut_of(in.total_local);
    const OrderedLayout y = ordered_layout(queries, n_queries, in, (unsigned long long)L.geo.rec_words, L.mine);
    const unsigned long long rank_waves = (unsigned long long)y.n_lists * ((y.list_cap + 63ULL) / 64ULL);
    if (rank_waves / 4ULL >= 0x7FFFFFFFULL) L.step.refuse("too many lists of too many rows to merge in one launch");
    else if (L.block.alloc((size_t)y.w_end * sizeof(uint32_t)) != hipSuccess) L.step.refuse("hipMalloc of the ordered merge's buffers failed");
    if (L.step.ok) {
        L.d_out = (uint32_t *)L.block.p + y.w_out;
        ordered_device_merge(queries, segment_index, n_queries, in, y, (uint32_t *)L.block.p, s, L);
    }
    if (!to_host) return IMM3_OK;
    const int rc = merge_local_result(L.verdict, L.step);
    if (rc) return rc;
    const size_t out_words = (size_t)L.mine * (size_t)L.geo.rec_words;
    L.recs.assign(out_words, 0u);
    if (out_words) HIPCHK(hipMemcpyAsync(L.recs.data(), L.d_out, out_words * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    L.total = L.mine;
    return IMM3_OK;
}

// The ranks' lists into one, in order, cut to the limit, on every rank: L.recs / L.total.
int ordered_exchange(imm3_comm *c, OrderedLocal &L) {
    hipStream_t s = c->ctx->stream;
    int rc = merge_vote(c, s, L.sp.vote(0, L.limit), L.sp.vote(1, L.limit), L.verdict, "the ranks' ordered queries differ in SELECT list, order keys or the merge's limit");
    if (rc) return rc;
    unsigned long long most = 0;
    rc = merge_list_length(c, s, L.step, L.mine, "a rank could not merge its own lists; no rank has merged anything", &most);
    if (rc) return rc;
    if (!most) return IMM3_OK; // (every rank's list is empty)
    const size_t R = (size_t)L.geo.rec_words;
    const unsigned long long entries = most * (unsigned long long)c->world;
    if (entries > kMergeOrderMaxRows) return fail(IMM3_ERR_ARG, "too many rows to merge (more than 2^30 enter the merge)"); // (the same figure on every rank: every rank leaves here)
    const unsigned long long slot_words = 2ULL + most * R, cut2 = L.cut_of(entries);
    // {send slot, the ranks' slots, total word, merged records}; a slot is its list's length word, then the records
    const unsigned long long x_recv = slot_words, x_total = x_recv + slot_words * (unsigned long long)c->world, x_out = x_total + 2, x_end = x_out + cut2 * R;
    DeviceBlock x;
    rc = merge_exchange_alloc(c, s, (size_t)x_end * sizeof(uint32_t), x);
    if (rc) return rc;
    uint32_t *const dx = (uint32_t *)x.p;
    rc = merge_gather(c, s, dx, dx + x_recv, (size_t)(slot_words / 2), &L.mine, L.d_out, (size_t)(L.mine * R) * sizeof(uint32_t));
    if (rc) return rc;
    MergeOrderArgs ma;
    std::memset(&ma, 0, sizeof(ma));
    ma.recs = dx + x_recv;
    ma.buf_words = slot_words * (unsigned long long)c->world;
    ma.slot_words = slot_words;
    ma.n_lists = c->world;
    ma.rec_words = (int32_t)R;
    ma.list_cap = (uint32_t)most;
    ma.cut = (uint32_t)cut2;
    ma.out = dx + x_out;
    ma.out_total = (unsigned long long *)(dx + x_total);
    launch_merge_order_rank(ma, s);
    HIPCHK(hipGetLastError());
    std::vector<uint32_t> h((size_t)(2 + cut2 * R)); // one copy: the total word and the records behind it
    HIPCHK(hipMemcpyAsync(h.data(), dx + x_total, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    unsigned long long all = 0;
    std::memcpy(&all, h.data(), sizeof(all));
    L.total = std::min(all, cut2);
    L.recs.assign(h.begin() + 2, h.begin() + 2 + (size_t)(L.total * R));
    return IMM3_OK;
}

} // namespace

extern "C" int imm3_comm_merge_ordered(imm3_comm *c, imm3_query *const *queries, const int32_t *segment_index, int32_t n_queries,
                                       int64_t limit, uint32_t *segment_out, uint32_t *row_out, void *const *col_out,
                                       uint64_t max_rows, uint64_t *n_rows) {
    if (!c || !n_rows || n_queries < 0 || (n_queries > 0 && (!queries || !segment_index))) return fail(IMM3_ERR_ARG, "bad argument");
    imm3::GateScope gate(&c->ctx->gate); // (held across both phases)
    OrderedLocal L;
    int rc = ordered_local(c->ctx, queries, segment_index, n_queries, limit, c->world == 1, L);
    if (!rc && c->world > 1) rc = ordered_exchange(c, L);
    if (rc) return rc;
    *n_rows = L.total;
    merge_order_unpack(L.recs.data(), L.total, merge_order_geometry(L.sp.widths), L.sp.widths, segment_out, row_out, col_out, max_rows);
    return IMM3_OK;
}

// Single-process flavour (comms from imm3_comm_create_all): per device the local phase above, cut to the limit, then one k-way
// merge of the devices' lists on the host.
extern "C" int imm3_comm_merge_ordered_all(imm3_comm *const *comms, int32_t n_comms, imm3_query *const *const *queries,
                                           const int32_t *const *segment_index, const int32_t *n_queries,
                                           int64_t limit, uint32_t *segment_out, uint32_t *row_out, void *const *col_out,
                                           uint64_t max_rows, uint64_t *n_rows) {
    if (!comms || n_comms < 1 || !queries || !segment_index || !n_queries || !n_rows) return fail(IMM3_ERR_ARG, "bad argument");
    bool have = false;
    MergeOrderSpec sp;
    std::vector<std::vector<uint32_t>> lists;
    std::vector<uint64_t> lens;
    for (int32_t i = 0; i < n_comms; ++i) {
        if (!comms[i] || n_queries[i] < 0 || (n_queries[i] > 0 && (!queries[i] || !segment_index[i]))) return fail(IMM3_ERR_ARG, "bad argument");
        if (n_queries[i] == 0) continue;
        OrderedLocal L;
        const int rc = ordered_local(comms[i]->ctx, queries[i], segment_index[i], n_queries[i], limit, true, L);
        if (rc) return rc;
        if (!have) { sp = L.sp; have = true; }
        else if (!(L.sp == sp)) return fail(IMM3_ERR_ARG, "the devices' ordered queries differ in SELECT list or order keys");
        lists.push_back(std::move(L.recs));
        lens.push_back(L.total);
    }
    const MergeOrderGeometry geo = merge_order_geometry(sp.widths);
    std::vector<const uint32_t *> ptrs;
    for (auto &l : lists) ptrs.push_back(l.data());
    std::vector<uint32_t> merged;
    merge_order_host(ptrs.data(), lens.data(), (int32_t)lists.size(), geo.rec_words, limit > 0 ? (uint64_t)limit : 0, merged);
    *n_rows = merged.size() / (size_t)geo.rec_words;
    merge_order_unpack(merged.data(), *n_rows, geo, sp.widths, segment_out, row_out, col_out, max_rows);
    return IMM3_OK;
}
