// imm3_merge_wide.cpp -- imm3_comm_merge_groups_wide and its single-process flavour.
//
// The merge of imm3_merge_groups.cpp by BYTE key: group keys of 0 .. IMM3_GROUP_KEY_MAX_WIDTH bytes and string maxima of any width.
// Every (query, group) becomes one immutable record (MergeWideArgs, imm3_internal.h); the records go through a device hash table
// whose slots hold the index of the record that claimed them, the occupied slots come out as records again (the local phase,
// wide_local), and with more than one rank those lists are exchanged with ncclAllGather -- fixed-size slots, sized by an
// all-reduce(max) of the list lengths -- and go through the same table once more (wide_exchange, built from the protocol of
// imm3_comm_internal.h).  imm3_comm_merge_groups_view[_all] (at the end) are this merge with its final list left on the device for
// the view's launches (imm3_merge_view_api.cpp / imm3_merge_view.hip).
#include "imm3_comm_internal.h"

#include <algorithm>
#include <cstring>
#include <map>

using namespace imm3;

namespace {

constexpr unsigned long long kMaxMergeEntries = 1ULL << 30; // (the table's slot fields and record indices are 32 bits; 0xFFFFFFFF is the empty marker)

struct WideSpec {
    int key_bytes = 0, n_agg = 0;
    int32_t kinds[kMaxAggs] = {0, 0, 0, 0}, is_str[kMaxAggs] = {0, 0, 0, 0};
    int32_t str_width[kMaxAggs] = {0, 0, 0, 0}; // of every MAX over a STRING column, narrow ones included; 0: another aggregate
    bool operator==(const WideSpec &o) const {
        if (key_bytes != o.key_bytes || n_agg != o.n_agg) return false;
        for (int j = 0; j < kMaxAggs; ++j)
            if (kinds[j] != o.kinds[j] || is_str[j] != o.is_str[j] || str_width[j] != o.str_width[j]) return false;
        return true;
    }
    // what the ranks vote on: {key width, aggregates, their kinds, which are strings}, {the string widths}
    unsigned long long vote(int word) const {
        unsigned long long v = 0;
        if (word == 0) {
            v = (unsigned long long)key_bytes | (unsigned long long)n_agg << 16;
            for (int j = 0; j < kMaxAggs; ++j) v |= (unsigned long long)(kinds[j] & 3) << (24 + 2 * j) | (unsigned long long)(is_str[j] & 1) << (32 + j);
        } else
            for (int j = 0; j < kMaxAggs; ++j) v |= (unsigned long long)str_width[j] << (16 * j);
        return v;
    }
};

WideSpec wide_spec_of(const imm3_query *q) {
    WideSpec sp;
    for (int32_t g : q->group_cols) sp.key_bytes += q->seg->cols[(size_t)q->used[(size_t)g]].width;
    sp.n_agg = (int)q->aggs.size();
    for (int j = 0; j < sp.n_agg; ++j) {
        const SegCol &sc = q->seg->cols[(size_t)q->used[(size_t)q->aggs[(size_t)j].column]];
        sp.kinds[j] = q->aggs[(size_t)j].kind;
        sp.is_str[j] = sc.vcodec == IMM3_DENSE_STRING;
        if (sp.kinds[j] == AGG_MAX && sp.is_str[j]) sp.str_width[j] = sc.width;
    }
    return sp;
}

// the record geometry of a spec (the table and list pointers stay null)
MergeWideArgs wide_geometry(const WideSpec &sp) {
    MergeWideArgs a;
    std::memset(&a, 0, sizeof(a));
    a.key_bytes = sp.key_bytes;
    a.key_words = (sp.key_bytes + 7) / 8;
    a.n_agg = sp.n_agg;
    int off = kMergeWideHead + a.key_words, planes = 0;
    for (int j = 0; j < kMaxAggs; ++j) {
        a.kinds[j] = sp.kinds[j];
        a.is_str[j] = sp.is_str[j];
        a.best_plane[j] = -1;
        if (sp.str_width[j] > 8) {
            a.str_off[j] = off;
            a.str_words[j] = (sp.str_width[j] + 7) / 8;
            a.str_width[j] = sp.str_width[j];
            a.best_plane[j] = planes++;
            off += a.str_words[j];
        }
    }
    a.rec_words = off;
    return a;
}
int wide_planes(const MergeWideArgs &a) {
    int n = 0;
    for (int j = 0; j < kMaxAggs; ++j) n += a.best_plane[j] >= 0;
    return n;
}

// one allocation: {counts, first, vals[kMaxAggs]} x slots, the collected list and its counter, then the 32-bit planes {claim, best ...}
size_t wide_table_bytes(const MergeWideArgs &geo, unsigned long long slots, unsigned long long list_cap) {
    return (size_t)((slots * (2 + kMaxAggs) + list_cap * (unsigned long long)geo.rec_words + 8) * sizeof(unsigned long long) +
                    slots * (unsigned long long)(1 + wide_planes(geo)) * sizeof(uint32_t));
}
void wide_bind(MergeWideArgs &a, void *p, unsigned long long slots, unsigned long long list_cap) {
    a.slots = (uint32_t)slots;
    a.mask = (uint32_t)(slots - 1);
    unsigned long long *w = (unsigned long long *)p;
    a.t_counts = w;
    a.t_first = a.t_counts + slots;
    a.t_vals = (long long *)(a.t_first + slots);
    a.out_recs = (unsigned long long *)(a.t_vals + (size_t)kMaxAggs * slots);
    a.out_n = a.out_recs + list_cap * (unsigned long long)a.rec_words;
    a.out_cap = (uint32_t)list_cap;
    a.t_claim = (uint32_t *)(a.out_n + 8);
    a.t_best = a.t_claim + slots;
}

void combine_wide(unsigned long long *into, const unsigned long long *g, const MergeWideArgs &geo) {
    into[0] = std::min(into[0], g[0]);
    into[1] += g[1];
    for (int j = 0; j < geo.n_agg; ++j) {
        unsigned long long &t = into[2 + j];
        const unsigned long long v = g[2 + j];
        if (geo.kinds[j] == AGG_MAX) t = geo.is_str[j] ? std::max(t, v) : (unsigned long long)std::max((long long)t, (long long)v);
        else if (geo.kinds[j] == AGG_MIN) t = (unsigned long long)std::min((long long)t, (long long)v);
        else if (geo.kinds[j] == AGG_SUM) t += v;
        if (geo.str_off[j] && std::memcmp(g + geo.str_off[j], into + geo.str_off[j], (size_t)geo.str_width[j]) > 0)
            std::memcpy(into + geo.str_off[j], g + geo.str_off[j], (size_t)geo.str_words[j] * sizeof(unsigned long long));
    }
}

// records (any order) -> the caller's arrays, ascending first arrival; in_list_order: as they come (a view ordered them already)
void unpack_wide(const std::vector<unsigned long long> &recs, const WideSpec &sp, const MergeWideArgs &geo, uint8_t *key_bytes_out, uint64_t *first,
                 uint64_t *counts, int64_t *vals, uint8_t *const *str_out, uint32_t max_groups, uint32_t *n_groups, bool in_list_order = false) {
    const size_t R = (size_t)geo.rec_words, n = recs.size() / R;
    std::vector<const unsigned long long *> order(n);
    for (size_t i = 0; i < n; ++i) order[i] = recs.data() + i * R;
    if (!in_list_order) std::sort(order.begin(), order.end(), [](const unsigned long long *x, const unsigned long long *y) { return x[0] < y[0]; }); // first arrival first
    *n_groups = (uint32_t)n;
    for (size_t o = 0; o < n && o < max_groups; ++o) {
        const unsigned long long *w = order[o];
        if (key_bytes_out && sp.key_bytes) std::memcpy(key_bytes_out + o * (size_t)sp.key_bytes, w + kMergeWideHead, (size_t)sp.key_bytes);
        if (first) first[o] = w[0];
        if (counts) counts[o] = w[1];
        for (int j = 0; j < sp.n_agg; ++j) {
            if (vals) vals[o * (size_t)sp.n_agg + (size_t)j] = sp.kinds[j] == AGG_COUNT ? (int64_t)w[1] : (int64_t)w[2 + j];
            if (!str_out || !str_out[j]) continue;
            const size_t wd = (size_t)sp.str_width[j];
            uint8_t *dst = str_out[j] + o * wd;
            if (geo.str_off[j]) std::memcpy(dst, w + geo.str_off[j], wd);
            else // (<= 8 bytes: the value packed big-endian)
                for (size_t b = 0; b < wd; ++b) dst[b] = (uint8_t)(w[2 + j] >> (8 * (wd - 1 - b)));
        }
    }
}

// what the local phase leaves: the verdicts, the spec and its record geometry, and this rank's merged records -- `mine` of them on
// the device (a1.out_recs, in `block`) or, as the final result, in `recs` (no particular order)
struct WideLocal {
    LocalVerdict verdict;
    LocalStep step;
    WideSpec sp;
    MergeWideArgs geo, a1;
    DeviceBlock block;
    unsigned long long mine = 0;
    std::vector<unsigned long long> recs;
};

// a device list of n records -> out
int read_records(const unsigned long long *d_list, unsigned long long n, size_t R, hipStream_t s, std::vector<unsigned long long> &out) {
    out.assign((size_t)n * R, 0ULL);
    if (n) HIPCHK(hipMemcpyAsync(out.data(), d_list, out.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return IMM3_OK;
}

// This rank's part: the checks into the verdict, every (query, group) packed into a record, the records merged by key.  Returns
// non-zero when the call ends here -- a context that cannot be used (before anything collective), or, with `to_host`, whatever went
// wrong: the caller then meets no other rank, and the result is in L.recs.
int wide_local(imm3_ctx *ctx, imm3_query *const *queries, const int32_t *segment_index, int32_t n_queries, uint8_t *const *str_out, bool to_host, WideLocal &L) {
    imm3::GateScope gate(&ctx->gate);
    if (ctx->closed) return fail(IMM3_ERR_STATE, "the context of this communicator has been destroyed");
    if (ctx->capture) return fail(IMM3_ERR_STATE, "a graph capture is open on this context");
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    LocalVerdict &verdict = L.verdict;
    WideSpec &sp = L.sp;
    merge_check_agg_queries(queries, n_queries, verdict);
    std::vector<uint32_t> n_local((size_t)std::max(n_queries, 0), 0u);
    unsigned long long total_local = 0;
    uint32_t most_local = 0;
    if (verdict.ok()) {
        sp = wide_spec_of(queries[0]);
        for (int32_t i = 1; i < n_queries && verdict.ok(); ++i) {
            const WideSpec si = wide_spec_of(queries[i]);
            if (si.key_bytes != sp.key_bytes) verdict.fail(IMM3_ERR_ARG, "the queries' group keys differ in width");
            else if (!(si == sp)) verdict.fail(IMM3_ERR_ARG, "the queries aggregate differently (kinds, or the widths of their string MAX columns)");
        }
        for (int j = 0; j < kMaxAggs && verdict.ok() && str_out; ++j)
            if (j < sp.n_agg && str_out[j] && !sp.str_width[j]) verdict.fail(IMM3_ERR_ARG, "str_out[" + std::to_string(j) + "] is set, but that aggregate is not a MAX over a STRING column");
        for (int32_t i = 0; i < n_queries && verdict.ok(); ++i) {
            if (queries[i]->ctx != ctx) { verdict.fail(IMM3_ERR_ARG, "the query runs on another context than the communicator"); break; }
            const int grc = query_groups(queries[i], &n_local[(size_t)i]);
            if (grc) verdict.fail(grc, imm3_last_error());
            total_local += n_local[(size_t)i];
            most_local = std::max(most_local, n_local[(size_t)i]);
        }
        if (total_local > kMaxMergeEntries) verdict.fail(IMM3_ERR_ARG, "too many groups to merge");
    }
    L.geo = wide_geometry(sp);
    if (!verdict.ok()) return to_host ? merge_local_result(verdict, L.step) : IMM3_OK;
    const MergeWideArgs &geo = L.geo;
    const size_t R = (size_t)geo.rec_words;
    auto round8 = [](size_t v) { return (v + 7) & ~(size_t)7; };
    // ---- this rank's records and their merge: {records, key bytes of one query, string bytes of one query per wide MAX, table} ----
    const unsigned long long n1 = std::max<unsigned long long>(total_local, 1), slots1 = pow2_at_least(2 * n1);
    const size_t rec_bytes = (size_t)n1 * R * sizeof(unsigned long long);
    const size_t keyb_bytes = sp.key_bytes > 8 ? round8((size_t)most_local * (size_t)sp.key_bytes) : 0;
    size_t strb_bytes[kMaxAggs], tmp_bytes = keyb_bytes;
    for (int j = 0; j < kMaxAggs; ++j) { strb_bytes[j] = geo.str_off[j] ? round8((size_t)most_local * (size_t)geo.str_width[j]) : 0; tmp_bytes += strb_bytes[j]; }
    LocalStep &step = L.step;
    MergeWideArgs &a1 = L.a1;
    a1 = geo;
    if (L.block.alloc(rec_bytes + tmp_bytes + wide_table_bytes(geo, slots1, n1)) != hipSuccess) step.refuse("hipMalloc of the merge table failed");
    if (step.ok) {
        unsigned long long *d_recs = (unsigned long long *)L.block.p;
        uint8_t *d_tmp = (uint8_t *)L.block.p + rec_bytes;
        uint8_t *d_keyb = d_tmp, *d_strb[kMaxAggs];
        d_tmp += keyb_bytes;
        for (int j = 0; j < kMaxAggs; ++j) { d_strb[j] = d_tmp; d_tmp += strb_bytes[j]; }
        wide_bind(a1, d_tmp, slots1, n1);
        launch_mergew_init(a1, s);
        step(hipGetLastError(), "merge table init");
        size_t at = 0;
        for (int32_t i = 0; i < n_queries && step.ok; ++i) {
            imm3_query *q = queries[i];
            const uint32_t ng = n_local[(size_t)i];
            if (!ng) continue;
            AggArgs qa;
            query_agg_args(q, qa);
            a1.q_keys = q->d_okeys;
            a1.q_key_bytes = nullptr;
            if (sp.key_bytes > 8) { // (the table holds tags: the bytes are read at each group's first row)
                launch_group_keys(qa, ng, sp.key_bytes, d_keyb, s);
                a1.q_key_bytes = d_keyb;
            }
            for (int j = 0; j < kMaxAggs; ++j) {
                a1.q_str[j] = nullptr;
                if (!geo.str_off[j]) continue;
                launch_strmax_collect(qa, j, ng, d_strb[j], s);
                a1.q_str[j] = d_strb[j];
            }
            a1.q_first = q->d_ofirst;
            a1.q_counts = q->d_ocounts;
            a1.q_vals = q->d_ovals;
            a1.n_groups = ng;
            a1.seg_hi = (unsigned long long)(uint32_t)segment_index[i] << 32;
            a1.rec_out = d_recs + at * R;
            launch_mergew_pack(a1, s); // (the next query's gathers overwrite d_keyb / d_strb behind this launch: same stream)
            step(hipGetLastError(), "merge pack");
            at += ng;
        }
        if (step.ok) {
            a1.recs = d_recs;
            a1.n_recs = (uint32_t)total_local;
            if (total_local) launch_mergew_insert(a1, s);
            launch_mergew_collect(a1, s);
            step(hipGetLastError(), "merge insert / collect");
        }
        if (step.ok) step(hipMemcpyAsync(&L.mine, a1.out_n, sizeof(L.mine), hipMemcpyDeviceToHost, s), "merge list length");
        if (step.ok) step(hipStreamSynchronize(s), "merge list length");
    }
    if (!to_host) return IMM3_OK;
    const int rc = merge_local_result(verdict, step);
    if (rc) return rc;
    return read_records(a1.out_recs, L.mine, R, s, L.recs);
}

// a view behind the merge (imm3_comm_merge_groups_view): the final list stays on the device -- n records at d_list, in `block` (the
// exchange's) or in the local phase's block -- for the launches of imm3_merge_view.hip
struct WideKeep {
    MergeViewCall *view = nullptr;
    DeviceBlock block;
    const unsigned long long *d_list = nullptr;
    unsigned long long n = 0;
};

// The ranks' records into one list, on every rank: L.recs -- or, with `keep`, left on the device once the ranks agree on the view.
int wide_exchange(imm3_comm *c, WideLocal &L, WideKeep *keep = nullptr) {
    hipStream_t s = c->ctx->stream;
    int rc = merge_vote(c, s, L.sp.vote(0), L.sp.vote(1), L.verdict, "the ranks' aggregation queries differ in key width, aggregates or string MAX widths");
    if (rc) return rc;
    if (keep) { // (every rank is here with a checked view: the same answer on all of them, before the gather)
        rc = merge_view_agree(c, s, *keep->view);
        if (rc) return rc;
    }
    unsigned long long most = 0;
    rc = merge_list_length(c, s, L.step, L.mine, "a rank could not build its merge table; no rank has merged anything", &most);
    if (rc) return rc;
    const size_t R = (size_t)L.geo.rec_words, per_rank = (size_t)most * R;
    if (!per_rank) return IMM3_OK;
    const unsigned long long entries = most * (unsigned long long)c->world;
    if (entries > kMaxMergeEntries) return fail(IMM3_ERR_ARG, "too many groups to merge"); // (the same figure on every rank: every rank leaves here)
    const unsigned long long slots2 = pow2_at_least(2 * entries);
    DeviceBlock x_here, &x = keep ? keep->block : x_here; // {send slot, the ranks' slots, second table}
    rc = merge_exchange_alloc(c, s, (per_rank + per_rank * (size_t)c->world) * sizeof(unsigned long long) + wide_table_bytes(L.geo, slots2, entries), x);
    if (rc) return rc;
    unsigned long long *d_send = (unsigned long long *)x.p, *d_recv = d_send + per_rank;
    rc = merge_gather(c, s, d_send, d_recv, per_rank, nullptr, L.a1.out_recs, (size_t)L.mine * R * sizeof(unsigned long long));
    if (rc) return rc;
    MergeWideArgs a2 = L.geo;
    wide_bind(a2, d_recv + per_rank * (size_t)c->world, slots2, entries);
    launch_mergew_init(a2, s);
    HIPCHK(hipGetLastError());
    a2.recs = d_recv;
    a2.n_recs = (uint32_t)entries;
    launch_mergew_insert(a2, s);
    HIPCHK(hipGetLastError());
    launch_mergew_collect(a2, s);
    HIPCHK(hipGetLastError());
    unsigned long long n2 = 0;
    HIPCHK(hipMemcpyAsync(&n2, a2.out_n, sizeof(n2), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (keep) {
        keep->d_list = a2.out_recs;
        keep->n = n2;
        return IMM3_OK;
    }
    return read_records(a2.out_recs, n2, R, s, L.recs);
}

// The single-process flavours' merge: per communicator the one-rank merge on its context, then one merge by byte key on the host
// into `merged` (no particular order).
int wide_all_records(imm3_comm *const *comms, int32_t n_comms, imm3_query *const *const *queries, const int32_t *const *segment_index, const int32_t *n_queries,
                     uint8_t *const *str_out, WideSpec &sp, MergeWideArgs &geo, std::vector<unsigned long long> &merged) {
    bool have = false;
    geo = wide_geometry(sp);
    std::map<std::string, std::vector<unsigned long long>> all;
    for (int32_t i = 0; i < n_comms; ++i) {
        if (!comms[i] || n_queries[i] < 0 || (n_queries[i] > 0 && (!queries[i] || !segment_index[i]))) return fail(IMM3_ERR_ARG, "bad argument");
        if (n_queries[i] == 0) continue;
        WideLocal L;
        const int rc = wide_local(comms[i]->ctx, queries[i], segment_index[i], n_queries[i], str_out, true, L);
        if (rc) return rc;
        if (!have) { sp = L.sp; geo = L.geo; have = true; }
        else if (!(L.sp == sp)) return fail(IMM3_ERR_ARG, "the devices' aggregation queries differ in key width, aggregates or string MAX widths");
        const size_t R = (size_t)geo.rec_words;
        for (size_t g = 0; g < L.recs.size() / R; ++g) {
            const unsigned long long *w = L.recs.data() + g * R;
            std::string key((const char *)(w + kMergeWideHead), (size_t)sp.key_bytes);
            auto it = all.find(key);
            if (it == all.end()) all.emplace(std::move(key), std::vector<unsigned long long>(w, w + R));
            else combine_wide(it->second.data(), w, geo);
        }
    }
    for (auto &kv : all) merged.insert(merged.end(), kv.second.begin(), kv.second.end());
    return IMM3_OK;
}

} // namespace

extern "C" int imm3_comm_merge_groups_wide(imm3_comm *c, imm3_query *const *queries, const int32_t *segment_index, int32_t n_queries,
                                           uint8_t *key_bytes_out, uint64_t *first, uint64_t *counts, int64_t *vals,
                                           uint8_t *const *str_out, uint32_t max_groups, uint32_t *n_groups) {
    if (!c || !n_groups || n_queries < 0 || (n_queries > 0 && (!queries || !segment_index))) return fail(IMM3_ERR_ARG, "bad argument");
    imm3::GateScope gate(&c->ctx->gate); // (held across both phases)
    WideLocal L;
    int rc = wide_local(c->ctx, queries, segment_index, n_queries, str_out, c->world == 1, L);
    if (!rc && c->world > 1) rc = wide_exchange(c, L);
    if (rc) return rc;
    unpack_wide(L.recs, L.sp, L.geo, key_bytes_out, first, counts, vals, str_out, max_groups, n_groups);
    return IMM3_OK;
}

// Single-process flavour (comms from imm3_comm_create_all): per device the local phase above, then one merge by byte key on the
// host.
extern "C" int imm3_comm_merge_groups_wide_all(imm3_comm *const *comms, int32_t n_comms, imm3_query *const *const *queries,
                                               const int32_t *const *segment_index, const int32_t *n_queries,
                                               uint8_t *key_bytes_out, uint64_t *first, uint64_t *counts, int64_t *vals,
                                               uint8_t *const *str_out, uint32_t max_groups, uint32_t *n_groups) {
    if (!comms || n_comms < 1 || !queries || !segment_index || !n_queries || !n_groups) return fail(IMM3_ERR_ARG, "bad argument");
    WideSpec sp;
    MergeWideArgs geo;
    std::vector<unsigned long long> merged;
    const int rc = wide_all_records(comms, n_comms, queries, segment_index, n_queries, str_out, sp, geo, merged);
    if (rc) return rc;
    unpack_wide(merged, sp, geo, key_bytes_out, first, counts, vals, str_out, max_groups, n_groups);
    return IMM3_OK;
}

// ---- views of the merged groups (include/imm3.h: imm3_comm_merge_groups_view; DESIGN.md section 21, "Views of merged groups") ----
// The merge above, unchanged, with its final record list left on the device; the view -- filter, then order, then limit -- is computed
// there (imm3_merge_view_api.cpp / .hip) and only its records are copied and unpacked, in list order.
extern "C" int imm3_comm_merge_groups_view(imm3_comm *c, imm3_query *const *queries, const int32_t *segment_index, int32_t n_queries,
                                           const imm3_group_view *view, uint8_t *key_bytes_out, uint64_t *first, uint64_t *counts, int64_t *vals,
                                           uint8_t *const *str_out, uint32_t max_groups, uint32_t *n_groups, uint64_t *n_kept) {
    if (!c || !n_groups || n_queries < 0 || (n_queries > 0 && (!queries || !segment_index))) return fail(IMM3_ERR_ARG, "bad argument");
    imm3::GateScope gate(&c->ctx->gate); // (held across all phases)
    c->view_path = GROUP_ORDER_NONE;
    WideLocal L;
    MergeViewCall view_call;
    WideKeep keep;
    keep.view = &view_call;
    int rc = wide_local(c->ctx, queries, segment_index, n_queries, str_out, false, L);
    if (rc) return rc;
    merge_view_check(queries, segment_index, n_queries, view, view_call, L.verdict); // (behind the queries' own checks: their error comes first)
    if (c->world > 1) rc = wide_exchange(c, L, &keep);
    else {
        rc = merge_local_result(L.verdict, L.step);
        if (!rc) rc = merge_view_agree(c, c->ctx->stream, view_call);
        keep.d_list = L.a1.out_recs;
        keep.n = L.mine;
    }
    if (rc) return rc;
    std::vector<unsigned long long> recs;
    uint64_t n_view = 0, kept = 0;
    rc = merge_view_device(c, view_call, L.geo, keep.d_list, keep.n, max_groups, recs, &n_view, &kept);
    if (rc) return rc;
    uint32_t unpacked = 0;
    unpack_wide(recs, L.sp, L.geo, key_bytes_out, first, counts, vals, str_out, max_groups, &unpacked, true);
    *n_groups = (uint32_t)n_view; // (the groups of the view, also when max_groups is smaller)
    if (n_kept) *n_kept = kept;
    return IMM3_OK;
}

// Single-process flavour: the merge finishes on the host (imm3_comm_merge_groups_wide_all), and so does its view (merge_view_host).
extern "C" int imm3_comm_merge_groups_view_all(imm3_comm *const *comms, int32_t n_comms, imm3_query *const *const *queries,
                                               const int32_t *const *segment_index, const int32_t *n_queries, const imm3_group_view *view,
                                               uint8_t *key_bytes_out, uint64_t *first, uint64_t *counts, int64_t *vals,
                                               uint8_t *const *str_out, uint32_t max_groups, uint32_t *n_groups, uint64_t *n_kept) {
    if (!comms || n_comms < 1 || !queries || !segment_index || !n_queries || !n_groups) return fail(IMM3_ERR_ARG, "bad argument");
    WideSpec sp;
    MergeWideArgs geo;
    std::vector<unsigned long long> merged;
    int rc = wide_all_records(comms, n_comms, queries, segment_index, n_queries, str_out, sp, geo, merged);
    if (rc) return rc;
    MergeViewCall view_call;
    LocalVerdict verdict;
    bool checked = false;
    uint32_t largest = 0;
    for (int32_t i = 0; i < n_comms; ++i) {
        if (n_queries[i] == 0) continue;
        if (!checked) merge_view_check(queries[i], segment_index[i], n_queries[i], view, view_call, verdict); // (every query has passed the merge's checks)
        checked = true;
        for (int32_t k = 0; k < n_queries[i]; ++k) largest = std::max(largest, (uint32_t)segment_index[i][k]);
    }
    if (!checked) { // (no communicator brought a query: the empty result of imm3_comm_merge_groups_wide_all)
        *n_groups = 0;
        if (n_kept) *n_kept = 0;
        return IMM3_OK;
    }
    if (!verdict.ok()) return fail(verdict.rc, verdict.why);
    rc = merge_view_tie(&view_call.plan.layout, largest, &view_call.plan.seg_bytes);
    if (rc) return rc;
    rc = merge_view_check_groups(merged.size() / (size_t)geo.rec_words);
    if (rc) return rc;
    std::vector<unsigned long long> recs;
    uint64_t n_view = 0, kept = 0;
    merge_view_of_host_records(view_call, geo, merged, recs, &n_view, &kept);
    uint32_t unpacked = 0;
    unpack_wide(recs, sp, geo, key_bytes_out, first, counts, vals, str_out, max_groups, &unpacked, true);
    *n_groups = (uint32_t)n_view;
    if (n_kept) *n_kept = kept;
    return IMM3_OK;
}
