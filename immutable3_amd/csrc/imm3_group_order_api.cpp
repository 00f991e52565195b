// imm3_group_order_api.cpp -- imm3_query_set_group_order (include/imm3.h): the ordered view of an aggregation's groups.  The order is
// no part of a run: a getter settles the groups as always (imm3_api.cpp: settle_groups), then this file orders the dense arrays on the
// device into arrays of their own (imm3_group_order.hip) and the getters copy the first min(groups, limit) of those to the host.  The
// argument checks and the key layout are imm3_group_order_plan.cpp's.  imm3_query_set_group_filter (HAVING) lives here too: the view is
// filter, then order, then limit, built by the same settle; the program's checks are imm3_group_filter_plan.cpp's.
#include "imm3_api_internal.h"
#include "../../include/imm3_diag.h"

#include <cstring>

using namespace imm3;
static_assert(kGroupOrderSmall == IMM3_GROUP_ORDER_SMALL_MAX, "include/imm3_diag.h names the small path's bound");

namespace {

int32_t packed_key_bytes(const imm3_query *q) {
    int32_t kb = 0;
    for (int32_t g : q->group_cols) kb += q->seg->cols[(size_t)q->used[(size_t)g]].width;
    return kb;
}
const SegCol &agg_col(const imm3_query *q, size_t j) { return q->seg->cols[(size_t)q->used[(size_t)q->aggs[j].column]]; }
bool wide_string_max(const imm3_query *q, size_t j) { return q->d_chunks[j] != nullptr; }
int32_t col_kind(const SegCol &sc) { return sc.vcodec == IMM3_DENSE_INT ? KIND_I32 : (sc.vcodec == IMM3_DENSE_TINYINT ? KIND_I8 : KIND_STR); }

int go_alloc(imm3_query *q, void **out, size_t bytes) {
    void *p = nullptr;
    HIPCHK(pool_alloc(q->ctx, &p, bytes ? bytes : 1));
    q->go_allocs.push_back(p);
    *out = p;
    return IMM3_OK;
}
#define GO_ALLOC(ptr, type, bytes)                          \
    do {                                                    \
        void *p_ = nullptr;                                 \
        const int rc_ = go_alloc(q, &p_, (size_t)(bytes));  \
        if (rc_) return rc_;                                \
        (ptr) = (type)p_;                                   \
    } while (0)

// the ordered arrays for as many groups as the dense arrays hold; the radix path's buffers on first need
int go_ensure(imm3_query *q, bool radix) {
    imm3_ctx *ctx = q->ctx;
    const uint32_t cap = q->out_cap ? q->out_cap : 1u;
    if (q->go_cap != cap) group_order_release(q);
    GroupOrderArgs &a = q->go;
    if (!q->go_cap) {
        const size_t n = cap;
        GO_ALLOC(a.dst_keys, unsigned long long *, n * sizeof(unsigned long long));
        GO_ALLOC(a.dst_first, uint32_t *, n * sizeof(uint32_t));
        GO_ALLOC(a.dst_counts, unsigned long long *, n * sizeof(unsigned long long));
        GO_ALLOC(a.dst_vals, long long *, n * kMaxAggs * sizeof(long long));
        GO_ALLOC(a.dst_n, unsigned long long *, 2 * sizeof(unsigned long long));
        a.n_word = a.dst_n + 1;
        if (q->agg_wide_key) {
            const size_t kb = (size_t)packed_key_bytes(q);
            uint8_t *src = nullptr;
            GO_ALLOC(src, uint8_t *, n * kb);
            a.src_keyb = src;
            GO_ALLOC(a.dst_keyb, uint8_t *, n * kb);
        }
        for (size_t j = 0; j < q->aggs.size(); ++j) {
            if (!wide_string_max(q, j)) continue;
            const size_t w = (size_t)agg_col(q, j).width;
            uint8_t *src = nullptr;
            GO_ALLOC(src, uint8_t *, n * w);
            a.src_str[j] = src;
            GO_ALLOC(a.dst_str[j], uint8_t *, n * w);
        }
        q->go_cap = cap;
    }
    if (radix && !q->go_radix_bufs) {
        const size_t n = cap;
        GO_ALLOC(a.key_col, uint8_t *, n * kOrderKeyMaxBytes);
        for (int b = 0; b < 2; ++b) {
            GO_ALLOC(q->d_go_keys[b], uint32_t *, n * kOrderKeyWords * sizeof(uint32_t));
            GO_ALLOC(q->d_go_perm[b], uint32_t *, n * sizeof(uint32_t));
        }
        GO_ALLOC(q->d_go_state, uint32_t *, OW_WORDS * sizeof(uint32_t));
        HIPCHK(hipMemsetAsync(q->d_go_state, 0, OW_WORDS * sizeof(uint32_t), ctx->stream));
        GO_ALLOC(q->d_go_counts, uint32_t *, (size_t)256 * kOrderWaves * sizeof(uint32_t));
        GO_ALLOC(q->d_go_diff, uint32_t *, (size_t)kOrderWaves * kOrderKeyWords * sizeof(uint32_t));
        GO_ALLOC(q->d_go_tally, uint32_t *, (size_t)kOrderWaves * 2 * sizeof(uint32_t));
        q->go_radix_bufs = true;
    }
    if (radix && q->group_filtered && !q->gf.map) GO_ALLOC(q->gf.map, uint32_t *, (size_t)cap * sizeof(uint32_t));
    return IMM3_OK;
}

} // namespace

void imm3::group_order_release(imm3_query *q) {
    for (void *p : q->go_allocs) pool_release(q->ctx, p); // stream-ordered: an order still in flight finishes before any reuse
    q->go_allocs.clear();
    q->go = GroupOrderArgs{};
    for (int b = 0; b < 2; ++b) q->d_go_keys[b] = q->d_go_perm[b] = nullptr;
    q->d_go_state = q->d_go_counts = q->d_go_diff = q->d_go_tally = nullptr;
    q->go_cap = 0;
    q->go_radix_bufs = false;
    q->gf.map = nullptr;
    q->run.group_order_valid = false;
}

// The view is complete in q->go.dst_*: filter (imm3_query_set_group_filter), then order, then limit -- *n_groups = min(groups kept,
// limit).  Settles the groups first; the dense arrays (and what imm3_comm_merge_groups* read) stay as they are.  A filter without an
// order takes the same two paths with first_row as the whole key: first-seen order comes from the device.
int imm3::group_order_settle(imm3_query *q, uint32_t *n_groups) {
    if (q->run.group_order_valid && q->run.ran_agg) {
        *n_groups = q->go_n_out;
        return IMM3_OK;
    }
    uint32_t n = 0;
    const int rc = query_groups(q, &n);
    if (rc) return rc;
    imm3_ctx *ctx = q->ctx;
    hipStream_t s = ctx->stream;
    const int fv = ctx->filter_variant;
    const bool radix = n > (uint32_t)kGroupOrderSmall || fv == TV_GROUP_ORDER_RADIX;
    {
        const int erc = go_ensure(q, radix);
        if (erc) return erc;
    }
    if (n > q->go_cap) return fail(IMM3_ERR_DEVICE, "more groups than the ordered arrays hold");
    AggArgs aa;
    query_agg_args(q, aa);
    GroupOrderArgs &a = q->go;
    const bool filt = q->group_filtered;
    const int64_t limit = q->group_ordered ? q->group_order_limit : 0; // (the limit belongs to the order)
    a.layout = q->group_ordered ? q->group_order_layout : group_filter_first_seen_layout();
    a.n = n;
    a.n_out = limit > 0 && (uint64_t)limit < (uint64_t)n ? (uint32_t)limit : n;
    a.n_agg = (int32_t)q->aggs.size();
    a.key_bytes = packed_key_bytes(q);
    a.wide_key = q->agg_wide_key ? 1 : 0;
    a.src_keys = q->d_okeys;
    a.src_first = q->d_ofirst;
    a.src_counts = q->d_ocounts;
    a.src_vals = q->d_ovals;
    if (q->agg_wide_key && n) launch_group_keys(aa, n, a.key_bytes, const_cast<uint8_t *>(a.src_keyb), s);
    for (size_t j = 0; j < q->aggs.size(); ++j) {
        a.str_width[j] = wide_string_max(q, j) ? agg_col(q, j).width : 0;
        if (a.str_width[j] && n) launch_strmax_collect(aa, (int)j, n, const_cast<uint8_t *>(a.src_str[j]), s);
    }
    HIPCHK(hipGetLastError());
    int32_t path = GROUP_ORDER_SMALL;
    {
        LaunchTimer t(ctx, 8); // (one record for the whole order: from its first kernel's start to its last one's end)
        if (!radix) {
            if (filt) launch_group_order_small_filtered(a, q->gf, s, t.start, t.stop);
            else launch_group_order_small(a, s, t.start, t.stop);
        } else {
            if (filt) { // the kept count grows in n_word, one atomic add per wave
                HIPCHK(hipMemsetAsync(a.n_word, 0, sizeof(unsigned long long), s));
                launch_group_order_keys_filtered(a, q->gf, s, t.start, nullptr);
            } else launch_group_order_keys(a, s, t.start, nullptr);
            OrderArgs o;
            std::memset(&o, 0, sizeof(o));
            o.n_emit = a.n_word;
            o.cap_rows = q->go_cap;
            o.limit = limit > 0 ? limit : 0;
            o.cols[0].src = a.key_col; // the whole normalised key as ONE string key: bytes as they are, never complemented again
            o.cols[0].width = a.layout.key_bytes;
            o.cols[0].kind = KIND_STR;
            o.n_cols = 1;
            o.key_bytes = a.layout.key_bytes;
            o.key_words = a.layout.key_words;
            o.force_full = fv == TV_ORDER_FULL_SORT ? 1 : (fv == TV_ORDER_SELECT_ALWAYS ? 2 : 0); // (0: the device decides)
            for (int b = 0; b < 2; ++b) {
                o.keys[b] = q->d_go_keys[b];
                o.perm[b] = q->d_go_perm[b];
                a.perm[b] = q->d_go_perm[b];
            }
            o.state = q->d_go_state;
            a.state = q->d_go_state;
            o.counts = q->d_go_counts;
            o.diff = q->d_go_diff;
            o.tally = q->d_go_tally;
            launch_order_keys(o, s, nullptr, nullptr);
            if (o.limit > 0) launch_order_select(o, s, nullptr, nullptr);
            for (int p = o.key_bytes - 1; p >= 0; --p) { // least significant byte first
                o.byte_pos = p;
                launch_order_pass(o, s, nullptr, nullptr);
            }
            if (filt) launch_group_order_apply_filtered(a, q->gf, s, nullptr, t.stop);
            else launch_group_order_apply(a, s, nullptr, t.stop);
        }
    }
    HIPCHK(hipGetLastError());
    unsigned long long words[2] = {a.n_out, n}; // {groups of the view, groups kept}: a filtered settle reads them back in one copy
    uint32_t st[OW_WORDS] = {0};
    if (filt) HIPCHK(hipMemcpyAsync(words, a.dst_n, sizeof(words), hipMemcpyDeviceToHost, s));
    if (radix) HIPCHK(hipMemcpyAsync(st, q->d_go_state, sizeof(st), hipMemcpyDeviceToHost, s)); // which of the two the device took
    if (filt || radix) HIPCHK(hipStreamSynchronize(s));
    if (radix) path = st[OW_SELECT] ? GROUP_ORDER_RADIX_SELECT : GROUP_ORDER_RADIX_FULL;
    if (filt && (words[1] > n || words[0] > a.n_out || words[0] > words[1])) return fail(IMM3_ERR_DEVICE, "the group filter's count words are out of range");
    q->go_path = path;
    q->go_n_out = (uint32_t)words[0];
    q->gf_groups_in = filt ? n : 0;
    q->gf_groups_kept = filt ? words[1] : 0;
    q->run.group_order_valid = true;
    *n_groups = q->go_n_out;
    return IMM3_OK;
}

int imm3::group_order_fetch_groups(imm3_query *q, uint64_t *keys, uint32_t *first_row, uint64_t *counts, int64_t *vals, uint32_t max_groups) {
    uint32_t n = 0;
    const int rc = group_order_settle(q, &n);
    if (rc) return rc;
    const size_t m = std::min(n, max_groups), kb = (size_t)packed_key_bytes(q), na = q->aggs.size();
    const GroupOrderArgs &a = q->go;
    const bool wide = q->agg_wide_key && keys;
    std::vector<unsigned long long> hk(m), hc(m);
    std::vector<uint32_t> hf(m);
    std::vector<long long> hv(m * kMaxAggs);
    std::vector<uint8_t> wk(wide ? m * kb : 0);
    hipStream_t s = q->ctx->stream;
    if (m) {
        HIPCHK(hipMemcpyAsync(hk.data(), a.dst_keys, m * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hf.data(), a.dst_first, m * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hc.data(), a.dst_counts, m * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hv.data(), a.dst_vals, m * kMaxAggs * sizeof(long long), hipMemcpyDeviceToHost, s));
        if (wide) HIPCHK(hipMemcpyAsync(wk.data(), a.dst_keyb, wk.size(), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    for (size_t o = 0; o < m; ++o) {
        if (wide) { // the first 8 bytes of the key, little-endian (the table holds tags)
            uint64_t k = 0;
            for (size_t b = 0; b < 8 && b < kb; ++b) k |= (uint64_t)wk[o * kb + b] << (8 * b);
            keys[o] = k;
        } else if (keys) keys[o] = hk[o];
        if (first_row) first_row[o] = hf[o];
        if (counts) counts[o] = hc[o];
        if (vals)
            for (size_t j = 0; j < na; ++j) vals[o * na + j] = q->aggs[j].kind == IMM3_AGG_COUNT ? (int64_t)hc[o] : (int64_t)hv[o * kMaxAggs + j];
    }
    return IMM3_OK;
}

int imm3::group_order_fetch_strings(imm3_query *q, int32_t agg, uint8_t *out, uint32_t max_groups) {
    uint32_t n = 0;
    const int rc = group_order_settle(q, &n);
    if (rc) return rc;
    const size_t m = std::min(n, max_groups), w = (size_t)agg_col(q, (size_t)agg).width;
    if (!m) return IMM3_OK;
    hipStream_t s = q->ctx->stream;
    if (wide_string_max(q, (size_t)agg)) {
        HIPCHK(hipMemcpyAsync(out, q->go.dst_str[agg], m * w, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return IMM3_OK;
    }
    std::vector<long long> hv(m * kMaxAggs);
    HIPCHK(hipMemcpyAsync(hv.data(), q->go.dst_vals, hv.size() * sizeof(long long), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (size_t o = 0; o < m; ++o) { // (<= 8 bytes: the value packed big-endian)
        const unsigned long long v = (unsigned long long)hv[o * kMaxAggs + (size_t)agg];
        for (size_t b = 0; b < w; ++b) out[o * w + b] = (uint8_t)(v >> (8 * (w - 1 - b)));
    }
    return IMM3_OK;
}

int imm3::group_order_fetch_keys(imm3_query *q, uint8_t *out, uint32_t max_groups) {
    uint32_t n = 0;
    const int rc = group_order_settle(q, &n);
    if (rc) return rc;
    const size_t m = std::min(n, max_groups), kb = (size_t)packed_key_bytes(q);
    if (!m || !kb) return IMM3_OK;
    hipStream_t s = q->ctx->stream;
    if (q->agg_wide_key) {
        HIPCHK(hipMemcpyAsync(out, q->go.dst_keyb, m * kb, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return IMM3_OK;
    }
    std::vector<unsigned long long> hk(m);
    HIPCHK(hipMemcpyAsync(hk.data(), q->go.dst_keys, m * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (size_t o = 0; o < m; ++o) // (<= 8 bytes: the u64 key, little-endian)
        for (size_t b = 0; b < kb; ++b) out[o * kb + b] = (uint8_t)(hk[o] >> (8 * b));
    return IMM3_OK;
}

namespace {
// what the checks of the order and of the filter read of a query; the arrays are the caller's
struct ShapeArrays {
    int32_t gk[kMaxGroupCols] = {0}, gw[kMaxGroupCols] = {0}, ak[kMaxAggs] = {0}, ck[kMaxAggs] = {0}, cw[kMaxAggs] = {0};
};
void query_shape(const imm3_query *q, ShapeArrays &arr, GroupOrderShape &sh) {
    int32_t *gk = arr.gk, *gw = arr.gw, *ak = arr.ak, *ck = arr.ck, *cw = arr.cw;
    std::memset(&sh, 0, sizeof(sh));
    sh.is_agg = q->is_agg ? 1 : 0;
    if (q->is_agg) {
        sh.n_group = (int32_t)q->group_cols.size();
        sh.n_aggs = (int32_t)q->aggs.size();
        for (size_t g = 0; g < q->group_cols.size() && g < (size_t)kMaxGroupCols; ++g) {
            const SegCol &sc = q->seg->cols[(size_t)q->used[(size_t)q->group_cols[g]]];
            gk[g] = col_kind(sc);
            gw[g] = sc.width;
        }
        for (size_t j = 0; j < q->aggs.size() && j < (size_t)kMaxAggs; ++j) {
            ak[j] = q->aggs[j].kind;
            ck[j] = col_kind(agg_col(q, j));
            cw[j] = agg_col(q, j).width;
        }
    }
    sh.group_kind = gk;
    sh.group_width = gw;
    sh.agg_kind = ak;
    sh.agg_col_kind = ck;
    sh.agg_col_width = cw;
}
} // namespace

extern "C" int imm3_query_set_group_order(imm3_query *q, const imm3_group_order_key *keys, int32_t n_keys, int64_t limit) {
    if (!q) return fail(IMM3_ERR_ARG, "query is null");
    CTX_LIVE(q->ctx);
    ShapeArrays arr;
    GroupOrderShape sh;
    query_shape(q, arr, sh);
    GroupOrderLayout layout;
    const int rc = group_order_plan(sh, keys, n_keys, &layout);
    if (rc) return rc;
    q->group_order_keys.assign(keys, keys + n_keys);
    q->group_order_limit = limit > 0 ? limit : 0;
    q->group_order_layout = layout;
    q->group_ordered = n_keys > 0;
    q->run.group_order_valid = false;
    return IMM3_OK;
}

extern "C" int imm3_query_group_order_path(const imm3_query *q, int32_t *path) {
    if (!q || !path) return fail(IMM3_ERR_ARG, "null argument");
    if (!q->is_agg) return fail(IMM3_ERR_ARG, "not an aggregation query");
    *path = (q->group_ordered || q->group_filtered) && q->run.group_order_valid ? q->go_path : GROUP_ORDER_NONE;
    return IMM3_OK;
}

extern "C" int imm3_query_set_group_filter(imm3_query *q, const imm3_group_filter_leaf *leaves, int32_t n_leaves, const int32_t *prog, int32_t n_prog) {
    if (!q) return fail(IMM3_ERR_ARG, "imm3_query_set_group_filter: query is null");
    CTX_LIVE(q->ctx);
    ShapeArrays arr;
    GroupOrderShape sh;
    query_shape(q, arr, sh);
    GroupFilterProg fp;
    const int rc = group_filter_plan(sh, leaves, n_leaves, prog, n_prog, &fp);
    if (rc) return rc;
    q->gf.prog = fp;
    q->group_filtered = fp.n_prog > 0;
    q->gf_groups_in = q->gf_groups_kept = 0;
    q->run.group_order_valid = false;
    return IMM3_OK;
}

extern "C" int imm3_query_group_filter_stats(const imm3_query *q, uint64_t *groups_in, uint64_t *groups_kept) {
    if (!q || !groups_in || !groups_kept) return fail(IMM3_ERR_ARG, "null argument");
    if (!q->is_agg) return fail(IMM3_ERR_ARG, "not an aggregation query");
    const bool live = q->group_filtered && q->run.group_order_valid && q->run.ran_agg;
    *groups_in = live ? q->gf_groups_in : 0;
    *groups_kept = live ? q->gf_groups_kept : 0;
    return IMM3_OK;
}

extern "C" int imm3_group_filter_check(int32_t is_agg, const int32_t *agg_kind, const int32_t *agg_col_kind, int32_t n_aggs, const imm3_group_filter_leaf *leaves,
                                       int32_t n_leaves, const int32_t *prog, int32_t n_prog, const int64_t *count_vals, int32_t *kept) {
    if (n_aggs < 0 || n_aggs > kMaxAggs || (n_aggs > 0 && (!agg_kind || !agg_col_kind))) return fail(IMM3_ERR_ARG, "imm3_group_filter_check: bad aggregates");
    GroupOrderShape sh;
    std::memset(&sh, 0, sizeof(sh));
    sh.is_agg = is_agg ? 1 : 0;
    sh.n_aggs = n_aggs;
    sh.agg_kind = agg_kind;
    sh.agg_col_kind = agg_col_kind;
    GroupFilterProg fp;
    const int rc = group_filter_plan(sh, leaves, n_leaves, prog, n_prog, &fp);
    if (rc) return rc;
    if (count_vals) {
        if (!kept) return fail(IMM3_ERR_ARG, "imm3_group_filter_check: kept is null");
        *kept = group_filter_eval(fp, (unsigned long long)count_vals[0], count_vals + 1) ? 1 : 0;
    }
    return IMM3_OK;
}
