// imm3_merge_view_api.cpp -- the host side of imm3_comm_merge_groups_view (include/imm3.h; DESIGN.md section 21, "Views of merged groups"):
// the view's checks against the queries' shape, the ranks' agreement on it, and the launches of imm3_merge_view.hip over the record
// list imm3_merge_wide.cpp leaves on the device.  The entry points themselves sit beside the merge they extend (imm3_merge_wide.cpp).
#include "imm3_api_internal.h"
#include "imm3_comm_internal.h"
#include "../../include/imm3_diag.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

using namespace imm3;

namespace {

int32_t col_kind(const SegCol &sc) { return sc.vcodec == IMM3_DENSE_INT ? KIND_I32 : (sc.vcodec == IMM3_DENSE_TINYINT ? KIND_I8 : KIND_STR); }

// what the checks of the order and of the filter read of an aggregation query (imm3_group_order_api.cpp: query_shape)
struct ViewShape {
    int32_t gk[kMaxGroupCols] = {0}, gw[kMaxGroupCols] = {0}, ak[kMaxAggs] = {0}, ck[kMaxAggs] = {0}, cw[kMaxAggs] = {0};
    GroupOrderShape sh;
    explicit ViewShape(const imm3_query *q) {
        std::memset(&sh, 0, sizeof(sh));
        sh.is_agg = 1;
        sh.n_group = (int32_t)q->group_cols.size();
        sh.n_aggs = (int32_t)q->aggs.size();
        for (size_t g = 0; g < q->group_cols.size() && g < (size_t)kMaxGroupCols; ++g) {
            const SegCol &sc = q->seg->cols[(size_t)q->used[(size_t)q->group_cols[g]]];
            gk[g] = col_kind(sc);
            gw[g] = sc.width;
        }
        for (size_t j = 0; j < q->aggs.size() && j < (size_t)kMaxAggs; ++j) {
            const SegCol &sc = q->seg->cols[(size_t)q->used[(size_t)q->aggs[j].column]];
            ak[j] = q->aggs[j].kind;
            ck[j] = col_kind(sc);
            cw[j] = sc.width;
        }
        sh.group_kind = gk;
        sh.group_width = gw;
        sh.agg_kind = ak;
        sh.agg_col_kind = ck;
        sh.agg_col_width = cw;
    }
};

// the view's workspace: one block of the context's caching allocator, back to it with the scope
struct PoolBlock {
    imm3_ctx *ctx;
    void *p = nullptr;
    explicit PoolBlock(imm3_ctx *c) : ctx(c) {}
    PoolBlock(const PoolBlock &) = delete;
    PoolBlock &operator=(const PoolBlock &) = delete;
    ~PoolBlock() { if (p) pool_release(ctx, p); }
};

void bind_geometry(MergeViewPlan &p, const MergeWideArgs &geo) {
    p.rec_words = geo.rec_words;
    for (int j = 0; j < kMaxAggs; ++j) p.str_off[j] = geo.str_off[j];
}

} // namespace

void imm3::merge_view_check(imm3_query *const *queries, const int32_t *segment_index, int32_t n_queries, const imm3_group_view *view, MergeViewCall &v,
                            LocalVerdict &verdict) {
    std::memset(&v.plan, 0, sizeof(v.plan));
    v.largest_segment = 0;
    if (!verdict.ok()) return;
    if (!view) { verdict.fail(IMM3_ERR_ARG, "imm3_comm_merge_groups_view: view is null"); return; }
    for (int32_t i = 0; i < n_queries; ++i) v.largest_segment = std::max(v.largest_segment, (uint32_t)segment_index[i]);
    const ViewShape shape(queries[0]);
    if (group_order_plan(shape.sh, view->order, view->n_order, &v.plan.layout) != IMM3_OK) { verdict.fail(IMM3_ERR_ARG, imm3_last_error()); return; }
    if (group_filter_plan(shape.sh, view->leaves, view->n_leaves, view->prog, view->n_prog, &v.plan.prog) != IMM3_OK) { verdict.fail(IMM3_ERR_ARG, imm3_last_error()); return; }
    v.plan.limit = view->limit > 0 ? view->limit : 0;
}

int imm3::merge_view_agree(imm3_comm *c, hipStream_t s, MergeViewCall &v) {
    unsigned long long largest = v.largest_segment;
    if (c->world > 1) {
        uint8_t canon[kMergeViewCanonMax];
        const size_t nb = merge_view_canonical(v.plan.layout, v.plan.prog, v.plan.limit, canon, sizeof(canon));
        const LocalVerdict fine;
        int rc = merge_vote(c, s, merge_view_hash(canon, nb), (unsigned long long)nb, fine,
                            "the ranks' views of the merged groups differ (order keys, filter or limit): every rank must bring the same view");
        if (rc) return rc;
        rc = merge_max_word(c, s, (unsigned long long)v.largest_segment, &largest);
        if (rc) return rc;
    }
    return merge_view_tie(&v.plan.layout, (uint32_t)largest, &v.plan.seg_bytes);
}

int imm3::merge_view_device(imm3_comm *c, MergeViewCall &v, const MergeWideArgs &geo, const unsigned long long *d_list, unsigned long long n, uint32_t max_groups,
                            std::vector<unsigned long long> &out, uint64_t *n_view, uint64_t *n_kept) {
    imm3_ctx *ctx = c->ctx;
    hipStream_t s = ctx->stream;
    c->view_path = GROUP_ORDER_NONE;
    out.clear();
    *n_view = *n_kept = 0;
    bind_geometry(v.plan, geo);
    {
        const int rc = merge_view_check_groups(n);
        if (rc) return rc;
    }
    if (!n) { // nothing on the device to order: the host's rule over an empty list
        size_t no = 0, nk = 0;
        merge_view_host(v.plan, nullptr, 0, nullptr, &no, &nk);
        return IMM3_OK;
    }
    const size_t R = (size_t)geo.rec_words;
    const int fv = ctx->filter_variant;
    const bool radix = n > (unsigned long long)kGroupOrderSmall || fv == TV_GROUP_ORDER_RADIX;
    const bool filt = v.plan.prog.n_prog > 0;
    MergeViewArgs a;
    std::memset(&a, 0, sizeof(a));
    a.plan = v.plan;
    a.recs = d_list;
    a.n = (uint32_t)n;
    a.n_out = v.plan.limit > 0 && (unsigned long long)v.plan.limit < n ? (uint32_t)v.plan.limit : (uint32_t)n;
    // ---- the workspace: {ordered records, the two count words}; radix path: {key column, keys x 2, perm x 2, state, counts, diff, tally, map} ----
    auto round16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t dst_bytes = round16((size_t)a.n_out * R * sizeof(unsigned long long)), keycol_bytes = round16((size_t)n * kOrderKeyMaxBytes);
    const size_t keys_bytes = round16((size_t)n * kOrderKeyWords * sizeof(uint32_t)), perm_bytes = round16((size_t)n * sizeof(uint32_t));
    const size_t counts_bytes = (size_t)256 * kOrderWaves * sizeof(uint32_t), diff_bytes = (size_t)kOrderWaves * kOrderKeyWords * sizeof(uint32_t);
    const size_t tally_bytes = (size_t)kOrderWaves * 2 * sizeof(uint32_t), state_bytes = round16(OW_WORDS * sizeof(uint32_t));
    size_t total = dst_bytes + 16;
    if (radix) total += keycol_bytes + 2 * keys_bytes + 2 * perm_bytes + state_bytes + counts_bytes + diff_bytes + tally_bytes + (filt ? perm_bytes : 0);
    PoolBlock ws(ctx);
    HIPCHK(pool_alloc(ctx, &ws.p, total));
    uint8_t *at = (uint8_t *)ws.p;
    auto take = [&](size_t bytes) { uint8_t *p = at; at += bytes; return p; };
    a.dst = (unsigned long long *)take(dst_bytes);
    a.dst_n = (unsigned long long *)take(16);
    a.n_word = a.dst_n + 1;
    uint32_t *d_state = nullptr;
    {
        LaunchTimer t(ctx, 9); // (one record for the whole view: from its first kernel's start to its last one's end)
        if (!radix) {
            launch_merge_view_small(a, s, t.start, t.stop);
        } else {
            OrderArgs o;
            std::memset(&o, 0, sizeof(o));
            a.key_col = take(keycol_bytes);
            for (int b = 0; b < 2; ++b) o.keys[b] = (uint32_t *)take(keys_bytes);
            for (int b = 0; b < 2; ++b) {
                o.perm[b] = (uint32_t *)take(perm_bytes);
                a.perm[b] = o.perm[b];
            }
            d_state = (uint32_t *)take(state_bytes);
            o.state = d_state;
            a.state = d_state;
            o.counts = (uint32_t *)take(counts_bytes);
            o.diff = (uint32_t *)take(diff_bytes);
            o.tally = (uint32_t *)take(tally_bytes);
            if (filt) a.map = (uint32_t *)take(perm_bytes);
            HIPCHK(hipMemsetAsync(d_state, 0, state_bytes, s));
            if (filt) HIPCHK(hipMemsetAsync(a.n_word, 0, sizeof(unsigned long long), s)); // the kept count grows there, one atomic add per wave
            launch_merge_view_keys(a, s, t.start, nullptr);
            o.n_emit = a.n_word;
            o.cap_rows = n;
            o.limit = v.plan.limit;
            o.cols[0].src = a.key_col; // the whole normalised key as ONE string key: bytes as they are, never complemented again
            o.cols[0].width = v.plan.layout.key_bytes;
            o.cols[0].kind = KIND_STR;
            o.n_cols = 1;
            o.key_bytes = v.plan.layout.key_bytes;
            o.key_words = v.plan.layout.key_words;
            o.force_full = fv == TV_ORDER_FULL_SORT ? 1 : (fv == TV_ORDER_SELECT_ALWAYS ? 2 : 0); // (0: the device decides)
            launch_order_keys(o, s, nullptr, nullptr);
            if (o.limit > 0) launch_order_select(o, s, nullptr, nullptr);
            for (int p = o.key_bytes - 1; p >= 0; --p) { // least significant byte first
                o.byte_pos = p;
                launch_order_pass(o, s, nullptr, nullptr);
            }
            launch_merge_view_apply(a, s, nullptr, t.stop);
        }
    }
    HIPCHK(hipGetLastError());
    // {records of the view, records kept}, which of the two radix forms the device took, and -- where their number is known or small --
    // the records themselves, behind ONE synchronisation
    unsigned long long words[2] = {0, 0};
    uint32_t st[OW_WORDS] = {0};
    HIPCHK(hipMemcpyAsync(words, a.dst_n, sizeof(words), hipMemcpyDeviceToHost, s));
    if (radix) HIPCHK(hipMemcpyAsync(st, d_state, sizeof(st), hipMemcpyDeviceToHost, s));
    const size_t most = std::min<size_t>(a.n_out, max_groups);
    const bool eager = !filt || most * R * sizeof(unsigned long long) <= ((size_t)1 << 20);
    out.assign(eager ? most * R : 0, 0ULL);
    if (eager && most) HIPCHK(hipMemcpyAsync(out.data(), a.dst, out.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (words[1] > n || words[0] > a.n_out || words[0] > words[1]) return fail(IMM3_ERR_DEVICE, "the merged view's count words are out of range");
    const size_t got = std::min<size_t>((size_t)words[0], max_groups);
    if (!eager && got) {
        out.assign(got * R, 0ULL);
        HIPCHK(hipMemcpyAsync(out.data(), a.dst, out.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    out.resize(got * R);
    c->view_path = !radix ? GROUP_ORDER_SMALL : (st[OW_SELECT] ? GROUP_ORDER_RADIX_SELECT : GROUP_ORDER_RADIX_FULL);
    *n_view = words[0];
    *n_kept = words[1];
    return IMM3_OK;
}

void imm3::merge_view_of_host_records(MergeViewCall &v, const MergeWideArgs &geo, const std::vector<unsigned long long> &recs, std::vector<unsigned long long> &out,
                                      uint64_t *n_view, uint64_t *n_kept) {
    bind_geometry(v.plan, geo);
    const size_t R = (size_t)geo.rec_words, n = recs.size() / R;
    std::vector<uint32_t> order(n);
    size_t no = 0, nk = 0;
    merge_view_host(v.plan, recs.data(), n, order.data(), &no, &nk);
    out.resize(no * R);
    for (size_t i = 0; i < no; ++i) std::memcpy(out.data() + i * R, recs.data() + (size_t)order[i] * R, R * sizeof(unsigned long long));
    *n_view = no;
    *n_kept = nk;
}

extern "C" int imm3_comm_merge_view_path(const imm3_comm *c, int32_t *path) {
    if (!c || !path) return fail(IMM3_ERR_ARG, "null argument");
    *path = c->view_path;
    return IMM3_OK;
}

// The host-only plan of a view, without a device or a handle (tests hold the tie width, the refusal and the hash against it).
extern "C" int imm3_merge_view_plan_json(int32_t n_group, const int32_t *group_kind, const int32_t *group_width, int32_t n_aggs, const int32_t *agg_kind,
                                         const int32_t *agg_col_kind, const int32_t *agg_col_width, const imm3_group_view *view, uint32_t largest_segment_index,
                                         char *json_out, int64_t cap, int64_t *needed) {
    if (!view || n_group < 0 || n_group > kMaxGroupCols || n_aggs < 0 || n_aggs > kMaxAggs) return fail(IMM3_ERR_ARG, "imm3_merge_view_plan_json: bad argument");
    GroupOrderShape sh;
    std::memset(&sh, 0, sizeof(sh));
    sh.is_agg = 1;
    sh.n_group = n_group;
    sh.n_aggs = n_aggs;
    sh.group_kind = group_kind;
    sh.group_width = group_width;
    sh.agg_kind = agg_kind;
    sh.agg_col_kind = agg_col_kind;
    sh.agg_col_width = agg_col_width;
    MergeViewPlan p;
    std::memset(&p, 0, sizeof(p));
    int rc = group_order_plan(sh, view->order, view->n_order, &p.layout);
    if (rc) return rc;
    rc = group_filter_plan(sh, view->leaves, view->n_leaves, view->prog, view->n_prog, &p.prog);
    if (rc) return rc;
    p.limit = view->limit > 0 ? view->limit : 0;
    uint8_t canon[kMergeViewCanonMax];
    const size_t nb = merge_view_canonical(p.layout, p.prog, p.limit, canon, sizeof(canon));
    rc = merge_view_tie(&p.layout, largest_segment_index, &p.seg_bytes);
    if (rc) return rc;
    char buf[256];
    const int len = std::snprintf(buf, sizeof(buf), "{\"seg_bytes\":%d,\"user_bytes\":%d,\"key_bytes\":%d,\"canonical_bytes\":%zu,\"hash\":\"%016llx\"}", (int)p.seg_bytes,
                                  (int)p.layout.user_bytes, (int)p.layout.key_bytes, nb, (unsigned long long)merge_view_hash(canon, nb));
    if (needed) *needed = len + 1;
    if (cap > 0) {
        if (!json_out || cap < len + 1) return fail(IMM3_ERR_ARG, "imm3_merge_view_plan_json: json_out is too small");
        std::memcpy(json_out, buf, (size_t)len + 1);
    }
    return IMM3_OK;
}
