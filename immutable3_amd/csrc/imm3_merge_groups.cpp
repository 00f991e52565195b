// imm3_merge_groups.cpp -- imm3_comm_merge_groups and its single-process flavour.
//
// Cross-segment / cross-GPU merge of group tables: ProjectAggregateQueueOp
// (engine/src/main/scala/immutabledb/engine/operator/ProjectAggregateQueue.scala:9-55) merges the per-segment maps by key --
// counts add, max / min combine, the first arrival keeps its place (here: ascending segment index, then first row).  Every
// rank brings the group tables of its own segments' aggregation queries; every rank gets the merged table.
//   keys of <= 2 bytes : the groups are scattered into a direct-indexed device table (k_merge_scatter) and the ranks' tables
//                        meet in element-wise all-reduces: sum on the counts, min on `segment << 32 | first row`, max / min
//                        on each aggregate -- no host work but the final compaction of the occupied slots;
//   wider keys         : merged by key ON THE DEVICE: this rank's queries' lists go into a hash table (compare-and-swap on the
//                        key, atomic add / min / max on the columns), its occupied slots come out as a packed list, the ranks'
//                        (locally merged) lists are exchanged with ncclAllGather -- fixed-size slots, sized by an
//                        all-reduce(max) of the list lengths -- and merged the same way.  The host only sorts the result by
//                        first arrival.
// The local phase (groups_local) is this rank's part and holds no collective; the exchange (groups_exchange) is built from the
// protocol of imm3_comm_internal.h and runs only with more than one rank.
#include "imm3_comm_internal.h"

#include <algorithm>
#include <cstring>
#include <map>

using namespace imm3;

void imm3::merge_check_agg_queries(imm3_query *const *queries, int32_t n, LocalVerdict &verdict) {
    for (int32_t i = 0; i < n; ++i) {
        imm3_query *q = queries[i], *q0 = queries[0];
        if (!q) return verdict.fail(IMM3_ERR_ARG, "query is null");
        if (!q->is_agg) return verdict.fail(IMM3_ERR_ARG, "not an aggregation query");
        if (!q->run.ran_agg) return verdict.fail(IMM3_ERR_STATE, "imm3_query_run has not been called");
        bool same = q->aggs.size() == q0->aggs.size() && q->group_cols.size() == q0->group_cols.size();
        for (size_t j = 0; same && j < q->aggs.size(); ++j) same = q->aggs[j].kind == q0->aggs[j].kind;
        if (!same) return verdict.fail(IMM3_ERR_ARG, "the queries aggregate differently");
        // Counts of distinct values do not add, and a merge sees the figures, not the sets.  Refused HERE, before the kinds are packed
        // into the vote's two bits each: the verdict travels through the vote like any other, and no rank is left in a collective.
        // OUT OF SCOPE: a getter for the sets themselves, and with it exact merges across queries and ranks
        for (size_t j = 0; j < q->aggs.size(); ++j)
            if (q->aggs[j].kind == IMM3_AGG_COUNT_DISTINCT)
                return verdict.fail(IMM3_ERR_ARG, "aggregate " + std::to_string(j) + " is a COUNT_DISTINCT: counts of distinct values do not add, so a merge of groups refuses the query");
    }
    if (n == 0) verdict.fail(IMM3_ERR_ARG, "a rank joins the merge with at least one aggregation query (the aggregates' kinds come from it)");
}

namespace {

// (hash path: this rank's entries must leave room for a table of twice their number + 1 slots in the kernels' 32-bit slot fields)
constexpr unsigned long long kMaxMergeEntries = 1ULL << 30;

struct MergedGroup {
    unsigned long long key, first, count;
    long long vals[kMaxAggs];
};

// what the local phase leaves: the verdicts, the shape, and this rank's merged groups -- on the device (`a` over `block`: the
// direct table of keys <= 2 bytes, else the hash table whose packed list holds `mine` entries) or, as the final result, in `merged`
struct GroupsLocal {
    LocalVerdict verdict;
    LocalStep step;
    int key_bytes = 0, n_agg = 0;
    int32_t kinds[kMaxAggs] = {0, 0, 0, 0}, is_str[kMaxAggs] = {0, 0, 0, 0};
    DeviceBlock block;
    MergeArgs a;
    uint32_t K = 1; // slots of the direct table
    unsigned long long mine = 0;
    std::vector<MergedGroup> merged;
    bool direct() const { return key_bytes <= 2; }
    size_t direct_words() const { return (size_t)K * (2 + kMaxAggs); }
};

void combine(MergedGroup &into, const MergedGroup &g, const int32_t *kinds, const int32_t *is_str, int n_agg) {
    into.count += g.count;
    into.first = std::min(into.first, g.first);
    for (int j = 0; j < n_agg; ++j) {
        if (kinds[j] == AGG_MAX) {
            if (is_str[j]) into.vals[j] = (long long)std::max((unsigned long long)into.vals[j], (unsigned long long)g.vals[j]);
            else into.vals[j] = std::max(into.vals[j], g.vals[j]);
        } else if (kinds[j] == AGG_MIN) into.vals[j] = std::min(into.vals[j], g.vals[j]);
        else if (kinds[j] == AGG_SUM) into.vals[j] += g.vals[j];
    }
}

// the hash table's one allocation: {keys, counts, first, vals[kMaxAggs]} x slots, then the packed list and its counter
size_t hash_bytes(unsigned long long slots, unsigned long long list_cap) {
    return (size_t)((slots * (3 + kMaxAggs) + list_cap * kMergeListWords + 8) * sizeof(unsigned long long));
}
void hash_bind(MergeArgs &a, const GroupsLocal &L, void *p, unsigned long long cap, unsigned long long list_cap) {
    std::memset(&a, 0, sizeof(a));
    a.mask = (uint32_t)(cap - 1);
    a.slots = (uint32_t)(cap + 1); // (+ the slot of the one key that equals the empty marker)
    a.t_keys = (unsigned long long *)p;
    a.t_counts = a.t_keys + a.slots;
    a.t_first = a.t_counts + a.slots;
    a.t_vals = (long long *)(a.t_first + a.slots);
    a.out_list = (unsigned long long *)(a.t_vals + (size_t)kMaxAggs * a.slots);
    a.out_n = a.out_list + list_cap * kMergeListWords;
    a.out_cap = (uint32_t)list_cap;
    a.n_agg = L.n_agg;
    for (int j = 0; j < kMaxAggs; ++j) { a.kinds[j] = L.kinds[j]; a.is_str[j] = L.is_str[j]; }
}
void direct_bind(MergeArgs &a, const GroupsLocal &L, void *p) {
    std::memset(&a, 0, sizeof(a));
    a.slots = L.K;
    a.t_counts = (unsigned long long *)p;
    a.t_first = a.t_counts + L.K;
    a.t_vals = (long long *)(a.t_first + L.K);
    a.n_agg = L.n_agg;
    for (int j = 0; j < kMaxAggs; ++j) { a.kinds[j] = L.kinds[j]; a.is_str[j] = L.is_str[j]; }
}

// the occupied slots of the direct table (after the all-reduces, with more than one rank) -> merged
int read_direct(GroupsLocal &L, hipStream_t s) {
    const uint32_t K = L.K;
    std::vector<unsigned long long> h(L.direct_words());
    HIPCHK(hipMemcpyAsync(h.data(), L.block.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (uint32_t k = 0; k < K; ++k) {
        if (!h[k]) continue;
        MergedGroup g;
        g.key = k;
        g.count = h[k];
        g.first = h[(size_t)K + k];
        for (int j = 0; j < kMaxAggs; ++j) g.vals[j] = (long long)h[(size_t)K * (2 + j) + k];
        L.merged.push_back(g);
    }
    return IMM3_OK;
}

// a packed list of n entries -> merged (empty before).  An entry of the list -- key, first, count, kMaxAggs values -- IS a MergedGroup,
// so the list is copied straight into the vector.
static_assert(sizeof(MergedGroup) == kMergeListWords * sizeof(unsigned long long), "MergedGroup must be the packed list's entry");
int read_list(const unsigned long long *d_list, unsigned long long n, hipStream_t s, std::vector<MergedGroup> &merged) {
    merged.resize((size_t)n);
    if (n) HIPCHK(hipMemcpyAsync(merged.data(), d_list, (size_t)n * sizeof(MergedGroup), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return IMM3_OK;
}

// merged groups (any order) -> the caller's arrays, ascending first arrival
void write_groups(std::vector<MergedGroup> &merged, int n_agg, const int32_t *kinds, uint64_t *keys, uint64_t *first, uint64_t *counts, int64_t *vals,
                  uint32_t max_groups, uint32_t *n_groups) {
    std::sort(merged.begin(), merged.end(), [](const MergedGroup &x, const MergedGroup &y) { return x.first < y.first; }); // first arrival first
    *n_groups = (uint32_t)merged.size();
    for (size_t o = 0; o < merged.size() && o < max_groups; ++o) {
        if (keys) keys[o] = merged[o].key;
        if (first) first[o] = merged[o].first;
        if (counts) counts[o] = merged[o].count;
        if (vals)
            for (int j = 0; j < n_agg; ++j) vals[o * (size_t)n_agg + (size_t)j] = kinds[j] == AGG_COUNT ? (int64_t)merged[o].count : (int64_t)merged[o].vals[j];
    }
}

// This rank's part: the checks into the verdict, the queries' groups merged into one device table.  Returns non-zero when the call
// ends here -- a context that cannot be used (before anything collective), or, with `to_host`, whatever went wrong: the caller
// then meets no other rank, and the result is in L.merged.
int groups_local(imm3_ctx *ctx, imm3_query *const *queries, const int32_t *segment_index, int32_t n_queries, bool to_host, GroupsLocal &L) {
    imm3::GateScope gate(&ctx->gate);
    if (ctx->closed) return fail(IMM3_ERR_STATE, "the context of this communicator has been destroyed");
    if (ctx->capture) return fail(IMM3_ERR_STATE, "a graph capture is open on this context");
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    LocalVerdict &verdict = L.verdict;
    merge_check_agg_queries(queries, n_queries, verdict);
    std::vector<uint32_t> n_local((size_t)std::max(n_queries, 0), 0u); // groups of each query (its dense list is complete in q->d_o*)
    unsigned long long total_local = 0;
    if (verdict.ok()) {
        imm3_query *q0 = queries[0];
        for (int32_t g : q0->group_cols) L.key_bytes += q0->seg->cols[(size_t)q0->used[(size_t)g]].width;
        L.n_agg = (int)q0->aggs.size();
        for (int j = 0; j < L.n_agg; ++j) {
            L.kinds[j] = q0->aggs[j].kind;
            L.is_str[j] = q0->seg->cols[(size_t)q0->used[(size_t)q0->aggs[j].column]].vcodec == IMM3_DENSE_STRING;
        }
        for (int32_t i = 0; i < n_queries && verdict.ok(); ++i) // (... and u64 keys: never a wide key's prefix)
            if (queries[i]->agg_wide_key) verdict.fail(IMM3_ERR_ARG, "a group key wider than 8 bytes cannot be merged (imm3_query_fetch_group_keys gives each query's keys)");
        for (int32_t i = 0; i < n_queries && verdict.ok(); ++i) // (the tables below hold 8 bytes per value: never a wide value's prefix)
            for (int32_t j = 0; j < (int32_t)queries[i]->aggs.size() && verdict.ok(); ++j)
                if (queries[i]->d_chunks[j]) verdict.fail(IMM3_ERR_ARG, "a MAX over a STRING column wider than 8 bytes cannot be merged (imm3_query_fetch_group_strings gives each query's values)");
        for (int32_t i = 0; i < n_queries && verdict.ok(); ++i) {
            if (queries[i]->ctx != ctx) { verdict.fail(IMM3_ERR_ARG, "the query runs on another context than the communicator"); break; }
            const int grc = query_groups(queries[i], &n_local[(size_t)i]);
            if (grc) verdict.fail(grc, imm3_last_error());
            total_local += n_local[(size_t)i];
        }
        if (!L.direct() && total_local > kMaxMergeEntries) verdict.fail(IMM3_ERR_ARG, "too many groups to merge");
    }
    if (verdict.ok()) {
        LocalStep &step = L.step;
        if (L.direct()) {
            L.K = L.key_bytes == 0 ? 1u : (L.key_bytes == 1 ? 256u : 65536u);
            const hipError_t e = L.block.alloc(L.direct_words() * sizeof(unsigned long long));
            if (e != hipSuccess) step.refuse(std::string("hipMalloc of the merge table: ") + hipGetErrorString(e));
            else direct_bind(L.a, L, L.block.p);
        } else {
            // (the table of the LOCAL merge is sized from counts every rank already has)
            const unsigned long long list1 = std::max<unsigned long long>(total_local, 1), cap1 = pow2_at_least(2 * list1);
            if (L.block.alloc(hash_bytes(cap1 + 1, list1)) != hipSuccess) step.refuse("hipMalloc of the merge table failed");
            else hash_bind(L.a, L, L.block.p, cap1, list1);
        }
        MergeArgs &a = L.a;
        if (step.ok) {
            launch_merge_init(a, s);
            step(hipGetLastError(), "merge table init");
        }
        for (int32_t i = 0; i < n_queries && step.ok; ++i) {
            imm3_query *q = queries[i];
            a.keys = q->d_okeys;
            a.first = q->d_ofirst;
            a.counts = q->d_ocounts;
            a.vals = q->d_ovals;
            a.n_groups = n_local[(size_t)i];
            a.seg_hi = (unsigned long long)(uint32_t)segment_index[i] << 32;
            if (a.n_groups) launch_merge_scatter(a, s);
            step(hipGetLastError(), "merge scatter");
        }
        if (!L.direct() && step.ok) {
            launch_merge_collect_list(a, s);
            step(hipGetLastError(), "merge collect");
            if (step.ok) step(hipMemcpyAsync(&L.mine, a.out_n, sizeof(L.mine), hipMemcpyDeviceToHost, s), "merge list length");
            if (step.ok) step(hipStreamSynchronize(s), "merge list length");
        }
        // (the direct table has no list-length exchange behind it: what went wrong on the device travels with the vote)
        if (L.direct() && !step.ok) verdict.fail(IMM3_ERR_DEVICE, step.why);
    }
    if (!to_host) return IMM3_OK;
    const int rc = merge_local_result(verdict, L.step);
    if (rc) return rc;
    return L.direct() ? read_direct(L, s) : read_list(L.a.out_list, L.mine, s, L.merged);
}

// The ranks' tables into one, on every rank: L.merged.
int groups_exchange(imm3_comm *c, GroupsLocal &L) {
    hipStream_t s = c->ctx->stream;
    // (the reduced words are not compared with this rank's own once more: max == min means every rank, this one included, sent them)
    int rc = merge_vote(c, s, (unsigned long long)L.key_bytes, (unsigned long long)L.n_agg, L.verdict, "the ranks' aggregation queries differ in key width or number of aggregates");
    if (rc) return rc;
    if (L.direct()) { // ---- direct table + element-wise all-reduces ----
        const MergeArgs &a = L.a;
        const uint32_t K = L.K;
        NCCLCHK(g_rccl.AllReduce(a.t_counts, a.t_counts, K, ncclUint64, ncclSum, c->nccl, s));
        NCCLCHK(g_rccl.AllReduce(a.t_first, a.t_first, K, ncclUint64, ncclMin, c->nccl, s));
        for (int j = 0; j < L.n_agg; ++j) {
            long long *t = a.t_vals + (size_t)j * K;
            if (L.kinds[j] == AGG_MAX) NCCLCHK(g_rccl.AllReduce(t, t, K, L.is_str[j] ? ncclUint64 : ncclInt64, ncclMax, c->nccl, s));
            else if (L.kinds[j] == AGG_MIN) NCCLCHK(g_rccl.AllReduce(t, t, K, ncclInt64, ncclMin, c->nccl, s));
            else if (L.kinds[j] == AGG_SUM) NCCLCHK(g_rccl.AllReduce(t, t, K, ncclInt64, ncclSum, c->nccl, s));
        }
        return read_direct(L, s);
    }
    // ---- hash lists: the common slot count, the exchange buffers, the gather, the second table ----
    unsigned long long most = 0;
    rc = merge_list_length(c, s, L.step, L.mine, "a rank could not build its merge table; no rank has merged anything", &most);
    if (rc) return rc;
    const size_t per_rank = (size_t)most * kMergeListWords;
    if (!per_rank) return IMM3_OK;
    const unsigned long long entries = most * (unsigned long long)c->world;
    if (entries > kMaxMergeEntries) return fail(IMM3_ERR_ARG, "too many groups to merge"); // (the same figure on every rank: every rank leaves here)
    const unsigned long long cap2 = pow2_at_least(2 * entries);
    DeviceBlock x; // {send slot, the ranks' slots, second table}
    rc = merge_exchange_alloc(c, s, (per_rank + per_rank * (size_t)c->world) * sizeof(unsigned long long) + hash_bytes(cap2 + 1, entries), x);
    if (rc) return rc;
    unsigned long long *d_send = (unsigned long long *)x.p, *d_recv = d_send + per_rank;
    rc = merge_gather(c, s, d_send, d_recv, per_rank, nullptr, L.a.out_list, (size_t)L.mine * kMergeListWords * sizeof(unsigned long long));
    if (rc) return rc;
    MergeArgs a2;
    hash_bind(a2, L, d_recv + per_rank * (size_t)c->world, cap2, entries);
    launch_merge_init(a2, s);
    HIPCHK(hipGetLastError());
    a2.list = d_recv;
    a2.n_groups = (uint32_t)entries;
    launch_merge_insert_list(a2, s);
    HIPCHK(hipGetLastError());
    launch_merge_collect_list(a2, s);
    HIPCHK(hipGetLastError());
    unsigned long long n2 = 0;
    HIPCHK(hipMemcpyAsync(&n2, a2.out_n, sizeof(n2), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return read_list(a2.out_list, n2, s, L.merged);
}

} // namespace

extern "C" int imm3_comm_merge_groups(imm3_comm *c, imm3_query *const *queries, const int32_t *segment_index, int32_t n_queries,
                                      uint64_t *keys, uint64_t *first, uint64_t *counts, int64_t *vals, uint32_t max_groups, uint32_t *n_groups) {
    if (!c || !n_groups || n_queries < 0 || (n_queries > 0 && (!queries || !segment_index))) return fail(IMM3_ERR_ARG, "bad argument");
    imm3::GateScope gate(&c->ctx->gate); // (held across both phases)
    GroupsLocal L;
    int rc = groups_local(c->ctx, queries, segment_index, n_queries, c->world == 1, L);
    if (!rc && c->world > 1) rc = groups_exchange(c, L);
    if (rc) return rc;
    write_groups(L.merged, L.n_agg, L.kinds, keys, first, counts, vals, max_groups, n_groups);
    return IMM3_OK;
}

// Single-process flavour (one JVM, every GPU: comms from imm3_comm_create_all): the group tables of all devices are in this
// process, so they are merged here -- per device the local phase above (no collective), then one merge by key on the host; the
// tables are a few KB.  comms[i] brings queries[i][0 .. n_queries[i]) with segment_index[i][...].
extern "C" int imm3_comm_merge_groups_all(imm3_comm *const *comms, int32_t n_comms, imm3_query *const *const *queries,
                                          const int32_t *const *segment_index, const int32_t *n_queries,
                                          uint64_t *keys, uint64_t *first, uint64_t *counts, int64_t *vals, uint32_t max_groups, uint32_t *n_groups) {
    if (!comms || n_comms < 1 || !queries || !segment_index || !n_queries || !n_groups) return fail(IMM3_ERR_ARG, "bad argument");
    int n_agg = -1;
    int32_t kinds[kMaxAggs] = {0, 0, 0, 0}, is_str[kMaxAggs] = {0, 0, 0, 0};
    std::map<unsigned long long, MergedGroup> all;
    for (int32_t i = 0; i < n_comms; ++i) {
        if (!comms[i] || n_queries[i] < 0 || (n_queries[i] > 0 && (!queries[i] || !segment_index[i]))) return fail(IMM3_ERR_ARG, "bad argument");
        if (n_queries[i] == 0) continue;
        GroupsLocal L;
        const int rc = groups_local(comms[i]->ctx, queries[i], segment_index[i], n_queries[i], true, L);
        if (rc) return rc;
        if (n_agg < 0) {
            n_agg = L.n_agg;
            std::copy(L.kinds, L.kinds + kMaxAggs, kinds);
            std::copy(L.is_str, L.is_str + kMaxAggs, is_str);
        } else if (L.n_agg != n_agg) return fail(IMM3_ERR_ARG, "the devices' aggregation queries differ");
        for (const MergedGroup &m : L.merged) {
            auto it = all.find(m.key);
            if (it == all.end()) all.emplace(m.key, m);
            else combine(it->second, m, kinds, is_str, n_agg);
        }
    }
    std::vector<MergedGroup> merged;
    for (auto &kv : all) merged.push_back(kv.second);
    write_groups(merged, n_agg, kinds, keys, first, counts, vals, max_groups, n_groups);
    return IMM3_OK;
}
