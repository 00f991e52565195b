// The two host-only units of a view of merged groups on their own (immutable3_amd/csrc/imm3_merge_view_plan.{h,cpp} and
// imm3_merge_view_host.cpp), for a build under -fsanitize=address,undefined: tests/test_merge_view_host.py compiles this file together
// with them (and the order's and the filter's checks, which build the layout and the program) and runs it.  No device and no handle.
// Parts: the tie width and its refusal; the canonical bytes' hash; the host view on synthetic records -- directed cases (ties across
// segments under descending keys, filters that keep none and all, the limits, an average at a count of 2^39) and random views held
// against a sort that compares the VALUES (never the normalised bytes).  Prints one line per part; exits non-zero on the first
// disagreement.
#include "../../immutable3_amd/csrc/imm3_merge_view_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

static std::string g_error;
namespace imm3 {
int fail(int code, const std::string &msg) {
    g_error = msg;
    return code;
}
} // namespace imm3
using namespace imm3;

// the aggregation: group by one int32 column; COUNT, SUM, MIN(int32), MAX(int8)
static const int32_t kGroupKind[1] = {0}, kGroupWidth[1] = {4};
static const int32_t kAggKind[4] = {IMM3_AGG_COUNT, IMM3_AGG_SUM, IMM3_AGG_MIN, IMM3_AGG_MAX};
static const int32_t kColKind[4] = {0, 0, 0, 1}, kColWidth[4] = {4, 4, 4, 1};
static GroupOrderShape shape() {
    GroupOrderShape s;
    std::memset(&s, 0, sizeof(s));
    s.is_agg = 1;
    s.n_group = 1;
    s.n_aggs = 4;
    s.group_kind = kGroupKind;
    s.group_width = kGroupWidth;
    s.agg_kind = kAggKind;
    s.agg_col_kind = kColKind;
    s.agg_col_width = kColWidth;
    return s;
}
constexpr int R = kMergeViewHead + 1; // a record: first, count, four values, one word of key

struct Rec {
    unsigned long long first, count;
    long long sum, mn, mx;
    int32_t key;
};
static void pack(const std::vector<Rec> &in, std::vector<unsigned long long> &out) {
    out.assign(in.size() * R, 0ULL);
    for (size_t i = 0; i < in.size(); ++i) {
        unsigned long long *w = out.data() + i * R;
        w[0] = in[i].first;
        w[1] = in[i].count;
        w[3] = (unsigned long long)in[i].sum;
        w[4] = (unsigned long long)in[i].mn;
        w[5] = (unsigned long long)in[i].mx;
        w[kMergeViewHead] = (unsigned long long)(uint32_t)in[i].key; // (little-endian: the key's four bytes first)
    }
}

// a plan from user arguments; largest: the largest segment index.  false: refused (g_error says why)
static bool make_plan(const std::vector<imm3_group_order_key> &order, const std::vector<imm3_group_filter_leaf> &leaves, const std::vector<int32_t> &prog, int64_t limit,
                      uint32_t largest, MergeViewPlan &p) {
    std::memset(&p, 0, sizeof(p));
    if (group_order_plan(shape(), order.data(), (int32_t)order.size(), &p.layout) != IMM3_OK) return false;
    if (group_filter_plan(shape(), leaves.data(), (int32_t)leaves.size(), prog.data(), (int32_t)prog.size(), &p.prog) != IMM3_OK) return false;
    p.limit = limit > 0 ? limit : 0;
    p.rec_words = R;
    return merge_view_tie(&p.layout, largest, &p.seg_bytes) == IMM3_OK;
}
static uint64_t hash_of(const MergeViewPlan &p) {
    std::vector<uint8_t> canon(kMergeViewCanonMax); // (heap: a write past it is the sanitizer's)
    const size_t n = merge_view_canonical(p.layout, p.prog, p.limit, canon.data(), canon.size());
    return merge_view_hash(canon.data(), n);
}
static std::vector<uint32_t> run_view(const MergeViewPlan &p, const std::vector<Rec> &recs, size_t *kept) {
    std::vector<unsigned long long> words;
    pack(recs, words);
    std::vector<uint32_t> order(recs.size());
    size_t n_out = 0;
    merge_view_host(p, words.data(), recs.size(), order.data(), &n_out, kept);
    order.resize(n_out);
    return order;
}
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

int main() {
    typedef imm3_group_order_key K;
    typedef imm3_group_filter_leaf L;
    const K by_key{IMM3_GROUP_ORDER_GROUP_COL, 0, 0}, by_count{IMM3_GROUP_ORDER_AGG, 0, 0}, by_sum{IMM3_GROUP_ORDER_AGG, 1, 0}, by_min{IMM3_GROUP_ORDER_AGG, 2, 0},
        by_max{IMM3_GROUP_ORDER_AGG, 3, 0};
    // ---- 1. the tie: S from the largest segment index; 16 key bytes accepted, 17 refused with the prefix
    const uint32_t seg[] = {0u, 1u, 255u, 256u, 65535u, 65536u, 16777215u, 16777216u, 0xFFFFFFFFu};
    const int32_t want_s[] = {0, 1, 1, 2, 2, 3, 3, 4, 4};
    for (int i = 0; i < 9; ++i) CHECK(merge_view_seg_bytes(seg[i]) == want_s[i]);
    MergeViewPlan p;
    CHECK(make_plan({by_sum, by_min}, {}, {}, 0, 0, p) && p.layout.user_bytes == 12 && p.seg_bytes == 0 && p.layout.key_bytes == 16 && p.layout.key_words == 4);
    CHECK(!make_plan({by_sum, by_min}, {}, {}, 0, 1, p) && g_error.rfind(IMM3_MERGE_VIEW_REFUSED, 0) == 0);
    CHECK(make_plan({by_count, by_min, by_max}, {}, {}, 0, 65535, p) && p.layout.user_bytes == 10 && p.seg_bytes == 2 && p.layout.key_bytes == 16);
    CHECK(!make_plan({by_count, by_min, by_max}, {}, {}, 0, 65536, p) && g_error.rfind(IMM3_MERGE_VIEW_REFUSED, 0) == 0);
    CHECK(make_plan({}, {}, {}, 0, 0xFFFFFFFFu, p) && p.layout.key_bytes == 8 && p.layout.key_words == 2);
    CHECK(merge_view_check_groups(kMergeViewMaxGroups) == IMM3_OK && merge_view_check_groups(kMergeViewMaxGroups + 1) == IMM3_ERR_ARG &&
          g_error.rfind(IMM3_MERGE_VIEW_REFUSED, 0) == 0);
    std::printf("tie ok\n");

    // ---- 2. the hash: equal for equal views, different in one descending flag, one threshold, the limit; the tie is no part of it
    MergeViewPlan a, b;
    const std::vector<L> leaf{L{1, 0, IMM3_GT, 100}};
    CHECK(make_plan({by_count, by_key}, leaf, {0}, 10, 3, a) && make_plan({by_count, by_key}, leaf, {0}, 10, 70000, b) && hash_of(a) == hash_of(b));
    K count_desc = by_count, sum_desc = by_sum;
    count_desc.descending = sum_desc.descending = 1;
    CHECK(make_plan({count_desc, by_key}, leaf, {0}, 10, 3, b) && hash_of(a) != hash_of(b));
    CHECK(make_plan({by_count, by_key}, {L{1, 0, IMM3_GT, 101}}, {0}, 10, 3, b) && hash_of(a) != hash_of(b));
    CHECK(make_plan({by_count, by_key}, leaf, {0}, 11, 3, b) && hash_of(a) != hash_of(b));
    CHECK(make_plan({by_count, by_key}, leaf, {0}, 0, 3, b) && hash_of(a) != hash_of(b));
    CHECK(make_plan({by_count, by_key}, leaf, {0}, -5, 3, a) && hash_of(a) == hash_of(b)); // (<= 0: no limit)
    std::printf("hash ok\n");

    // ---- 3. directed views.  Six groups over the segments 0, 2 and 300; the sums tie in threes
    const std::vector<Rec> six{{(300ULL << 32) | 5, 4, 7, -1, 3, 10},  {(2ULL << 32) | 9, 1, 7, 0, 3, -20}, {(0ULL << 32) | 1, 9, -7, 5, 1, 30},
                               {(2ULL << 32) | 4, 2, 7, 2, 3, 40},     {(300ULL << 32) | 0, 6, -7, 9, 1, 5}, {(0ULL << 32) | 70000, 3, -7, 1, 1, 0}};
    size_t kept = 0;
    CHECK(make_plan({sum_desc}, {}, {}, 0, 300, p) && p.seg_bytes == 2);
    CHECK((run_view(p, six, &kept) == std::vector<uint32_t>{3, 1, 0, 2, 5, 4}) && kept == 6); // ties in ascending (segment, row) under the descending key
    CHECK(make_plan({}, {}, {}, 0, 300, p) && (run_view(p, six, &kept) == std::vector<uint32_t>{2, 5, 3, 1, 4, 0}));
    K key_desc = by_key;
    key_desc.descending = 1;
    CHECK(make_plan({key_desc}, {}, {}, 2, 300, p) && (run_view(p, six, &kept) == std::vector<uint32_t>{3, 2}) && kept == 6);
    CHECK(make_plan({by_key}, {L{IMM3_GROUP_FILTER_COUNT, 0, IMM3_GT, 100}}, {0}, 0, 300, p) && run_view(p, six, &kept).empty() && kept == 0); // keeps none
    CHECK(make_plan({by_key}, {L{IMM3_GROUP_FILTER_COUNT, 0, IMM3_GT, 0}}, {0}, 0, 300, p) &&
          (run_view(p, six, &kept) == std::vector<uint32_t>{1, 5, 4, 0, 2, 3}) && kept == 6); // keeps all; -20 < 0 < 5 < 10 < 30 < 40 as signed
    const std::vector<L> sum_pos{L{1, 0, IMM3_GT, 0}};
    for (int64_t limit : {1, 3, 4}) { // limit 1, = kept, > kept
        CHECK(make_plan({by_count}, sum_pos, {0}, limit, 300, p));
        const std::vector<uint32_t> all{1, 3, 0}, got = run_view(p, six, &kept);
        CHECK(kept == 3 && got == std::vector<uint32_t>(all.begin(), all.begin() + (limit < 3 ? limit : 3)));
    }
    CHECK(run_view(p, {}, &kept).empty() && kept == 0); // no record
    // an average at a count of 2^39: threshold * count leaves int64 (it would wrap to -2^39 and to 0); the leaf compares in 128 bits
    const unsigned long long big = 1ULL << 39;
    const std::vector<Rec> one{{1, big, 5, 0, 0, 1}}, low{{1, big, INT64_MIN, 0, 0, 1}}, high{{1, big, INT64_MAX, 0, 0, 1}};
    struct Avg { const std::vector<Rec> *recs; int cond; int64_t value; bool keep; };
    const int64_t hi = 2147483647LL, lo = -2147483647LL - 1;
    const Avg avgs[] = {{&one, IMM3_GT, hi, false}, {&one, IMM3_LT, hi, true}, {&one, IMM3_EQ, hi, false}, {&one, IMM3_GT, lo, true}, {&one, IMM3_LT, lo, false},
                        {&one, IMM3_EQ, lo, false}, {&low, IMM3_GT, lo, true}, {&low, IMM3_LT, lo, false}, {&high, IMM3_LT, hi, true}, {&high, IMM3_GT, hi, false},
                        {&one, IMM3_GT, 0, true}, {&one, IMM3_EQ, 0, false}};
    for (const Avg &e : avgs) {
        CHECK(make_plan({}, {L{1, 1, e.cond, e.value}}, {0}, 0, 0, p));
        CHECK(run_view(p, *e.recs, &kept).size() == (e.keep ? 1u : 0u) && kept == (e.keep ? 1u : 0u));
    }
    std::printf("directed views ok\n");

    // ---- 4. random views against a sort on the values
    std::mt19937_64 rng(20261020);
    int done = 0;
    for (; done < 300; ++done) {
        const size_t n = (size_t)(rng() % 70);
        static const uint32_t kSpans[3] = {1u, 200u, 70000u};
        const uint32_t seg_span = kSpans[rng() % 3];
        std::vector<Rec> recs(n);
        for (size_t i = 0; i < n; ++i)
            recs[i] = Rec{((unsigned long long)(rng() % seg_span) << 32) | (unsigned long long)i, 1 + rng() % 5, (long long)(rng() % 7) - 3, (long long)(rng() % 5) - 2,
                          (long long)(rng() % 3) - 1, (int32_t)(rng() % 9) - 4};
        std::vector<K> pool{by_key, by_count, by_max, by_min}, order;
        std::shuffle(pool.begin(), pool.end(), rng);
        const size_t nk = (size_t)(rng() % 4); // key 4 + COUNT 5 + MAX(int8) 1 = 10 bytes at most with three of the four ... checked below
        int bytes = 0;
        for (size_t i = 0; i < nk; ++i) {
            const int w = pool[i].kind == IMM3_GROUP_ORDER_GROUP_COL ? 4 : (pool[i].index == 0 ? 5 : (pool[i].index == 2 ? 4 : 1));
            if (bytes + w + 4 + merge_view_seg_bytes(seg_span - 1) > kMergeViewKeyBytes) break;
            bytes += w;
            pool[i].descending = (int32_t)(rng() & 1);
            order.push_back(pool[i]);
        }
        const bool filtered = rng() & 1;
        const std::vector<L> leaves = filtered ? std::vector<L>{L{1, 0, IMM3_GT, (int64_t)(rng() % 5) - 2}, L{IMM3_GROUP_FILTER_COUNT, 0, IMM3_LT, 4}} : std::vector<L>{};
        const std::vector<int32_t> prog = filtered ? std::vector<int32_t>{0, 1, IMM3_EXPR_NOT, IMM3_EXPR_OR} : std::vector<int32_t>{};
        const int64_t limit = (int64_t)(rng() % 4 == 0 ? 0 : rng() % 80);
        if (!make_plan(order, leaves, prog, limit, seg_span - 1, p)) { std::printf("view %d refused: %s\n", done, g_error.c_str()); return 1; }
        std::vector<uint32_t> want;
        for (size_t i = 0; i < n; ++i)
            if (!filtered || recs[i].sum > leaves[0].value || !(recs[i].count < 4)) want.push_back((uint32_t)i);
        const size_t want_kept = want.size();
        auto value = [&](const Rec &r, const K &k) -> long long {
            return k.kind == IMM3_GROUP_ORDER_GROUP_COL ? r.key : (k.index == 0 ? (long long)r.count : (k.index == 2 ? r.mn : r.mx));
        };
        std::sort(want.begin(), want.end(), [&](uint32_t x, uint32_t y) {
            for (const K &k : order) {
                const long long vx = value(recs[x], k), vy = value(recs[y], k);
                if (vx != vy) return k.descending ? vx > vy : vx < vy;
            }
            return recs[x].first < recs[y].first;
        });
        if (limit > 0 && (size_t)limit < want.size()) want.resize((size_t)limit);
        const std::vector<uint32_t> got = run_view(p, recs, &kept);
        if (got != want || kept != want_kept) { std::printf("view %d: %zu records, got %zu want %zu (kept %zu / %zu)\n", done, n, got.size(), want.size(), kept, want_kept); return 1; }
    }
    std::printf("%d random views ok\n", done);
    return 0;
}
