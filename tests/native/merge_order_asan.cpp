// The host-only unit of imm3_comm_merge_ordered (immutable3_amd/csrc/imm3_merge_order_host.cpp) on its own, for a build under
// -fsanitize=address,undefined: tests/test_merge_ordered_host.py compiles this file together with the unit and runs it.  No device and
// no other part of the library.  Checks the record geometry for SELECT lists of odd widths, the vote words of equal and unequal
// specs, the argument rules, and the host k-way merge against std::stable_sort of the concatenation.  Prints one line per check;
// exits non-zero when one fails.
#include "../../immutable3_amd/csrc/imm3_merge_order.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

using namespace imm3;

static int bad = 0;
static void check(const char *what, bool ok) {
    std::printf("%-64s %s\n", what, ok ? "ok" : "FAILED");
    if (!ok) ++bad;
}

// records with few distinct keys, every buffer of exactly its size on the heap: a read past one is a sanitizer finding
static std::vector<uint32_t> random_list(std::mt19937 &rng, size_t n, int rec_words, uint32_t segment) {
    std::vector<uint32_t> recs(n * (size_t)rec_words);
    std::vector<std::vector<uint32_t>> keys(n);
    for (size_t i = 0; i < n; ++i) keys[i] = {rng() % 2, 0u, rng() % 3, 0x80000000u * (rng() % 2), segment, (uint32_t)i};
    std::sort(keys.begin(), keys.end());
    for (size_t i = 0; i < n; ++i) {
        uint32_t *r = recs.data() + i * (size_t)rec_words;
        std::copy(keys[i].begin(), keys[i].end(), r);
        for (int w = kMergeOrderKeyWords; w < rec_words; ++w) r[w] = rng();
    }
    return recs;
}

static bool merge_case(const char *what, std::mt19937 &rng, const std::vector<size_t> &lens, const std::vector<uint32_t> &segments, int rec_words, uint64_t limit) {
    std::vector<std::vector<uint32_t>> lists;
    for (size_t l = 0; l < lens.size(); ++l) lists.push_back(random_list(rng, lens[l], rec_words, segments[l]));
    std::vector<const uint32_t *> ptrs;
    std::vector<uint64_t> n;
    std::vector<const uint32_t *> all; // the concatenation, by record
    for (size_t l = 0; l < lists.size(); ++l) {
        ptrs.push_back(lists[l].data());
        n.push_back(lens[l]);
        for (size_t i = 0; i < lens[l]; ++i) all.push_back(lists[l].data() + i * (size_t)rec_words);
    }
    std::stable_sort(all.begin(), all.end(), [](const uint32_t *x, const uint32_t *y) { return merge_order_cmp(x, y) < 0; });
    if (limit && limit < all.size()) all.resize((size_t)limit);
    std::vector<uint32_t> out;
    merge_order_host(ptrs.data(), n.data(), (int32_t)lists.size(), rec_words, limit, out);
    bool ok = out.size() == all.size() * (size_t)rec_words;
    for (size_t i = 0; ok && i < all.size(); ++i) ok = std::memcmp(out.data() + i * (size_t)rec_words, all[i], (size_t)rec_words * sizeof(uint32_t)) == 0;
    check(what, ok);
    return ok;
}

int main() {
    // ---- geometry ----
    {
        const MergeOrderGeometry g = merge_order_geometry({1, 4, 5, 12, 256});
        check("geometry: offsets of widths 1, 4, 5, 12, 256", g.col_off == std::vector<int32_t>({6, 7, 8, 10, 13}));
        check("geometry: 77 words padded to an even 78", g.rec_words == 78);
        check("geometry: no columns", merge_order_geometry({}).rec_words == 6 && merge_order_geometry({}).col_off.empty());
        check("geometry: one byte", merge_order_geometry({1}).rec_words == 8);
        check("geometry: two words stay even", merge_order_geometry({4, 4}).rec_words == 8);
        // unpack reads exactly width bytes of every column and writes max_rows rows
        const std::vector<int32_t> widths = {1, 5};
        const MergeOrderGeometry g2 = merge_order_geometry(widths);
        std::vector<uint32_t> recs(3 * (size_t)g2.rec_words);
        for (size_t i = 0; i < recs.size(); ++i) recs[i] = 0x01020304u * (uint32_t)(i + 1);
        std::vector<uint32_t> seg(2), row(2);
        std::vector<uint8_t> c0(2 * 1), c1(2 * 5);
        void *cols[2] = {c0.data(), c1.data()};
        merge_order_unpack(recs.data(), 3, g2, widths, seg.data(), row.data(), cols, 2);
        bool ok = seg[1] == recs[(size_t)g2.rec_words + 4] && row[1] == recs[(size_t)g2.rec_words + 5];
        ok = ok && std::memcmp(c1.data() + 5, recs.data() + (size_t)g2.rec_words + g2.col_off[1], 5) == 0 && c0[0] == (uint8_t)recs[(size_t)g2.col_off[0]];
        merge_order_unpack(recs.data(), 3, g2, widths, nullptr, nullptr, nullptr, 3);
        check("unpack: two of three rows, odd widths, null outputs", ok);
    }
    // ---- vote words ----
    {
        MergeOrderSpec a;
        a.widths = {4, 1, 5};
        a.kinds = {0, 1, 2};
        a.key_proj = {1, 0};
        a.key_desc = {1, 0};
        MergeOrderSpec b = a;
        check("vote: equal specs vote alike", a == b && a.vote(0, 10) == b.vote(0, 10) && a.vote(1, 10) == b.vote(1, 10));
        b.key_desc = {0, 0};
        check("vote: another direction", !(a == b) && a.vote(1, 10) != b.vote(1, 10));
        b = a;
        b.key_proj = {0, 1};
        check("vote: the keys in another sequence", !(a == b) && a.vote(1, 10) != b.vote(1, 10));
        b = a;
        b.widths = {4, 1, 6};
        check("vote: another width", !(a == b) && a.vote(1, 10) != b.vote(1, 10));
        b = a;
        b.widths.push_back(4);
        b.kinds.push_back(0);
        check("vote: another column count", a.vote(0, 10) != b.vote(0, 10));
        b = a;
        b.key_proj.pop_back();
        b.key_desc.pop_back();
        check("vote: another key count", a.vote(0, 10) != b.vote(0, 10));
        check("vote: another limit", a.vote(1, 10) != a.vote(1, 11) && a.vote(1, 0) == a.vote(1, -7));
    }
    // ---- the argument rules ----
    {
        std::string why;
        const int64_t own0[3] = {0, 0, -1};
        const int32_t one[3] = {1, 1, 1};
        const int32_t idx[3] = {4, 0, 2};
        check("rules: plain", merge_order_check(0, own0, one, 3, idx, &why) && merge_order_check(10, own0, one, 3, idx, &why));
        const int64_t own5[3] = {0, 5, 0};
        check("rules: own limit 5 under 10", !merge_order_check(10, own5, one, 3, idx, &why) && !why.empty());
        check("rules: own limit 5 under none", !merge_order_check(0, own5, one, 3, idx, &why));
        check("rules: own limit 5 under 5 and under 3", merge_order_check(5, own5, one, 3, idx, &why) && merge_order_check(3, own5, one, 3, idx, &why));
        const int32_t twice[3] = {4, 0, 4};
        check("rules: a repeated index", !merge_order_check(0, own0, one, 3, twice, &why));
        const int32_t neg[3] = {4, -1, 2};
        check("rules: a negative index", !merge_order_check(0, own0, one, 3, neg, &why));
        const int32_t entries[2] = {3, 1};
        const int32_t flat[4] = {6, 2, 4, 0}; // a table over global segments 6, 2, 4, then segment 0
        const int64_t own2[2] = {0, 0}, own2l[2] = {9, 9};
        check("rules: a table's indices need not ascend", merge_order_check(0, own2, entries, 2, flat, &why));
        check("rules: ... unless it has a limit of its own", !merge_order_check(9, own2l, entries, 2, flat, &why));
        const int32_t up[4] = {2, 4, 6, 0};
        check("rules: ascending table with its own limit", merge_order_check(9, own2l, entries, 2, up, &why));
        check("rules: no query", merge_order_check(0, nullptr, nullptr, 0, nullptr, &why));
    }
    // ---- the host merge ----
    {
        std::mt19937 rng(12345);
        merge_case("merge: lengths 0, 1, 64, 65", rng, {0, 1, 64, 65}, {0, 1, 2, 3}, 8, 0);
        merge_case("merge: segments out of list order", rng, {65, 64, 1, 0}, {3, 0, 2, 1}, 8, 0);
        merge_case("merge: equal six-word keys in two lists", rng, {64, 64, 65}, {5, 5, 7}, 6, 0);
        merge_case("merge: a limit inside a tie group", rng, {65, 64, 1}, {0, 1, 2}, 10, 37);
        merge_case("merge: limit 1", rng, {65, 64}, {1, 0}, 8, 1);
        merge_case("merge: a limit above the total", rng, {1, 64}, {1, 0}, 8, 1000);
        merge_case("merge: every list empty", rng, {0, 0}, {0, 1}, 8, 5);
        merge_case("merge: one list", rng, {65}, {0}, 78, 0);
        merge_case("merge: no list", rng, {}, {}, 8, 0);
    }
    return bad ? 1 : 0;
}
