// imm3_merge_order_host.cpp -- the host-only unit of the ordered merge (imm3_merge_order.h): no device, no other part of the library.
#include "imm3_merge_order.h"

#include <algorithm>
#include <cstring>
#include <queue>

namespace imm3 {

unsigned long long MergeOrderSpec::vote(int word, int64_t limit) const {
    if (word == 0) return (unsigned long long)widths.size() | (unsigned long long)key_proj.size() << 32;
    unsigned long long h = 0xcbf29ce484222325ULL;
    auto mix = [&](unsigned long long v) {
        for (int b = 0; b < 8; ++b) {
            h ^= (v >> (8 * b)) & 0xFFULL;
            h *= 0x100000001b3ULL;
        }
    };
    mix(widths.size());
    for (size_t j = 0; j < widths.size(); ++j) { mix((unsigned long long)(uint32_t)widths[j]); mix((unsigned long long)(uint32_t)kinds[j]); }
    mix(key_proj.size());
    for (size_t j = 0; j < key_proj.size(); ++j) { mix((unsigned long long)(uint32_t)key_proj[j]); mix(key_desc[j] ? 1ULL : 0ULL); }
    mix(limit > 0 ? (unsigned long long)limit : 0ULL);
    return h;
}

MergeOrderGeometry merge_order_geometry(const std::vector<int32_t> &widths) {
    MergeOrderGeometry g;
    int32_t off = kMergeOrderKeyWords;
    for (int32_t w : widths) {
        g.col_off.push_back(off);
        off += (w + 3) / 4;
    }
    g.rec_words = (off + 1) & ~1;
    return g;
}

int merge_order_cmp(const uint32_t *x, const uint32_t *y) {
    for (int w = 0; w < kMergeOrderKeyWords; ++w)
        if (x[w] != y[w]) return x[w] < y[w] ? -1 : 1;
    return 0;
}

bool merge_order_check(int64_t limit, const int64_t *own_limit, const int32_t *n_entries, int32_t n_queries, const int32_t *segment_index, std::string *why) {
    std::vector<int32_t> all;
    size_t at = 0;
    for (int32_t i = 0; i < n_queries; ++i) {
        const int64_t own = own_limit[i] > 0 ? own_limit[i] : 0;
        if (limit > 0 && own > 0 && own < limit) {
            *why = "query " + std::to_string(i) + " is ordered with limit " + std::to_string(own) + ", below the merge's limit " + std::to_string(limit) +
                   ": its list may lack rows the merge needs";
            return false;
        }
        if (limit <= 0 && own > 0) {
            *why = "query " + std::to_string(i) + " is ordered with limit " + std::to_string(own) + " but the merge has none: its list may lack rows the merge needs";
            return false;
        }
        bool ascending = true;
        for (int32_t e = 0; e < n_entries[i]; ++e) {
            const int32_t s = segment_index[at + (size_t)e];
            if (s < 0) {
                *why = "negative segment index " + std::to_string(s);
                return false;
            }
            if (e > 0 && s < segment_index[at + (size_t)e - 1]) ascending = false;
            all.push_back(s);
        }
        if (!ascending && own > 0) {
            *why = "query " + std::to_string(i) + " runs over a table whose global segment indices are not ascending and is ordered with a limit: its ties were cut in table order";
            return false;
        }
        at += (size_t)n_entries[i];
    }
    std::sort(all.begin(), all.end());
    for (size_t j = 1; j < all.size(); ++j)
        if (all[j] == all[j - 1]) {
            *why = "segment index " + std::to_string(all[j]) + " is given twice";
            return false;
        }
    return true;
}

void merge_order_host(const uint32_t *const *lists, const uint64_t *lens, int32_t n_lists, int32_t rec_words, uint64_t limit, std::vector<uint32_t> &out) {
    uint64_t total = 0;
    for (int32_t l = 0; l < n_lists; ++l) total += lens[l];
    const uint64_t want = limit > 0 && limit < total ? limit : total;
    out.clear();
    out.reserve((size_t)want * (size_t)rec_words);
    struct Head {
        const uint32_t *rec;
        int32_t list;
    };
    auto later = [](const Head &x, const Head &y) { // (a max-heap on "comes later": the top is the next record)
        const int c = merge_order_cmp(x.rec, y.rec);
        return c != 0 ? c > 0 : x.list > y.list;
    };
    std::priority_queue<Head, std::vector<Head>, decltype(later)> heap(later);
    std::vector<uint64_t> at((size_t)std::max(n_lists, 0), 0);
    for (int32_t l = 0; l < n_lists; ++l)
        if (lens[l]) heap.push(Head{lists[l], l});
    for (uint64_t o = 0; o < want; ++o) {
        const Head h = heap.top();
        heap.pop();
        out.insert(out.end(), h.rec, h.rec + rec_words);
        if (++at[(size_t)h.list] < lens[h.list]) heap.push(Head{h.rec + rec_words, h.list});
    }
}

void merge_order_unpack(const uint32_t *recs, uint64_t n, const MergeOrderGeometry &geo, const std::vector<int32_t> &widths, uint32_t *segment_out,
                        uint32_t *row_out, void *const *col_out, uint64_t max_rows) {
    const uint64_t rows = std::min(n, max_rows);
    for (uint64_t i = 0; i < rows; ++i) {
        const uint32_t *r = recs + i * (uint64_t)geo.rec_words;
        if (segment_out) segment_out[i] = r[4];
        if (row_out) row_out[i] = r[5];
        if (!col_out) continue;
        for (size_t j = 0; j < widths.size(); ++j)
            if (col_out[j]) std::memcpy((uint8_t *)col_out[j] + i * (uint64_t)widths[j], r + geo.col_off[j], (size_t)widths[j]);
    }
}

} // namespace imm3
