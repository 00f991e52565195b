// imm3_merge_order.h -- the host-only part of imm3_comm_merge_ordered (imm3_merge_order_host.cpp; no HIP in either file, so the two
// build and run alone: tests/native/merge_order_asan.cpp): the record geometry, what the ranks vote on, the argument rules that need
// no device, and the host k-way merge of imm3_comm_merge_ordered_all.
//
// A record is rec_words 32-bit words: the six-word sort key {four words of normalised key (zero-padded to 16 bytes), global segment,
// row in segment}, then the SELECT-list columns' bytes, each column padded to a word; rec_words is even, so records are 8-byte
// aligned.  Unsigned word-wise comparison of the first six words is the order ("Merging ordered results").
#ifndef IMM3_MERGE_ORDER_H
#define IMM3_MERGE_ORDER_H
#include <cstdint>
#include <string>
#include <vector>

namespace imm3 {

constexpr int kMergeOrderKeyWords = 6;
constexpr unsigned long long kMergeOrderMaxRows = 1ULL << 30; // rows entering one merge (places and list lengths are 32-bit)

// what must be the same in every query of every rank
struct MergeOrderSpec {
    std::vector<int32_t> widths, kinds; // the SELECT list: bytes per row and ColKind of each column
    std::vector<int32_t> key_proj, key_desc; // the order keys: index into the SELECT list, descending (0 / 1)
    bool operator==(const MergeOrderSpec &o) const { return widths == o.widths && kinds == o.kinds && key_proj == o.key_proj && key_desc == o.key_desc; }
    // the two words the ranks vote on (all-reduce(max) of each and of its complement: max == min means all ranks agree):
    // word 0 = the counts, word 1 = a 64-bit FNV-1a hash of every field and of the merge's limit
    unsigned long long vote(int word, int64_t limit) const;
};

struct MergeOrderGeometry {
    int32_t rec_words = kMergeOrderKeyWords; // even
    std::vector<int32_t> col_off;            // word offset of column j's bytes in a record
};
MergeOrderGeometry merge_order_geometry(const std::vector<int32_t> &widths);

// -1 / 0 / 1: the six-word keys of two records
int merge_order_cmp(const uint32_t *x, const uint32_t *y);

// The limit rule and the segment indices of ONE rank; false and *why on a violation.
//   own_limit[i]  query i's own order limit (<= 0: none);  n_entries[i] segment_index entries query i consumes (1, or its table's
//   segments);  a table query whose entries are not ascending keeps its ties in another order than the merge's: its own limit must be <= 0
bool merge_order_check(int64_t limit, const int64_t *own_limit, const int32_t *n_entries, int32_t n_queries, const int32_t *segment_index, std::string *why);

// k sorted lists of records -> the first `limit` (0: all) records of their merge by six-word key, equal keys in list order: what
// std::stable_sort of the concatenation gives
void merge_order_host(const uint32_t *const *lists, const uint64_t *lens, int32_t n_lists, int32_t rec_words, uint64_t limit, std::vector<uint32_t> &out);

// records -> the caller's arrays (any of them null), at most max_rows rows
void merge_order_unpack(const uint32_t *recs, uint64_t n, const MergeOrderGeometry &geo, const std::vector<int32_t> &widths, uint32_t *segment_out,
                        uint32_t *row_out, void *const *col_out, uint64_t max_rows);

} // namespace imm3
#endif
