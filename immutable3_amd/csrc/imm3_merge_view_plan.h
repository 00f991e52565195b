// imm3_merge_view_plan.h -- the view of MERGED groups (imm3_comm_merge_groups_view, include/imm3.h; DESIGN.md section 21, "Views of
// merged groups"): filter, then order, then limit over the record list a merge by byte key leaves behind (imm3_internal.h:
// MergeWideArgs).  Plain values only -- no handle, no HIP: the tie width, the refusal, the canonical bytes the ranks vote on, and the
// key builder that reads a record directly -- __host__ __device__ under hipcc (the kernels of imm3_merge_view.hip), plain inline
// under g++ (imm3_merge_view_host.cpp, tests/native/merge_view_asan.cpp).
#ifndef IMM3_MERGE_VIEW_PLAN_H
#define IMM3_MERGE_VIEW_PLAN_H
#include "imm3_group_filter_plan.h"

#include <stddef.h>

namespace imm3 {

constexpr int kMergeViewAggs = 4;      // kMaxAggs (imm3_internal.h)
constexpr int kMergeViewHead = 2 + kMergeViewAggs; // kMergeWideHead: the word a record's key bytes start at
constexpr int kMergeViewKeyBytes = 16; // kOrderKeyMaxBytes: the order's key
constexpr unsigned long long kMergeViewMaxGroups = 1ULL << 30; // what the order launches index with 32 bits, with room to spare

// A view, checked: the user keys of group_order_plan (layout.k, n_keys, user_bytes), behind them the TIE -- the `first` word of a
// record, segment << 32 | first row: seg_bytes bytes of segment, then 4 of row, big-endian and never complemented -- and the program.
// layout.key_bytes = user_bytes + seg_bytes + 4 <= 16.
struct MergeViewPlan {
    GroupOrderLayout layout;
    int32_t seg_bytes;               // 0 .. 4: the bytes the largest segment index of any rank needs
    int32_t rec_words;               // a record's u64 words
    int32_t str_off[kMergeViewAggs]; // word offset of aggregate j's wide string in a record, 0: none
    GroupFilterProg prog;            // n_prog == 0: every group is kept
    int64_t limit;                   // <= 0: none
};

// bytes of the largest segment index: 0 when it is 0, 1 up to 255, 2 up to 65535, 3 up to 2^24 - 1, else 4
inline int32_t merge_view_seg_bytes(uint32_t largest_segment_index) {
    int32_t s = 0;
    for (uint32_t v = largest_segment_index; v; v >>= 8) ++s;
    return s;
}

// The tie behind the user's part of `layout`: IMM3_OK and layout.key_bytes / key_words / *seg_bytes set, or IMM3_ERR_ARG with a
// message that begins with IMM3_MERGE_VIEW_REFUSED when user_bytes + 4 + seg_bytes > 16.
int merge_view_tie(GroupOrderLayout *layout, uint32_t largest_segment_index, int32_t *seg_bytes);
// IMM3_ERR_ARG with the same prefix for more merged groups than the order launches take
int merge_view_check_groups(unsigned long long n_groups);

// What the ranks must agree on, as bytes: the user keys (src, width, at, descending each), the program's leaves and entries, the
// limit (<= 0 as 0).  Returns the bytes written (cap >= kMergeViewCanonMax always suffices).
constexpr size_t kMergeViewCanonMax = 4 + IMM3_ORDER_MAX_KEYS * 16 + 8 + IMM3_GROUP_FILTER_MAX_LEAVES * 20 + IMM3_GROUP_FILTER_MAX_PROG + 8;
size_t merge_view_canonical(const GroupOrderLayout &layout, const GroupFilterProg &prog, int64_t limit, uint8_t *out, size_t cap);
uint64_t merge_view_hash(const uint8_t *bytes, size_t n); // FNV-1a, 64 bits

// The normalised key of one record: key byte 0 in the top byte of k[0], zero-padded to 16 bytes (imm3_group_order.hip's go_build_key
// with the record as the source of every part).
IMM3_GF_HD void merge_view_key(const MergeViewPlan &p, const unsigned long long *rec, uint32_t k[4]) {
    unsigned long long hi = 0, lo = 0;
    auto push = [&](uint32_t byte) {
        hi = (hi << 8) | (lo >> 56);
        lo = (lo << 8) | (unsigned long long)(byte & 0xFFu);
    };
    const uint8_t *keyb = (const uint8_t *)(rec + kMergeViewHead);
    for (int c = 0; c < p.layout.n_keys; ++c) {
        const GroupOrderKeyDesc &d = p.layout.k[c];
        const uint32_t flip = d.descending ? 0xFFu : 0u;
        if (d.src == GO_KEY_I32) {
            push((uint32_t)keyb[d.at + 3] ^ 0x80u ^ flip);
            push((uint32_t)keyb[d.at + 2] ^ flip);
            push((uint32_t)keyb[d.at + 1] ^ flip);
            push((uint32_t)keyb[d.at] ^ flip);
        } else if (d.src == GO_KEY_I8) {
            push((uint32_t)keyb[d.at] ^ 0x80u ^ flip);
        } else if (d.src == GO_KEY_STR) {
            for (int x = 0; x < d.width; ++x) push((uint32_t)keyb[d.at + x] ^ flip);
        } else if (d.src == GO_COUNT) { // (5 bytes: a merged count of 2^40 or more is outside the contract)
            const unsigned long long v = rec[1];
            for (int x = 4; x >= 0; --x) push((uint32_t)(v >> (8 * x)) ^ flip);
        } else if (d.src == GO_WIDE_STR) {
            const uint8_t *s = (const uint8_t *)(rec + p.str_off[d.at]);
            for (int x = 0; x < d.width; ++x) push((uint32_t)s[x] ^ flip);
        } else {
            unsigned long long v = rec[2 + d.at];
            int bytes = d.width; // GO_VAL_STR: the value's bytes packed big-endian in the low `width` bytes
            if (d.src == GO_VAL_I32) { v = (v & 0xFFFFFFFFULL) ^ 0x80000000ULL; bytes = 4; }
            else if (d.src == GO_VAL_I8) { v = (v & 0xFFULL) ^ 0x80ULL; bytes = 1; }
            else if (d.src == GO_SUM) { v ^= 1ULL << 63; bytes = 8; }
            for (int x = bytes - 1; x >= 0; --x) push((uint32_t)(v >> (8 * x)) ^ flip);
        }
    }
    const unsigned long long first = rec[0];
    for (int x = p.seg_bytes - 1; x >= 0; --x) push((uint32_t)(first >> (32 + 8 * x)));
    for (int x = 3; x >= 0; --x) push((uint32_t)(first >> (8 * x)));
    for (int b = p.layout.key_bytes; b < kMergeViewKeyBytes; ++b) push(0u);
    k[0] = (uint32_t)(hi >> 32);
    k[1] = (uint32_t)hi;
    k[2] = (uint32_t)(lo >> 32);
    k[3] = (uint32_t)lo;
}

// the program on one record, exact for merged counts (the 128-bit leaf)
IMM3_GF_HD bool merge_view_keep(const MergeViewPlan &p, const unsigned long long *rec) {
    return group_filter_eval<long long, true>(p.prog, rec[1], (const long long *)(rec + 2));
}

// imm3_merge_view_host.cpp -- the view on the HOST, under the same rule: the indices of the view's records, in the view's order, and
// the number the filter kept.  What imm3_comm_merge_groups_view_all runs behind its host combine, and the library's answer for an
// empty list.
void merge_view_host(const MergeViewPlan &p, const unsigned long long *recs, size_t n, uint32_t *order_out /* min(kept, limit) used, room for n */,
                     size_t *n_out, size_t *n_kept);

} // namespace imm3
#endif
