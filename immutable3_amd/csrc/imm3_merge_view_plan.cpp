// imm3_merge_view_plan.cpp -- the host-only part of a view of merged groups (imm3_merge_view_plan.h): the tie width and its refusal,
// the canonical bytes and their hash.  No handle, no device: imm3_merge_view_api.cpp calls it with what the queries and the ranks give,
// imm3_merge_view_plan_json (include/imm3_diag.h) and tests/native/merge_view_asan.cpp drive it alone.
#include "imm3_merge_view_plan.h"

#include <string>

namespace imm3 {
int fail(int code, const std::string &msg); // sets the calling thread's imm3_last_error() text

int merge_view_tie(GroupOrderLayout *layout, uint32_t largest_segment_index, int32_t *seg_bytes) {
    const int32_t s = merge_view_seg_bytes(largest_segment_index), total = layout->user_bytes + s + kGroupOrderFirstBytes;
    *seg_bytes = s;
    if (total > kMergeViewKeyBytes)
        return fail(IMM3_ERR_ARG, std::string(IMM3_MERGE_VIEW_REFUSED) + "order keys of at most " + std::to_string(kMergeViewKeyBytes - kGroupOrderFirstBytes - s) +
                                      " bytes when the largest segment index is " + std::to_string(largest_segment_index) + " (" + std::to_string(s) +
                                      " bytes of segment and 4 of row break the ties); these keys are " + std::to_string(layout->user_bytes) + " bytes wide");
    layout->key_bytes = total;
    layout->key_words = (total + 3) / 4;
    return IMM3_OK;
}

int merge_view_check_groups(unsigned long long n_groups) {
    if (n_groups > kMergeViewMaxGroups)
        return fail(IMM3_ERR_ARG, std::string(IMM3_MERGE_VIEW_REFUSED) + "at most " + std::to_string(kMergeViewMaxGroups) + " merged groups, not " + std::to_string(n_groups));
    return IMM3_OK;
}

size_t merge_view_canonical(const GroupOrderLayout &layout, const GroupFilterProg &prog, int64_t limit, uint8_t *out, size_t cap) {
    size_t n = 0;
    auto put = [&](uint64_t v, int bytes) {
        for (int b = 0; b < bytes; ++b)
            if (n < cap) out[n++] = (uint8_t)(v >> (8 * b));
    };
    put((uint64_t)(uint32_t)layout.n_keys, 4);
    for (int32_t i = 0; i < layout.n_keys && i < IMM3_ORDER_MAX_KEYS; ++i) {
        put((uint64_t)(uint32_t)layout.k[i].src, 4);
        put((uint64_t)(uint32_t)layout.k[i].width, 4);
        put((uint64_t)(uint32_t)layout.k[i].at, 4);
        put((uint64_t)(uint32_t)layout.k[i].descending, 4);
    }
    put((uint64_t)(uint32_t)prog.n_leaves, 4);
    put((uint64_t)(uint32_t)prog.n_prog, 4);
    for (int32_t i = 0; i < prog.n_leaves && i < IMM3_GROUP_FILTER_MAX_LEAVES; ++i) {
        put((uint64_t)(uint32_t)prog.leaf[i].src, 4);
        put((uint64_t)(uint32_t)prog.leaf[i].at, 4);
        put((uint64_t)(uint32_t)prog.leaf[i].cond, 4);
        put((uint64_t)prog.leaf[i].value, 8);
    }
    for (int32_t i = 0; i < prog.n_prog && i < IMM3_GROUP_FILTER_MAX_PROG; ++i) put((uint64_t)(uint8_t)prog.prog[i], 1);
    put((uint64_t)(limit > 0 ? limit : 0), 8);
    return n;
}

uint64_t merge_view_hash(const uint8_t *bytes, size_t n) {
    uint64_t h = 1469598103934665603ULL;
    for (size_t i = 0; i < n; ++i) h = (h ^ bytes[i]) * 1099511628211ULL;
    return h;
}

} // namespace imm3
