// imm3_group_order_plan.h -- the key layout of imm3_query_set_group_order (include/imm3.h; DESIGN.md section 21, "Ordering groups"): which
// bytes of a group's dense record make up its normalised order key.  Plain values only -- no handle, no HIP: the host-only checks
// (imm3_group_order_plan.cpp) fill it, the kernels of imm3_group_order.hip read it, tests/native/group_order_asan.cpp drives it alone.
#ifndef IMM3_GROUP_ORDER_PLAN_H
#define IMM3_GROUP_ORDER_PLAN_H
#include "../../include/imm3.h"

#include <stdint.h>

namespace imm3 {

// where a user key's bytes come from, and how they are normalised
enum GroupOrderSrc : int32_t {
    GO_KEY_I32 = 0,  // int32 group column: 4 bytes of the packed group key at `at`, little-endian; value ^ 0x80000000, big-endian
    GO_KEY_I8 = 1,   // int8 group column: the byte at `at` ^ 0x80
    GO_KEY_STR = 2,  // string group column: `width` bytes at `at`, as stored
    GO_COUNT = 3,    // COUNT: the group's count, 5 bytes big-endian (a query's rows are indexed by 32 bits: a count fits 33)
    GO_VAL_I32 = 4,  // MIN / MAX on an int32 column: vals[at] (sign-extended int64), its low 32 bits ^ 0x80000000, big-endian
    GO_VAL_I8 = 5,   // MIN / MAX on an int8 column: the low byte of vals[at] ^ 0x80
    GO_SUM = 6,      // SUM: vals[at] ^ (1 << 63), 8 bytes big-endian
    GO_VAL_STR = 7,  // MAX on a string of <= 8 bytes: vals[at] holds them packed big-endian
    GO_WIDE_STR = 8, // MAX on a wider string: `width` bytes of the collected value of aggregate `at`
};
struct GroupOrderKeyDesc {
    int32_t src;        // GroupOrderSrc
    int32_t width;      // bytes the key takes in the normalised key
    int32_t at;         // GO_KEY_*: byte offset in the packed group key; every other source: the aggregate's index
    int32_t descending; // 1: the key's bytes are complemented
};
constexpr int kGroupOrderFirstBytes = 4; // first_row, big-endian and never complemented, behind the user's bytes
struct GroupOrderLayout {
    GroupOrderKeyDesc k[IMM3_ORDER_MAX_KEYS];
    int32_t n_keys;
    int32_t user_bytes; // the user keys' widths summed, <= IMM3_GROUP_ORDER_KEY_MAX_WIDTH
    int32_t key_bytes;  // user_bytes + kGroupOrderFirstBytes: 5 .. 16
    int32_t key_words;  // ceil(key_bytes / 4)
};

// what the checks read of an aggregation query: column kinds are 0 = int32, 1 = int8, 2 = string (csrc/imm3_internal.h's ColKind)
struct GroupOrderShape {
    int32_t is_agg;
    int32_t n_group, n_aggs;
    const int32_t *group_kind, *group_width; // n_group each
    const int32_t *agg_kind;                 // n_aggs: IMM3_AGG_*
    const int32_t *agg_col_kind, *agg_col_width; // n_aggs: the aggregated column
};
// IMM3_OK and *out filled, or IMM3_ERR_ARG with the cause in imm3_last_error().  n_keys == 0 is valid (no order): *out is zeroed.
int group_order_plan(const GroupOrderShape &shape, const imm3_group_order_key *keys, int32_t n_keys, GroupOrderLayout *out);

} // namespace imm3
#endif
