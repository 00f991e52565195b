// imm3_group_filter_plan.h -- the program of imm3_query_set_group_filter (include/imm3.h; DESIGN.md section 21, "Filtering groups"): a
// predicate over one group's (count, vals) as plain values, small enough to travel in kernel arguments, and its evaluator.  No handle,
// no HIP: the host-only checks (imm3_group_filter_plan.cpp) fill the program, the filtered kernels of imm3_group_order.hip, the host's
// tests and tests/native/group_filter_asan.cpp all run group_filter_eval below -- __host__ __device__ under hipcc, plain inline under g++.
#ifndef IMM3_GROUP_FILTER_PLAN_H
#define IMM3_GROUP_FILTER_PLAN_H
#include "imm3_group_order_plan.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define IMM3_GF_HD __host__ __device__ inline
#else
#define IMM3_GF_HD inline
#endif

namespace imm3 {

// what a leaf compares
enum GroupFilterSrc : int32_t {
    GF_COUNT = 0, // the group's selected-row count (IMM3_GROUP_FILTER_COUNT, or a COUNT aggregate)
    GF_VAL = 1,   // vals[at]: MIN / MAX on int32 / int8 (sign-extended) or the exact int64 SUM
    GF_AVG = 2,   // vals[at] / count as a rational: vals[at] <cond> value * count (|value| <= 2^31, count < 2^32: no overflow)
};
struct GroupFilterLeaf {
    int32_t src;  // GroupFilterSrc
    int32_t at;   // GF_VAL / GF_AVG: the aggregate's index
    int32_t cond; // IMM3_GT / IMM3_LT / IMM3_EQ
    int32_t pad;
    int64_t value;
};
struct GroupFilterProg {
    GroupFilterLeaf leaf[IMM3_GROUP_FILTER_MAX_LEAVES];
    int8_t prog[IMM3_GROUP_FILTER_MAX_PROG]; // postfix: a leaf index, or IMM3_EXPR_AND / _OR / _NOT
    int32_t n_leaves, n_prog;                // n_prog == 0: no filter, every group is kept
};

// one leaf on a group.  V: the element type of the group's kMaxAggs values (int64_t on the host, long long on the device); `vals` may
// point into global memory -- the one dynamically indexed load is from there, never from a register array.
// WIDE (a view of MERGED groups, imm3_merge_view_plan.h): a merged count can pass 2^32, where value * count no longer fits int64 -- the
// leaf then compares in 128 bits.  The instances without the flag are what they always were.
template <class V, bool WIDE = false>
IMM3_GF_HD bool group_filter_leaf(const GroupFilterLeaf &l, unsigned long long count, const V *vals) {
    if constexpr (WIDE) {
        __int128 lhs, rhs = (__int128)l.value;
        if (l.src == GF_COUNT) lhs = (__int128)count;
        else {
            lhs = (__int128)(long long)vals[l.at];
            if (l.src == GF_AVG) rhs = rhs * (__int128)count;
        }
        return l.cond == IMM3_GT ? lhs > rhs : (l.cond == IMM3_LT ? lhs < rhs : lhs == rhs);
    }
    long long lhs, rhs = (long long)l.value;
    if (l.src == GF_COUNT) lhs = (long long)count;
    else {
        lhs = (long long)vals[l.at];
        if (l.src == GF_AVG) rhs = rhs * (long long)count;
    }
    return l.cond == IMM3_GT ? lhs > rhs : (l.cond == IMM3_LT ? lhs < rhs : lhs == rhs);
}

// The program on one group.  The stack is the bits of one 32-bit word, its top in bit 0: a checked program of at most
// IMM3_GROUP_FILTER_MAX_PROG entries that ends with one result never holds more than 17.  The program is the same for every group, so
// on the device the walk is uniform across a wave.
template <class V, bool WIDE = false>
IMM3_GF_HD bool group_filter_eval(const GroupFilterProg &f, unsigned long long count, const V *vals) {
    if (f.n_prog <= 0) return true;
    uint32_t st = 0;
    for (int32_t i = 0; i < f.n_prog; ++i) {
        const int32_t op = f.prog[i];
        if (op >= 0) st = (st << 1) | (group_filter_leaf<V, WIDE>(f.leaf[op], count, vals) ? 1u : 0u);
        else if (op == IMM3_EXPR_NOT) st ^= 1u;
        else {
            const uint32_t b = st & 1u;
            st >>= 1;
            st = op == IMM3_EXPR_AND ? (st & (b | ~1u)) : (st | b);
        }
    }
    return (st & 1u) != 0;
}

// IMM3_OK and *out filled, or IMM3_ERR_ARG with the cause in imm3_last_error().  n_leaves == 0 && n_prog == 0 is valid (no filter):
// *out is zeroed.  `shape` is imm3_query_set_group_order's; only is_agg, n_aggs and the aggregates' kinds are read.
int group_filter_plan(const GroupOrderShape &shape, const imm3_group_filter_leaf *leaves, int32_t n_leaves, const int32_t *prog, int32_t n_prog,
                      GroupFilterProg *out);

// the key layout of a filter without an order: no user key, first_row alone -- the device then answers in first-seen order
inline GroupOrderLayout group_filter_first_seen_layout() {
    GroupOrderLayout l{};
    l.key_bytes = kGroupOrderFirstBytes;
    l.key_words = (kGroupOrderFirstBytes + 3) / 4;
    return l;
}

} // namespace imm3
#endif
