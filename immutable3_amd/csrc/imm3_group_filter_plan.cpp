// imm3_group_filter_plan.cpp -- the argument checks of imm3_query_set_group_filter (include/imm3.h) and the program the kernels take,
// pure host code over plain values: no handle, no device.  imm3_group_order_api.cpp calls it with what the query handle holds;
// tests/native/group_filter_asan.cpp builds it (with imm3_expr_norm.cpp for the program's checks) under the sanitizers.
#include "imm3_group_filter_plan.h"

#include <cstring>
#include <string>

namespace imm3 {
int fail(int code, const std::string &msg); // sets the calling thread's imm3_last_error() text
int expr_check_program(const int32_t *prog, int32_t n_prog, int32_t n_leaves, bool *has_or, bool *has_not); // imm3_expr_norm.cpp

int group_filter_plan(const GroupOrderShape &shape, const imm3_group_filter_leaf *leaves, int32_t n_leaves, const int32_t *prog, int32_t n_prog,
                      GroupFilterProg *out) {
    const std::string fn = "imm3_query_set_group_filter: ";
    if (!out) return fail(IMM3_ERR_ARG, fn + "null program");
    std::memset(out, 0, sizeof(*out));
    if (!shape.is_agg) return fail(IMM3_ERR_ARG, fn + "not an aggregation query (rows are filtered by the select)");
    if (n_leaves < 0 || n_leaves > IMM3_GROUP_FILTER_MAX_LEAVES)
        return fail(IMM3_ERR_ARG, fn + "n_leaves must be 0 .. " + std::to_string(IMM3_GROUP_FILTER_MAX_LEAVES));
    if (n_prog < 0 || n_prog > IMM3_GROUP_FILTER_MAX_PROG) return fail(IMM3_ERR_ARG, fn + "n_prog must be 0 .. " + std::to_string(IMM3_GROUP_FILTER_MAX_PROG));
    if (n_leaves > 0 && !leaves) return fail(IMM3_ERR_ARG, fn + "leaves is null");
    {
        const int rc = expr_check_program(prog, n_prog, n_leaves, nullptr, nullptr);
        if (rc) return rc;
    }
    for (int32_t i = 0; i < n_leaves; ++i) {
        const imm3_group_filter_leaf &l = leaves[i];
        GroupFilterLeaf &d = out->leaf[i];
        const std::string leaf = "leaf " + std::to_string(i);
        if (l.cond != IMM3_GT && l.cond != IMM3_LT && l.cond != IMM3_EQ)
            return fail(IMM3_ERR_ARG, fn + leaf + " has the unknown cond " + std::to_string(l.cond) + " (IMM3_GT, IMM3_LT or IMM3_EQ)");
        d.cond = l.cond;
        d.value = l.value;
        if (l.agg == IMM3_GROUP_FILTER_COUNT) {
            if (l.average) return fail(IMM3_ERR_ARG, fn + leaf + ": average is for a SUM aggregate only");
            d.src = GF_COUNT;
            continue;
        }
        if (l.agg < 0 || l.agg >= shape.n_aggs)
            return fail(IMM3_ERR_ARG, fn + leaf + " names aggregate " + std::to_string(l.agg) + " of " + std::to_string(shape.n_aggs));
        const int32_t ak = shape.agg_kind[l.agg], ck = shape.agg_col_kind[l.agg];
        // (a COUNT over a STRING column is a count like any other: only the string MAXIMUM has nothing a threshold compares with;
        // so is a COUNT_DISTINCT: the number of distinct strings, an int64 in the value table)
        if (ck == 2 && ak != IMM3_AGG_COUNT && ak != IMM3_AGG_COUNT_DISTINCT) return fail(IMM3_ERR_ARG, fn + leaf + ": aggregate " + std::to_string(l.agg) + " is a MAX over a STRING column, which a filter does not compare");
        if (l.average && ak != IMM3_AGG_SUM) return fail(IMM3_ERR_ARG, fn + leaf + ": average is for a SUM aggregate only");
        if (l.average && (l.value < -(int64_t)2147483648LL || l.value > (int64_t)2147483647LL))
            return fail(IMM3_ERR_ARG, fn + leaf + ": an average is compared as sum <cond> value * count in int64, so value must lie in [-2^31, 2^31 - 1]");
        d.at = l.agg;
        d.src = ak == IMM3_AGG_COUNT ? GF_COUNT : (l.average ? GF_AVG : GF_VAL);
        if (d.src == GF_COUNT) d.at = 0;
    }
    for (int32_t i = 0; i < n_prog; ++i) out->prog[i] = (int8_t)prog[i];
    out->n_leaves = n_leaves;
    out->n_prog = n_prog;
    return IMM3_OK;
}
} // namespace imm3
