// imm3_group_order_plan.cpp -- the argument checks and the key layout of imm3_query_set_group_order (include/imm3.h), pure host code over
// plain values: no handle, no device.  imm3_group_order_api.cpp calls it with what the query handle holds;
// tests/native/group_order_asan.cpp builds it alone under the sanitizers.
#include "imm3_group_order_plan.h"

#include <cstring>
#include <string>

namespace imm3 {
int fail(int code, const std::string &msg); // sets the calling thread's imm3_last_error() text

int group_order_plan(const GroupOrderShape &shape, const imm3_group_order_key *keys, int32_t n_keys, GroupOrderLayout *out) {
    const std::string fn = "imm3_query_set_group_order: ";
    if (!out) return fail(IMM3_ERR_ARG, fn + "null layout");
    std::memset(out, 0, sizeof(*out));
    if (!shape.is_agg) return fail(IMM3_ERR_ARG, fn + "not an aggregation query (a projection is ordered by imm3_query_set_order)");
    if (n_keys < 0 || n_keys > IMM3_ORDER_MAX_KEYS) return fail(IMM3_ERR_ARG, fn + "n_keys must be 0 .. " + std::to_string(IMM3_ORDER_MAX_KEYS));
    if (n_keys == 0) return IMM3_OK;
    if (!keys) return fail(IMM3_ERR_ARG, fn + "keys is null");
    int32_t bytes = 0;
    for (int32_t i = 0; i < n_keys; ++i) {
        const imm3_group_order_key &k = keys[i];
        GroupOrderKeyDesc &d = out->k[i];
        d.descending = k.descending ? 1 : 0;
        if (k.kind == IMM3_GROUP_ORDER_GROUP_COL) {
            if (k.index < 0 || k.index >= shape.n_group)
                return fail(IMM3_ERR_ARG, fn + "key " + std::to_string(i) + " names group column " + std::to_string(k.index) + " of " + std::to_string(shape.n_group));
            int32_t at = 0;
            for (int32_t g = 0; g < k.index; ++g) at += shape.group_width[g];
            d.at = at;
            d.width = shape.group_width[k.index];
            d.src = shape.group_kind[k.index] == 0 ? GO_KEY_I32 : (shape.group_kind[k.index] == 1 ? GO_KEY_I8 : GO_KEY_STR);
        } else if (k.kind == IMM3_GROUP_ORDER_AGG) {
            if (k.index < 0 || k.index >= shape.n_aggs)
                return fail(IMM3_ERR_ARG, fn + "key " + std::to_string(i) + " names aggregate " + std::to_string(k.index) + " of " + std::to_string(shape.n_aggs));
            d.at = k.index;
            const int32_t ak = shape.agg_kind[k.index], ck = shape.agg_col_kind[k.index], cw = shape.agg_col_width[k.index];
            if (ak == IMM3_AGG_COUNT) { d.src = GO_COUNT; d.width = 5; }
            else if (ak == IMM3_AGG_SUM || ak == IMM3_AGG_COUNT_DISTINCT) { d.src = GO_SUM; d.width = 8; } // (COUNT_DISTINCT: an int64 in the value table, whatever its column)
            else if (ck == 0) { d.src = GO_VAL_I32; d.width = 4; }
            else if (ck == 1) { d.src = GO_VAL_I8; d.width = 1; }
            else { d.src = cw <= 8 ? GO_VAL_STR : GO_WIDE_STR; d.width = cw; }
        } else return fail(IMM3_ERR_ARG, fn + "key " + std::to_string(i) + " has the unknown kind " + std::to_string(k.kind));
        for (int32_t j = 0; j < i; ++j)
            if (keys[j].kind == k.kind && keys[j].index == k.index)
                return fail(IMM3_ERR_ARG, fn + (k.kind == IMM3_GROUP_ORDER_AGG ? "aggregate " : "group column ") + std::to_string(k.index) + " is an order key twice");
        if (d.width <= 0 || d.width > IMM3_GROUP_ORDER_KEY_MAX_WIDTH)
            return fail(IMM3_ERR_ARG, fn + "key " + std::to_string(i) + " is " + std::to_string(d.width) + " bytes wide, more than " + std::to_string(IMM3_GROUP_ORDER_KEY_MAX_WIDTH));
        bytes += d.width;
    }
    if (bytes > IMM3_GROUP_ORDER_KEY_MAX_WIDTH)
        return fail(IMM3_ERR_ARG, fn + "the keys are " + std::to_string(bytes) + " bytes wide together, more than " + std::to_string(IMM3_GROUP_ORDER_KEY_MAX_WIDTH));
    out->n_keys = n_keys;
    out->user_bytes = bytes;
    out->key_bytes = bytes + kGroupOrderFirstBytes;
    out->key_words = (out->key_bytes + 3) / 4;
    return IMM3_OK;
}
} // namespace imm3
