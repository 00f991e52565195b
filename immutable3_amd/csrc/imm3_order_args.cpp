// imm3_order_args.cpp -- the argument checks of imm3_query_set_order (include/imm3.h), pure host code over plain values: no handle, no
// device.  imm3_api.cpp calls it with what the query handle holds; tests/native/order_args_asan.cpp builds it alone under the sanitizers.
#include "../../include/imm3.h"

#include <string>

namespace imm3 {
int fail(int code, const std::string &msg); // sets the calling thread's imm3_last_error() text

// proj_widths: bytes per value of each SELECT-list column (n_proj of them); create_limit: the limit the query was created with;
// has_run: any run call has been made on it.  *key_bytes_out: the summed width of the key columns.
int order_check_args(bool is_agg, int32_t n_proj, const int32_t *proj_widths, int64_t create_limit, bool has_run,
                     const imm3_order_key *keys, int32_t n_keys, int64_t limit, int32_t *key_bytes_out) {
    if (is_agg) return fail(IMM3_ERR_ARG, "imm3_query_set_order: an aggregation query's groups are ordered by imm3_query_set_group_order");
    if (n_proj <= 0) return fail(IMM3_ERR_ARG, "imm3_query_set_order: the query projects no column (n_proj == 0): there are no rows to order");
    if (has_run) return fail(IMM3_ERR_STATE, "imm3_query_set_order: the query has already run; set the order before the first run");
    if (n_keys < 1 || n_keys > IMM3_ORDER_MAX_KEYS) return fail(IMM3_ERR_ARG, "imm3_query_set_order: n_keys must be 1 .. " + std::to_string(IMM3_ORDER_MAX_KEYS));
    if (!keys) return fail(IMM3_ERR_ARG, "imm3_query_set_order: keys is null");
    int32_t bytes = 0;
    for (int32_t i = 0; i < n_keys; ++i) {
        if (keys[i].proj < 0 || keys[i].proj >= n_proj)
            return fail(IMM3_ERR_ARG, "imm3_query_set_order: key " + std::to_string(i) + " names SELECT-list entry " + std::to_string(keys[i].proj) + " of " + std::to_string(n_proj));
        for (int32_t j = 0; j < i; ++j)
            if (keys[j].proj == keys[i].proj) return fail(IMM3_ERR_ARG, "imm3_query_set_order: SELECT-list entry " + std::to_string(keys[i].proj) + " is an order key twice");
        const int32_t w = proj_widths[keys[i].proj];
        if (w <= 0 || w > IMM3_ORDER_KEY_MAX_WIDTH) return fail(IMM3_ERR_ARG, "imm3_query_set_order: the order key is wider than " + std::to_string(IMM3_ORDER_KEY_MAX_WIDTH) + " bytes");
        bytes += w;
    }
    if (bytes > IMM3_ORDER_KEY_MAX_WIDTH)
        return fail(IMM3_ERR_ARG, "imm3_query_set_order: the key columns are " + std::to_string(bytes) + " bytes wide together, more than " + std::to_string(IMM3_ORDER_KEY_MAX_WIDTH));
    (void)limit;
    if (create_limit > 0)
        return fail(IMM3_ERR_ARG, "imm3_query_set_order: the query was created with a limit, which stops the scan before the order is known; "
                                  "create it with limit <= 0 and pass the limit here (it is applied after the order)");
    if (key_bytes_out) *key_bytes_out = bytes;
    return IMM3_OK;
}
} // namespace imm3
