// imm3_int_set_plan.cpp -- the host's decisions of imm3_int_set_create (imm3_int_set_plan.h), over plain values: no handle, no device.
// imm3_int_set_api.cpp and imm3_expr_norm.cpp call it; tests/native/int_set_asan.cpp builds it (with imm3_int_list_plan.cpp) alone
// under the sanitizers.
#include "../../include/imm3.h"
#include "imm3_int_set_plan.h"

#include <algorithm>
#include <cstdint>
#include <vector>

namespace imm3 {

bool int_set_pick_empty(int32_t min, int32_t max, int32_t *empty) {
    if (min > INT32_MIN) { *empty = min - 1; return true; }
    if (max < INT32_MAX) { *empty = max + 1; return true; }
    return false;
}

int64_t int_set_scratch_values(int64_t selected_rows, int32_t min, int32_t max, int64_t cap) {
    if (selected_rows <= 0 || min > max || cap <= 0) return 0;
    const int64_t span = (int64_t)max - (int64_t)min + 1;
    return std::min(std::min(selected_rows, span), cap);
}

uint32_t int_set_scratch_slots(int64_t selected_rows, int32_t min, int32_t max, int64_t cap) {
    if (cap < 0 || cap > kIntListMaxValues) return 0;
    return int_list_slots(int_set_scratch_values(selected_rows, min, max, cap));
}

void int_set_table_values(const int32_t *slots, int64_t n_slots, int32_t empty, bool has_extra, int32_t extra, std::vector<int32_t> &out) {
    out.clear();
    for (int64_t i = 0; i < n_slots; ++i)
        if (slots[i] != empty) out.push_back(slots[i]);
    if (has_extra) out.push_back(extra);
    int_list_sort(out);
}

void int_set_fold_interval(int64_t &lo, int64_t &hi, int64_t n, int32_t min, int32_t max) {
    if (n > 0) {
        lo = std::max<int64_t>(lo, min);
        hi = std::min<int64_t>(hi, max);
    }
    if (n <= 0 || lo > hi) { lo = 1; hi = 0; }
}

} // namespace imm3

// diagnostics (include/imm3_diag.h)
extern "C" int64_t imm3_plan_int_set_scratch_slots(int64_t selected_rows, int32_t min, int32_t max, int64_t cap) {
    const uint32_t slots = imm3::int_set_scratch_slots(selected_rows, min, max, cap);
    return slots ? (int64_t)slots : -1;
}
