// imm3_int_set_plan.h -- imm3_int_set_create (include/imm3.h) without a device: what the host decides between the
// device passes of imm3_intset.hip -- the free sentinel, the scratch table's size, what a table read back holds, the interval a set
// leaf folds to.  Pure code over plain values (imm3_int_set_plan.cpp), unit-tested on its own (tests/native/int_set_asan.cpp).
#pragma once
#include "imm3_int_list_plan.h"

#include <cstdint>
#include <vector>

namespace imm3 {

// `empty` for a table whose values all lie in [min, max]: min - 1, else max + 1; false: the set holds both INT32_MIN and INT32_MAX,
// no int32 just outside the span is free (the host route builds such a set)
bool int_set_pick_empty(int32_t min, int32_t max, int32_t *empty);
// The values the scratch table is sized for: no more distinct values than selected rows, than integers in [min, max], than `cap`
// (IMM3_INT_IN_MAX_VALUES, or a diagnostic creator's lower one).  0 for no rows or min > max.
int64_t int_set_scratch_values(int64_t selected_rows, int32_t min, int32_t max, int64_t cap);
// ... and its slots: int_list_slots of that (0: cap outside 0 .. kIntListMaxValues)
uint32_t int_set_scratch_slots(int64_t selected_rows, int32_t min, int32_t max, int64_t cap);
// the values of a table read back from the device (every slot that is not `empty`), ascending, each once, plus `extra` when has_extra
void int_set_table_values(const int32_t *slots, int64_t n_slots, int32_t empty, bool has_extra, int32_t extra, std::vector<int32_t> &out);
// the interval [lo, hi] of a column's GT / LT / EQ leaves intersected with a set of n values spanning [min, max]; an empty set or an
// empty intersection: lo = 1, hi = 0 (what every caller reads as "selects nothing")
void int_set_fold_interval(int64_t &lo, int64_t &hi, int64_t n, int32_t min, int32_t max);

} // namespace imm3
