// imm3_distinct_plan.cpp -- see imm3_distinct_plan.h
#include "imm3_distinct_plan.h"

namespace imm3 {

int64_t distinct_capacity(int64_t rows, int32_t key_bytes, int32_t width) {
    if (rows < 0 || key_bytes < 0 || width < 1 || width > kDistinctMaxWidth) return -2;
    const int64_t r = rows > 0 ? rows : 1;
    // G = min(r, 256^key_bytes): a key of 8 bytes or more has a larger domain than any row count
    int64_t groups = r;
    if (key_bytes < 8 && (int64_t)1 << (8 * key_bytes) < r) groups = (int64_t)1 << (8 * key_bytes);
    // pairs = min(r, G x 256^width) without forming a product that could overflow: G x 2^(8 width) >= r  <=>  G >= ceil(r / 2^(8 width))
    const int sh = 8 * width;
    const int64_t need_groups = (r >> sh) + ((r & (((int64_t)1 << sh) - 1)) != 0 ? 1 : 0);
    const int64_t pairs = groups >= need_groups ? r : groups << sh; // (else G x 2^sh < r <= 2^63: no overflow)
    if (pairs > kDistinctMaxEntries / 2) return -1;
    int64_t cap = kDistinctMinEntries;
    while (cap < 2 * pairs) cap <<= 1;
    return cap;
}

} // namespace imm3

extern "C" int64_t imm3_plan_distinct_capacity(int64_t rows, int32_t key_bytes, int32_t width) { return imm3::distinct_capacity(rows, key_bytes, width); }
