// imm3_distinct_plan.h -- how large the pair set of one COUNT(DISTINCT) aggregate is (IMM3_AGG_COUNT_DISTINCT).
// Pure host code without a device call: decided once at creation, unit-tested on its own (tests/native/distinct_plan_asan.cpp).
#pragma once
#include <cstdint>

namespace imm3 {

constexpr int kDistinctMaxWidth = 4;                 // widest value column, bytes: an entry holds the value's raw bytes in its low 32 bits
constexpr int64_t kDistinctMinEntries = 1024;
constexpr int64_t kDistinctMaxEntries = 1LL << 28;   // 2 GiB of 64-bit entries: what more than 2^27 rows would need (the aggregation's own slot cap)

// Entries (a power of two) of the open-addressing table of (group slot << 32 | value) pairs for a query over `rows` rows whose packed
// group key is `key_bytes` wide and whose value column is `width` bytes wide: the power of two at or above
// 2 x min(rows, G x 256^width), G = min(rows, 256^key_bytes) being the bound on groups that sizes the aggregation's own table;
// never below kDistinctMinEntries.  At most half the table is ever occupied, so a probe always ends.
// Returns -1 when that is more than kDistinctMaxEntries, -2 for an argument outside rows >= 0, key_bytes >= 0, width 1 .. 4.
int64_t distinct_capacity(int64_t rows, int32_t key_bytes, int32_t width);

} // namespace imm3
