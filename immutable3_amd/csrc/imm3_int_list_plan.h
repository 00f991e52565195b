// imm3_int_list_plan.h -- IMM3_INT_IN (include/imm3.h) without a device: the leaf's checks and values, a folded list's order and
// intersections, which kernel form a list takes, and the probe table the int32 forms read.  The hash and the probe
// are inline here for host AND device: k_filter_int_list (imm3_intlist.hip), eval_row (imm3_device.h) and the host run the same
// few lines.  Pure host code otherwise (imm3_int_list_plan.cpp), unit-tested on its own (tests/native/int_list_asan.cpp).
#pragma once
#include <cstdint>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IMM3_HOST_DEVICE __host__ __device__
#else
#define IMM3_HOST_DEVICE
#endif

namespace imm3 {

constexpr int64_t kIntListMaxValues = 1LL << 24; // IMM3_INT_IN_MAX_VALUES: a 2^25-slot table, 128 MiB of device memory
constexpr uint32_t kIntListMinSlots = 16;
constexpr int kIntListArgValues = 8;              // values the kernel arguments carry (kMaxMatch)
// The largest table a work-group copies into LDS.  A work-group may hold 64 KiB of static LDS and the kernel keeps 16 bytes of its
// own (block_partial_store), so a 16 384-slot table does not fit: 8192 slots = 32 KiB, lists of up to 4096 values.
constexpr uint32_t kIntListLdsSlots = 8192;

// which form of k_filter_int_list a folded list takes (int_list_form)
enum IntListForm : int32_t { INT_LIST_I8 = 0, INT_LIST_ARGS = 1, INT_LIST_LDS = 2, INT_LIST_GLOBAL = 3 };

// ---- the hash and the probe: host and device ----
// home slot: the top bits of v * 0x9E3779B1 (shift = 32 - log2(slots), slots >= 16)
IMM3_HOST_DEVICE inline uint32_t int_list_home(int32_t v, uint32_t shift) { return ((uint32_t)v * 0x9E3779B1u) >> shift; }

// v is in the table: linear probing from the home slot, AT MOST max_probe steps -- the loop never depends on meeting an empty slot,
// and every index is masked, so a corrupted table gives a wrong answer, never a hang or a read outside the table.  `empty` is a
// value the list does not hold: it is never a member, whatever the slots say.
IMM3_HOST_DEVICE inline bool int_list_probe(const int32_t *slots, uint32_t mask, uint32_t shift, int32_t empty, uint32_t max_probe, int32_t v) {
    if (v == empty) return false;
    const uint32_t home = int_list_home(v, shift);
    for (uint32_t i = 0; i < max_probe; ++i) {
        const int32_t x = slots[(home + i) & mask];
        if (x == v) return true;
        if (x == empty) return false;
    }
    return false;
}

// bit (uint8_t)v of the 256-bit membership set of an int8 column's list
IMM3_HOST_DEVICE inline bool int_list_set_has(const uint32_t *set, int32_t v) {
    const uint32_t b = (uint32_t)v & 255u;
    return (set[b >> 5] >> (b & 31u)) & 1u;
}

// ---- host ----
struct IntListTable {
    std::vector<int32_t> slots; // a power of two >= max(16, 2 n)
    int32_t empty = 0;          // what an empty slot holds: the smallest int32 the list does not hold
    uint32_t mask = 0, shift = 0, max_probe = 0; // slots - 1; 32 - log2(slots); the longest insertion distance + 1
};

// the leaf's own checks: IMM3_ERR_ARG for a negative count, a null pointer with values, a count above kIntListMaxValues
int int_list_check_leaf(int32_t n_match, const uint8_t *bytes);
// the leaf's values (n_match little-endian int32) as a list on a column of `width` bytes (4: int32, 1: int8 -- a value outside
// -128 .. 127 is no member of anything and is dropped): ascending, each once
int int_list_parse(int32_t n_match, const uint8_t *bytes, int32_t width, std::vector<int32_t> &out);
void int_list_sort(std::vector<int32_t> &list);                                        // ascending, duplicates once
void int_list_clip(std::vector<int32_t> &list, int64_t lo, int64_t hi);                // the values in [lo, hi]
void int_list_intersect(std::vector<int32_t> &list, const std::vector<int32_t> &other); // both sorted
bool int_list_has(const std::vector<int32_t> &list, int32_t v);                         // sorted
void int_list_set256(const std::vector<int32_t> &list, uint32_t set[8]);               // int8: bit (uint8_t)v per value
uint32_t int_list_slots(int64_t n);                                                     // 0: n outside 0 .. kIntListMaxValues
int int_list_form(int32_t width, int64_t n);                                            // IntListForm, -1 for a bad argument
void int_list_build_table(const std::vector<int32_t> &list, IntListTable &t);          // list: sorted, each value once; deterministic

} // namespace imm3
