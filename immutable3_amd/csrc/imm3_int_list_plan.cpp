// imm3_int_list_plan.cpp -- IMM3_INT_IN (include/imm3.h) on the host: the leaf's checks, its values as a sorted list on an int32 or
// int8 column, what lists and intervals on one column fold to, which kernel form a list takes, and the open-addressing table the
// int32 forms probe.  Pure code over plain values: no handle, no device.  imm3_expr_norm.cpp, imm3_api.cpp and imm3_run.cpp call it;
// tests/native/int_list_asan.cpp builds it alone under the sanitizers.
#include "../../include/imm3.h"
#include "imm3_int_list_plan.h"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace imm3 {
int fail(int code, const std::string &msg); // sets the calling thread's imm3_last_error() text

static_assert(kIntListMaxValues == IMM3_INT_IN_MAX_VALUES, "the cap of imm3.h");

int int_list_check_leaf(int32_t n_match, const uint8_t *bytes) {
    if (n_match < 0) return fail(IMM3_ERR_ARG, "IntIn: negative value count (n_match is " + std::to_string(n_match) + ")");
    if (n_match > 0 && !bytes) return fail(IMM3_ERR_ARG, "IntIn without values: match_bytes is null");
    if ((int64_t)n_match > kIntListMaxValues)
        return fail(IMM3_ERR_ARG, "IntIn: " + std::to_string(n_match) + " values, more than IMM3_INT_IN_MAX_VALUES (" + std::to_string(kIntListMaxValues) + ")");
    return IMM3_OK;
}

void int_list_sort(std::vector<int32_t> &list) {
    std::sort(list.begin(), list.end());
    list.erase(std::unique(list.begin(), list.end()), list.end());
}

int int_list_parse(int32_t n_match, const uint8_t *bytes, int32_t width, std::vector<int32_t> &out) {
    out.clear();
    const int rc = int_list_check_leaf(n_match, bytes);
    if (rc) return rc;
    if (width != 4 && width != 1) return fail(IMM3_ERR_ARG, "IntIn: the column is neither int32 nor int8");
    out.reserve((size_t)n_match);
    for (int32_t m = 0; m < n_match; ++m) {
        const uint8_t *p = bytes + 4 * (size_t)m; // little-endian two's complement, wherever the caller's bytes are aligned
        const uint32_t u = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
        int32_t v;
        std::memcpy(&v, &u, sizeof(v));
        if (width == 1 && (v < -128 || v > 127)) continue; // no int8 row holds it
        out.push_back(v);
    }
    int_list_sort(out);
    return IMM3_OK;
}

void int_list_clip(std::vector<int32_t> &list, int64_t lo, int64_t hi) {
    list.erase(std::remove_if(list.begin(), list.end(), [=](int32_t v) { return (int64_t)v < lo || (int64_t)v > hi; }), list.end());
}

void int_list_intersect(std::vector<int32_t> &list, const std::vector<int32_t> &other) {
    std::vector<int32_t> both;
    std::set_intersection(list.begin(), list.end(), other.begin(), other.end(), std::back_inserter(both));
    list.swap(both);
}

bool int_list_has(const std::vector<int32_t> &list, int32_t v) { return std::binary_search(list.begin(), list.end(), v); }

void int_list_set256(const std::vector<int32_t> &list, uint32_t set[8]) {
    for (int i = 0; i < 8; ++i) set[i] = 0;
    for (int32_t v : list) {
        const uint32_t b = (uint32_t)v & 255u;
        set[b >> 5] |= 1u << (b & 31u);
    }
}

uint32_t int_list_slots(int64_t n) {
    if (n < 0 || n > kIntListMaxValues) return 0;
    uint32_t slots = kIntListMinSlots;
    while ((int64_t)slots < 2 * n) slots <<= 1;
    return slots;
}

int int_list_form(int32_t width, int64_t n) {
    if ((width != 1 && width != 4) || n < 0 || n > kIntListMaxValues) return -1;
    if (width == 1) return INT_LIST_I8;
    if (n <= kIntListArgValues) return INT_LIST_ARGS;
    return int_list_slots(n) <= kIntListLdsSlots ? INT_LIST_LDS : INT_LIST_GLOBAL;
}

void int_list_build_table(const std::vector<int32_t> &list, IntListTable &t) {
    const uint32_t slots = int_list_slots((int64_t)std::min<size_t>(list.size(), (size_t)kIntListMaxValues));
    uint32_t log2 = 0;
    while ((1u << log2) < slots) ++log2;
    t.mask = slots - 1;
    t.shift = 32 - log2;
    // the smallest int32 the (ascending) list does not hold: there are fewer values than int32s, so one exists
    int64_t e = INT32_MIN;
    for (int32_t v : list) {
        if ((int64_t)v != e) break;
        ++e;
    }
    t.empty = (int32_t)e;
    t.slots.assign(slots, t.empty);
    t.max_probe = 1; // (an empty list: one step meets an empty slot)
    for (int32_t v : list) { // ascending: the same list always gives the same table
        const uint32_t home = int_list_home(v, t.shift);
        uint32_t d = 0;
        while (t.slots[(home + d) & t.mask] != t.empty) ++d; // (at most half the slots are taken)
        t.slots[(home + d) & t.mask] = v;
        t.max_probe = std::max(t.max_probe, d + 1);
    }
}

} // namespace imm3

using namespace imm3;

// diagnostics (include/imm3_diag.h): the table creation would upload for these values (any order, duplicates allowed)
extern "C" int imm3_plan_int_list_table(const int32_t *values, int64_t n, int32_t *slots_out, int64_t cap, int64_t *n_slots, int32_t *empty, int32_t *max_probe) {
    if (n < 0 || (n > 0 && !values) || n > kIntListMaxValues || cap < 0 || (cap > 0 && !slots_out)) return fail(IMM3_ERR_ARG, "bad argument");
    std::vector<int32_t> list(values, values + n);
    int_list_sort(list);
    IntListTable t;
    int_list_build_table(list, t);
    if (n_slots) *n_slots = (int64_t)t.slots.size();
    if (empty) *empty = t.empty;
    if (max_probe) *max_probe = (int32_t)t.max_probe;
    if (cap == 0) return IMM3_OK;
    if (cap < (int64_t)t.slots.size()) return fail(IMM3_ERR_ARG, "slots_out is too small");
    std::memcpy(slots_out, t.slots.data(), t.slots.size() * sizeof(int32_t));
    return IMM3_OK;
}

extern "C" int imm3_plan_int_list_form(int32_t width, int64_t n) { return int_list_form(width, n); }

// diagnostics: the probe the kernels run, on the host: 1 = v is found in the table within max_probe steps, 0 = not, -1 = bad argument
extern "C" int imm3_plan_int_list_probe(const int32_t *slots, int64_t n_slots, int32_t empty, int32_t max_probe, int32_t v) {
    if (!slots || n_slots < (int64_t)kIntListMinSlots || (n_slots & (n_slots - 1)) || n_slots > (1LL << 25) || max_probe < 0) return -1;
    uint32_t log2 = 0;
    while ((1LL << log2) < n_slots) ++log2;
    return int_list_probe(slots, (uint32_t)n_slots - 1, 32 - log2, empty, (uint32_t)max_probe, v) ? 1 : 0;
}
