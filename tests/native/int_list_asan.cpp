// The host logic of IMM3_INT_IN (immutable3_amd/csrc/imm3_int_list_plan.cpp) on its own, for a build under -fsanitize=address,undefined:
// tests/test_int_in_host.py compiles this file together with that unit and runs it.  Every buffer handed in is an allocation of
// exactly the bytes it should hold (the leaf's values at an odd address), so a read or write past a list, a set or a table is a
// sanitizer finding.  The one function the unit takes from the rest of the library (imm3::fail) is defined here.  Prints one line
// per check; exits non-zero when one fails.
#include "../../include/imm3.h"
#include "../../immutable3_amd/csrc/imm3_int_list_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

static std::string g_error;
namespace imm3 {
int fail(int code, const std::string &msg) {
    g_error = msg;
    return code;
}
} // namespace imm3
using namespace imm3;

static int bad = 0;
static void expect(const char *what, bool ok) {
    std::printf("%-64s %s\n", what, ok ? "ok" : "FAILED");
    if (!ok) ++bad;
}

// the leaf's bytes for `v`: 4-byte little-endian values in an allocation of exactly 4 n bytes that starts at an odd address
struct LeafBytes {
    std::vector<uint8_t> store;
    const uint8_t *p = nullptr;
    explicit LeafBytes(const std::vector<int32_t> &v) {
        uint8_t *raw = (uint8_t *)std::malloc(4 * v.size() + 1);
        for (size_t i = 0; i < v.size(); ++i) {
            const uint32_t u = (uint32_t)v[i];
            for (int b = 0; b < 4; ++b) raw[1 + 4 * i + b] = (uint8_t)(u >> (8 * b));
        }
        keep = raw;
        p = v.empty() ? nullptr : raw + 1;
    }
    ~LeafBytes() { std::free(keep); }
    uint8_t *keep = nullptr;
};

static bool table_ok(const std::vector<int32_t> &list) { // list: sorted, each value once
    IntListTable t;
    int_list_build_table(list, t);
    const size_t slots = t.slots.size();
    bool ok = slots >= 16 && slots >= 2 * list.size() && (slots & (slots - 1)) == 0 && t.mask == slots - 1 && (1ull << (32 - t.shift)) == slots;
    ok = ok && !int_list_has(list, t.empty) && t.max_probe >= 1;
    for (int32_t v : list) ok = ok && int_list_probe(t.slots.data(), t.mask, t.shift, t.empty, t.max_probe, v);
    ok = ok && !int_list_probe(t.slots.data(), t.mask, t.shift, t.empty, t.max_probe, t.empty);
    uint32_t x = 12345u;
    for (int i = 0; i < 10000; ++i) { // non-members: some random, some next to the members
        x = x * 1664525u + 1013904223u;
        int32_t v = (int32_t)x;
        if (!list.empty() && (i & 1)) v = (int32_t)((uint32_t)list[x % list.size()] + 1u + (x >> 30));
        if (int_list_has(list, v)) continue;
        ok = ok && !int_list_probe(t.slots.data(), t.mask, t.shift, t.empty, t.max_probe, v);
    }
    IntListTable again;
    int_list_build_table(list, again);
    return ok && again.slots == t.slots && again.empty == t.empty && again.max_probe == t.max_probe;
}

int main() {
    std::vector<int32_t> out;
    // ---- the leaf's checks ----
    expect("a negative count is refused", int_list_check_leaf(-1, nullptr) == IMM3_ERR_ARG && g_error.find("negative") != std::string::npos);
    expect("values without a pointer are refused", int_list_check_leaf(3, nullptr) == IMM3_ERR_ARG && g_error.find("null") != std::string::npos);
    {
        const uint8_t one[4] = {1, 0, 0, 0};
        expect("a count above the cap is refused", int_list_check_leaf(IMM3_INT_IN_MAX_VALUES + 1, one) == IMM3_ERR_ARG && g_error.find("IMM3_INT_IN_MAX_VALUES") != std::string::npos);
        expect("the cap itself passes the check", int_list_check_leaf(IMM3_INT_IN_MAX_VALUES, one) == IMM3_OK);
    }
    expect("an empty leaf is an empty list", int_list_parse(0, nullptr, 4, out) == IMM3_OK && out.empty());
    // ---- parse, narrow, sort ----
    {
        LeafBytes lb({5, -1, 5, INT32_MAX, INT32_MIN, 0, 300, -129, 127, -128});
        expect("int32: every value, ascending, each once", int_list_parse(10, lb.p, 4, out) == IMM3_OK &&
                   out == std::vector<int32_t>({INT32_MIN, -129, -128, -1, 0, 5, 127, 300, INT32_MAX}));
        expect("int8: values outside -128 .. 127 are dropped", int_list_parse(10, lb.p, 1, out) == IMM3_OK && out == std::vector<int32_t>({-128, -1, 0, 5, 127}));
        expect("a column of another width is refused", int_list_parse(10, lb.p, 2, out) == IMM3_ERR_ARG);
    }
    // ---- clip, intersect, membership, the int8 set ----
    {
        std::vector<int32_t> l = {-9, -3, 0, 4, 8, 100};
        int_list_clip(l, -3, 8);
        expect("clip keeps the values inside the closed interval", l == std::vector<int32_t>({-3, 0, 4, 8}));
        int_list_clip(l, (int64_t)INT32_MAX + 5, (int64_t)INT32_MAX + 9);
        expect("clip by an interval outside int32 leaves nothing", l.empty());
        std::vector<int32_t> a = {1, 3, 5, 7, 9}, b = {0, 3, 4, 9, 12};
        int_list_intersect(a, b);
        expect("two lists intersect", a == std::vector<int32_t>({3, 9}));
        int_list_intersect(a, std::vector<int32_t>());
        expect("... with an empty list to nothing", a.empty());
        expect("membership in a sorted list", int_list_has({-5, 2, 9}, 2) && !int_list_has({-5, 2, 9}, 3) && !int_list_has({}, 0));
        uint32_t set[8];
        int_list_set256({-128, -1, 0, 127}, set);
        bool ok = true;
        for (int v = -128; v < 128; ++v) ok = ok && int_list_set_has(set, v) == (v == -128 || v == -1 || v == 0 || v == 127);
        expect("the 256-bit set holds exactly the list", ok);
        std::vector<int32_t> all;
        for (int v = -128; v < 128; ++v) all.push_back(v);
        int_list_set256(all, set);
        ok = true;
        for (int i = 0; i < 8; ++i) ok = ok && set[i] == 0xFFFFFFFFu;
        expect("all 256 values fill the set", ok);
    }
    // ---- slots and forms ----
    // (the thresholds between the forms are the unit's own: the largest list of the LDS form is read from int_list_form)
    int64_t lds_n = kIntListArgValues + 1;
    while (int_list_form(4, lds_n + 1) == INT_LIST_LDS) ++lds_n;
    expect("slots: at least 16, at least 2 n, a power of two", int_list_slots(0) == 16 && int_list_slots(8) == 16 && int_list_slots(9) == 32 &&
               int_list_slots(lds_n) == kIntListLdsSlots && int_list_slots(lds_n + 1) == 2 * kIntListLdsSlots && int_list_slots(kIntListMaxValues) == (1u << 25) &&
               int_list_slots(kIntListMaxValues + 1) == 0 && int_list_slots(-1) == 0);
    expect("forms by width and length", int_list_form(1, 0) == INT_LIST_I8 && int_list_form(1, 256) == INT_LIST_I8 && int_list_form(4, kIntListArgValues) == INT_LIST_ARGS &&
               int_list_form(4, kIntListArgValues + 1) == INT_LIST_LDS && int_list_form(4, lds_n) == INT_LIST_LDS && lds_n == kIntListLdsSlots / 2 &&
               int_list_form(4, lds_n + 1) == INT_LIST_GLOBAL && int_list_form(2, 1) == -1 && int_list_form(4, -1) == -1 &&
               int_list_form(4, kIntListMaxValues + 1) == -1);
    // ---- the probe table ----
    expect("table of no value", table_ok({}));
    expect("table of one value", table_ok({42}));
    expect("table of the ends of int32, -1 and 0", table_ok({INT32_MIN, -1, 0, INT32_MAX}));
    {
        std::vector<int32_t> l;
        for (int v = INT32_MIN; l.size() < 40; ++v) l.push_back(v);
        expect("table of INT32_MIN and its successors (empty moves up)", table_ok(l));
    }
    for (size_t n : {(size_t)2, (size_t)kIntListArgValues, (size_t)kIntListArgValues + 1, (size_t)16, (size_t)17, (size_t)lds_n, (size_t)lds_n + 1, (size_t)100000}) {
        std::set<int32_t> s;
        uint32_t x = (uint32_t)n * 2654435761u;
        while (s.size() < n) {
            x = x * 1664525u + 1013904223u;
            s.insert((int32_t)x);
        }
        const std::string what = "table of " + std::to_string(n) + " random values";
        expect(what.c_str(), table_ok(std::vector<int32_t>(s.begin(), s.end())));
    }
    {
        std::vector<int32_t> l;
        for (int v = -3000; v < 3000; ++v) l.push_back(v);
        expect("table of consecutive integers", table_ok(l));
    }
    {
        // every value shares one home slot of the 64-slot table 24 values get
        std::vector<int32_t> l;
        const uint32_t shift = 32 - 6, want = int_list_home(1000, shift);
        for (int32_t v = 1000; l.size() < 24; ++v)
            if (int_list_home(v, shift) == want) l.push_back(v);
        IntListTable t;
        int_list_build_table(l, t);
        expect("table of values that share one home slot", table_ok(l) && t.slots.size() == 64 && t.max_probe == 24);
        // a corrupted table: no empty slot left, a step bound far past the table -- the probe still ends, inside the table
        for (auto &sl : t.slots) sl = 7;
        expect("a table without an empty slot ends its probes", !int_list_probe(t.slots.data(), t.mask, t.shift, t.empty, 1u << 20, 5) &&
                   int_list_probe(t.slots.data(), t.mask, t.shift, t.empty, 1u << 20, 7));
    }
    return bad ? 1 : 0;
}
