// The host decisions of imm3_int_set_create (immutable3_amd/csrc/imm3_int_set_plan.cpp) on their own, for a build under
// -fsanitize=address,undefined: tests/test_int_in_query_host.py compiles this file together with that unit and imm3_int_list_plan.cpp
// and runs it.  Every table handed in is an allocation of exactly its slots, so a read past one is a sanitizer finding; the extremes of
// int32 go through every function that does arithmetic on them.  The one function the units take from the rest of the library
// (imm3::fail) is defined here.  Prints one line per check; exits non-zero when one fails.
#include "../../include/imm3.h"
#include "../../immutable3_amd/csrc/imm3_int_set_plan.h"

#include <cstdio>
#include <cstdlib>
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
extern "C" int64_t imm3_plan_int_set_scratch_slots(int64_t selected_rows, int32_t min, int32_t max, int64_t cap);

static int bad = 0;
static void expect(const char *what, bool ok) {
    std::printf("%-72s %s\n", what, ok ? "ok" : "FAILED");
    if (!ok) ++bad;
}

int main() {
    int32_t e = 0;
    expect("empty: min - 1 when there is one", int_set_pick_empty(-5, 9, &e) && e == -6);
    expect("empty: max + 1 when min is INT32_MIN", int_set_pick_empty(INT32_MIN, 9, &e) && e == 10);
    expect("empty: min - 1 when max is INT32_MAX", int_set_pick_empty(0, INT32_MAX, &e) && e == -1);
    expect("empty: none when the set holds both extremes", !int_set_pick_empty(INT32_MIN, INT32_MAX, &e));
    expect("empty: a single value", int_set_pick_empty(7, 7, &e) && e == 6);

    expect("scratch values: the rows bound", int_set_scratch_values(100, 0, 1 << 20, kIntListMaxValues) == 100);
    expect("scratch values: the span bound", int_set_scratch_values(1 << 20, -3, 6, kIntListMaxValues) == 10);
    expect("scratch values: the cap bound", int_set_scratch_values(1LL << 40, INT32_MIN, INT32_MAX, kIntListMaxValues) == kIntListMaxValues);
    expect("scratch values: the whole int32 span does not overflow", int_set_scratch_values(INT64_MAX, INT32_MIN, INT32_MAX, 16) == 16);
    expect("scratch values: nothing selected, an empty span, no cap", int_set_scratch_values(0, 0, 9, 5) == 0 && int_set_scratch_values(5, 9, 0, 5) == 0 &&
                                                                         int_set_scratch_values(5, 0, 9, 0) == 0 && int_set_scratch_values(-1, 0, 9, 5) == 0);
    expect("scratch slots: a power of two, >= 16, >= 2 x", int_set_scratch_slots(100, 0, 1 << 20, kIntListMaxValues) == 256 && int_set_scratch_slots(3, 0, 9, 8) == 16 &&
                                                             int_set_scratch_slots(1 << 20, -3, 6, kIntListMaxValues) == 32 && int_set_scratch_slots(0, 0, 0, 8) == 16);
    expect("scratch slots: the largest table", int_set_scratch_slots(1LL << 40, INT32_MIN, INT32_MAX, kIntListMaxValues) == (1u << 25));
    expect("scratch slots: a cap outside the range is refused", int_set_scratch_slots(5, 0, 9, -1) == 0 && int_set_scratch_slots(5, 0, 9, kIntListMaxValues + 1) == 0);
    expect("scratch slots: the diagnostic export", imm3_plan_int_set_scratch_slots(100, 0, 1 << 20, kIntListMaxValues) == 256 && imm3_plan_int_set_scratch_slots(5, 0, 9, -1) == -1);

    {
        int32_t *slots = (int32_t *)std::malloc(16 * sizeof(int32_t)); // exactly the table
        for (int i = 0; i < 16; ++i) slots[i] = -9;
        slots[3] = 40;
        slots[15] = INT32_MIN;
        slots[0] = 7;
        std::vector<int32_t> out;
        int_set_table_values(slots, 16, -9, false, 0, out);
        expect("table values: every slot that is not empty, ascending", out == std::vector<int32_t>({INT32_MIN, 7, 40}));
        int_set_table_values(slots, 16, -9, true, INT32_MAX, out);
        expect("table values: with the value the device passed over", out == std::vector<int32_t>({INT32_MIN, 7, 40, INT32_MAX}));
        int_set_table_values(slots, 16, -9, true, 40, out);
        expect("table values: each value once", out == std::vector<int32_t>({INT32_MIN, 7, 40}));
        int_set_table_values(slots, 0, -9, false, 0, out);
        expect("table values: no table, no value", out.empty());
        std::free(slots);
        // the host route's table: both extremes in it, a sentinel between them, every member found
        std::vector<int32_t> both = {INT32_MIN, -1, 0, 5, INT32_MAX};
        IntListTable t;
        int_list_build_table(both, t);
        bool ok = t.empty != INT32_MIN && t.empty != INT32_MAX;
        for (int32_t v : both) ok = ok && int_list_probe(t.slots.data(), t.mask, t.shift, t.empty, t.max_probe, v);
        ok = ok && !int_list_probe(t.slots.data(), t.mask, t.shift, t.empty, t.max_probe, t.empty) && !int_list_probe(t.slots.data(), t.mask, t.shift, t.empty, t.max_probe, 6);
        expect("the host route's table holds both extremes", ok);
    }
    {
        int64_t lo = INT32_MIN, hi = INT32_MAX;
        int_set_fold_interval(lo, hi, 3, -4, 90);
        expect("fold: the full interval becomes the set's span", lo == -4 && hi == 90);
        lo = 0, hi = 50;
        int_set_fold_interval(lo, hi, 3, -4, 90);
        expect("fold: an interval inside the span stays", lo == 0 && hi == 50);
        lo = 91, hi = INT32_MAX;
        int_set_fold_interval(lo, hi, 3, -4, 90);
        expect("fold: an interval disjoint from the span is empty", lo == 1 && hi == 0);
        lo = INT32_MIN, hi = INT32_MAX;
        int_set_fold_interval(lo, hi, 0, 0, 0);
        expect("fold: an empty set is empty", lo == 1 && hi == 0);
        lo = 5, hi = 4;
        int_set_fold_interval(lo, hi, 3, INT32_MIN, INT32_MAX);
        expect("fold: an empty interval stays empty", lo == 1 && hi == 0);
        lo = (int64_t)INT32_MAX + 1, hi = INT32_MAX; // (GT INT32_MAX folds to this)
        int_set_fold_interval(lo, hi, 3, INT32_MIN, INT32_MAX);
        expect("fold: bounds beyond int32 do not wrap", lo == 1 && hi == 0);
    }
    return bad ? 1 : 0;
}
