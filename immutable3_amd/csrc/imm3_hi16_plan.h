// imm3_hi16_plan.h -- the 16-bit high-half plane of a DENSE_INT column (SegCol::d_hi16) without a device: what a
// closed int32 interval becomes over the halves `v >> 16`, which columns get a plane, and which tile passes scan it.  The kernel
// (ColRegs<TK_H16>, imm3_tile.h) runs the same two window tests hi16_class() runs here.  Pure code over plain values
// (imm3_hi16_plan.cpp), unit-tested without a GPU (tests/test_hi16_plan_host.py).
#pragma once
#include <cstdint>

namespace imm3 {

// A column whose halves span fewer distinct values than this gets no plane: most of its rows would share a half with a threshold
// and need their full value anyway (values in [0, 50 000): one half).
constexpr int kHi16MinSpan = 64;

// [lo, hi] (lo <= hi) over the halves, as two windows of 16-bit wrap-around arithmetic -- a half h is in a window when
// (uint16_t)(h - first) < count:
//   possible  the halves lo >> 16 .. hi >> 16: a row outside it fails
//   certain   the possible window without a boundary half that does not decide itself: a row inside it passes.  The low boundary
//             half decides itself when lo & 0xFFFF == 0 (every value of that half is >= lo), the high one when hi & 0xFFFF == 0xFFFF.
// A row in the possible window and outside the certain one is UNDECIDED: its full value is compared.  certain_count may be 0
// (both boundaries in one half, or in adjacent halves); then every possible row is undecided.
struct Hi16Bounds {
    uint32_t possible_first, possible_count; // first: 16 bits; count: 1 .. 65536
    uint32_t certain_first, certain_count;   // count: 0 .. 65536
};
Hi16Bounds hi16_bounds(int32_t lo, int32_t hi);

enum Hi16Class : int32_t { HI16_FAIL = 0, HI16_PASS = 1, HI16_UNDECIDED = 2 };
inline int hi16_class(const Hi16Bounds &b, int16_t half) {
    const uint32_t h = (uint16_t)half;
    if (((h - b.possible_first) & 0xFFFFu) >= b.possible_count) return HI16_FAIL;
    return ((h - b.certain_first) & 0xFFFFu) < b.certain_count ? HI16_PASS : HI16_UNDECIDED;
}

// the halves a column spans (what the plane's build reduces) are worth a plane
inline bool hi16_span_ok(int32_t min_half, int32_t max_half) { return (int64_t)max_half - (int64_t)min_half + 1 >= kHi16MinSpan; }

// What the planner sees of one int32 predicate of a tile pass.  Creation asks with `has_plane` = "the column has one or may get
// one" and the run-time facts (stages, chunked) false: is a plane worth making.  A run asks with all of them.
struct Hi16Inputs {
    bool table = false, tree = false;   // the query is over a table / is a select tree with an OR or a NOT
    bool ragged = false;                // the segment's layout is not uniform: no tile pass at all
    bool dense_int = false;             // the column is DENSE_INT (not PFOR_INT / snappy: those read d_dense)
    bool has_list = false;              // the folded predicate is an IN-list, not a plain closed interval
    bool stages = false;                // the pass compacts survivor records (they carry the column's values)
    bool chunked = false;               // the pass is the select of a projection with a limit: a chunk of its limit scan (or the whole of a segment one chunk covers)
    bool has_plane = false;             // SegCol::d_hi16
    bool pinned_i32 = false;            // the tuning variant that keeps the int32 scan (A/B runs of the tools)
    int32_t n_i32 = 0, n_i8 = 0, n_s2 = 0; // the pass's columns by kind (this one included in n_i32)
};
bool hi16_eligible(const Hi16Inputs &in);
// the kind combinations that have a TK_H16 instance: the lone int32 column, and int8 + int32
inline bool hi16_has_instance(int32_t n_i32, int32_t n_i8, int32_t n_s2) { return n_i32 == 1 && n_s2 == 0 && (n_i8 == 0 || n_i8 == 1); }

} // namespace imm3
