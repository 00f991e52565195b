// imm3_hi16_plan.cpp -- the host side of the 16-bit high-half plane (imm3_hi16_plan.h): an interval's windows over the halves and the
// rule that says which tile pass scans the plane.  No handle, no device: imm3_api.cpp asks it at creation, imm3_run.cpp at every run,
// tests/test_hi16_plan_host.py through the diagnostics below.
#include "../../include/imm3.h"
#include "imm3_hi16_plan.h"

namespace imm3 {

Hi16Bounds hi16_bounds(int32_t lo, int32_t hi) {
    Hi16Bounds b;
    const int32_t lo_half = lo >> 16, hi_half = hi >> 16; // (arithmetic shifts: the plane's own)
    const bool lo_decides = ((uint32_t)lo & 0xFFFFu) == 0u, hi_decides = ((uint32_t)hi & 0xFFFFu) == 0xFFFFu;
    b.possible_first = (uint32_t)lo_half & 0xFFFFu;
    b.possible_count = lo <= hi ? (uint32_t)(hi_half - lo_half + 1) : 0u; // (an empty interval never reaches a kernel: always_false)
    const int32_t first = lo_half + (lo_decides ? 0 : 1), last = hi_half - (hi_decides ? 0 : 1);
    b.certain_first = (uint32_t)first & 0xFFFFu;
    b.certain_count = (lo <= hi && first <= last) ? (uint32_t)(last - first + 1) : 0u;
    return b;
}

bool hi16_eligible(const Hi16Inputs &in) {
    if (in.table || in.tree || in.ragged) return false;
    if (!in.dense_int || in.has_list) return false;
    if (in.stages || in.chunked) return false;
    if (!in.has_plane || in.pinned_i32) return false;
    return hi16_has_instance(in.n_i32, in.n_i8, in.n_s2);
}

} // namespace imm3

using namespace imm3;

// diagnostics (include/imm3_diag.h)
extern "C" int imm3_plan_hi16_bounds(int32_t lo, int32_t hi, uint32_t *out4) {
    if (!out4) return IMM3_ERR_ARG;
    const Hi16Bounds b = hi16_bounds(lo, hi);
    out4[0] = b.possible_first;
    out4[1] = b.possible_count;
    out4[2] = b.certain_first;
    out4[3] = b.certain_count;
    return IMM3_OK;
}

extern "C" int imm3_plan_hi16_class(int32_t lo, int32_t hi, int32_t half) {
    if (half < -32768 || half > 32767) return -1;
    return hi16_class(hi16_bounds(lo, hi), (int16_t)half);
}

extern "C" int imm3_plan_hi16_span_ok(int32_t min_half, int32_t max_half) { return hi16_span_ok(min_half, max_half) ? 1 : 0; }

// flags: bit 0 table, 1 tree, 2 ragged, 3 dense_int, 4 has_list, 5 stages, 6 chunked, 7 has_plane, 8 pinned_i32
extern "C" int imm3_plan_hi16_eligible(uint32_t flags, int32_t n_i32, int32_t n_i8, int32_t n_s2) {
    Hi16Inputs in;
    in.table = flags & 1u;
    in.tree = flags & 2u;
    in.ragged = flags & 4u;
    in.dense_int = flags & 8u;
    in.has_list = flags & 16u;
    in.stages = flags & 32u;
    in.chunked = flags & 64u;
    in.has_plane = flags & 128u;
    in.pinned_i32 = flags & 256u;
    in.n_i32 = n_i32;
    in.n_i8 = n_i8;
    in.n_s2 = n_s2;
    return hi16_eligible(in) ? 1 : 0;
}
