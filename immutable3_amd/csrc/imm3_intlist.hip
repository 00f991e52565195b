// imm3_intlist.hip -- k_filter_int_list: IMM3_INT_IN, "the row's value is a member of the list", over one DENSE_INT / DENSE_TINYINT
// column (or its decoded form), for gfx950 (wave64).  A one-column pass of the select chain: geometry, tile addressing, the
// partial-tile rule, the bitmap line and the count are imm3_pass.h's; what is here is the loads and the test.
//
// Loads.  All 16 loads of a tile (one dword or one byte per lane and row block) are issued before the first test, non-temporal: the
// column is read once.
//
// Test.  Every form first holds the value against the folded interval [lo, hi] = [the list's minimum, its maximum]; what is left to
// do is wave-uniform over "any candidate left", so a tile of a sorted key outside the list's span costs a plain scan.  The forms
// (int_list_form, imm3_int_list_plan.h):
//   I8     the 256-bit membership set (8 dwords, kernel arguments) is copied to 32 bytes of LDS once per work-group; a row's test is one
//          ds_read_b32 at (value >> 5), a shift and a mask, whatever the list's length
//   ARGS   up to 8 values in the kernel arguments: the list is walked once per tile, 16 compares per value (as k_filter_str_rows)
//   LDS    the host-built open-addressing table (imm3_int_list_plan.cpp; at most kIntListLdsSlots slots) is copied from device memory
//          into LDS once per work-group; every candidate row probes it from its home slot
//   GLOBAL the same probe against the table in device memory with ordinary cached loads -- the table is what should stay in L2 / MALL
// The probe: step 0 of all 16 row blocks at once (16 independent reads in flight), then a rolled loop over the steps 1 ..
// max_probe - 1 for the rows that met another value, wave-uniform over "any row still undecided".  No loop depends on meeting an
// empty slot, and every slot index is masked: a corrupted table can give a wrong answer, never a hang or a read outside the table.
#include "imm3_internal.h"
#include "imm3_pass.h"
#include <hip/hip_ext.h>

namespace imm3 {

template <int FORM, bool TABLE>
__global__ __launch_bounds__(kBlockThreads) void k_filter_int_list(const IntListArgs a) {
    constexpr bool I8 = FORM == INT_LIST_I8;
    const PassWave w = pass_wave();
    const int lane = w.lane;
    const int32_t lo = a.lo, hi = a.hi;
    const uint32_t mask = FORM == INT_LIST_LDS ? (a.mask & (kIntListLdsSlots - 1)) : a.mask; // (the LDS copy is never indexed outside itself)
    const int32_t *tab = nullptr;
    if constexpr (FORM == INT_LIST_I8) {
        __shared__ uint32_t s_set[8];
        if (threadIdx.x < 8) s_set[threadIdx.x] = a.set[threadIdx.x];
        __syncthreads();
        tab = (const int32_t *)s_set;
    } else if constexpr (FORM == INT_LIST_LDS) {
        __shared__ int32_t s_tab[kIntListLdsSlots];
        for (uint32_t i = threadIdx.x; i <= mask; i += kBlockThreads) s_tab[i] = a.table[i];
        __syncthreads();
        tab = s_tab;
    } else if constexpr (FORM == INT_LIST_GLOBAL) {
        tab = a.table;
    }
    uint32_t lane_total = 0; // lanes 0..15: survivors in the words they stored
    for (int64_t tile = w.first; tile < a.pass.n_tiles; tile += w.step) {
        const PassTile t = pass_tile<TABLE>(a.pass, tile, I8 ? 1 : 4);
        const uint8_t *base = t.base;
        const uint32_t rows_here = t.rows_here;
        const uint64_t mine = pass_line_begin(a.pass, tile, lane);
        int32_t v[kTileWords];
        uint32_t valid = 0xFFFFu; // bit j: row 64 j + lane exists
        if (rows_here == (uint32_t)kTileRows) { // wave-uniform
#pragma unroll
            for (int j = 0; j < kTileWords; ++j) {
                if constexpr (I8) v[j] = (int32_t)__builtin_nontemporal_load((const int8_t *)base + 64 * j + lane);
                else v[j] = __builtin_nontemporal_load((const int32_t *)base + 64 * j + lane);
            }
        } else { // the end of a segment: nothing at or beyond the valid count is read
            valid = 0;
#pragma unroll
            for (int j = 0; j < kTileWords; ++j) {
                v[j] = 0;
                if ((uint32_t)(64 * j + lane) < rows_here) {
                    if constexpr (I8) v[j] = (int32_t)__builtin_nontemporal_load((const int8_t *)base + 64 * j + lane);
                    else v[j] = __builtin_nontemporal_load((const int32_t *)base + 64 * j + lane);
                    valid |= 1u << j;
                }
            }
        }
        uint32_t cand = 0; // bit j: row 64 j + lane exists and lies inside the folded interval
#pragma unroll
        for (int j = 0; j < kTileWords; ++j) cand |= in_closed(v[j], lo, hi) ? 1u << j : 0u;
        cand &= valid;
        const bool some = ballot64(cand != 0) != 0; // wave-uniform: some row of the tile lies inside the list's span
        uint64_t acc[kTileWords]; // wave-uniform words: bit l of word j = row 64 j + l is a member
        if constexpr (FORM == INT_LIST_ARGS) {
            // One flag per row block, not bits of one word: a flag is a lane mask in scalar registers, so a compare is ONE vector
            // instruction (its OR into the flag is a scalar one) and the ballot behind it is the flag itself.
            bool member[kTileWords];
#pragma unroll
            for (int j = 0; j < kTileWords; ++j) member[j] = false;
            if (some) {
#pragma unroll
                for (int m = 0; m < kMaxMatch; ++m) { // the list once per tile: the value is wave-uniform (a shorter list repeats its first value: no branch)
                    const int32_t x = a.inl[m];
#pragma unroll
                    for (int j = 0; j < kTileWords; ++j) member[j] = member[j] || v[j] == x;
                }
            }
#pragma unroll
            for (int j = 0; j < kTileWords; ++j) acc[j] = ballot64(member[j] && ((cand >> j) & 1u));
        } else {
            uint32_t found = 0; // bit j: row 64 j + lane is a member
            if (some) {
                if constexpr (FORM == INT_LIST_I8) {
                    const uint32_t *set = (const uint32_t *)tab;
#pragma unroll
                    for (int j = 0; j < kTileWords; ++j) found |= int_list_set_has(set, v[j]) ? 1u << j : 0u;
                    found &= cand;
                } else {
                    const int32_t empty = a.empty;
                    const uint32_t shift = a.shift, max_probe = a.max_probe;
                    uint32_t home[kTileWords];
                    uint32_t pend = 0; // bit j: row 64 j + lane has met neither its value nor an empty slot yet
#pragma unroll
                    for (int j = 0; j < kTileWords; ++j) { // step 0 of every row block: 16 reads in flight
                        home[j] = int_list_home(v[j], shift);
                        const bool c = ((cand >> j) & 1u) && v[j] != empty; // (`empty` is never a member, whatever the slots say)
                        int32_t x = empty;
                        if (c) x = tab[home[j] & mask];
                        found |= (c && x == v[j]) ? 1u << j : 0u;
                        pend |= (c && x != v[j] && x != empty) ? 1u << j : 0u;
                    }
#pragma unroll 1
                    for (uint32_t i = 1; i < max_probe && ballot64(pend != 0); ++i) { // wave-uniform over "any row still undecided"
#pragma unroll
                        for (int j = 0; j < kTileWords; ++j) {
                            if ((pend >> j) & 1u) {
                                const int32_t x = tab[(home[j] + i) & mask];
                                if (x == v[j]) found |= 1u << j;
                                if (x == v[j] || x == empty) pend &= ~(1u << j);
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < kTileWords; ++j) acc[j] = ballot64((found >> j) & 1u);
        }
        lane_total += pass_line_end(a.pass, tile, lane, rows_here, mine, acc);
    }
    pass_count_end(a.pass, lane_total, w);
}

// An int8 column: k_filter_tile's 6 work-groups per CU (filter_grid; a tile is 1 KiB).  An int32 column: 4 per CU -- a wave has ONE tile,
// 4 KiB, of loads in flight and none while it tests, so twice k_filter_tile's 512 work-groups pays (16 M rows, us at 512 / 1024 / 2048 /
// 4096 work-groups: 8 values 24.3 / 17.6 / 16.5 / 16.4, 9 values (LDS) 20.4 / 15.8 / 16.4 / 18.3, 4096 values (LDS) 157.2 / 96.4 / 96.0 /
// 96.8, 100 000 values (GLOBAL) 207.5 / 152.7 / 151.4 / 154.4: profiles/int_in.txt).  The LDS form's work-groups each copy the table
// (up to 32 KiB), so the finest grid is not the best one there; four of them fit a CU's 160 KiB.
int int_list_grid(int64_t n_tiles, int grid_blocks, int32_t width) {
    if (width != 4 || grid_blocks > 0) return filter_grid(n_tiles, false, width == 4, grid_blocks, 1);
    return (int)std::max<int64_t>(1, std::min<int64_t>((n_tiles + kWavesPerBlock - 1) / kWavesPerBlock, 1024));
}

// false: arguments no instance takes -- the form does not fit the width, the values or the table are not where the form reads them,
// or the table is not a power of two of slots the form can index
bool launch_filter_int_list(const IntListArgs &a, int grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (!column_pass_ok(a.pass, grid)) return false;
    if (a.form == INT_LIST_I8) {
        if (a.pass.width != 1) return false;
        IMM3_COLUMN_PASS_LAUNCH(k_filter_int_list, INT_LIST_I8);
    }
    if (a.pass.width != 4) return false;
    if (a.form == INT_LIST_ARGS) {
        if (a.n_values < 1 || a.n_values > kMaxMatch) return false;
        for (int m = a.n_values; m < kMaxMatch; ++m)
            if (a.inl[m] != a.inl[0]) return false; // (the kernel compares all kMaxMatch: the unused ones repeat the first)
        IMM3_COLUMN_PASS_LAUNCH(k_filter_int_list, INT_LIST_ARGS);
    }
    const uint64_t slots = (uint64_t)a.mask + 1;
    if (!a.table || slots < kIntListMinSlots || (slots & a.mask) != 0 || slots > (1ull << 25) || a.shift >= 32 || (32 - a.shift) != (uint32_t)__builtin_ctzll(slots)) return false;
    if (a.form == INT_LIST_LDS) {
        if (slots > kIntListLdsSlots) return false;
        IMM3_COLUMN_PASS_LAUNCH(k_filter_int_list, INT_LIST_LDS);
    }
    if (a.form == INT_LIST_GLOBAL) IMM3_COLUMN_PASS_LAUNCH(k_filter_int_list, INT_LIST_GLOBAL);
    return false;
}

} // namespace imm3
