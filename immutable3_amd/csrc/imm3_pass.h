// imm3_pass.h -- the device pieces of a ONE-COLUMN PASS of the select chain (k_filter_str_rows, k_filter_str_range,
// k_filter_int_list; arguments: ColumnPassArgs, imm3_internal.h; the contract in words: DESIGN.md §3b).  A kernel keeps its
// `for (tile ...)` loop, its loads and its test, and calls: pass_tile, pass_line_begin, [loads under the row's validity; test],
// pass_line_end; once per wave pass_count_end.
#pragma once

#include "imm3_device.h"

namespace imm3 {

// the wave's place in the launch: tiles first, first + step, ...
struct PassWave {
    int lane, wave;
    int64_t first, step;
};
__device__ __forceinline__ PassWave pass_wave() {
    const int wave = threadIdx.x >> 6;
    return {(int)(threadIdx.x & 63), wave, (int64_t)blockIdx.x * kWavesPerBlock + wave, (int64_t)gridDim.x * kWavesPerBlock};
}

struct PassTile {
    const uint8_t *base; // the tile's first row
    uint32_t rows_here;  // valid rows (kTileRows: a full tile); wave-uniform
};
// TABLE: the tiles come from a tile table (one partial tile per segment)
template <bool TABLE>
__device__ __forceinline__ PassTile pass_tile(const ColumnPassArgs &p, int64_t tile, uint32_t row_bytes) {
    if constexpr (TABLE) {
        return {(const uint8_t *)as_global(p.tile_ptrs[tile]), p.tile_rows[tile]}; // (as_global: no flat loads through a pointer read from memory)
    } else {
        const int64_t left = p.n_rows - tile * kTileRows;
        return {(const uint8_t *)p.data + (size_t)tile * kTileRows * row_bytes, left >= kTileRows ? (uint32_t)kTileRows : (uint32_t)left};
    }
}

// lane j < 16 owns bitmap word j of the tile: what the passes before this one left there (and_existing), else all ones
__device__ __forceinline__ uint64_t pass_line_begin(const ColumnPassArgs &p, int64_t tile, int lane) {
    uint64_t mine = ~0ULL;
    if (p.and_existing) mine = lane < kTileWords ? p.bitmap[tile * kTileWords + lane] : 0ULL;
    return mine;
}

// ANDs the 16 wave-uniform words (bit l of word j = row 64 j + l passes) into the line, stores it -- 16 lanes x 8 B = one 128-B
// non-temporal line; the bitmap is allocated in whole tiles -- and returns the lane's survivors
__device__ __forceinline__ uint32_t pass_line_store(const ColumnPassArgs &p, int64_t tile, int lane, uint64_t mine, const uint64_t (&acc)[kTileWords]) {
    mine &= words_to_lanes(acc);
    if (lane >= kTileWords) mine = 0;
    if (lane < kTileWords) __builtin_nontemporal_store(mine, p.bitmap + tile * kTileWords + lane);
    return (uint32_t)__popcll(mine);
}
// The line end: first CLEARS THE BITS OF ROWS AT OR BEYOND rows_here, so the kernel's test may say anything about a row that
// does not exist.  A scalar branch (readfirstlane: rows_here is the wave's): a full tile skips it.
__device__ __forceinline__ uint32_t pass_line_end(const ColumnPassArgs &p, int64_t tile, int lane, uint32_t rows_here, uint64_t mine, const uint64_t (&acc)[kTileWords]) {
    if (__builtin_amdgcn_readfirstlane((int)rows_here) != kTileRows) mine &= low_mask((int64_t)rows_here - 64 * (int64_t)lane);
    return pass_line_store(p, tile, lane, mine, acc);
}

// lane_total: the sum of the lane's line-end results; per-work-group partials that k_total sums
__device__ __forceinline__ void pass_count_end(const ColumnPassArgs &p, uint32_t lane_total, const PassWave &w) {
    block_partial_store(p.block_partials, wave_sum(lane_total), w.lane, w.wave);
}

} // namespace imm3
