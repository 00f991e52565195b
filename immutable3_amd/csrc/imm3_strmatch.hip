// imm3_strmatch.hip -- k_filter_str_rows: SelectIteratorMatch (Select.scala:25-51) over a DENSE_STRING / decoded SNAPPY_STRING column
// whose width is a whole number of dwords (4 .. 256 bytes), for gfx950 (wave64); and k_filter_str_range, its sibling for a
// byte-order range on such a column (IMM3_STR_RANGE; described at the kernel, below).
//
// k_filter_tile's geometry: one wave per 1024-row tile, grid-stride; lane l holds row 64 j + l of the tile in register set j, so the
// ballot over "row matches" IS bitmap word j, and the tile's 16 words leave as one 128-byte line (lanes 0..15, 8 bytes each).
//
// Loads.  A tile starts at a multiple of 1024 * width bytes from a 16-byte-aligned base and width is a multiple of 4, so every row is
// dword-aligned: a lane reads the first P = min(width / 4, 4) dwords of each of its 16 rows with dword / dwordx2 / dwordx4 loads
// (as wide as width's alignment allows), all 16 issued before the first compare -- up to 16 KiB in flight per wave.
//
// Compare.  The IN-list is walked ONCE PER TILE, not once per row: for value m (its dwords wave-uniform -- kernel arguments when the
// list fits them, else the device blob the fold step uploaded, read with scalar loads) every lane compares its 16 prefixes and
// collects a 16-bit candidate mask, bit j = row 64 j + l.  Up to 16 bytes the prefix is the whole row.  Wider rows: the candidates'
// remaining dwords are compared in a rolled loop that is wave-uniform over "any candidate left" -- per row block j with a candidate,
// chunk after chunk until the value ends or no lane of the wave is still a candidate.  A selective IN-list never enters it.
//
// Bounds.  A partial last tile (the end of a segment) loads under the row's validity: no byte of a row at or beyond the tile's valid
// count is read, so the kernel needs no readable slack behind the column however wide its rows are.
//
// Count: per-work-group partials (block_partial_store), summed by k_total, like the word-at-a-time kernel's.
#include "imm3_internal.h"
#include "imm3_device.h"
#include <hip/hip_ext.h>

namespace imm3 {

namespace {

template <int C> struct StrChunk;
template <> struct StrChunk<1> { typedef uint32_t type; };
template <> struct StrChunk<2> { typedef uint32_t type __attribute__((ext_vector_type(2))); };
template <> struct StrChunk<4> { typedef uint32_t type __attribute__((ext_vector_type(4))); };

// N dwords at p (aligned to 4 * C bytes, N % C == 0), read once: non-temporal
template <int N, int C>
__device__ __forceinline__ void load_dwords(uint32_t (&v)[N], const uint8_t *p) {
    typedef typename StrChunk<C>::type vec;
#pragma unroll
    for (int i = 0; i < N / C; ++i) {
        const vec x = __builtin_nontemporal_load((const vec *)p + i);
        if constexpr (C == 1) v[i] = x;
        else {
#pragma unroll
            for (int k = 0; k < C; ++k) v[i * C + k] = x[k];
        }
    }
}

} // namespace

// P: dwords of the prefix (the whole row when !TAIL); C: dwords per load (width's alignment / 4); TAIL: width > 16 bytes;
// TABLE: the tiles come from a tile table (one partial tile per segment)
template <int P, int C, bool TAIL, bool TABLE>
__global__ __launch_bounds__(kBlockThreads) void k_filter_str_rows(const StrRowsArgs a) {
    static_assert(P % C == 0 && P <= kStrPrefixDwords, "the prefix is whole chunks");
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t wave_id = (int64_t)blockIdx.x * kWavesPerBlock + wave;
    const int64_t n_waves = (int64_t)gridDim.x * kWavesPerBlock;
    const uint32_t W = (uint32_t)a.width;   // bytes per row
    const int D = a.width >> 2;             // dwords per row
    uint32_t lane_total = 0;                // lanes 0..15: survivors in the words they stored
    for (int64_t tile = wave_id; tile < a.n_tiles; tile += n_waves) {
        const uint8_t *base;
        uint32_t rows_here;
        if constexpr (TABLE) {
            rows_here = a.tile_rows[tile];
            base = (const uint8_t *)as_global(a.tile_ptrs[tile]); // (as_global: no flat loads through a pointer read from memory)
        } else {
            const int64_t left = a.n_rows - tile * kTileRows;
            rows_here = left >= kTileRows ? (uint32_t)kTileRows : (uint32_t)left;
            base = (const uint8_t *)a.data + (size_t)tile * kTileRows * W;
        }
        const int64_t w = tile * kTileWords + lane; // lane j < 16 owns bitmap word j of the tile
        uint64_t mine = ~0ULL;
        if (a.and_existing) mine = lane < kTileWords ? a.bitmap[w] : 0ULL;
        uint32_t pre[kTileWords][P];
        uint32_t valid = 0xFFFFu; // bit j: row 64 j + lane exists
        if (rows_here == (uint32_t)kTileRows) { // wave-uniform
#pragma unroll
            for (int j = 0; j < kTileWords; ++j) load_dwords<P, C>(pre[j], base + (uint32_t)(64 * j + lane) * W);
        } else { // the end of a segment: nothing at or beyond the valid count is read
            valid = 0;
#pragma unroll
            for (int j = 0; j < kTileWords; ++j) {
#pragma unroll
                for (int d = 0; d < P; ++d) pre[j][d] = 0;
                if ((uint32_t)(64 * j + lane) < rows_here) {
                    load_dwords<P, C>(pre[j], base + (uint32_t)(64 * j + lane) * W);
                    valid |= 1u << j;
                }
            }
        }
        uint32_t found = 0; // bit j: row 64 j + lane equals an IN-list value
        // one IN-list value (v: its dwords, wave-uniform) against the lane's 16 rows
        auto test_value = [&](const uint32_t *v) {
            uint32_t vp[P];
#pragma unroll
            for (int d = 0; d < P; ++d) vp[d] = v[d];
            uint32_t cand = 0;
#pragma unroll
            for (int j = 0; j < kTileWords; ++j) {
                bool eq = true;
#pragma unroll
                for (int d = 0; d < P; ++d) eq &= pre[j][d] == vp[d];
                cand |= eq ? 1u << j : 0u;
            }
            cand &= valid;
            if constexpr (TAIL) {
                if (ballot64(cand != 0)) { // wave-uniform: some row of the tile shares the value's first 16 bytes
#pragma unroll 1
                    for (int j = 0; j < kTileWords; ++j) {
                        bool c = (cand >> j) & 1u;
                        if (!ballot64(c)) continue;
                        const uint8_t *rp = base + (uint32_t)(64 * j + lane) * W;
#pragma unroll 1
                        for (int d = P; d < D && ballot64(c); d += C) { // wave-uniform over "any candidate left"
                            if (c) {
                                uint32_t x[C];
                                load_dwords<C, C>(x, rp + 4 * d);
#pragma unroll
                                for (int k = 0; k < C; ++k) c &= x[k] == v[d + k];
                            }
                        }
                        if (!c) cand &= ~(1u << j);
                    }
                }
            }
            found |= cand;
        };
        if (TAIL || a.values) { // (a row wider than 8 bytes always has its values in the blob)
            for (int m = 0; m < a.n_match; ++m) test_value(a.values + (size_t)m * D);
        } else { // the list fits the kernel arguments (width <= 8, <= kMaxMatch values)
            for (int m = 0; m < a.n_match; ++m) test_value(a.inl[m]);
        }
        uint64_t acc[kTileWords]; // wave-uniform words
#pragma unroll
        for (int j = 0; j < kTileWords; ++j) acc[j] = ballot64((found >> j) & 1u);
        mine &= words_to_lanes(acc);
        if (lane >= kTileWords) mine = 0;
        if (lane < kTileWords) __builtin_nontemporal_store(mine, a.bitmap + w); // 16 lanes x 8 B = one 128-B line (the bitmap is allocated in whole tiles)
        lane_total += (uint32_t)__popcll(mine);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) lane_total += __shfl_xor(lane_total, d);
    block_partial_store(a.block_partials, lane_total, lane, wave);
}

// ---- k_filter_str_range: IMM3_STR_RANGE, lo' <= row <= hi' in unsigned byte order, on the same columns --------------------------
// k_filter_str_rows' geometry, loads, partial-tile rule, bitmap line and partials; the compare is an ORDER test where Match's is an
// equality test.  Byte order is unsigned dword order once a dword's bytes are swapped (one v_perm_b32 per dword); the host hands the
// bounds already swapped (str_range_pack), wave-uniform: the first 16 bytes as kernel arguments, the tails of wider rows in device
// memory.  Against each bound a row's prefix is below, tied or above -- the first dword that differs decides, which is what the
// chain below computes from the last prefix dword to the first (the lane masks it combines are scalar registers: the vector unit
// issues the swaps and two compares per dword and bound).  A row below lo's prefix or above hi's is out; up to 16 bytes a tie is in
// (the interval is closed).  Wider rows: only the rows TIED with a bound's prefix are undecided, and the wave enters a rolled loop
// only if some lane has one -- per row block with such a row, chunk after chunk until the first differing dword decides, wave-uniform
// over "any row still undecided" as Match's candidate loop; a row tied with both bounds (they share their first 16 bytes) walks
// both.  A range whose bounds no row's prefix touches never enters it.
template <int P, int C, bool TAIL, bool TABLE>
__global__ __launch_bounds__(kBlockThreads) void k_filter_str_range(const StrRangeArgs a) {
    static_assert(P % C == 0 && P <= kStrPrefixDwords, "the prefix is whole chunks");
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t wave_id = (int64_t)blockIdx.x * kWavesPerBlock + wave;
    const int64_t n_waves = (int64_t)gridDim.x * kWavesPerBlock;
    const uint32_t W = (uint32_t)a.width;   // bytes per row
    const int D = a.width >> 2;             // dwords per row
    uint32_t lo[P], hi[P];
#pragma unroll
    for (int d = 0; d < P; ++d) { lo[d] = a.lo[d]; hi[d] = a.hi[d]; }
    uint32_t lane_total = 0;                // lanes 0..15: survivors in the words they stored
    for (int64_t tile = wave_id; tile < a.n_tiles; tile += n_waves) {
        const uint8_t *base;
        uint32_t rows_here;
        if constexpr (TABLE) {
            rows_here = a.tile_rows[tile];
            base = (const uint8_t *)as_global(a.tile_ptrs[tile]);
        } else {
            const int64_t left = a.n_rows - tile * kTileRows;
            rows_here = left >= kTileRows ? (uint32_t)kTileRows : (uint32_t)left;
            base = (const uint8_t *)a.data + (size_t)tile * kTileRows * W;
        }
        const int64_t w = tile * kTileWords + lane; // lane j < 16 owns bitmap word j of the tile
        uint64_t mine = ~0ULL;
        if (a.and_existing) mine = lane < kTileWords ? a.bitmap[w] : 0ULL;
        uint32_t pre[kTileWords][P];
        uint32_t valid = 0xFFFFu; // bit j: row 64 j + lane exists
        if (rows_here == (uint32_t)kTileRows) { // wave-uniform
#pragma unroll
            for (int j = 0; j < kTileWords; ++j) load_dwords<P, C>(pre[j], base + (uint32_t)(64 * j + lane) * W);
        } else { // the end of a segment: nothing at or beyond the valid count is read
            valid = 0;
#pragma unroll
            for (int j = 0; j < kTileWords; ++j) {
#pragma unroll
                for (int d = 0; d < P; ++d) pre[j][d] = 0;
                if ((uint32_t)(64 * j + lane) < rows_here) {
                    load_dwords<P, C>(pre[j], base + (uint32_t)(64 * j + lane) * W);
                    valid |= 1u << j;
                }
            }
            // (a row that does not exist compares as zeros, which a range may hold: its bit goes with the word's valid mask)
            mine &= low_mask((int64_t)rows_here - 64 * (int64_t)lane);
        }
        uint64_t acc[kTileWords]; // wave-uniform words
        uint32_t in = 0, tie_lo = 0, tie_hi = 0; // TAIL: bit j = row 64 j + lane is in by its prefix / tied with lo's / with hi's
#pragma unroll
        for (int j = 0; j < kTileWords; ++j) {
            // ge: prefix >= lo's (tied included), le: prefix <= hi's; tl / th: tied
            bool ge = true, le = true, tl = true, th = true;
#pragma unroll
            for (int d = P - 1; d >= 0; --d) {
                const uint32_t x = __builtin_bswap32(pre[j][d]);
                const bool el = x == lo[d], eh = x == hi[d];
                ge = x > lo[d] || (el && ge);
                le = x < hi[d] || (eh && le);
                if constexpr (TAIL) { tl = tl && el; th = th && eh; }
            }
            if constexpr (TAIL) {
                in |= (ge && le) ? 1u << j : 0u;
                tie_lo |= tl ? 1u << j : 0u;
                tie_hi |= th ? 1u << j : 0u;
            } else acc[j] = ballot64(ge && le);
        }
        if constexpr (TAIL) {
            // the rows tied with bound `b`'s prefix (below: lo, a row under it is out; else hi, a row over it is out): out of `in`
            // once a dword of the tail says so
            auto walk = [&](uint32_t tie, const uint32_t *b, bool below) {
                tie &= valid & in; // (no row beyond the valid count is read; a row the other bound has put out needs no walk)
                if (!ballot64(tie != 0)) return; // wave-uniform
#pragma unroll 1
                for (int j = 0; j < kTileWords; ++j) {
                    bool c = (tie >> j) & 1u; // still undecided
                    if (!ballot64(c)) continue;
                    const uint8_t *rp = base + (uint32_t)(64 * j + lane) * W;
                    bool out = false;
#pragma unroll 1
                    for (int d = P; d < D && ballot64(c); d += C) { // wave-uniform over "any row still undecided"
                        if (c) {
                            uint32_t x[C];
                            load_dwords<C, C>(x, rp + 4 * d);
#pragma unroll
                            for (int k = 0; k < C; ++k) {
                                const uint32_t xs = __builtin_bswap32(x[k]), bs = b[d + k];
                                if (c && xs != bs) {
                                    out = below ? xs < bs : xs > bs;
                                    c = false;
                                }
                            }
                        }
                    }
                    if (out) in &= ~(1u << j);
                }
            };
            walk(tie_lo, a.tails, true);
            walk(tie_hi, a.tails + D, false);
#pragma unroll
            for (int j = 0; j < kTileWords; ++j) acc[j] = ballot64((in >> j) & 1u);
        }
        mine &= words_to_lanes(acc);
        if (lane >= kTileWords) mine = 0;
        if (lane < kTileWords) __builtin_nontemporal_store(mine, a.bitmap + w); // one 128-B line, as k_filter_str_rows
        lane_total += (uint32_t)__popcll(mine);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) lane_total += __shfl_xor(lane_total, d);
    block_partial_store(a.block_partials, lane_total, lane, wave);
}

bool str_rows_width_ok(int32_t width) { return width >= 4 && width <= kStrMaxWidth && width % 4 == 0; }

// 2 work-groups per CU, as k_filter_tile with an int32 column: a wave keeps 4 KiB (width 4) to 16 KiB of loads in flight, and the
// 16-byte instances hold ~200 vector registers (two waves per SIMD)
int str_rows_grid(int64_t n_tiles, int grid_blocks) {
    const int64_t cap = grid_blocks > 0 ? std::min(grid_blocks, kMaxFilterGrid) : 512;
    return (int)std::max<int64_t>(1, std::min<int64_t>((n_tiles + kWavesPerBlock - 1) / kWavesPerBlock, cap));
}

#define IMM3_STR_LAUNCH(P, C, TAIL)                                                                                \
    do {                                                                                                           \
        if (a.tile_rows) IMM3_LAUNCH((k_filter_str_rows<P, C, TAIL, true>), grid, kBlockThreads, s, ev0, ev1, a);  \
        else IMM3_LAUNCH((k_filter_str_rows<P, C, TAIL, false>), grid, kBlockThreads, s, ev0, ev1, a);             \
        return true;                                                                                               \
    } while (0)

// false: no instance for this width, or the IN-list's values are not where the instance reads them
bool launch_filter_str_rows(const StrRowsArgs &a, int grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (!str_rows_width_ok(a.width) || !a.bitmap || grid < 1 || grid > kMaxFilterGrid || a.n_match < 0) return false;
    if (!a.values && (a.width > 8 || a.n_match > kMaxMatch)) return false;
    if (a.width == 4) IMM3_STR_LAUNCH(1, 1, false);
    if (a.width == 8) IMM3_STR_LAUNCH(2, 2, false);
    if (a.width == 12) IMM3_STR_LAUNCH(3, 1, false);
    if (a.width == 16) IMM3_STR_LAUNCH(4, 4, false);
    if (a.width % 16 == 0) IMM3_STR_LAUNCH(4, 4, true);
    if (a.width % 8 == 0) IMM3_STR_LAUNCH(4, 2, true);
    IMM3_STR_LAUNCH(4, 1, true);
}

#define IMM3_STR_RANGE_LAUNCH(P, C, TAIL)                                                                          \
    do {                                                                                                           \
        if (a.tile_rows) IMM3_LAUNCH((k_filter_str_range<P, C, TAIL, true>), grid, kBlockThreads, s, ev0, ev1, a); \
        else IMM3_LAUNCH((k_filter_str_range<P, C, TAIL, false>), grid, kBlockThreads, s, ev0, ev1, a);            \
        return true;                                                                                               \
    } while (0)

// the same seven instances by width; false: no instance for this width, or the tails are not where the instance reads them
bool launch_filter_str_range(const StrRangeArgs &a, int grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (!str_rows_width_ok(a.width) || !a.bitmap || grid < 1 || grid > kMaxFilterGrid) return false;
    if (a.width > 16 && !a.tails) return false;
    if (a.width == 4) IMM3_STR_RANGE_LAUNCH(1, 1, false);
    if (a.width == 8) IMM3_STR_RANGE_LAUNCH(2, 2, false);
    if (a.width == 12) IMM3_STR_RANGE_LAUNCH(3, 1, false);
    if (a.width == 16) IMM3_STR_RANGE_LAUNCH(4, 4, false);
    if (a.width % 16 == 0) IMM3_STR_RANGE_LAUNCH(4, 4, true);
    if (a.width % 8 == 0) IMM3_STR_RANGE_LAUNCH(4, 2, true);
    IMM3_STR_RANGE_LAUNCH(4, 1, true);
}

} // namespace imm3
