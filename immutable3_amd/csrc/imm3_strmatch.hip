// imm3_strmatch.hip -- k_filter_str_rows: SelectIteratorMatch (Select.scala:25-51) over a DENSE_STRING / decoded SNAPPY_STRING column
// whose width is a whole number of dwords (4 .. 256 bytes), for gfx950 (wave64); and k_filter_str_range, its sibling for a
// byte-order range on such a column (IMM3_STR_RANGE; described at the kernel, below).
//
// Both are one-column passes of the select chain: geometry, tile addressing, the partial-tile rule, the bitmap line and the count are
// imm3_pass.h's; what is here is the loads and the two tests.
//
// Loads.  A tile starts at a multiple of 1024 * width bytes from a 16-byte-aligned base and width is a multiple of 4, so every row
// is dword-aligned: a lane reads the first P = min(width / 4, 4) dwords of each of its 16 rows with dword / dwordx2 / dwordx4
// loads (as wide as width's alignment allows), all 16 issued before the first compare -- up to 16 KiB in flight per wave.
// Two pieces are NOT shared, on measurements (profiles/column_pass.txt).  Each kernel carries the load block itself, and
// k_filter_str_range clears a partial tile's padding bits in that block's partial branch and ends its line with pass_line_store:
// with the loads as one function of both kernels, or with the rule left to pass_line_end, the compiler drops the range kernel's
// counted waits (s_waitcnt vmcnt(15) .. vmcnt(0)) behind a full tile's loads, and every compare waits for all 16 (S4: 70 -> 90 us).
//
// Compare.  The IN-list is walked ONCE PER TILE, not once per row: for value m (its dwords wave-uniform -- kernel arguments when the
// list fits them, else the device blob the fold step uploaded, read with scalar loads) every lane compares its 16 prefixes and
// collects a 16-bit candidate mask, bit j = row 64 j + l.  Up to 16 bytes the prefix is the whole row.  Wider rows: the candidates'
// remaining dwords are compared in a rolled loop that is wave-uniform over "any candidate left" -- per row block j with a candidate,
// chunk after chunk until the value ends or no lane of the wave is still a candidate.  A selective IN-list never enters it.
#include "imm3_internal.h"
#include "imm3_pass.h"
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
    const PassWave w = pass_wave();
    const int lane = w.lane;
    const uint32_t W = (uint32_t)a.pass.width; // bytes per row
    const int D = a.pass.width >> 2;           // dwords per row
    uint32_t lane_total = 0;                   // lanes 0..15: survivors in the words they stored
    for (int64_t tile = w.first; tile < a.pass.n_tiles; tile += w.step) {
        const PassTile t = pass_tile<TABLE>(a.pass, tile, W);
        const uint8_t *base = t.base;
        const uint64_t mine = pass_line_begin(a.pass, tile, lane);
        uint32_t pre[kTileWords][P];
        uint32_t valid = 0xFFFFu; // bit j: row 64 j + lane exists
        if (t.rows_here == (uint32_t)kTileRows) { // wave-uniform
#pragma unroll
            for (int j = 0; j < kTileWords; ++j) load_dwords<P, C>(pre[j], base + (uint32_t)(64 * j + lane) * W);
        } else { // the end of a segment: nothing at or beyond the valid count is read
            valid = 0;
#pragma unroll
            for (int j = 0; j < kTileWords; ++j) {
#pragma unroll
                for (int d = 0; d < P; ++d) pre[j][d] = 0;
                if ((uint32_t)(64 * j + lane) < t.rows_here) {
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
        lane_total += pass_line_end(a.pass, tile, lane, t.rows_here, mine, acc);
    }
    pass_count_end(a.pass, lane_total, w);
}

// ---- k_filter_str_range: IMM3_STR_RANGE, lo' <= row <= hi' in unsigned byte order, on the same columns --------------------------
// k_filter_str_rows' loads; the compare is an ORDER test where Match's is an equality test.  Byte order is unsigned dword order
// once a dword's bytes are swapped (one v_perm_b32 per dword); the host hands the
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
    const PassWave w = pass_wave();
    const int lane = w.lane;
    const uint32_t W = (uint32_t)a.pass.width; // bytes per row
    const int D = a.pass.width >> 2;           // dwords per row
    uint32_t lo[P], hi[P];
#pragma unroll
    for (int d = 0; d < P; ++d) { lo[d] = a.lo[d]; hi[d] = a.hi[d]; }
    uint32_t lane_total = 0;                   // lanes 0..15: survivors in the words they stored
    for (int64_t tile = w.first; tile < a.pass.n_tiles; tile += w.step) {
        const PassTile t = pass_tile<TABLE>(a.pass, tile, W);
        const uint8_t *base = t.base;
        uint64_t mine = pass_line_begin(a.pass, tile, lane);
        uint32_t pre[kTileWords][P];
        uint32_t valid = 0xFFFFu; // bit j: row 64 j + lane exists
        if (t.rows_here == (uint32_t)kTileRows) { // wave-uniform
#pragma unroll
            for (int j = 0; j < kTileWords; ++j) load_dwords<P, C>(pre[j], base + (uint32_t)(64 * j + lane) * W);
        } else { // the end of a segment: nothing at or beyond the valid count is read
            valid = 0;
#pragma unroll
            for (int j = 0; j < kTileWords; ++j) {
#pragma unroll
                for (int d = 0; d < P; ++d) pre[j][d] = 0;
                if ((uint32_t)(64 * j + lane) < t.rows_here) {
                    load_dwords<P, C>(pre[j], base + (uint32_t)(64 * j + lane) * W);
                    valid |= 1u << j;
                }
            }
            // This kernel's own partial-tile rule, where the parent had it (a row that does not exist compares as zeros, which a
            // range may hold), and pass_line_store below instead of pass_line_end: see the file-head comment
            mine &= low_mask((int64_t)t.rows_here - 64 * (int64_t)lane);
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
        lane_total += pass_line_store(a.pass, tile, lane, mine, acc);
    }
    pass_count_end(a.pass, lane_total, w);
}

bool str_rows_width_ok(int32_t width) { return width >= 4 && width <= kStrMaxWidth && width % 4 == 0; }

// 2 work-groups per CU, as k_filter_tile with an int32 column: a wave keeps 4 KiB (width 4) to 16 KiB of loads in flight, and the
// 16-byte instances hold ~200 vector registers (two waves per SIMD)
int str_rows_grid(int64_t n_tiles, int grid_blocks) {
    const int64_t cap = grid_blocks > 0 ? std::min(grid_blocks, kMaxFilterGrid) : 512;
    return (int)std::max<int64_t>(1, std::min<int64_t>((n_tiles + kWavesPerBlock - 1) / kWavesPerBlock, cap));
}

// the seven <P, C, TAIL> instances of either kernel, by width (a multiple of 4); launches one and returns true
#define IMM3_STR_LAUNCH_BY_WIDTH(kern)                                               \
    do {                                                                             \
        const int32_t width = a.pass.width;                                          \
        if (width == 4) IMM3_COLUMN_PASS_LAUNCH(kern, 1, 1, false);                  \
        if (width == 8) IMM3_COLUMN_PASS_LAUNCH(kern, 2, 2, false);                  \
        if (width == 12) IMM3_COLUMN_PASS_LAUNCH(kern, 3, 1, false);                 \
        if (width == 16) IMM3_COLUMN_PASS_LAUNCH(kern, 4, 4, false);                 \
        if (width % 16 == 0) IMM3_COLUMN_PASS_LAUNCH(kern, 4, 4, true);              \
        if (width % 8 == 0) IMM3_COLUMN_PASS_LAUNCH(kern, 4, 2, true);               \
        IMM3_COLUMN_PASS_LAUNCH(kern, 4, 1, true);                                   \
    } while (0)

// false: no instance for this width, or the IN-list's values are not where the instance reads them
bool launch_filter_str_rows(const StrRowsArgs &a, int grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (!column_pass_ok(a.pass, grid) || !str_rows_width_ok(a.pass.width) || a.n_match < 0) return false;
    if (!a.values && (a.pass.width > 8 || a.n_match > kMaxMatch)) return false;
    IMM3_STR_LAUNCH_BY_WIDTH(k_filter_str_rows);
}

// false: no instance for this width, or the tails are not where the instance reads them
bool launch_filter_str_range(const StrRangeArgs &a, int grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (!column_pass_ok(a.pass, grid) || !str_rows_width_ok(a.pass.width)) return false;
    if (a.pass.width > 16 && !a.tails) return false;
    IMM3_STR_LAUNCH_BY_WIDTH(k_filter_str_range);
}

} // namespace imm3
