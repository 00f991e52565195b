// imm3_expr.hip -- the scan+select kernels of a select TREE (AND / OR / NOT over SelectOp leaves), gfx950, wave64.
//
// The reference's PipelineThread.runOps applies every SelectOp of a SelectADT one after the other whatever the node's tag says
// (engine/Engine.scala:236-245, "TODO: use AND/OR operators"): every tree is a conjunction there, and so it is through
// imm3_query_create.  A query made by imm3_query_create_expr honours the tags.  The host rewrites the tree into a disjunction of
// TERMS (imm3_expr_norm.cpp), each a conjunction with at most one folded predicate per column -- what a flat select list folds to -- and
// ONE launch of one of the two kernels here writes the batch-major bitmap that everything behind it (count, k_scan, k_gather, the
// aggregation kernels) reads.
//
//   k_filter_expr<K0, K1, K2>   k_filter_tile's geometry: one wave per 1024-row tile, grid-stride, every load of a tile issued before
//                               the first compare, one 128-byte bitmap line per tile, the count reduced in the kernel.  A column is
//                               loaded (and, when narrow, transposed through LDS) ONCE per tile and tested once per term that
//                               constrains it: per term the columns' words AND into a fresh accumulator (s_and_b64), the terms'
//                               accumulators OR into the tile's words (s_or_b64).  The narrow-only kinds evaluate in the lane, as
//                               k_filter_tile's do: one 16-bit mask per term and column, AND / OR in the vector unit, and the same
//                               DPP assembly of the bitmap word.
//                               Its TABLE instances walk an imm3_table's tile table as k_filter_tile's do (one tile per step, the
//                               partial tile that ends each segment rolled): the select tree over ALL segments is one launch.
//                               A term's string predicate may be a NEGATED list (a complemented Match under IMM3_EXPR_NOT): the
//                               flag travels with the list and turns the match around where it is taken, inside every bounds check.
//   k_filter_expr_generic       any column kind, any layout, up to 64 terms: one row per lane, one bitmap word per wave and step,
//                               the terms' ColPreds read from device memory.  One segment only.
#include "imm3_internal.h"
#include "imm3_device.h"
#include "imm3_tile.h"
#include <hip/hip_ext.h>
#include <type_traits>

namespace imm3 {

// narrow-only kinds are evaluated in the lane (imm3_kernels.hip, lane_tile(): 1 = the lane's 16 consecutive rows, 2 = two runs of 8
// rows beside a 2-byte-string column), everything else row-strided with one ballot per bitmap word
constexpr int expr_lane_tile(int k0, int k1, int k2) {
    if (!(k0 == TK_I8 || k0 == TK_S2) || k1 == TK_I32 || k2 == TK_I32) return 0;
    return (k0 == TK_S2 || k1 == TK_S2 || k2 == TK_S2) ? 2 : 1;
}

template <int LANE, int K>
__device__ __forceinline__ void expr_load(ColRegs<K> &c, const void *data, int64_t row0, int lane) {
    if constexpr (LANE == 1) c.load_lane_rows(data, row0, lane);
    else if constexpr (LANE == 2) c.load_lane_rows_split(data, row0, lane);
    else c.load(data, row0, lane);
}

// A string predicate of a tree may be NEGATED (a complemented Match: TileCol::negated, wave-uniform, read from the kernel arguments
// with the list): keep the rows that equal NONE of the values.  Only a 2-byte string column has a list, and only the NEG instances
// of the kernels look at the flag: the host launches them for a tree that carries a negated list (launch_filter_expr) and the
// plain instances for every other tree, which therefore run the code they ran before NOT existed -- the test of the flag inside the
// term loops of ONE instance cost the trees without NOT 3 - 13 % (more SGPR spills around the row-strided kinds' 32 word pairs).
// Within a NEG instance the flag is one scalar test per term and string column.
// in-lane: the term's 16-bit match mask XORed with the lane's all-rows mask (full tiles only: every one of the 16 rows exists)
template <bool NEG, int K>
__device__ __forceinline__ uint32_t expr_col_lane_mask(const ColRegs<K> &c, const TileCol &col) {
    uint32_t m = c.lane_mask(col);
    if constexpr (NEG && K == TK_S2) {
        if (col.negated) m ^= 0xFFFFu;
    }
    return m;
}
// row-strided: the ballot of "not matched"
template <bool NEG, int K>
__device__ __forceinline__ void expr_col_test(ColRegs<K> &c, const TileCol &col, uint64_t (&ta)[kTileWords]) {
    if constexpr (NEG && K == TK_S2) {
        if (col.negated) {
            c.test_not(col, ta);
            return;
        }
    }
    c.test(col, ta);
}
// one row of the rolled partial tile (the caller has it inside its bounds check: a row that does not exist is never evaluated as "not matched")
template <bool NEG, int K>
__device__ __forceinline__ bool expr_col_row(ColRegs<K> &c, const void *data, const TileCol &col, int64_t r) {
    const bool hit = c.row(data, col, r);
    if constexpr (NEG && K == TK_S2) return hit != (col.negated != 0);
    else return hit;
}

// the in-lane kinds: OR over the terms of the AND of the constrained columns' masks (wave-uniform control flow: `use` is scalar)
template <int K0, int K1, int K2, bool NEG>
__device__ __forceinline__ uint32_t expr_lane_mask(const ExprTermArgs &a, const ColRegs<K0> &c0, const ColRegs<K1> &c1, const ColRegs<K2> &c2) {
    uint32_t m = 0;
    for (int t = 0; t < a.n_terms; ++t) {
        const uint32_t u = a.use[t];
        uint32_t tm = 0xFFFFu;
        if (K0 != TK_NONE && (u & 1u)) tm &= expr_col_lane_mask<NEG>(c0, a.cols[t][0]);
        if (K1 != TK_NONE && (u & 2u)) tm &= expr_col_lane_mask<NEG>(c1, a.cols[t][1]);
        if (K2 != TK_NONE && (u & 4u)) tm &= expr_col_lane_mask<NEG>(c2, a.cols[t][2]);
        m |= tm;
    }
    return m;
}

// One full tile whose columns are in registers -> its bitmap line (unless count-only); returns the lane's share of the survivors
// (whichever lanes count: every lane, the word owners, or lane 0 -- the caller sums over the wave).
template <int K0, int K1, int K2, bool NEG>
__device__ __forceinline__ uint32_t expr_full_tile(const ExprTermArgs &a, int64_t tile, int lane, ColRegs<K0> &c0, ColRegs<K1> &c1, ColRegs<K2> &c2, uint8_t *xp) {
    constexpr int kLane = expr_lane_tile(K0, K1, K2);
    if constexpr (kLane == 2) {
        const uint32_t m = expr_lane_mask<K0, K1, K2, NEG>(a, c0, c1, c2); // byte 0: rows 8 lane .. + 7, byte 1: 512 + 8 lane .. + 7
        if (!a.bitmap) return (uint32_t)__popc(m);
        // eight lanes' bytes -> one word, for both runs at once (k_filter_tile's assembly: pairs, quads, then the upper quad's half)
        const uint32_t odd = (uint32_t)__builtin_amdgcn_mov_dpp((int)m, 0xF5, 0xF, 0xF, true);      // quad_perm [1,1,3,3]
        const uint32_t x = __builtin_amdgcn_perm(odd, m, 0x05010400u);
        const uint32_t y = (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xAA, 0xF, 0xF, true);         // quad_perm [2,2,2,2]
        const uint32_t lo_a = __builtin_amdgcn_perm(y, x, 0x05040100u), lo_b = __builtin_amdgcn_perm(y, x, 0x07060302u);
        const uint32_t hi_a = (uint32_t)__builtin_amdgcn_mov_dpp((int)lo_a, 0x104, 0xF, 0xF, true);  // row_shl:4: the quad above
        const uint32_t hi_b = (uint32_t)__builtin_amdgcn_mov_dpp((int)lo_b, 0x104, 0xF, 0xF, true);
        const bool owner = (lane & 7) == 0; // lane 8 w owns words w and 8 + w
        const int64_t wl = tile * kTileWords + (lane >> 3);
        uint64_t word_a = ((uint64_t)hi_a << 32) | (uint64_t)lo_a, word_b = ((uint64_t)hi_b << 32) | (uint64_t)lo_b;
        if (!owner) word_a = word_b = 0;
        if (owner) {
            __builtin_nontemporal_store(word_a, a.bitmap + wl);
            __builtin_nontemporal_store(word_b, a.bitmap + wl + kTileWords / 2);
        }
        return (uint32_t)(__popcll(word_a) + __popcll(word_b));
    } else if constexpr (kLane == 1) {
        const uint32_t m = expr_lane_mask<K0, K1, K2, NEG>(a, c0, c1, c2); // rows 16 lane .. 16 lane + 15
        if (!a.bitmap) return (uint32_t)__popc(m);
        const uint32_t odd = (uint32_t)__builtin_amdgcn_mov_dpp((int)m, 0xF5, 0xF, 0xF, true);       // quad_perm [1,1,3,3]
        const uint32_t pair = m | (odd << 16);
        const uint32_t high = (uint32_t)__builtin_amdgcn_mov_dpp((int)pair, 0xAA, 0xF, 0xF, true);    // quad_perm [2,2,2,2]
        const bool owner = (lane & 3) == 0; // lane 4 w owns word w
        uint64_t word = ((uint64_t)high << 32) | (uint64_t)pair;
        if (!owner) word = 0;
        if (owner) __builtin_nontemporal_store(word, a.bitmap + tile * kTileWords + (lane >> 2));
        return (uint32_t)__popcll(word);
    } else {
        // narrow columns: transposed through LDS once per tile (the values stay in registers for every term)
        c0.stage(lane, xp);
        c1.stage(lane, xp);
        c2.stage(lane, xp);
        uint64_t acc[kTileWords]; // wave-uniform words (SGPR pairs)
#pragma unroll
        for (int j = 0; j < kTileWords; ++j) acc[j] = 0ULL;
        for (int t = 0; t < a.n_terms; ++t) {
            const uint32_t u = a.use[t];
            uint64_t ta[kTileWords];
#pragma unroll
            for (int j = 0; j < kTileWords; ++j) ta[j] = ~0ULL;
            if (K0 != TK_NONE && (u & 1u)) expr_col_test<NEG>(c0, a.cols[t][0], ta);
            if (K1 != TK_NONE && (u & 2u)) expr_col_test<NEG>(c1, a.cols[t][1], ta);
            if (K2 != TK_NONE && (u & 4u)) expr_col_test<NEG>(c2, a.cols[t][2], ta);
#pragma unroll
            for (int j = 0; j < kTileWords; ++j) acc[j] |= ta[j];
        }
        if (!a.bitmap) { // count-only run: the words never leave the scalar registers
            uint32_t cnt = 0;
#pragma unroll
            for (int j = 0; j < kTileWords; ++j) cnt += (uint32_t)__popcll(acc[j]);
            return lane == 0 ? cnt : 0u;
        }
        uint64_t mine = words_to_lanes(acc); // lane j < 16 owns bitmap word j of the tile
        if (lane >= kTileWords) mine = 0;
        if (lane < kTileWords) __builtin_nontemporal_store(mine, a.bitmap + tile * kTileWords + lane); // 16 lanes x 8 B = one 128-B line
        return (uint32_t)__popcll(mine);
    }
}

// A tile with fewer than 1024 valid rows (the end of a segment): rolled, bounds-checked, row-at-a-time.
// `valid_rows` rows starting at element `row0` of each column pointer.
template <int K0, int K1, int K2, bool NEG>
__device__ __forceinline__ uint32_t expr_partial_tile(const ExprTermArgs &a, int64_t tile, int lane, const void *d0, const void *d1, const void *d2, int64_t row0,
                                                      int64_t valid_rows, ColRegs<K0> &c0, ColRegs<K1> &c1, ColRegs<K2> &c2) {
    const int64_t w = tile * kTileWords + lane;
    uint64_t mine = 0ULL;
#pragma unroll 1
    for (int j = 0; j < kTileWords; ++j) {
        const int64_t i = 64 * j + lane;
        const bool valid = i < valid_rows;
        const int64_t r = row0 + (valid ? i : 0);
        bool keep = false;
        for (int t = 0; t < a.n_terms; ++t) {
            const uint32_t u = a.use[t];
            bool k = valid; // (the bounds check FIRST: a negated list keeps "no match", and a row past valid_rows matches nothing)
            if (K0 != TK_NONE && (u & 1u)) k = k && expr_col_row<NEG>(c0, d0, a.cols[t][0], r);
            if (K1 != TK_NONE && (u & 2u)) k = k && expr_col_row<NEG>(c1, d1, a.cols[t][1], r);
            if (K2 != TK_NONE && (u & 4u)) k = k && expr_col_row<NEG>(c2, d2, a.cols[t][2], r);
            keep = keep || k;
        }
        const uint64_t m = ballot64(keep);
        if (lane == j) mine = m;
    }
    mine &= low_mask(valid_rows - 64 * (int64_t)lane); // rows past the end are not rows
    if (lane >= kTileWords) mine = 0;
    if (lane < kTileWords && w < a.n_words && a.bitmap) a.bitmap[w] = mine;
    return (uint32_t)__popcll(mine);
}

// T = tiles per wave iteration (narrow columns take several tiles at once so that every wave keeps >= 4 KiB of loads in flight),
// the same values as k_filter_tile's instances.
// TABLE selects the tile-table walk (table queries) at compile time, as in k_filter_tile: the single-segment kernel carries none of
// it, not even the tile table's words in its argument block (ExprTermArgs, imm3_internal.h).
// NEG: the instance that honours TileCol::negated (only kinds with a 2-byte string column have one)
template <int K0, int K1, int K2, int T, bool TABLE, bool NEG = false>
__global__ __launch_bounds__(kBlockThreads) void k_filter_expr(const std::conditional_t<TABLE, ExprTileArgs, ExprTermArgs> a) {
    constexpr int kLane = expr_lane_tile(K0, K1, K2);
    constexpr bool kXpose = kLane == 0 && (K0 == TK_I8 || K0 == TK_S2 || K1 == TK_I8 || K1 == TK_S2 || K2 == TK_I8 || K2 == TK_S2);
    // narrow-only kinds spend longer on a tile than its loads take to issue: the next group's loads go out BEFORE the current group
    // is evaluated (k_filter_tile: with an int32 column the same pipeline measured slower)
    constexpr bool kPipe = kLane != 0 || (kXpose && K0 != TK_I32 && K1 != TK_I32 && K2 != TK_I32);
    __shared__ __attribute__((aligned(16))) uint8_t s_xpose[kWavesPerBlock][kXpose ? kXposeBytes : 16];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    uint8_t *xp = s_xpose[wave];
    const void *d0 = a.cols[0][0].data, *d1 = a.cols[0][1].data, *d2 = a.cols[0][2].data; // (one segment; a table's come from its tile table)
    uint32_t lane_total = 0;
    const int64_t wave_id = (int64_t)blockIdx.x * kWavesPerBlock + wave;
    const int64_t n_waves = (int64_t)gridDim.x * kWavesPerBlock;

    if constexpr (TABLE) { // table query: tiles come from the tile table (one partial tile per segment), one tile per step
        static_assert(T == 1, "the table walk takes one tile per step");
        for (int64_t tile = wave_id; tile < a.n_tiles; tile += n_waves) {
            const uint32_t rows_here = a.tile_rows[tile];
            const void *t0 = K0 != TK_NONE ? as_global(a.tile_ptrs[0][tile]) : nullptr; // (as_global: no flat loads through a pointer read from memory)
            const void *t1 = K1 != TK_NONE ? as_global(a.tile_ptrs[1][tile]) : nullptr;
            const void *t2 = K2 != TK_NONE ? as_global(a.tile_ptrs[2][tile]) : nullptr;
            ColRegs<K0> c0;
            ColRegs<K1> c1;
            ColRegs<K2> c2;
            if (rows_here == kTileRows) {
                expr_load<kLane>(c0, t0, 0, lane);
                expr_load<kLane>(c1, t1, 0, lane);
                expr_load<kLane>(c2, t2, 0, lane);
                lane_total += expr_full_tile<K0, K1, K2, NEG>(a, tile, lane, c0, c1, c2, xp);
            } else {
                lane_total += expr_partial_tile<K0, K1, K2, NEG>(a, tile, lane, t0, t1, t2, 0, rows_here, c0, c1, c2);
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) lane_total += __shfl_xor(lane_total, d);
        if (a.finish) block_partial_finish(a.finish, lane_total, lane, wave);
        else block_partial_store(a.block_partials, lane_total, lane, wave);
        return;
    } else {
    const int64_t n_full = a.n_rows / kTileRows;
    const int64_t n_groups = n_full / T;

    ColRegs<K0> n0[T]; // kPipe: the group after the current one, already loading
    ColRegs<K1> n1[T];
    ColRegs<K2> n2[T];
    auto load_group = [&](ColRegs<K0> (&r0)[T], ColRegs<K1> (&r1)[T], ColRegs<K2> (&r2)[T], int64_t grp) {
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int64_t row0 = (grp * T + t) * kTileRows;
            expr_load<kLane>(r0[t], d0, row0, lane);
            expr_load<kLane>(r1[t], d1, row0, lane);
            expr_load<kLane>(r2[t], d2, row0, lane);
        }
    };
    if (kPipe && wave_id < n_groups) load_group(n0, n1, n2, wave_id);
    for (int64_t grp = wave_id; grp < n_groups; grp += n_waves) {
        ColRegs<K0> c0[T];
        ColRegs<K1> c1[T];
        ColRegs<K2> c2[T];
        if constexpr (kPipe) {
#pragma unroll
            for (int t = 0; t < T; ++t) { // (touch(): the wait for this group's loads sits here, ahead of the prefetch)
                c0[t] = n0[t];
                c1[t] = n1[t];
                c2[t] = n2[t];
                c0[t].touch();
                c1[t].touch();
                c2[t].touch();
            }
            load_group(n0, n1, n2, grp + n_waves < n_groups ? grp + n_waves : grp); // (unconditional: the last iteration re-reads its own group)
        } else {
            load_group(c0, c1, c2, grp);
        }
#pragma unroll
        for (int t = 0; t < T; ++t) lane_total += expr_full_tile<K0, K1, K2, NEG>(a, grp * T + t, lane, c0[t], c1[t], c2[t], xp);
    }
    // leftovers: fewer than T full tiles, then the one partial tile at the end of the segment
    for (int64_t tile = n_groups * T + wave_id; tile < a.n_tiles; tile += n_waves) {
        const int64_t row0 = tile * kTileRows;
        ColRegs<K0> c0;
        ColRegs<K1> c1;
        ColRegs<K2> c2;
        if (tile < n_full) {
            expr_load<kLane>(c0, d0, row0, lane);
            expr_load<kLane>(c1, d1, row0, lane);
            expr_load<kLane>(c2, d2, row0, lane);
            lane_total += expr_full_tile<K0, K1, K2, NEG>(a, tile, lane, c0, c1, c2, xp);
        } else {
            lane_total += expr_partial_tile<K0, K1, K2, NEG>(a, tile, lane, d0, d1, d2, row0, a.n_rows - row0, c0, c1, c2);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) lane_total += __shfl_xor(lane_total, d);
    if (a.finish) block_partial_finish(a.finish, lane_total, lane, wave);
    else block_partial_store(a.block_partials, lane_total, lane, wave);
    }
}

// ---------------------------------------------------------------------------------------------
// k_filter_expr_generic: k_filter_generic's walk (uniform or ragged layout, one bitmap word per wave and step) over the terms.
// ---------------------------------------------------------------------------------------------
template <bool NEG> // NEG: the instance that honours ColPred::negated (launched for a tree that carries a negated list)
__global__ __launch_bounds__(kBlockThreads) void k_filter_expr_generic(const ExprGenericArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    uint32_t wave_total = 0;
    for (int64_t w = (int64_t)blockIdx.x * kWavesPerBlock + wave; w < a.n_words; w += (int64_t)gridDim.x * kWavesPerBlock) {
        int64_t base;
        int nv;
        if (a.word_row_base) {
            base = a.word_row_base[w];
            nv = a.word_nvalid[w];
        } else {
            base = 64 * w;
            const int64_t rem = a.n_rows - base;
            nv = rem >= 64 ? 64 : (int)rem;
        }
        const bool valid = lane < nv;
        const int64_t row = valid ? base + lane : base;
        uint64_t acc = 0ULL;
        for (int t = 0; t < a.n_terms; ++t) {
            uint64_t ta = ~0ULL;
            // (wave-uniform exit: no row of the word is left in the term.  A NEGATED list -- ColPred::negated, set on string predicates
            // only -- keeps the rows that match none of its values, INSIDE the bounds check: a lane past word_nvalid sets no bit)
            for (int p = a.term_start[t]; p < a.term_start[t + 1] && ta; ++p) {
                if constexpr (NEG) ta &= ballot64(valid && (eval_row(a.preds[p], row) != (a.preds[p].negated != 0)));
                else ta &= ballot64(valid && eval_row(a.preds[p], row));
            }
            acc |= ta;
        }
        acc &= low_mask(nv);
        if (lane == 0) a.bitmap[w] = acc;
        wave_total += (uint32_t)__popcll(acc);
    }
    block_partial_store(a.block_partials, wave_total, lane, wave);
}

#define IMM3_EXPR_CASE(k0, k1, k2, T)                                                                  \
    if (a.kinds[0] == k0 && a.kinds[1] == k1 && a.kinds[2] == k2) {                                    \
        constexpr bool has_s2 = k0 == TK_S2 || k1 == TK_S2 || k2 == TK_S2;                             \
        if (has_s2 && neg) IMM3_LAUNCH((k_filter_expr<k0, k1, k2, T, false, has_s2>), grid, kBlockThreads, s, ev0, ev1, seg); \
        else IMM3_LAUNCH((k_filter_expr<k0, k1, k2, T, false>), grid, kBlockThreads, s, ev0, ev1, seg); \
        return true;                                                                                   \
    }
// the table instances: one tile per step whatever the kinds
#define IMM3_EXPR_TABLE_CASE(k0, k1, k2, T)                                                            \
    if (a.kinds[0] == k0 && a.kinds[1] == k1 && a.kinds[2] == k2) {                                    \
        constexpr bool has_s2 = k0 == TK_S2 || k1 == TK_S2 || k2 == TK_S2;                             \
        if (has_s2 && neg) IMM3_LAUNCH((k_filter_expr<k0, k1, k2, 1, true, has_s2>), grid, kBlockThreads, s, ev0, ev1, a); \
        else IMM3_LAUNCH((k_filter_expr<k0, k1, k2, 1, true>), grid, kBlockThreads, s, ev0, ev1, a);   \
        return true;                                                                                   \
    }
// k_filter_tile's column-kind combinations (and tiles per iteration), except the one without any column: a tree has leaves
#define IMM3_EXPR_KINDS(X)                                                                        \
    X(TK_I32, TK_NONE, TK_NONE, 1) X(TK_I8, TK_NONE, TK_NONE, 2) X(TK_S2, TK_NONE, TK_NONE, 1) \
    X(TK_I32, TK_I32, TK_NONE, 1) X(TK_I32, TK_I8, TK_NONE, 1) X(TK_I8, TK_I8, TK_NONE, 1) \
    X(TK_I32, TK_S2, TK_NONE, 1) X(TK_I8, TK_S2, TK_NONE, 1) \
    X(TK_I32, TK_I32, TK_I32, 1) X(TK_I32, TK_I32, TK_I8, 1) X(TK_I32, TK_I8, TK_I8, 1)              \
    X(TK_I8, TK_I8, TK_I8, 2) X(TK_I32, TK_I32, TK_S2, 1) X(TK_I32, TK_I8, TK_S2, 1) X(TK_I8, TK_I8, TK_S2, 1)

bool launch_filter_expr(const ExprTileArgs &a, int grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    bool neg = false; // a negated list among the terms' predicates: the NEG instance
    for (int t = 0; t < a.n_terms; ++t)
        for (int k = 0; k < kMaxTileCols; ++k) neg = neg || ((a.use[t] >> k & 1u) && a.cols[t][k].negated);
    if (a.tile_rows) { // a table query: the tile table replaces cols[..].data / n_rows
        IMM3_EXPR_KINDS(IMM3_EXPR_TABLE_CASE)
        return false;
    }
    const ExprTermArgs &seg = a; // (one segment: the kernel takes the terms alone)
    IMM3_EXPR_KINDS(IMM3_EXPR_CASE)
    return false;
}

void launch_filter_expr_generic(const ExprGenericArgs &a, bool negated, int grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (negated) IMM3_LAUNCH(k_filter_expr_generic<true>, grid, kBlockThreads, s, ev0, ev1, a);
    else IMM3_LAUNCH(k_filter_expr_generic<false>, grid, kBlockThreads, s, ev0, ev1, a);
}

} // namespace imm3
