// imm3_order.hip -- ORDER BY behind the projection (imm3_query_set_order): the projected rows ordered by up to four SELECT-list columns,
// all of them or the first `limit`.
//
//   k_order_keys     one pass over the projected key columns: a normalised big-endian key of 1 .. 16 bytes per row (int32 ^ 0x80000000,
//                    int8 ^ 0x80, strings as they are, a descending key complemented: unsigned byte order of the key == the order asked
//                    for), the identity permutation, and per wave the OR of key ^ first key
//   k_order_plan     from that OR: the key bytes in which the rows differ at all (a byte position that one value fills is skipped by
//                    every later launch: its pass would move nothing); full sort or select; the row counts
//   select (top-k)   from the most significant byte down: k_order_count<true> (digit counts among the rows that match the threshold
//                    found so far) + k_order_find (the bucket that holds the limit-th row; the per-wave below / equal tally); then
//                    k_order_offsets / k_order_compact: the rows below the threshold and the first rows equal to it, in row order, to the other buffer
//   sort             a stable LSD radix sort, 8 bits a pass, least significant byte first: k_order_count<false>, k_order_scan,
//                    k_order_scatter over (key, permutation), ping-pong between two buffers
//   k_order_apply    row index and SELECT-list columns gathered through the final permutation
//
// Determinism: no atomic anywhere.  Every launch cuts the rows into kOrderWaves contiguous pieces, one per wave; a wave walks its piece
// in ascending order 64 rows a step; a row's place among the rows of its step with the same digit is v_mbcnt over the digit's peer
// mask (eight ballots), the running per-digit place lives in wave-private LDS, updated by the last peer alone.  The scatter therefore
// keeps row order within a digit (stable), and since the input is in ascending row order, rows with equal keys stay in it.
// The grid never depends on the row count (a device word): nothing here makes the host wait.
#include "imm3_internal.h"
#include "imm3_order_key.h"

#include <hip/hip_runtime.h>

namespace imm3 {
namespace {

constexpr int kWavesPerOrderBlock = kOrderBlockThreads / 64;
// A wave walks its piece kOrderAhead steps at a time: the loads of all of them are issued before the first is ranked, so that a wave
// (one per SIMD at this grid) has several loads in flight instead of one; the steps are still ranked in ascending order.
constexpr int kOrderAhead = 4;

struct Piece {
    int64_t begin, end;
};
// the contiguous piece of [0, n) this wave owns: whole steps of 64 rows, the same cut in every launch
__device__ inline Piece wave_piece(int64_t n, int gw) {
    const int64_t steps = (n + 63) / 64;
    const int64_t per = (steps + kOrderWaves - 1) / kOrderWaves;
    Piece p;
    p.begin = (int64_t)gw * per * 64;
    if (p.begin > n) p.begin = n;
    p.end = p.begin + per * 64;
    if (p.end > n) p.end = n;
    return p;
}
__device__ inline int global_wave() { return (int)blockIdx.x * kWavesPerOrderBlock + ((int)threadIdx.x >> 6); }
__device__ inline uint32_t lanes_below(uint64_t m) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); }
// the lanes of this step that hold the same digit as this lane (among the valid ones): eight ballots
__device__ inline uint64_t digit_peers(uint32_t digit, bool valid) {
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (digit >> b) & 1u;
        const uint64_t bal = __ballot(valid && bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}
// LDS traffic of ONE wave is issued in program order; this keeps the compiler from moving it across a step
__device__ inline void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
__device__ inline uint32_t rows_emitted(const OrderArgs &a) {
    const unsigned long long e = *a.n_emit;
    return (uint32_t)(e < a.cap_rows ? e : a.cap_rows);
}

// the normalised key of projected row i (the rule itself: imm3_order_key.h)
__device__ inline void build_key(const OrderArgs &a, int64_t i, uint32_t k[kOrderKeyWords]) { order_build_key(a.cols, a.n_cols, a.key_bytes, i, k); }

__device__ inline uint32_t key_digit(const uint32_t k[kOrderKeyWords], int p) {
    const int w = p >> 2;
    const uint32_t word = w == 0 ? k[0] : (w == 1 ? k[1] : (w == 2 ? k[2] : k[3]));
    return (word >> ((3 - (p & 3)) * 8)) & 0xFFu;
}
__device__ inline void load_key(const uint32_t *keys, uint64_t cap, int key_words, int64_t i, uint32_t k[kOrderKeyWords]) {
#pragma unroll
    for (int w = 0; w < kOrderKeyWords; ++w) k[w] = w < key_words ? keys[(uint64_t)w * cap + (uint64_t)i] : 0u;
}
__device__ inline void store_key(uint32_t *keys, uint64_t cap, int key_words, int64_t i, const uint32_t k[kOrderKeyWords]) {
#pragma unroll
    for (int w = 0; w < kOrderKeyWords; ++w)
        if (w < key_words) keys[(uint64_t)w * cap + (uint64_t)i] = k[w];
}
// the buffer the pass on key byte p reads: the select's compaction and every active pass behind p (bytes p + 1 ..) flipped it
__device__ inline int pass_source(const uint32_t *st, int p) { return (int)((st[OW_SELECT] + (uint32_t)__popc(st[OW_ACTIVE] >> (p + 1))) & 1u); }

// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kOrderBlockThreads) void k_order_keys(const OrderArgs a) {
    const int lane = (int)threadIdx.x & 63, gw = global_wave();
    const uint32_t n = rows_emitted(a);
    const Piece pc = wave_piece(n, gw);
    uint32_t k0[kOrderKeyWords] = {0u, 0u, 0u, 0u}, d[kOrderKeyWords] = {0u, 0u, 0u, 0u};
    if (pc.begin < pc.end) build_key(a, 0, k0);
    for (int64_t base = pc.begin; base < pc.end; base += 64) {
        const int64_t i = base + lane;
        if (i < pc.end) {
            uint32_t k[kOrderKeyWords];
            build_key(a, i, k);
            store_key(a.keys[0], a.cap_rows, a.key_words, i, k);
            a.perm[0][i] = (uint32_t)i;
#pragma unroll
            for (int w = 0; w < kOrderKeyWords; ++w) d[w] |= k[w] ^ k0[w];
        }
    }
#pragma unroll
    for (int w = 0; w < kOrderKeyWords; ++w) {
        uint32_t v = d[w];
        for (int off = 32; off > 0; off >>= 1) v |= (uint32_t)__shfl_xor((int)v, off, 64);
        if (lane == 0) a.diff[gw * kOrderKeyWords + w] = v;
    }
}

__global__ __launch_bounds__(256) void k_order_plan(const OrderArgs a) {
    __shared__ uint32_t s_or[256][kOrderKeyWords];
    const int t = (int)threadIdx.x;
    uint32_t d[kOrderKeyWords] = {0u, 0u, 0u, 0u};
    for (int w = t; w < kOrderWaves; w += 256)
#pragma unroll
        for (int j = 0; j < kOrderKeyWords; ++j) d[j] |= a.diff[w * kOrderKeyWords + j];
#pragma unroll
    for (int j = 0; j < kOrderKeyWords; ++j) s_or[t][j] = d[j];
    // the select's per-wave tally starts as "no row below the threshold, every row of the piece equal to it" (no byte found yet);
    // k_order_find narrows it byte by byte
    for (int w = t; w < kOrderWaves; w += 256) {
        const Piece pc = wave_piece(rows_emitted(a), w);
        a.tally[w * 2] = 0u;
        a.tally[w * 2 + 1] = (uint32_t)(pc.end - pc.begin);
    }
    __syncthreads();
    if (t != 0) return;
    for (int r = 1; r < 256; ++r)
#pragma unroll
        for (int j = 0; j < kOrderKeyWords; ++j) d[j] |= s_or[r][j];
    uint32_t active = 0;
    for (int p = 0; p < a.key_bytes; ++p)
        if (key_digit(d, p)) active |= 1u << p;
    const uint32_t n = rows_emitted(a);
    const bool limited = a.limit > 0 && (unsigned long long)a.limit < (unsigned long long)n;
    const uint32_t n_out = limited ? (uint32_t)a.limit : n;
    const bool select = limited && a.force_full != 1 && (a.force_full == 2 || (unsigned long long)n >= (unsigned long long)kOrderSelectFactor * (unsigned long long)a.limit);
    uint32_t k0[kOrderKeyWords] = {0u, 0u, 0u, 0u};
    if (n > 0) build_key(a, 0, k0);
    uint32_t *st = a.state;
    st[OW_N] = n;
    st[OW_N_SORT] = select ? n_out : n;
    st[OW_N_OUT] = n_out;
    st[OW_N_OUT + 1] = 0u;
    st[OW_ACTIVE] = active;
    st[OW_SELECT] = select ? 1u : 0u;
    st[OW_NEED] = n_out;
#pragma unroll
    for (int j = 0; j < kOrderKeyWords; ++j) {
        st[OW_THR + j] = 0u;
        st[OW_KEY0 + j] = k0[j];
    }
}

// Digit counts of key byte a.byte_pos per wave: counts[digit * kOrderWaves + wave].  SELECT: among the rows of the key buffer 0 whose
// bytes before byte_pos equal the threshold's; else: among the rows the sort moves, from the pass's source buffer.
template <bool SELECT> __global__ __launch_bounds__(kOrderBlockThreads) void k_order_count(const OrderArgs a) {
    __shared__ uint32_t s_cnt[kWavesPerOrderBlock][256];
    const uint32_t *st = a.state;
    const int p = a.byte_pos;
    if (!((st[OW_ACTIVE] >> p) & 1u)) return;
    if (SELECT && !st[OW_SELECT]) return;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, gw = global_wave();
    const uint32_t n = SELECT ? st[OW_N] : st[OW_N_SORT];
    const uint32_t *keys = a.keys[SELECT ? 0 : pass_source(st, p)];
    const Piece pc = wave_piece(n, gw);
    uint32_t thr[kOrderKeyWords];
#pragma unroll
    for (int w = 0; w < kOrderKeyWords; ++w) thr[w] = st[OW_THR + w];
    const int pw = p >> 2;
    const uint32_t part_mask = (p & 3) ? (0xFFFFFFFFu << (32 - 8 * (p & 3))) : 0u;
    for (int d = lane; d < 256; d += 64) s_cnt[wave][d] = 0u;
    wave_lds_fence();
    for (int64_t base = pc.begin; base < pc.end; base += 64 * kOrderAhead) {
        bool valid[kOrderAhead];
        uint32_t digit[kOrderAhead];
#pragma unroll
        for (int u = 0; u < kOrderAhead; ++u) {
            const int64_t i = base + 64 * u + lane;
            valid[u] = i < pc.end;
            digit[u] = 0;
            if (valid[u]) {
                if (SELECT) {
                    uint32_t k[kOrderKeyWords];
                    load_key(keys, a.cap_rows, pw + 1 < a.key_words ? pw + 1 : a.key_words, i, k);
#pragma unroll
                    for (int w = 0; w < kOrderKeyWords; ++w) {
                        if (w < pw) valid[u] = valid[u] && k[w] == thr[w];
                        else if (w == pw) valid[u] = valid[u] && ((k[w] ^ thr[w]) & part_mask) == 0u;
                    }
                    digit[u] = key_digit(k, p);
                } else {
                    digit[u] = (keys[(uint64_t)pw * a.cap_rows + (uint64_t)i] >> ((3 - (p & 3)) * 8)) & 0xFFu;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kOrderAhead; ++u) {
            const uint64_t peers = digit_peers(digit[u], valid[u]);
            if (valid[u] && (peers >> lane) == 1ULL) s_cnt[wave][digit[u]] += (uint32_t)__popcll(peers); // (the last peer alone)
            wave_lds_fence();
        }
    }
    for (int d = lane; d < 256; d += 64) a.counts[d * kOrderWaves + gw] = s_cnt[wave][d];
}

// select: the bucket of key byte a.byte_pos that holds the OW_NEED-th matching row -> the threshold's next byte, and the per-wave
// tally {rows below the threshold, rows equal to it so far} that the compaction's offsets are made of (no extra walk over the rows)
__global__ __launch_bounds__(256) void k_order_find(const OrderArgs a) {
    __shared__ uint32_t s_tot[256];
    __shared__ int s_pick;
    uint32_t *st = a.state;
    if (!st[OW_SELECT]) return;
    const int p = a.byte_pos, t = (int)threadIdx.x, shift = (3 - (p & 3)) * 8;
    if (!((st[OW_ACTIVE] >> p) & 1u)) { // every row holds the first row's byte here
        if (t == 0) st[OW_THR + (p >> 2)] |= st[OW_KEY0 + (p >> 2)] & (0xFFu << shift);
        return;
    }
    uint32_t sum = 0;
    const uint4 *c = (const uint4 *)(a.counts + t * kOrderWaves);
#pragma unroll 8
    for (int w = 0; w < kOrderWaves / 4; ++w) {
        const uint4 v = c[w];
        sum += v.x + v.y + v.z + v.w;
    }
    s_tot[t] = sum;
    __syncthreads();
    if (t == 0) {
        const uint32_t need = st[OW_NEED];
        uint32_t cum = 0;
        int d = 0;
        for (; d < 255; ++d) {
            if (cum + s_tot[d] >= need) break;
            cum += s_tot[d];
        }
        st[OW_NEED] = need - cum;
        st[OW_THR + (p >> 2)] |= (uint32_t)d << shift;
        s_pick = d;
    }
    __syncthreads();
    // per wave: the matching rows with a smaller digit are below the threshold for good, those with the picked digit still equal it
    const int pick = s_pick;
    for (int w = t; w < kOrderWaves; w += 256) {
        uint32_t below = 0;
#pragma unroll 8
        for (int d = 0; d < pick; ++d) below += a.counts[d * kOrderWaves + w];
        a.tally[w * 2] += below;
        a.tally[w * 2 + 1] = a.counts[pick * kOrderWaves + w];
    }
}

// key of row i against the threshold: -1 below, 0 equal, 1 above
__device__ inline int key_cmp(const uint32_t k[kOrderKeyWords], const uint32_t thr[kOrderKeyWords]) {
    int r = 0;
#pragma unroll
    for (int w = 0; w < kOrderKeyWords; ++w)
        if (r == 0 && k[w] != thr[w]) r = k[w] < thr[w] ? -1 : 1;
    return r;
}

// exclusive scan of one value per thread over a work-group of kOrderWaves threads
__device__ inline uint32_t block_scan_exclusive(uint32_t v, uint32_t *s) {
    const int t = (int)threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int off = 1; off < kOrderWaves; off <<= 1) {
        const uint32_t x = t >= off ? s[t - off] : 0u;
        __syncthreads();
        s[t] += x;
        __syncthreads();
    }
    const uint32_t incl = s[t];
    __syncthreads();
    return incl - v;
}

// select: per wave, the first output row and the equal rows before it -- thread w is wave w
__global__ __launch_bounds__(kOrderWaves) void k_order_offsets(const OrderArgs a) {
    __shared__ uint32_t s[kOrderWaves];
    const uint32_t *st = a.state;
    if (!st[OW_SELECT]) return;
    const int t = (int)threadIdx.x;
    const uint32_t need = st[OW_NEED];
    const uint32_t lt = a.tally[t * 2], eq = a.tally[t * 2 + 1];
    const uint32_t eq_before = block_scan_exclusive(eq, s);
    const uint32_t left = need > eq_before ? need - eq_before : 0u;
    const uint32_t take = lt + (eq < left ? eq : left);
    const uint32_t first = block_scan_exclusive(take, s);
    a.tally[t * 2] = first;
    a.tally[t * 2 + 1] = eq_before;
}

// select: the rows below the threshold and the first OW_NEED rows equal to it, in row order, into buffer 1
__global__ __launch_bounds__(kOrderBlockThreads) void k_order_compact(const OrderArgs a) {
    const uint32_t *st = a.state;
    if (!st[OW_SELECT]) return;
    const int lane = (int)threadIdx.x & 63, gw = global_wave();
    const Piece pc = wave_piece(st[OW_N], gw);
    const uint32_t need = st[OW_NEED], n_sort = st[OW_N_SORT];
    uint32_t thr[kOrderKeyWords];
#pragma unroll
    for (int w = 0; w < kOrderKeyWords; ++w) thr[w] = st[OW_THR + w];
    uint32_t out = a.tally[gw * 2], eq_seen = a.tally[gw * 2 + 1];
    for (int64_t base = pc.begin; base < pc.end; base += 64 * kOrderAhead) {
        uint32_t k[kOrderAhead][kOrderKeyWords];
        int c[kOrderAhead];
#pragma unroll
        for (int u = 0; u < kOrderAhead; ++u) {
            const int64_t i = base + 64 * u + lane;
            c[u] = 1;
#pragma unroll
            for (int w = 0; w < kOrderKeyWords; ++w) k[u][w] = 0u;
            if (i < pc.end) {
                load_key(a.keys[0], a.cap_rows, a.key_words, i, k[u]);
                c[u] = key_cmp(k[u], thr);
            }
        }
#pragma unroll
        for (int u = 0; u < kOrderAhead; ++u) {
            const int64_t i = base + 64 * u + lane;
            const uint64_t eqm = __ballot(c[u] == 0);
            const bool take = c[u] < 0 || (c[u] == 0 && eq_seen + lanes_below(eqm) < need);
            const uint64_t tm = __ballot(take);
            if (take) {
                const uint32_t pos = out + lanes_below(tm);
                if (pos < n_sort) { // (always: below + need == limit; the bound keeps a wrong count from writing past the candidates)
                    store_key(a.keys[1], a.cap_rows, a.key_words, pos, k[u]);
                    a.perm[1][pos] = a.perm[0][i];
                }
            }
            out += (uint32_t)__popcll(tm);
            eq_seen += (uint32_t)__popcll(eqm);
        }
    }
}

// counts[digit][wave] -> first position of that wave's rows with that digit: an exclusive scan in (digit, wave) order, in place
__global__ __launch_bounds__(kOrderWaves) void k_order_scan(const OrderArgs a) {
    __shared__ uint32_t s[kOrderWaves];
    const uint32_t *st = a.state;
    if (!((st[OW_ACTIVE] >> a.byte_pos) & 1u)) return;
    constexpr int kPer = 256 * kOrderWaves / kOrderWaves; // entries per thread: consecutive
    uint4 *c = (uint4 *)(a.counts + (size_t)threadIdx.x * kPer);
    uint32_t sum = 0;
#pragma unroll 8
    for (int j = 0; j < kPer / 4; ++j) {
        const uint4 v = c[j];
        sum += v.x + v.y + v.z + v.w;
    }
    uint32_t run = block_scan_exclusive(sum, s);
    for (int j = 0; j < kPer / 4; ++j) {
        const uint4 v = c[j];
        uint4 o;
        o.x = run;
        o.y = o.x + v.x;
        o.z = o.y + v.y;
        o.w = o.z + v.z;
        run = o.w + v.w;
        c[j] = o;
    }
}

// the stable scatter of the pass on key byte a.byte_pos: (key, permutation) from the pass's source buffer to the other one
__global__ __launch_bounds__(kOrderBlockThreads) void k_order_scatter(const OrderArgs a) {
    __shared__ uint32_t s_off[kWavesPerOrderBlock][256];
    const uint32_t *st = a.state;
    const int p = a.byte_pos;
    if (!((st[OW_ACTIVE] >> p) & 1u)) return;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, gw = global_wave();
    const uint32_t n = st[OW_N_SORT];
    const int src = pass_source(st, p);
    const uint32_t *keys = a.keys[src], *perm = a.perm[src];
    uint32_t *keys_out = a.keys[src ^ 1], *perm_out = a.perm[src ^ 1];
    const Piece pc = wave_piece(n, gw);
    for (int d = lane; d < 256; d += 64) s_off[wave][d] = a.counts[d * kOrderWaves + gw];
    wave_lds_fence();
    for (int64_t base = pc.begin; base < pc.end; base += 64 * kOrderAhead) {
        uint32_t k[kOrderAhead][kOrderKeyWords], pv[kOrderAhead];
        bool valid[kOrderAhead];
#pragma unroll
        for (int u = 0; u < kOrderAhead; ++u) {
            const int64_t i = base + 64 * u + lane;
            valid[u] = i < pc.end;
            pv[u] = 0u;
#pragma unroll
            for (int w = 0; w < kOrderKeyWords; ++w) k[u][w] = 0u;
            if (valid[u]) {
                load_key(keys, a.cap_rows, a.key_words, i, k[u]);
                pv[u] = perm[i];
            }
        }
#pragma unroll
        for (int u = 0; u < kOrderAhead; ++u) {
            const uint32_t digit = key_digit(k[u], p);
            const uint64_t peers = digit_peers(digit, valid[u]);
            uint32_t pos = 0;
            if (valid[u]) pos = s_off[wave][digit] + lanes_below(peers);
            wave_lds_fence();
            if (valid[u] && (peers >> lane) == 1ULL) s_off[wave][digit] = pos + 1u; // (the last peer: the digit's next free place)
            wave_lds_fence();
            if (valid[u] && pos < n) {
                store_key(keys_out, a.cap_rows, a.key_words, pos, k[u]);
                perm_out[pos] = pv[u];
            }
        }
    }
}

// the ordered rows: row index and SELECT-list columns through the final permutation (all loads of a row before its first store)
__global__ __launch_bounds__(256) void k_order_apply(const OrderApplyArgs a) {
    const uint32_t *st = a.state;
    const uint32_t n_out = st[OW_N_OUT], n = st[OW_N];
    const uint32_t *perm = a.perm[(st[OW_SELECT] + (uint32_t)__popc(st[OW_ACTIVE])) & 1u];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (int64_t)n_out; i += (int64_t)gridDim.x * 256) {
        const uint32_t p = perm[i];
        if (p >= n) continue; // (never: the permutation holds positions of emitted rows)
        uint32_t ri = 0, v[kMaxProj];
        if (a.row_index) ri = a.row_index[p];
#pragma unroll
        for (int c = 0; c < kMaxProj; ++c) {
            v[c] = 0u;
            if (c < a.n_cols) {
                const int w = a.cols[c].width;
                if (w == 4) v[c] = ((const uint32_t *)a.cols[c].src)[p];
                else if (w == 2) v[c] = ((const uint16_t *)a.cols[c].src)[p];
                else if (w == 1) v[c] = a.cols[c].src[p];
            }
        }
        if (a.row_index) a.row_index_out[i] = ri;
#pragma unroll
        for (int c = 0; c < kMaxProj; ++c) {
            if (c < a.n_cols) {
                const int w = a.cols[c].width;
                if (w == 4) ((uint32_t *)a.cols[c].dst)[i] = v[c];
                else if (w == 2) ((uint16_t *)a.cols[c].dst)[i] = (uint16_t)v[c];
                else if (w == 1) a.cols[c].dst[i] = (uint8_t)v[c];
                else { // a string column: 16 bytes at a time, a chunk's loads before its stores (dwords when the width allows: rows are then dword aligned)
                    const uint8_t *s = a.cols[c].src + (uint64_t)p * (uint64_t)w;
                    uint8_t *d = a.cols[c].dst + (uint64_t)i * (uint64_t)w;
                    if ((w & 3) == 0) {
                        for (int b = 0; b < w; b += 16) {
                            uint32_t x[4];
#pragma unroll
                            for (int k = 0; k < 4; ++k) x[k] = b + 4 * k < w ? ((const uint32_t *)(s + b))[k] : 0u;
#pragma unroll
                            for (int k = 0; k < 4; ++k)
                                if (b + 4 * k < w) ((uint32_t *)(d + b))[k] = x[k];
                        }
                    } else {
                        for (int b = 0; b < w; b += 16) {
                            uint8_t x[16];
#pragma unroll
                            for (int k = 0; k < 16; ++k) x[k] = b + k < w ? s[b + k] : (uint8_t)0;
#pragma unroll
                            for (int k = 0; k < 16; ++k)
                                if (b + k < w) d[b + k] = x[k];
                        }
                    }
                }
            }
        }
    }
}

} // namespace

static const hipEvent_t none = nullptr;

void launch_order_keys(const OrderArgs &a, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    IMM3_LAUNCH(k_order_keys, kOrderGrid, kOrderBlockThreads, s, ev0, none, a);
    IMM3_LAUNCH(k_order_plan, 1, 256, s, none, ev1, a);
}

void launch_order_select(const OrderArgs &a0, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    OrderArgs a = a0;
    for (int p = 0; p < a.key_bytes; ++p) {
        a.byte_pos = p;
        const hipEvent_t first = p == 0 ? ev0 : none;
        IMM3_LAUNCH(k_order_count<true>, kOrderGrid, kOrderBlockThreads, s, first, none, a);
        IMM3_LAUNCH(k_order_find, 1, 256, s, none, none, a);
    }
    IMM3_LAUNCH(k_order_offsets, 1, kOrderWaves, s, none, none, a);
    IMM3_LAUNCH(k_order_compact, kOrderGrid, kOrderBlockThreads, s, none, ev1, a);
}

void launch_order_pass(const OrderArgs &a, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    IMM3_LAUNCH(k_order_count<false>, kOrderGrid, kOrderBlockThreads, s, ev0, none, a);
    IMM3_LAUNCH(k_order_scan, 1, kOrderWaves, s, none, none, a);
    IMM3_LAUNCH(k_order_scatter, kOrderGrid, kOrderBlockThreads, s, none, ev1, a);
}

void launch_order_apply(const OrderApplyArgs &a, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    IMM3_LAUNCH(k_order_apply, 1024, 256, s, ev0, ev1, a);
}

} // namespace imm3
