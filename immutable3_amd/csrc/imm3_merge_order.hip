// imm3_merge_order.hip -- the device side of imm3_comm_merge_ordered: ordered results of several queries (segments, tables, ranks)
// merged into one ordered list ("Merging ordered results").
//
//   k_merge_order_pack   one lane per ordered row of one query: the record {normalised key (imm3_order_key.h: the order's own rule,
//                        applied to the ORDERED key columns), global segment, row in segment, SELECT-list bytes}.  A table query's
//                        virtual row goes through the table's tile starts (binary search) to (table segment, row) and through the
//                        caller's global indices to the global segment: imm3_query_locate_rows on the device.
//   k_merge_order_split  a table query whose global indices are not ascending is in (key, TABLE segment, row) order, which is not
//                        the six-word order: its records are cut into one list per table segment (each a subsequence, hence
//                        sorted) -- one wave per table segment walks the query's records in order, count launch, then move launch.
//   k_merge_order_rank   the merge: a rank-by-search over sorted lists.  One lane per record, 64 consecutive records of one list per
//                        wave; a record's place is its index in its own list plus, per other list, the records there that come
//                        before it -- `<=` in the lists before its own, `<` in those behind: a permutation even when two lists
//                        hold equal keys -- by binary search on the six-word key.  Records whose place is below the cut are stored
//                        whole, the others dropped.  No atomic, no sort; the same kernel merges a rank's queries and, behind the
//                        all-gather, the ranks' slots.
//
// The searches of a wave's 64 consecutive records walk monotone paths through each other list and share its cache lines; a lane
// runs kRankAhead of them at a time (their loads are independent), which is what hides the latency when the merge is small -- a
// top-k of a few thousand records is a few hundred waves.
#include "imm3_internal.h"
#include "imm3_merge_order.h"
#include "imm3_order_key.h"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace imm3 {
namespace {

constexpr int kRankAhead = 4;
constexpr int kKeyPairs = kMergeOrderKeyWords / 2;

__device__ inline uint32_t lanes_below(uint64_t m) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); }

// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_merge_order_pack(const MergeOrderPackArgs a) {
    const uint32_t i = (uint32_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n_rows) return;
    uint32_t *rec = a.recs + (uint64_t)i * (uint64_t)a.rec_words;
    if (a.with_key) {
        uint32_t k[kOrderKeyWords];
        order_build_key(a.keys, a.n_keys, a.key_bytes, (int64_t)i, k);
        const uint32_t ri = a.row_index[i];
        uint32_t seg = a.segment, row = ri;
        if (a.n_tsegs > 0) { // the last table segment whose first tile is <= the row's tile (an empty segment shares its successor's first tile)
            const uint32_t tile = ri >> 10;
            int lo = 0, hi = a.n_tsegs; // tile_start[lo] <= tile < tile_start[hi] (tile_start[0] == 0, tile_start[n_tsegs] == the table's tiles)
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (a.tile_start[mid] <= tile) lo = mid;
                else hi = mid;
            }
            seg = a.global_index[lo];
            row = (tile - a.tile_start[lo]) * (uint32_t)kTileRows + (ri & (uint32_t)(kTileRows - 1));
        }
        uint2 *r2 = (uint2 *)rec; // (records are 8-byte aligned: rec_words is even)
        r2[0] = make_uint2(k[0], k[1]);
        r2[1] = make_uint2(k[2], k[3]);
        r2[2] = make_uint2(seg, row);
    }
#pragma unroll
    for (int c = 0; c < kMaxProj; ++c) {
        if (c >= a.n_cols) break;
        const int w = a.cols[c].width;
        uint32_t *d = rec + a.cols[c].rec_off;
        const uint8_t *s = a.cols[c].src + (uint64_t)i * (uint64_t)w;
        if (w == 4) d[0] = *(const uint32_t *)s;
        else if (w == 1) d[0] = s[0];
        else if ((w & 3) == 0) { // (rows of such a column are dword aligned)
            for (int b = 0; b < w; b += 4) d[b >> 2] = *(const uint32_t *)(s + b);
        } else {
            for (int b = 0; b < w; b += 4) { // bytes in memory order, the last word zero-padded
                uint32_t v = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (b + k < w) v |= (uint32_t)s[b + k] << (8 * k);
                d[b >> 2] = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// wave t = table segment t.  MOVE == false: counts[t] = the query's records of that segment.  MOVE == true: those records, in
// order, to the list that starts behind the lists of the segments before it; the list table's entry.
template <bool MOVE> __global__ __launch_bounds__(256) void k_merge_order_split(const MergeOrderSplitArgs a) {
    const int lane = (int)threadIdx.x & 63, t = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (t >= a.n_tsegs) return;
    const uint32_t want = a.global_index[t];
    uint32_t before = 0;
    if (MOVE) {
        for (int u = lane; u < t; u += 64) before += a.counts[u];
        for (int off = 32; off > 0; off >>= 1) before += (uint32_t)__shfl_xor((int)before, off, 64);
    }
    const unsigned long long first_word = a.dst_word + (unsigned long long)before * (unsigned long long)a.rec_words;
    uint32_t seen = 0;
    for (uint32_t base = 0; base < a.n_rows; base += 64) {
        const uint32_t i = base + (uint32_t)lane;
        const uint32_t *r = a.src + (uint64_t)i * (uint64_t)a.rec_words;
        const bool mine = i < a.n_rows && r[4] == want;
        const uint64_t m = __ballot(mine);
        if (MOVE && mine) {
            const uint32_t pos = seen + lanes_below(m);
            if (before + pos < a.n_rows) { // (always: the counts of all segments sum to n_rows)
                uint2 *d = (uint2 *)(a.dst + first_word + (unsigned long long)pos * (unsigned long long)a.rec_words);
                const uint2 *s2 = (const uint2 *)r;
                for (int w = 0; w < a.rec_words / 2; ++w) d[w] = s2[w];
            }
        }
        seen += (uint32_t)__popcll(m);
    }
    if (lane != 0) return;
    if (MOVE) {
        a.lists[2 * t] = first_word;
        a.lists[2 * t + 1] = seen;
    } else a.counts[t] = seen;
}

// ---------------------------------------------------------------------------------------------
struct ListRef {
    const uint32_t *recs; // null: empty
    uint32_t len;
};
// list l of the merge; a list that would reach past the buffer, or past list_cap, counts as empty / is clamped
__device__ inline ListRef list_of(const MergeOrderArgs &a, int l) {
    unsigned long long off, len;
    if (a.slot_words) {
        off = (unsigned long long)l * a.slot_words + 2ULL;
        len = *(const unsigned long long *)(a.recs + (unsigned long long)l * a.slot_words);
    } else {
        off = a.lists[2 * l];
        len = a.lists[2 * l + 1];
    }
    ListRef r;
    r.recs = nullptr;
    r.len = 0;
    if (len > a.list_cap) len = a.list_cap;
    if (len == 0 || off > a.buf_words || len * (unsigned long long)a.rec_words > a.buf_words - off) return r;
    r.recs = a.recs + off;
    r.len = (uint32_t)len;
    return r;
}

// the record at `r` against the key `k`: true when it comes before k (or_equal: before or equal)
__device__ inline bool key_before(const uint2 v[kKeyPairs], const uint32_t k[kMergeOrderKeyWords], bool or_equal) {
    const uint32_t w[kMergeOrderKeyWords] = {v[0].x, v[0].y, v[1].x, v[1].y, v[2].x, v[2].y};
    int c = 0;
#pragma unroll
    for (int j = 0; j < kMergeOrderKeyWords; ++j)
        if (c == 0 && w[j] != k[j]) c = w[j] < k[j] ? -1 : 1;
    return c < 0 || (or_equal && c == 0);
}

__global__ __launch_bounds__(256) void k_merge_order_rank(const MergeOrderArgs a) {
    const int lane = (int)threadIdx.x & 63;
    const unsigned long long gw = (unsigned long long)blockIdx.x * 4ULL + (threadIdx.x >> 6);
    if (gw == 0) { // the lists' lengths summed: what the host reports as the total
        unsigned long long sum = 0;
        for (int l = lane; l < a.n_lists; l += 64) sum += list_of(a, l).len;
        for (int off = 32; off > 0; off >>= 1) sum += (unsigned long long)__shfl_xor((long long)sum, off, 64);
        if (lane == 0) *a.out_total = sum;
    }
    const uint32_t waves_per_list = (a.list_cap + 63u) / 64u;
    if (waves_per_list == 0) return;
    const unsigned long long lw = gw / waves_per_list;
    if (lw >= (unsigned long long)a.n_lists) return;
    const int l = (int)lw;
    const uint32_t i = (uint32_t)(gw % waves_per_list) * 64u + (uint32_t)lane;
    const ListRef own = list_of(a, l);
    if (i >= own.len) return;
    const int R = a.rec_words;
    const uint2 *rec = (const uint2 *)(own.recs + (uint64_t)i * (uint64_t)R);
    uint32_t k[kMergeOrderKeyWords];
    {
        const uint2 k0 = rec[0], k1 = rec[1], k2 = rec[2];
        k[0] = k0.x; k[1] = k0.y; k[2] = k1.x; k[3] = k1.y; k[4] = k2.x; k[5] = k2.y;
    }
    unsigned long long place = i;
    // the other lists, kRankAhead at a time: one step of each search per round, the rounds' loads issued together
    for (int m0 = 0; m0 < a.n_lists; m0 += kRankAhead) {
        const uint32_t *base[kRankAhead];
        uint32_t lo[kRankAhead], hi[kRankAhead];
        bool or_equal[kRankAhead];
#pragma unroll
        for (int u = 0; u < kRankAhead; ++u) {
            const int m = m0 + u;
            base[u] = nullptr;
            lo[u] = hi[u] = 0;
            or_equal[u] = m < l;
            if (m < a.n_lists && m != l) {
                const ListRef o = list_of(a, m);
                base[u] = o.recs;
                hi[u] = o.len;
            }
        }
        bool any = true;
        while (any) {
            uint2 v[kRankAhead][kKeyPairs];
            uint32_t mid[kRankAhead];
#pragma unroll
            for (int u = 0; u < kRankAhead; ++u) {
                mid[u] = lo[u] + ((hi[u] - lo[u]) >> 1);
                if (lo[u] < hi[u]) {
                    const uint2 *p = (const uint2 *)(base[u] + (uint64_t)mid[u] * (uint64_t)R);
#pragma unroll
                    for (int j = 0; j < kKeyPairs; ++j) v[u][j] = p[j];
                } else {
#pragma unroll
                    for (int j = 0; j < kKeyPairs; ++j) v[u][j] = make_uint2(0u, 0u);
                }
            }
            any = false;
#pragma unroll
            for (int u = 0; u < kRankAhead; ++u) {
                if (lo[u] < hi[u]) {
                    if (key_before(v[u], k, or_equal[u])) lo[u] = mid[u] + 1u;
                    else hi[u] = mid[u];
                }
                any = any || lo[u] < hi[u];
            }
        }
#pragma unroll
        for (int u = 0; u < kRankAhead; ++u) place += lo[u];
    }
    if (place >= (unsigned long long)a.cut) return;
    uint2 *dst = (uint2 *)(a.out + place * (unsigned long long)R);
    for (int w = 0; w < R / 2; w += 4) { // a chunk's loads before its stores
        uint2 x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = w + j < R / 2 ? rec[w + j] : make_uint2(0u, 0u);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (w + j < R / 2) dst[w + j] = x[j];
    }
}

} // namespace

void launch_merge_order_pack(const MergeOrderPackArgs &a, hipStream_t s) {
    if (!a.n_rows) return;
    hipLaunchKernelGGL(k_merge_order_pack, dim3((a.n_rows + 255u) / 256u), dim3(256), 0, s, a);
}

void launch_merge_order_split(const MergeOrderSplitArgs &a, hipStream_t s) {
    if (a.n_tsegs <= 0) return;
    const unsigned grid = ((unsigned)a.n_tsegs + 3u) / 4u;
    hipLaunchKernelGGL(k_merge_order_split<false>, dim3(grid), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_merge_order_split<true>, dim3(grid), dim3(256), 0, s, a);
}

void launch_merge_order_rank(const MergeOrderArgs &a, hipStream_t s) {
    const unsigned long long waves = (unsigned long long)std::max(a.n_lists, 1) * std::max<unsigned long long>((a.list_cap + 63u) / 64u, 1ULL);
    hipLaunchKernelGGL(k_merge_order_rank, dim3((unsigned)((waves + 3ULL) / 4ULL)), dim3(256), 0, s, a);
}

} // namespace imm3
