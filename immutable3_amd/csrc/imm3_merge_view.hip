// imm3_merge_view.hip -- a view of MERGED groups (imm3_comm_merge_groups_view; DESIGN.md section 21, "Views of merged groups"): filter,
// then order, then limit over the record list of a merge by byte key, on the device, so that only the records of the view cross to
// the host.  The rule is the group order's (imm3_group_order.hip); the source of every key part is the record itself
// (merge_view_key, imm3_merge_view_plan.h), the tie is the record's `first` word, and the filter compares in 128 bits.
//
//   k_merge_view_small   n <= kGroupOrderSmall: ONE launch of one work-group.  Keys and indices in LDS, the bitonic network of
//                        k_group_order_small RESTATED here (sharing it through a header changed that kernel's register allocation;
//                        its instructions are to stay what they are), the first n_out records written in order with {n_out, kept}.
//   k_merge_view_keys    larger n: the key column and the count word the launches of imm3_order.hip read; filtered: the kept records'
//                        keys compacted by one atomic add per wave, and map[kept position] = record index;
//   k_merge_view_apply   ... and the records gathered through map[perm[i]], one work-item per 64-bit WORD of the output list: a
//                        record is 7 to 70 and more words, so consecutive work-items store consecutive words.
// No kernel waits on another work-group, spins or polls.
#include "imm3_internal.h"

#include <hip/hip_runtime.h>

namespace imm3 {
namespace {

static_assert(kGroupOrderSmall * (kOrderKeyWords + 1) * 4 <= 64 * 1024, "keys + indices of the small path fit a work-group's static LDS");
static_assert(kGroupOrderSmallThreads % 64 == 0 && kBlockThreads % 64 == 0, "whole waves: every lane of a wave is in its ballot");

// One element of the network: a key and the index of its record.  Padded BY INDEX: an element whose index is >= n is a pad, greater
// than every record and ordered among pads by index.  The tie makes every key unique, so `less` is a strict total order.
struct MvElem {
    uint32_t k[kOrderKeyWords];
    uint32_t idx;
};
__device__ inline bool mv_less(const MvElem &x, const MvElem &y, uint32_t n) {
    if (x.idx >= n || y.idx >= n) return x.idx < y.idx;
    bool less = false, decided = false;
#pragma unroll
    for (int w = 0; w < kOrderKeyWords; ++w) {
        if (!decided && x.k[w] != y.k[w]) {
            less = x.k[w] < y.k[w];
            decided = true;
        }
    }
    return less;
}

// LDS layout and steps: k_group_order_small's (structure-of-arrays words; the steps at distance < 64 stay in a wave's registers).  A
// dropped record becomes a pad -- index P + e, above every record's and every natural pad's --; the kept records are counted in LDS
// (a wave ballot, one ds_add per wave).  P is whole waves, so every wave runs the load loop as one.
template <bool FILT>
__global__ __launch_bounds__(kGroupOrderSmallThreads) void k_merge_view_small(const MergeViewArgs a) {
    __shared__ uint32_t s_k[kOrderKeyWords][kGroupOrderSmall];
    __shared__ uint32_t s_i[kGroupOrderSmall];
    __shared__ uint32_t s_kept;
    const uint32_t t = threadIdx.x, n = a.n < (uint32_t)kGroupOrderSmall ? a.n : (uint32_t)kGroupOrderSmall;
    const size_t R = (size_t)a.plan.rec_words;
    uint32_t P = 64;
    while (P < n) P <<= 1;
    if constexpr (FILT) {
        if (t == 0) s_kept = 0u;
        __syncthreads();
    }
    for (uint32_t e = t; e < P; e += kGroupOrderSmallThreads) {
        uint32_t k[kOrderKeyWords] = {0u, 0u, 0u, 0u};
        uint32_t idx = e;
        if constexpr (FILT) {
            const bool keep = e < n && merge_view_keep(a.plan, a.recs + (size_t)e * R);
            const unsigned long long m = __ballot(keep);
            if ((t & 63u) == 0u && m) atomicAdd(&s_kept, (uint32_t)__popcll(m));
            if (keep) merge_view_key(a.plan, a.recs + (size_t)e * R, k);
            else if (e < n) idx = P + e;
        } else {
            if (e < n) merge_view_key(a.plan, a.recs + (size_t)e * R, k);
        }
#pragma unroll
        for (int w = 0; w < kOrderKeyWords; ++w) s_k[w][e] = k[w];
        s_i[e] = idx;
    }
    __syncthreads();
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j >= 64; j >>= 1) { // partners in different waves: through LDS
            for (uint32_t p = t; p < P / 2; p += kGroupOrderSmallThreads) {
                const uint32_t lo = ((p & ~(j - 1)) << 1) | (p & (j - 1)), up = lo + j;
                MvElem x, y;
#pragma unroll
                for (int w = 0; w < kOrderKeyWords; ++w) {
                    x.k[w] = s_k[w][lo];
                    y.k[w] = s_k[w][up];
                }
                x.idx = s_i[lo];
                y.idx = s_i[up];
                const bool ascending = (lo & k) == 0;
                if (mv_less(y, x, n) == ascending) {
#pragma unroll
                    for (int w = 0; w < kOrderKeyWords; ++w) {
                        s_k[w][lo] = y.k[w];
                        s_k[w][up] = x.k[w];
                    }
                    s_i[lo] = y.idx;
                    s_i[up] = x.idx;
                }
            }
            __syncthreads();
        }
        for (uint32_t e = t; e < P; e += kGroupOrderSmallThreads) { // partners in this wave (P is whole waves: a wave is in or out as one)
            MvElem x;
#pragma unroll
            for (int w = 0; w < kOrderKeyWords; ++w) x.k[w] = s_k[w][e];
            x.idx = s_i[e];
            const bool ascending = (e & k) == 0;
            for (uint32_t j = (k >> 1) < 32u ? (k >> 1) : 32u; j >= 1; j >>= 1) {
                MvElem y;
#pragma unroll
                for (int w = 0; w < kOrderKeyWords; ++w) y.k[w] = (uint32_t)__shfl_xor((int)x.k[w], (int)j, 64);
                y.idx = (uint32_t)__shfl_xor((int)x.idx, (int)j, 64);
                const bool keep_min = ((e & j) == 0) == ascending;
                const bool y_less = mv_less(y, x, n);
                if (keep_min ? y_less : !y_less) x = y;
            }
#pragma unroll
            for (int w = 0; w < kOrderKeyWords; ++w) s_k[w][e] = x.k[w];
            s_i[e] = x.idx;
        }
        __syncthreads();
    }
    uint32_t kept = n;
    if constexpr (FILT) kept = s_kept;
    const uint32_t n_out = a.n_out < kept ? a.n_out : kept;
    const uint32_t words = n_out * (uint32_t)R; // (<= 2048 records of far fewer than 2^20 words)
    for (uint32_t w = t; w < words; w += kGroupOrderSmallThreads) {
        const uint32_t i = w / (uint32_t)R, j = w - i * (uint32_t)R;
        const uint32_t g = s_i[i];
        if (g < n) a.dst[w] = a.recs[(size_t)g * R + j]; // (always: the records sort in front of the pads)
    }
    if (t == 0) {
        a.dst_n[0] = n_out;
        a.dst_n[1] = kept;
    }
}

// the key of record g as row `row` of the key column
__device__ inline void mv_store_key(const MergeViewArgs &a, uint32_t g, uint32_t row) {
    const int kb = a.plan.layout.key_bytes;
    uint32_t k[kOrderKeyWords];
    merge_view_key(a.plan, a.recs + (size_t)g * (size_t)a.plan.rec_words, k);
    uint8_t *dst = a.key_col + (size_t)row * (size_t)kb;
    for (int b = 0; b < kb; ++b) {
        const int w = b >> 2;
        const uint32_t word = w == 0 ? k[0] : (w == 1 ? k[1] : (w == 2 ? k[2] : k[3]));
        dst[b] = (uint8_t)(word >> ((3 - (b & 3)) * 8));
    }
}
// FILT: a wave claims its rows with ONE atomic add on n_word (zeroed on the stream before the launch; the kept count once the launch
// is over) and places them by the ballot's prefix.  The compaction is not stable -- the tie is part of every key, so the sort gives
// the same bytes whatever the order of its input.  The loop's bound is the same for a whole work-group: every lane of a wave is in
// the ballot.
template <bool FILT>
__global__ __launch_bounds__(kBlockThreads) void k_merge_view_keys(const MergeViewArgs a) {
    if constexpr (!FILT) {
        for (uint32_t g = blockIdx.x * kBlockThreads + threadIdx.x; g < a.n; g += gridDim.x * kBlockThreads) mv_store_key(a, g, g);
        if (blockIdx.x == 0 && threadIdx.x == 0) *a.n_word = a.n;
    } else {
        const uint32_t lane = threadIdx.x & 63u;
        for (uint32_t base = blockIdx.x * kBlockThreads; base < a.n; base += gridDim.x * kBlockThreads) {
            const uint32_t g = base + threadIdx.x;
            const bool keep = g < a.n && merge_view_keep(a.plan, a.recs + (size_t)g * (size_t)a.plan.rec_words);
            const unsigned long long m = __ballot(keep);
            uint32_t first = 0;
            if (lane == 0u && m) first = (uint32_t)atomicAdd(a.n_word, (unsigned long long)__popcll(m));
            first = (uint32_t)__shfl((int)first, 0, 64);
            if (keep) {
                const uint32_t row = first + (uint32_t)__popcll(m & ((1ULL << lane) - 1ULL));
                if (row < a.n) { // (always: no more rows are claimed than records evaluated)
                    mv_store_key(a, g, row);
                    a.map[row] = g;
                }
            }
        }
    }
}

// the ordered records through the order's final permutation (k_order_apply's reading of the order's state words); FILT: the
// permutation holds kept positions (st[OW_N] = the kept count), map turns them into record indices.  dst_n[1] is n_word, which holds
// the kept count already.
template <bool FILT>
__global__ __launch_bounds__(kBlockThreads) void k_merge_view_apply(const MergeViewArgs a) {
    const uint32_t *st = a.state;
    const uint32_t n = st[OW_N] < a.n ? st[OW_N] : a.n;
    const uint32_t n_out = st[OW_N_OUT] < a.n_out ? st[OW_N_OUT] : a.n_out;
    const uint32_t *perm = a.perm[(st[OW_SELECT] + (uint32_t)__popc(st[OW_ACTIVE])) & 1u];
    const unsigned long long R = (unsigned long long)a.plan.rec_words, words = (unsigned long long)n_out * R;
    for (unsigned long long w = (unsigned long long)blockIdx.x * kBlockThreads + threadIdx.x; w < words; w += (unsigned long long)gridDim.x * kBlockThreads) {
        const unsigned long long i = w / R, j = w - i * R;
        const uint32_t p = perm[i];
        if (p >= n) continue; // (never: the permutation holds positions below the count)
        uint32_t g = p;
        if constexpr (FILT) g = a.map[p];
        if (g < a.n) a.dst[w] = a.recs[(unsigned long long)g * R + j];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) a.dst_n[0] = n_out;
}

int mv_grid(unsigned long long items) {
    const unsigned long long blocks = (items + kBlockThreads - 1) / kBlockThreads;
    return (int)std::max<unsigned long long>(1ULL, std::min<unsigned long long>(blocks, 2048ULL));
}

} // namespace

void launch_merge_view_small(const MergeViewArgs &a, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (a.plan.prog.n_prog > 0) IMM3_LAUNCH(k_merge_view_small<true>, 1, kGroupOrderSmallThreads, s, ev0, ev1, a);
    else IMM3_LAUNCH(k_merge_view_small<false>, 1, kGroupOrderSmallThreads, s, ev0, ev1, a);
}
void launch_merge_view_keys(const MergeViewArgs &a, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (a.plan.prog.n_prog > 0) IMM3_LAUNCH(k_merge_view_keys<true>, mv_grid(a.n), kBlockThreads, s, ev0, ev1, a);
    else IMM3_LAUNCH(k_merge_view_keys<false>, mv_grid(a.n), kBlockThreads, s, ev0, ev1, a);
}
void launch_merge_view_apply(const MergeViewArgs &a, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    const int grid = mv_grid((unsigned long long)a.n_out * (unsigned long long)a.plan.rec_words);
    if (a.plan.prog.n_prog > 0) IMM3_LAUNCH(k_merge_view_apply<true>, grid, kBlockThreads, s, ev0, ev1, a);
    else IMM3_LAUNCH(k_merge_view_apply<false>, grid, kBlockThreads, s, ev0, ev1, a);
}

} // namespace imm3
