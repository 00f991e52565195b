// imm3_group_order.hip -- ORDER BY over groups (imm3_query_set_group_order): the dense groups of a settled aggregation ordered by up to
// four keys -- group columns and aggregates --, all of them or the first `limit` ("Ordering groups").
//
// One normalised big-endian key per group (go_build_key; the layout: imm3_group_order_plan.h): the user's keys in imm3_order_key.h's
// normal form (signed values sign-flipped, a descending key complemented), then first_row, never complemented.  first_row makes every
// key unique -- k_group_collect emits the groups in the order of an atomicAdd, which differs from run to run -- so any correct sort
// gives the same result, and groups whose user keys are equal stay in first-seen order.
//
//   k_group_order_small   n <= kGroupOrderSmall: ONE launch of one work-group.  Keys and indices in LDS, a bitonic sort over the next
//                         power of two, the ordered dense arrays and the ordered count written by the same launch.
//   k_group_order_keys    larger n: the key as one byte-string column of 5 .. 16 bytes per group plus the group count as the 64-bit word
//                         the launches of imm3_order.hip read; those then sort (or select and sort) it as ONE KIND_STR key, unchanged;
//   k_group_order_apply   ... and the dense arrays are gathered through the final permutation.
//
// HAVING (imm3_query_set_group_filter; "Filtering groups" in the same section): each of the three has a FILTERED instance that takes the
// checked program (imm3_group_filter_plan.h) as a second argument and runs group_filter_eval on a group as it loads it -- the view is
// filter, then order, then limit, in the same launches.  A query without a filter launches the instances above, unchanged.
#include "imm3_internal.h"

#include <hip/hip_runtime.h>

namespace imm3 {
namespace {

static_assert(kGroupOrderSmall * (kOrderKeyWords + 1) * 4 <= 64 * 1024, "keys + indices of the small path fit a work-group's static LDS");
static_assert((kGroupOrderSmall & (kGroupOrderSmall - 1)) == 0 && kGroupOrderSmall >= 64, "the bitonic network is a power of two of whole waves");
static_assert(IMM3_GROUP_ORDER_KEY_MAX_WIDTH + kGroupOrderFirstBytes <= kOrderKeyMaxBytes, "the whole key fits the order's 16-byte key");

// the normalised key of dense group g: key byte 0 in the top byte of k[0], zero-padded to 16 bytes
__device__ inline void go_build_key(const GroupOrderArgs &a, uint32_t g, uint32_t k[kOrderKeyWords]) {
    unsigned long long hi = 0, lo = 0;
    auto push = [&](uint32_t byte) {
        hi = (hi << 8) | (lo >> 56);
        lo = (lo << 8) | (unsigned long long)(byte & 0xFFu);
    };
    const unsigned long long packed = a.wide_key ? 0ULL : a.src_keys[g];
    const uint8_t *keyb = a.wide_key ? a.src_keyb + (size_t)g * (size_t)a.key_bytes : nullptr;
    auto key_byte = [&](int b) -> uint32_t { return keyb ? (uint32_t)keyb[b] : (uint32_t)(packed >> (8 * b)) & 0xFFu; };
    for (int c = 0; c < a.layout.n_keys; ++c) {
        const GroupOrderKeyDesc &d = a.layout.k[c];
        const uint32_t flip = d.descending ? 0xFFu : 0u;
        if (d.src == GO_KEY_I32) {
            push(key_byte(d.at + 3) ^ 0x80u ^ flip);
            push(key_byte(d.at + 2) ^ flip);
            push(key_byte(d.at + 1) ^ flip);
            push(key_byte(d.at) ^ flip);
        } else if (d.src == GO_KEY_I8) {
            push(key_byte(d.at) ^ 0x80u ^ flip);
        } else if (d.src == GO_KEY_STR) {
            for (int x = 0; x < d.width; ++x) push(key_byte(d.at + x) ^ flip);
        } else if (d.src == GO_COUNT) {
            const unsigned long long v = a.src_counts[g];
            for (int x = 4; x >= 0; --x) push((uint32_t)(v >> (8 * x)) ^ flip);
        } else if (d.src == GO_WIDE_STR) {
            const uint8_t *p = a.src_str[d.at] + (size_t)g * (size_t)d.width;
            for (int x = 0; x < d.width; ++x) push((uint32_t)p[x] ^ flip);
        } else {
            unsigned long long v = (unsigned long long)a.src_vals[(size_t)g * kMaxAggs + d.at];
            int bytes = d.width; // GO_VAL_STR: the value's bytes packed big-endian in the low `width` bytes
            if (d.src == GO_VAL_I32) { v = (v & 0xFFFFFFFFULL) ^ 0x80000000ULL; bytes = 4; }
            else if (d.src == GO_VAL_I8) { v = (v & 0xFFULL) ^ 0x80ULL; bytes = 1; }
            else if (d.src == GO_SUM) { v ^= 1ULL << 63; bytes = 8; }
            for (int x = bytes - 1; x >= 0; --x) push((uint32_t)(v >> (8 * x)) ^ flip);
        }
    }
    const uint32_t first = a.src_first[g];
    push(first >> 24);
    push(first >> 16);
    push(first >> 8);
    push(first);
    for (int b = a.layout.key_bytes; b < kOrderKeyMaxBytes; ++b) push(0u);
    k[0] = (uint32_t)(hi >> 32);
    k[1] = (uint32_t)hi;
    k[2] = (uint32_t)(lo >> 32);
    k[3] = (uint32_t)lo;
}

// dense group g becomes ordered group i (all loads of the fixed-size part before its first store)
__device__ inline void go_gather(const GroupOrderArgs &a, uint32_t i, uint32_t g) {
    const unsigned long long key = a.src_keys[g], cnt = a.src_counts[g];
    const uint32_t first = a.src_first[g];
    long long v[kMaxAggs];
#pragma unroll
    for (int j = 0; j < kMaxAggs; ++j) v[j] = a.src_vals[(size_t)g * kMaxAggs + j];
    a.dst_keys[i] = key;
    a.dst_counts[i] = cnt;
    a.dst_first[i] = first;
#pragma unroll
    for (int j = 0; j < kMaxAggs; ++j) a.dst_vals[(size_t)i * kMaxAggs + j] = v[j];
    if (a.wide_key) {
        const uint8_t *s = a.src_keyb + (size_t)g * (size_t)a.key_bytes;
        uint8_t *d = a.dst_keyb + (size_t)i * (size_t)a.key_bytes;
        for (int b = 0; b < a.key_bytes; ++b) d[b] = s[b];
    }
    for (int j = 0; j < a.n_agg; ++j) {
        const int w = a.str_width[j];
        if (!w) continue;
        const uint8_t *s = a.src_str[j] + (size_t)g * (size_t)w;
        uint8_t *d = a.dst_str[j] + (size_t)i * (size_t)w;
        for (int b = 0; b < w; ++b) d[b] = s[b];
    }
}

// One element of the bitonic network: a key and the dense index it belongs to.  The network is padded BY INDEX: an element whose index
// is >= n is a pad, greater than every group and ordered among pads by index (an all-ones key would be no safe sentinel next to
// complemented bytes).  With first_row in the key no two groups compare equal, so `less` is a strict total order.
struct GoElem {
    uint32_t k[kOrderKeyWords];
    uint32_t idx;
};
__device__ inline bool go_less(const GoElem &x, const GoElem &y, uint32_t n) {
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

// LDS layout: structure-of-arrays words, s_k[w][e] and s_i[e].  A work-item touches element e of each array with one ds_read_b32 /
// ds_write_b32 (bank = dword address % 32, conflicts counted per 32-lane half): in the steps at distance >= 64 the 32 lanes of a half
// hold 32 consecutive elements -- 32 distinct banks, no conflict.  The steps at distance < 64 never touch LDS: a wave keeps its 64
// consecutive elements in registers and exchanges them with its own lanes.
//
// FILT (imm3_query_set_group_filter): the program runs when group e is loaded.  A dropped group becomes a pad -- index P + e, unique and
// above every group's and every natural pad's -- so the network, go_less and the gather stay as they are; the kept groups are counted
// in LDS (a wave ballot, one ds_add per wave) and the launch writes {min(kept, n_out), kept}.  P is whole waves, so every wave runs the
// load loop as one and the ballot sees all of its lanes.
template <bool FILT>
__device__ __forceinline__ void go_small_body(const GroupOrderArgs &a, const GroupFilterArgs *f) {
    __shared__ uint32_t s_k[kOrderKeyWords][kGroupOrderSmall];
    __shared__ uint32_t s_i[kGroupOrderSmall];
    __shared__ uint32_t s_kept;
    const uint32_t t = threadIdx.x, n = a.n < (uint32_t)kGroupOrderSmall ? a.n : (uint32_t)kGroupOrderSmall;
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
            const bool keep = e < n && group_filter_eval(f->prog, a.src_counts[e], a.src_vals + (size_t)e * kMaxAggs);
            const unsigned long long m = __ballot(keep);
            if ((t & 63u) == 0u && m) atomicAdd(&s_kept, (uint32_t)__popcll(m));
            if (keep) go_build_key(a, e, k);
            else if (e < n) idx = P + e;
        } else {
            if (e < n) go_build_key(a, e, k);
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
                GoElem x, y;
#pragma unroll
                for (int w = 0; w < kOrderKeyWords; ++w) {
                    x.k[w] = s_k[w][lo];
                    y.k[w] = s_k[w][up];
                }
                x.idx = s_i[lo];
                y.idx = s_i[up];
                const bool ascending = (lo & k) == 0;
                if (go_less(y, x, n) == ascending) {
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
            GoElem x;
#pragma unroll
            for (int w = 0; w < kOrderKeyWords; ++w) x.k[w] = s_k[w][e];
            x.idx = s_i[e];
            const bool ascending = (e & k) == 0;
            for (uint32_t j = (k >> 1) < 32u ? (k >> 1) : 32u; j >= 1; j >>= 1) {
                GoElem y;
#pragma unroll
                for (int w = 0; w < kOrderKeyWords; ++w) y.k[w] = (uint32_t)__shfl_xor((int)x.k[w], (int)j, 64);
                y.idx = (uint32_t)__shfl_xor((int)x.idx, (int)j, 64);
                const bool keep_min = ((e & j) == 0) == ascending;
                const bool y_less = go_less(y, x, n);
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
    for (uint32_t i = t; i < n_out; i += kGroupOrderSmallThreads) {
        const uint32_t g = s_i[i];
        if (g < n) go_gather(a, i, g); // (always: the groups sort in front of the pads)
    }
    if (t == 0) {
        a.dst_n[0] = n_out;
        if constexpr (FILT) a.dst_n[1] = kept;
    }
}
__global__ __launch_bounds__(kGroupOrderSmallThreads) void k_group_order_small(const GroupOrderArgs a) { go_small_body<false>(a, nullptr); }
__global__ __launch_bounds__(kGroupOrderSmallThreads) void k_group_order_small_filtered(const GroupOrderArgs a, const GroupFilterArgs f) {
    go_small_body<true>(a, &f);
}

// the key of dense group g as row `row` of the key column
__device__ inline void go_store_key(const GroupOrderArgs &a, uint32_t g, uint32_t row) {
    const int kb = a.layout.key_bytes;
    uint32_t k[kOrderKeyWords];
    go_build_key(a, g, k);
    uint8_t *dst = a.key_col + (size_t)row * (size_t)kb;
    for (int b = 0; b < kb; ++b) {
        const int w = b >> 2;
        const uint32_t word = w == 0 ? k[0] : (w == 1 ? k[1] : (w == 2 ? k[2] : k[3]));
        dst[b] = (uint8_t)(word >> ((3 - (b & 3)) * 8));
    }
}
__global__ __launch_bounds__(kBlockThreads) void k_group_order_keys(const GroupOrderArgs a) {
    for (uint32_t g = blockIdx.x * kBlockThreads + threadIdx.x; g < a.n; g += gridDim.x * kBlockThreads) go_store_key(a, g, g);
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.n_word = a.n;
}
// FILTERED: the keys of the groups the program keeps, compacted, and map[kept position] = dense index.  A wave claims its rows with
// ONE atomic add on n_word (zeroed on the stream before the launch; the kept count once the launch is over) and places them by the
// ballot's prefix.  The compaction is not stable -- first_row is part of every key, so the sort gives the same bytes whatever the
// order of its input.  The loop's bound is the same for a whole work-group: every lane of a wave is in the ballot.  No work-group
// waits on another.
__global__ __launch_bounds__(kBlockThreads) void k_group_order_keys_filtered(const GroupOrderArgs a, const GroupFilterArgs f) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t base = blockIdx.x * kBlockThreads; base < a.n; base += gridDim.x * kBlockThreads) {
        const uint32_t g = base + threadIdx.x;
        const bool keep = g < a.n && group_filter_eval(f.prog, a.src_counts[g], a.src_vals + (size_t)g * kMaxAggs);
        const unsigned long long m = __ballot(keep);
        uint32_t first = 0;
        if (lane == 0u && m) first = (uint32_t)atomicAdd(a.n_word, (unsigned long long)__popcll(m));
        first = (uint32_t)__shfl((int)first, 0, 64);
        if (keep) {
            const uint32_t row = first + (uint32_t)__popcll(m & ((1ULL << lane) - 1ULL));
            if (row < a.n) { // (always: no more rows are claimed than groups evaluated)
                go_store_key(a, g, row);
                f.map[row] = g;
            }
        }
    }
}

// the ordered groups through the order's final permutation (k_order_apply's reading of the order's state words)
__global__ __launch_bounds__(kBlockThreads) void k_group_order_apply(const GroupOrderArgs a) {
    const uint32_t *st = a.state;
    const uint32_t n = st[OW_N] < a.n ? st[OW_N] : a.n;
    const uint32_t n_out = st[OW_N_OUT] < a.n_out ? st[OW_N_OUT] : a.n_out;
    const uint32_t *perm = a.perm[(st[OW_SELECT] + (uint32_t)__popc(st[OW_ACTIVE])) & 1u];
    for (uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x; i < n_out; i += gridDim.x * kBlockThreads) {
        const uint32_t g = perm[i];
        if (g < n) go_gather(a, i, g); // (always: the permutation holds dense indices)
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.dst_n = n_out;
}
// FILTERED: the permutation holds kept positions (st[OW_N] = the kept count); map turns them into dense indices.  dst_n[1] is n_word,
// which holds the kept count already.
__global__ __launch_bounds__(kBlockThreads) void k_group_order_apply_filtered(const GroupOrderArgs a, const GroupFilterArgs f) {
    const uint32_t *st = a.state;
    const uint32_t kept = st[OW_N] < a.n ? st[OW_N] : a.n;
    const uint32_t n_out = st[OW_N_OUT] < a.n_out ? st[OW_N_OUT] : a.n_out;
    const uint32_t *perm = a.perm[(st[OW_SELECT] + (uint32_t)__popc(st[OW_ACTIVE])) & 1u];
    for (uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x; i < n_out; i += gridDim.x * kBlockThreads) {
        const uint32_t p = perm[i];
        if (p >= kept) continue; // (never: the permutation holds kept positions)
        const uint32_t g = f.map[p];
        if (g < a.n) go_gather(a, i, g);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.dst_n = n_out;
}

int go_grid(uint32_t n) { return (int)std::max<uint32_t>(1u, std::min<uint32_t>((n + kBlockThreads - 1) / kBlockThreads, 1024u)); }

} // namespace

void launch_group_order_small(const GroupOrderArgs &a, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    IMM3_LAUNCH(k_group_order_small, 1, kGroupOrderSmallThreads, s, ev0, ev1, a);
}
void launch_group_order_keys(const GroupOrderArgs &a, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    IMM3_LAUNCH(k_group_order_keys, go_grid(a.n), kBlockThreads, s, ev0, ev1, a);
}
void launch_group_order_apply(const GroupOrderArgs &a, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    IMM3_LAUNCH(k_group_order_apply, go_grid(a.n_out), kBlockThreads, s, ev0, ev1, a);
}

void launch_group_order_small_filtered(const GroupOrderArgs &a, const GroupFilterArgs &f, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    IMM3_LAUNCH(k_group_order_small_filtered, 1, kGroupOrderSmallThreads, s, ev0, ev1, a, f);
}
void launch_group_order_keys_filtered(const GroupOrderArgs &a, const GroupFilterArgs &f, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    IMM3_LAUNCH(k_group_order_keys_filtered, go_grid(a.n), kBlockThreads, s, ev0, ev1, a, f);
}
void launch_group_order_apply_filtered(const GroupOrderArgs &a, const GroupFilterArgs &f, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    IMM3_LAUNCH(k_group_order_apply_filtered, go_grid(a.n_out), kBlockThreads, s, ev0, ev1, a, f);
}

} // namespace imm3
