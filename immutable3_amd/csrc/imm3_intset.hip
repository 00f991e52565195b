// imm3_intset.hip -- the device passes of imm3_int_set_create (include/imm3.h), for gfx950 (wave64): the set of the
// distinct values one column takes among the rows a query selects, as the open-addressing table k_filter_int_list and eval_row
// already probe (imm3_int_list_plan.h: int_list_home, int_list_probe) -- so neither of them changes.
//
//   k_int_set_stats    walks a source's select bitmap: minimum, maximum and number of the selected rows' values.  The host then picks
//                      `empty` just outside [min, max] and sizes the scratch table (imm3_int_set_plan.cpp).
//   k_int_set_fill     every slot of a table = empty.
//   k_int_set_insert   the same walk: every selected row's value into the scratch table by linear probing, compare-and-swap on the slot.
//   k_int_set_rehash   one pass over a table's slots: every value into the final, smaller table (the same insert), and the values in
//                      -128 .. 127 into the 256-bit set int8 consumers test.
//
// The walk is k_distinct_mark's (imm3_agg.hip): a lane reads one bitmap word of 64, the wave skips the zero words with one ballot,
// then takes the others one at a time, a lane per row; the row's value is read through the table's tile pointers or, on a ragged
// layout, at word_row_base[word] + lane.  Bits at or beyond a word's valid rows are masked off: padding contributes nothing.
//
// The insert keeps k_distinct_mark's discipline.  The PLAIN READ in front of the compare-and-swap: within one launch a slot goes
// from empty to its final value exactly once (the fill is an earlier operation on the stream, and nothing ever empties or rewrites a
// slot).  The XCDs' L2s are not coherent and a vector L1 is never refreshed by another CU's stores, so the read may be stale -- but a
// stale read can only show the EARLIER state, "empty", and then the compare-and-swap (performed at the memory side, on the current
// value) settles it; a non-empty read is the slot's final value, whoever wrote it.  Neither outcome can place a value twice or miss one.
// Every probe loop is bounded by the slot count and every index is masked: a table without a free slot raises the overflow flag and
// the lane leaves -- no loop depends on meeting an empty slot, and no work-group waits on another.  The slot count is not what bounds
// the work of an overflowing build, though: the insert keeps a running count against the cap and raises the flag the moment it is
// passed, and walks and probes leave when they see the flag (k_int_set_insert).  The slots a value's probe passed
// were taken when it passed them and stay taken, so a later probe of at most (its insertion distance + 1) steps finds it before any
// empty slot: the wave-reduced maximum of those is the table's max_probe.  The layout depends on the arrival order; membership does not.
//
// Bookkeeping: counts and maxima are kept per lane over the whole grid-stride loop and reduced once per wave -- one atomic each per
// wave, none at all from a wave that saw no selected row.
#include "imm3_internal.h"
#include "imm3_device.h"
#include <hip/hip_ext.h>

namespace imm3 {

namespace {

__device__ __forceinline__ uint32_t wave_max(uint32_t x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t y = (uint32_t)__shfl_xor((int)x, d);
        x = y > x ? y : x;
    }
    return x;
}
__device__ __forceinline__ int32_t wave_min_i32(int32_t x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int32_t y = __shfl_xor(x, d);
        x = y < x ? y : x;
    }
    return x;
}
__device__ __forceinline__ int32_t wave_max_i32(int32_t x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int32_t y = __shfl_xor(x, d);
        x = y > x ? y : x;
    }
    return x;
}

// the valid rows of bitmap word wi: a ragged layout's own table, a table's tile, else the segment's row count
__device__ __forceinline__ int64_t word_valid_rows(const IntSetSource &a, int64_t wi) {
    if (a.word_nvalid) return (int64_t)a.word_nvalid[wi];
    if (a.tile_rows) return (int64_t)a.tile_rows[wi / kTileWords] - (wi % kTileWords) * 64;
    return a.n_rows - wi * 64;
}

// f(v) for the value of every selected row, a lane per row; all 64 lanes of a wave come back together.  The two hooks are called by
// the whole wave and answer wave-uniformly "stop the walk": batch() in front of every batch of 64 bitmap words, word() behind every
// word that had a selected row.
template <class F, class B, class W>
__device__ __forceinline__ void walk_selected(const IntSetSource &a, uint32_t &rows_seen, F &&f, B &&batch, W &&word_done) {
    const int lane = threadIdx.x & 63;
    for (int64_t base = (int64_t)blockIdx.x * kBlockThreads + (threadIdx.x & ~63); base < a.n_words; base += (int64_t)gridDim.x * kBlockThreads) {
        if (batch()) return;
        uint64_t mine = 0ULL;
        if (base + lane < a.n_words) mine = a.bitmap[base + lane] & low_mask(word_valid_rows(a, base + lane));
        rows_seen += (uint32_t)__popcll(mine);
        uint64_t todo = ballot64(mine != 0ULL);
        while (todo) { // wave-uniform
            const int b = __builtin_ctzll(todo);
            todo &= todo - 1ULL;
            const int64_t wi = base + b;
            const uint64_t word = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(mine >> 32), b) << 32) | (uint32_t)__shfl((int)(uint32_t)mine, b);
            if ((word >> lane) & 1ULL) { // (all lanes meet again before the next shuffle)
                const int64_t row = a.word_row_base ? (int64_t)a.word_row_base[wi] + lane : wi * 64 + lane;
                const uint8_t *p;
                if (a.tile_ptrs) p = (const uint8_t *)as_global(a.tile_ptrs[row / kTileRows]) + (row % kTileRows) * (int64_t)a.width;
                else p = (const uint8_t *)a.data + row * (int64_t)a.width;
                const int32_t v = a.width == 4 ? *(const int32_t *)p : (int32_t)*(const int8_t *)p;
                if (!(a.has_skip && v == a.skip)) f(v);
            }
            if (word_done()) return;
        }
    }
}

// the overflow flag as another work-group may just have raised it (a relaxed device-scope load: never served from a stale vector L1 line)
__device__ __forceinline__ bool overflow_raised(const uint32_t *header) {
    return __hip_atomic_load(header + ISH_OVERFLOW, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
}

// one value into the table (see the head of the file); claimed / far / full are the lane's running bookkeeping.  `header` (may be
// null): a probe that has gone kIntSetFlagSteps steps looks at the overflow flag and leaves when another lane has raised it
constexpr uint32_t kIntSetFlagSteps = 64;
__device__ __forceinline__ void set_insert(const IntSetTable &t, int32_t v, uint32_t &claimed, uint32_t &far, uint32_t &full, const uint32_t *header) {
    if (v == t.empty) return; // (never a member; the host picked `empty` outside every source's values)
    const uint32_t home = int_list_home(v, t.shift);
    for (uint32_t d = 0; d <= t.mask; ++d) {
        if (header && (d % kIntSetFlagSteps) == kIntSetFlagSteps - 1 && overflow_raised(header)) return;
        int32_t *slot = t.slots + ((home + d) & t.mask);
        int32_t cur = *slot; // (plain: see above)
        if (cur == t.empty) {
            cur = atomicCAS(slot, t.empty, v);
            if (cur == t.empty) { // this lane's is the value's first arrival
                ++claimed;
                far = far > d + 1 ? far : d + 1;
                return;
            }
        }
        if (cur == v) return;
    }
    full = 1u; // every slot holds another value
}

// the lanes' bookkeeping of an insert pass into the header: one atomic each per wave, and only from waves that have something to say
__device__ __forceinline__ void report_inserts(uint32_t *header, int count_word, int probe_word, uint32_t claimed, uint32_t far, uint32_t full) {
    claimed = wave_sum(claimed);
    far = wave_max(far);
    full = wave_max(full);
    if ((threadIdx.x & 63) != 0) return;
    if (claimed) atomicAdd(header + count_word, claimed);
    if (far > 1u) atomicMax(header + probe_word, far);
    if (full) atomicOr(header + ISH_OVERFLOW, 1u);
}

} // namespace

__global__ __launch_bounds__(64) void k_int_set_init(uint32_t *header) {
    const int i = threadIdx.x;
    if (i >= ISH_WORDS) return;
    uint32_t v = 0u;
    if (i == ISH_MIN) v = (uint32_t)INT32_MAX;
    if (i == ISH_MAX) v = (uint32_t)INT32_MIN;
    if (i == ISH_PROBE0 || i == ISH_PROBE1) v = 1u; // (an empty table: one step meets an empty slot)
    header[i] = v;
}

__global__ __launch_bounds__(kBlockThreads) void k_int_set_stats(const IntSetSource a, uint32_t *header) {
    int32_t mn = INT32_MAX, mx = INT32_MIN;
    uint32_t rows = 0;
    walk_selected(a, rows, [&](int32_t v) {
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
    }, [] { return false; }, [] { return false; });
    rows = wave_sum(rows);
    mn = wave_min_i32(mn);
    mx = wave_max_i32(mx);
    if ((threadIdx.x & 63) == 0 && rows) { // one atomic pair per wave (and the wave's rows)
        if (mn <= mx) {
            atomicMin((int *)header + ISH_MIN, mn);
            atomicMax((int *)header + ISH_MAX, mx);
        }
        atomicAdd((unsigned long long *)(header + ISH_ROWS_LO), (unsigned long long)rows);
    }
}

__global__ __launch_bounds__(kBlockThreads) void k_int_set_fill(const IntSetTable t) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x; i <= (uint64_t)t.mask; i += (uint64_t)gridDim.x * kBlockThreads) t.slots[i] = t.empty;
}

// The running count against the cap.  A wave adds its claims to ISH_COUNT0 whenever kIntSetFlushClaims of them are pending (and once
// at its end); the add's return value is the count before it, so the wave that takes the count past `cap` KNOWS it and raises the
// overflow flag at once -- the count only grows, so that is never a false alarm.  Every wave looks at the flag in front of each batch
// of 64 bitmap words, every probe every kIntSetFlagSteps steps: behind the flag a wave does at most one batch of 64-step probes.
// Before the flag the table holds at most cap + (waves x (kIntSetFlushClaims + 63)) values: with 8192 waves 2.6 M above the cap, in a
// table of at least 2 x cap slots -- at the real cap of 2^24 a load of 58 % at the worst, so the probes stay short; a table sized
// below that (a small cap) is exhausted after at most `slots` steps per value, which is what bounds the work there.
constexpr uint32_t kIntSetFlushClaims = 256;
__global__ __launch_bounds__(kBlockThreads) void k_int_set_insert(const IntSetSource a, const IntSetTable t, const uint32_t cap, uint32_t *header) {
    const int lane = threadIdx.x & 63;
    uint32_t rows = 0, claimed = 0, far = 0, full = 0;
    uint32_t counted = 0;  // the lane's claims that the wave has already taken into `pending`
    uint32_t pending = 0;  // wave-uniform: claims not yet added to the header
    auto flush = [&]() -> bool { // wave-uniform; true: the count has passed the cap
        uint32_t before = 0;
        if (lane == 0) before = atomicAdd(header + ISH_COUNT0, pending);
        before = (uint32_t)__shfl((int)before, 0);
        const bool over = (uint64_t)before + pending > (uint64_t)cap;
        if (over && lane == 0) atomicOr(header + ISH_OVERFLOW, 1u);
        pending = 0;
        return over;
    };
    walk_selected(a, rows, [&](int32_t v) { set_insert(t, v, claimed, far, full, header); },
                  [&] { return ballot64(overflow_raised(header)) != 0ULL; },
                  [&] {
                      pending += (uint32_t)__popcll(ballot64(claimed != counted));
                      counted = claimed; // (a lane claims at most one slot per word)
                      return pending >= kIntSetFlushClaims && flush();
                  });
    if (pending) flush();
    report_inserts(header, ISH_COUNT0, ISH_PROBE0, 0u, far, full); // (the claims have gone through flush)
}

template <bool INSERT>
__global__ __launch_bounds__(kBlockThreads) void k_int_set_rehash(const IntSetTable from, const IntSetTable to, uint32_t *header) {
    __shared__ uint32_t s_set[8];
    if (threadIdx.x < 8) s_set[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t claimed = 0, far = 0, full = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x; i <= (uint64_t)from.mask; i += (uint64_t)gridDim.x * kBlockThreads) {
        const int32_t v = from.slots[i];
        if (v == from.empty) continue;
        if constexpr (INSERT) set_insert(to, v, claimed, far, full, nullptr); // (n values into int_list_slots(n) slots: it cannot overflow)
        if (v >= -128 && v <= 127) {
            const uint32_t b = (uint32_t)v & 255u;
            atomicOr(&s_set[b >> 5], 1u << (b & 31u));
        }
    }
    if constexpr (INSERT) report_inserts(header, ISH_COUNT1, ISH_PROBE1, claimed, far, full);
    __syncthreads();
    if (threadIdx.x < 8 && s_set[threadIdx.x]) atomicOr(header + ISH_SET256 + threadIdx.x, s_set[threadIdx.x]); // the work-group's copy, flushed with at most 8 atomics
}

namespace {
int walk_grid(int64_t n_words) {
    const int64_t waves = (n_words + 63) / 64; // one bitmap word per lane
    return (int)std::max<int64_t>(1, std::min<int64_t>((waves + kWavesPerBlock - 1) / kWavesPerBlock, 2048));
}
int slot_grid(uint32_t mask) {
    const int64_t slots = (int64_t)mask + 1;
    return (int)std::max<int64_t>(1, std::min<int64_t>((slots + kBlockThreads - 1) / kBlockThreads, 2048));
}
} // namespace

void launch_int_set_init(uint32_t *header, hipStream_t s) { hipLaunchKernelGGL(k_int_set_init, dim3(1), dim3(64), 0, s, header); }
void launch_int_set_stats(const IntSetSource &src, uint32_t *header, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    IMM3_LAUNCH(k_int_set_stats, walk_grid(src.n_words), kBlockThreads, s, ev0, ev1, src, header);
}
void launch_int_set_fill(const IntSetTable &t, hipStream_t s) { hipLaunchKernelGGL(k_int_set_fill, dim3(slot_grid(t.mask)), dim3(kBlockThreads), 0, s, t); }
void launch_int_set_insert(const IntSetSource &src, const IntSetTable &t, uint32_t cap, uint32_t *header, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    IMM3_LAUNCH(k_int_set_insert, walk_grid(src.n_words), kBlockThreads, s, ev0, ev1, src, t, cap, header);
}
void launch_int_set_rehash(const IntSetTable &from, const IntSetTable &to, uint32_t *header, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (to.slots) IMM3_LAUNCH(k_int_set_rehash<true>, slot_grid(from.mask), kBlockThreads, s, ev0, ev1, from, to, header);
    else IMM3_LAUNCH(k_int_set_rehash<false>, slot_grid(from.mask), kBlockThreads, s, ev0, ev1, from, to, header);
}

} // namespace imm3
