// The sizing of a COUNT(DISTINCT) aggregate's pair set on its own (immutable3_amd/csrc/imm3_distinct_plan.{h,cpp}), for a build under
// -fsanitize=address,undefined: tests/test_count_distinct_host.py compiles this file together with the unit and runs it.  No device:
// distinct_capacity is pure.  Every (rows, key bytes, width) of a sweep -- the edges of every power of two, the widest arguments, the
// refusals -- is held against an evaluation in 128-bit integers, which cannot overflow where the unit's 64-bit arithmetic might (the
// sanitizer would say so).  Prints one line per part; exits non-zero on the first disagreement.
#include "../../immutable3_amd/csrc/imm3_distinct_plan.h"

#include <cstdio>
#include <random>
#include <vector>

using namespace imm3;
typedef unsigned __int128 u128;

static int64_t model(int64_t rows, int32_t key_bytes, int32_t width) {
    if (rows < 0 || key_bytes < 0 || width < 1 || width > 4) return -2;
    const u128 r = rows > 0 ? (u128)rows : 1;
    u128 domain = 1;
    for (int b = 0; b < key_bytes && domain <= r; ++b) domain <<= 8; // (saturates: past r it no longer matters)
    const u128 groups = domain < r ? domain : r;
    u128 pairs = groups << (8 * width);
    if (pairs > r) pairs = r;
    u128 cap = 1024;
    while (cap < 2 * pairs) cap <<= 1;
    return cap > ((u128)1 << 28) ? -1 : (int64_t)cap;
}

int main() {
    std::vector<int64_t> rows = {0, 1, 2, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 65535, 65536, 65537, 100000000, INT64_MAX, INT64_MAX - 1};
    for (int s = 8; s < 63; ++s)
        for (int64_t d = -1; d <= 1; ++d) rows.push_back(((int64_t)1 << s) + d);
    std::mt19937_64 rng(5);
    for (int i = 0; i < 2000; ++i) rows.push_back((int64_t)(rng() >> (1 + rng() % 62)));
    long checked = 0, refused = 0;
    for (int64_t r : rows)
        for (int32_t kb : {0, 1, 2, 3, 4, 7, 8, 9, 16, 256, 1 << 30})
            for (int32_t w = 1; w <= 4; ++w) {
                const int64_t got = distinct_capacity(r, kb, w), want = model(r, kb, w);
                if (got != want) {
                    std::printf("distinct_capacity(%lld, %d, %d) = %lld, the model says %lld\n", (long long)r, kb, w, (long long)got, (long long)want);
                    return 1;
                }
                if (got > 0 && ((got & (got - 1)) != 0 || got < kDistinctMinEntries || got > kDistinctMaxEntries)) {
                    std::printf("distinct_capacity(%lld, %d, %d) = %lld is no power of two in [2^10, 2^28]\n", (long long)r, kb, w, (long long)got);
                    return 1;
                }
                ++checked;
                refused += got == -1;
            }
    std::printf("%ld capacities ok, %ld of them refusals\n", checked, refused);
    int bad = 0;
    for (int32_t w : {0, 5, -1, 1 << 30}) bad += distinct_capacity(100, 2, w) == -2;
    bad += distinct_capacity(-1, 2, 1) == -2;
    bad += distinct_capacity(100, -1, 1) == -2;
    if (bad != 6) {
        std::printf("bad arguments: %d of 6 refused\n", bad);
        return 1;
    }
    std::printf("6 bad arguments ok\n");
    return 0;
}
